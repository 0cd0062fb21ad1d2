"""Mints tests/golden/aligner_ref.npz / aligner_ref.json from the reference's EXECUTED code: models/aligner/model.py,
loader.py and alignment_extractor.py are imported by file path (the fairseq2 names replaced by
tests/golden/_aligner_stub.py) and ``UnitY2AlignmentEncoder.forward``, ``_monotonic_alignment_search``,
``viterbi_decode``, ``postprocess_alignment`` and ``convert_unity2_aligner_checkpoint`` run on seeded inputs.  The fixture
holds inputs, outputs and the signatures of ``AlignmentExtractor.__init__`` / ``extract_alignment``; the tests read only
the fixture.

Search cases: matrices whose entries are multiples of 2^-6 (every sum is exact and ties are frequent, so the tie rule and
the i > j triangle are pinned bit for bit) and random float32 log-softmax matrices.  The reference fills row 0 of Q with
float32 ``sum()`` calls (numpy's pairwise order) while the project's oracle and kernel run the sequential float64
recurrence; on the dyadic matrices both are exact, and a random matrix is kept only if its path margin
(tests/aligner_oracle.py) is at least 1e-3 - the row-0 order noise is about 1e-5 at these lengths.  Discarded draws are
counted; more than half discarded would mean the generator is wrong, not the threshold.

    python tests/golden/make_aligner_goldens.py   # needs the reference tree
"""
from __future__ import annotations

import importlib.util
import inspect
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference/src/seamless_communication")
OUT_NPZ = HERE / "aligner_ref.npz"
OUT_JSON = HERE / "aligner_ref.json"

sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
import _aligner_stub  # noqa: E402
from tests import aligner_oracle as ao  # noqa: E402

CHAR_PIECES = ["<s>", "<pad>", "</s>", "<unk>", "▁", "e", "t", "a", "o", "!", "z", "é", "b", ","]
MIN_MARGIN = 1e-3
N_RANDOM = 20


def load_by_path(name: str, rel: str):
    spec = importlib.util.spec_from_file_location(name, REF / rel)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def signature_of(fn):
    out = []
    for p in inspect.signature(fn).parameters.values():
        d = None if p.default is inspect.Parameter.empty else repr(p.default)
        out.append({"name": p.name, "kind": p.kind.name, "default": d})
    return out


def half_rounded(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float16).to(torch.float32)


def log_softmax_rows(rng, t_feat, t_text, scale):
    x = (rng.standard_normal((t_feat, t_text)) * scale).astype(np.float32)
    return torch.log_softmax(torch.from_numpy(x), dim=-1).numpy()


def main():
    _aligner_stub.install(CHAR_PIECES)
    model = load_by_path("seamless_communication.models.aligner.model", "models/aligner/model.py")
    loader = load_by_path("seamless_communication.models.aligner.loader", "models/aligner/loader.py")
    extractor = load_by_path("ref_alignment_extractor", "models/aligner/alignment_extractor.py")
    rng = np.random.default_rng(20240918)
    arrays, meta = {}, {}
    A = extractor.AlignmentExtractor
    meta["signatures"] = {"__init__": signature_of(A.__init__), "extract_alignment": signature_of(A.extract_alignment)}

    # ---- the search: _monotonic_alignment_search + viterbi_decode -------------------------------------------------------
    def run_search(lp):
        t_feat, t_text = lp.shape
        path = model._monotonic_alignment_search(lp)
        dur = model.viterbi_decode(torch.from_numpy(lp)[None], torch.tensor([t_text]), torch.tensor([t_feat]))[0].numpy()
        assert (np.bincount(path, minlength=t_text) == dur).all()
        return np.asarray(path, dtype=np.int64), dur.astype(np.int64)

    search = []
    dyadic_shapes = [(1, 1), (1, 5), (7, 1), (6, 6), (24, 24), (9, 4), (40, 13), (64, 37), (5, 9), (33, 32), (80, 50), (120, 3)]
    for k, (t_feat, t_text) in enumerate(dyadic_shapes):
        lp = (-rng.integers(1, 5, size=(t_feat, t_text)) / 64.0).astype(np.float32)  # multiples of 2^-6, few values: many ties
        path, dur = run_search(lp)
        name = f"search_dyadic_{k}"
        arrays[name + "_lprob"], arrays[name + "_path"], arrays[name + "_dur"] = lp, path, dur
        search.append({"name": name, "kind": "dyadic", "t_feat": t_feat, "t_text": t_text})
    random_shapes = [(1, 1), (12, 1), (10, 10), (30, 30), (1, 4)] + [(int(rng.integers(8, 97)), 0) for _ in range(64)]
    kept = discarded = 0
    for t_feat, t_text in random_shapes:
        if kept >= N_RANDOM:
            break
        if t_text == 0:
            t_text = int(rng.integers(2, t_feat + 1))
        lp = log_softmax_rows(rng, t_feat, t_text, float(rng.uniform(0.5, 3.0)))
        _, margin = ao.monotonic_alignment_search(lp)
        if margin < MIN_MARGIN:
            discarded += 1
            continue
        path, dur = run_search(lp)
        name = f"search_random_{kept}"
        arrays[name + "_lprob"], arrays[name + "_path"], arrays[name + "_dur"] = lp, path, dur
        search.append({"name": name, "kind": "random", "t_feat": t_feat, "t_text": t_text, "margin": margin})
        kept += 1
    assert kept >= 16 and discarded <= (kept + discarded) / 2, (kept, discarded)
    meta["search"] = search
    meta["search_random_discarded"] = discarded
    meta["search_min_margin"] = MIN_MARGIN

    # ---- the encoder: UnitY2AlignmentEncoder.forward at model_dim 64 (weights and inputs exactly fp16-representable) --------
    enc_cases = []
    for rf in (1, 2):
        torch.manual_seed(100 + rf)
        enc = model.UnitY2AlignmentEncoder(embed_dim=64, feat_dim=64, text_layers=2, feat_layers=3, dropout=0.1, temperature=1.0,
                                           reduction_factor=rf, dtype=torch.float32)
        enc.eval()
        with torch.no_grad():
            for n, p in enc.named_parameters():
                p.copy_(half_rounded(p * (4.0 if n.endswith("weight") else 1.0)))
        for n, p in enc.state_dict().items():
            arrays[f"enc_rf{rf}_sd_alignment_encoder.{n}"] = p.numpy()
        for k, (t_text, t_feat) in enumerate([(1, 1), (5, 17), (12, 12), (23, 90)]):
            te = half_rounded(torch.randn(1, t_text, 64))
            fe = half_rounded(torch.randn(1, t_feat, 64))
            with torch.inference_mode():
                lprob, dur = enc(te, fe, torch.tensor([t_text]), torch.tensor([t_feat]))
            name = f"enc_rf{rf}_{k}"
            arrays[name + "_text"], arrays[name + "_feat"] = te[0].numpy(), fe[0].numpy()
            arrays[name + "_lprob"], arrays[name + "_dur"] = lprob[0].numpy(), dur[0].numpy().astype(np.int64)
            enc_cases.append({"name": name, "reduction_factor": rf, "t_text": t_text, "t_feat": t_feat})
    meta["encoder"] = enc_cases

    # ---- postprocess_alignment (reduction_factor > 1) ----------------------------------------------------------------------
    post = []
    for k, rf in enumerate((2, 3, 4, 2)):
        enc = model.UnitY2AlignmentEncoder(embed_dim=8, feat_dim=8, text_layers=1, feat_layers=1, dropout=0.0, temperature=1.0,
                                           reduction_factor=rf, dtype=torch.float32)
        b, t = 3, 7
        text_lens = rng.integers(1, t + 1, b)
        dur = np.zeros((b, t), dtype=np.int64)
        feat_lens = np.zeros(b, dtype=np.int64)
        for i in range(b):
            dur[i, : text_lens[i]] = rng.integers(0, 4, text_lens[i])
            dur[i, text_lens[i] - 1] += 1
            feat_lens[i] = dur[i].sum() * rf - int(rng.integers(0, rf))  # ceil(feat_len / rf) reduced frames
        out = enc.postprocess_alignment(torch.from_numpy(dur.copy()), torch.from_numpy(text_lens), torch.from_numpy(feat_lens))
        post.append({"reduction_factor": rf, "durations": dur.tolist(), "text_lens": text_lens.tolist(), "feat_lens": feat_lens.tolist(),
                     "out": out.numpy().tolist()})
    meta["postprocess"] = post

    # ---- convert_unity2_aligner_checkpoint (both input layouts) --------------------------------------------------------------
    class Cfg:
        model_name_or_card = "nar_t2u_aligner"

    v = len(CHAR_PIECES)
    ckpt = {
        "text_emb_state": {"weight": torch.arange(v * 3, dtype=torch.float32).reshape(v, 3)},
        "unit_emb_state": {"weight": torch.arange(10, dtype=torch.float32).reshape(5, 2) + 100},
        "aligner_state": {"t_conv.1.weight": torch.ones(2, 2, 3), "t_conv.1.bias": torch.zeros(2), "f_conv.7.weight": torch.ones(2, 2, 1)},
    }
    text_rows_in = ckpt["text_emb_state"]["weight"][:, 0].clone()
    mapping = loader._get_char_index_mapping(Cfg())
    converted = loader.convert_unity2_aligner_checkpoint(ckpt, Cfg())
    again = loader.convert_unity2_aligner_checkpoint(converted, Cfg())
    assert again is converted
    meta["checkpoint"] = {
        "char_pieces": CHAR_PIECES,
        "index_mapping": [int(i) for i in mapping],
        "in_keys": {k: sorted(val) for k, val in ckpt.items() if k != "model"},
        "out_keys": sorted(converted["model"]),
        "text_row_ids_in": [int(x) // 3 for x in text_rows_in.tolist()],
        "text_row_ids_out": [int(x) // 3 for x in converted["model"]["alignment_frontend.embed_text.weight"][:, 0].tolist()],
        "unit_weight": converted["model"]["alignment_frontend.embed_unit.weight"].tolist(),
    }

    np.savez_compressed(OUT_NPZ, **arrays)
    OUT_JSON.write_text(json.dumps(meta, indent=1, ensure_ascii=False) + "\n")
    print(f"wrote {OUT_NPZ} ({OUT_NPZ.stat().st_size} bytes), {OUT_JSON} ({OUT_JSON.stat().st_size} bytes); "
          f"random search cases kept {kept}, discarded {discarded}")


if __name__ == "__main__":
    main()
