"""Child process of tests/test_vocoder_packed_gpu.py: the library reads SC_VOC_PACKED / SC_VOC_PACK_ROWS / SC_VOC_SPLIT once
per process, so every side of the comparison is a fresh process.  Usage: python -m tests.vocoder_packed_child OUT.npz [full]

Runs the cases of CASES on the tiny test model (and, with `full`, on the base_v2 vocoder) and stores every waveform together
with the number of packed groups the library reports for the call (sc_op_last_vocoder_packed_groups; 0 = padded batch or
length buckets)."""
import sys

import numpy as np
import torch

# name -> (unit lengths, T or None for the longest, pass unit_lens?)
CASES = {
    "ragged": ([46, 1224, 230, 565, 47, 900, 333, 612, 1100, 75, 480, 481], None, True),
    "single": ([311], None, True),
    "short": ([5, 200, 1, 64, 12], None, True),  # shorter than the halo, length 1
    "equal": ([150, 150, 150, 150], None, True),
    "capped": ([300, 297, 299, 120], 300, True),  # len + halo > T: need = T
    "padded": ([200, 90, 33], None, False),  # unit_lens == NULL: the padded batch
}
TINY_SCALE = 5  # the tiny model's unit_max_seq_len is shorter: lengths divided by this


def units_for(lens, T, n_emb, pad, seed):
    rng = np.random.RandomState(seed)
    u = np.full((len(lens), T), pad, dtype=np.int32)
    for i, l in enumerate(lens):
        u[i, :l] = rng.randint(2, n_emb, size=l)
    return u


def run(model, cfg, tag, scale, out):
    for ci, (name, (lens, T, ragged)) in enumerate(CASES.items()):
        lens = [max(1, l // scale) for l in lens]
        T = max(lens) if T is None else max(max(lens), T // scale)
        u = units_for(lens, T, cfg.vocoder.num_embeddings, cfg.unit_pad_idx, 100 + ci)
        n = len(lens)
        wav = model.vocode(u, [0] * n, [n % 2] * n, lens if ragged else None)
        out[f"{tag}_{name}_wav"] = wav.cpu().numpy()
        out[f"{tag}_{name}_lens"] = np.asarray(lens, dtype=np.int64)
        out[f"{tag}_{name}_groups"] = np.asarray(model.lib.sc_op_last_vocoder_packed_groups(model.handle))
        out[f"{tag}_{name}_rows"] = np.asarray(model.last_padding()["vocoder_rows_computed"])
        again = model.vocode(u, [0] * n, [n % 2] * n, lens if ragged else None)  # recycled scratch: the same bits
        out[f"{tag}_{name}_repeat_equal"] = np.asarray(bool(torch.equal(wav, again)))


def main():
    out_path, full = sys.argv[1], "full" in sys.argv[2:]
    from tests import common

    out = {}
    tiny = common.make_hip()
    run(tiny, tiny.cfg, "tiny", TINY_SCALE, out)
    out["hop"] = np.asarray(tiny.hop)
    if full:
        from seamless_communication_amd.inference import Translator
        from seamless_communication_amd.inference.translator import DEFAULT_CARDS, Modality

        card = dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="base_v2")
        tr = Translator(card, "vocoder_v2", device="cuda:0", input_modality=Modality.SPEECH)
        run(tr.model, tr.cfg, "full", 1, out)
        out["full_hop"] = np.asarray(tr.model.hop)
    np.savez(out_path, **out)
    print("vocoder_packed_child: wrote", out_path)


if __name__ == "__main__":
    main()
