"""Mints tests/golden/seamless_streaming_policy_ref.json and seamless_streaming_ref.npz.  Data only.

1. The policy traces.  The reference's streaming/agents/pretssel_vocoder.py, dual_vocoder_agent.py and seamless_s2st.py are loaded
   from where they lie and EXECUTED, with the stand-in technique of make_streaming_goldens.py (its helpers are imported): simuleval
   is the restated contract of seamless_communication_amd/streaming/simul.py, fairseq2 and the model packages are placeholders,
   and the PRETSSEL vocoder is a script that records its call (tests/seamless_streaming_script.py): tokens, durations, the number
   of samples the stage had flattened from stage 1's state, the language.  Recorded: the scenarios of ``stage_scenarios()`` through
   PretsselVocoderAgent and DualVocoderAgent, and ``chain_scenarios()`` through the linear SeamlessS2STAgent (its ``pipeline``
   list names the classes the chain is assembled from); every output segment and the vocoder calls behind it.  Also the argparse
   defaults of the two agents, read from their source with ``ast``.  The Silero VAD stage needs ``soundfile`` and the tree pipelines
   SimulEval's TreeAgentPipeline: neither is loaded.

2. The waveforms.  The real reference ``PretsselVocoder`` at arch ``small``, built as make_pretssel_wave_goldens.py builds it
   (seeded synthetic weights of both halves, fp32, CPU), called as the agent calls it - ``durations=`` given,
   ``normalize_before=True``, the gcmvn-normalised fbank (oracle/fbank.py, scale 2**15) of everything heard - for three successive
   chunks of 1, 6 and 17 units against a heard source of 0.32, 0.64 and 0.96 s.  Recorded per chunk: units, tokens, durations, the
   prosody vector, the mel, the waveform; the heard source; the gap of the fp32 oracle (tests/pretssel_oracle.py) to the recorded
   mel and the float64 oracle's smallest |vuv| (the source seed is advanced until it is >= 1e-3).  Asserted: peak |wav| >= 0.3 for
   every chunk.

    python tests/golden/make_seamless_streaming_goldens.py <reference tree>/src/seamless_communication
"""
from __future__ import annotations

import ast
import copy
import importlib.util
import json
import sys
import types
from argparse import Namespace
from pathlib import Path

import numpy as np
import torch
import yaml

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(ROOT))

import make_streaming_goldens as msg  # noqa: E402
from seamless_communication_amd.streaming import simul  # noqa: E402
from seamless_communication_amd.tokenizer import UnitTokenizer  # noqa: E402
from tests import seamless_streaming_script as sx  # noqa: E402
from tests import streaming_script as ss  # noqa: E402

ARCH, SEED, UNIT_SEED = "small", 3, 5
CHUNK_UNITS, HEARD_SECONDS = (1, 6, 17), (0.32, 0.64, 0.96)
TGT_LANG = 1
VUV_MARGIN = 1e-3


# ------------------------------------------------------------------------------------------------------------ 1. policy
class _Converter:
    """WaveformToFbankConverter(channel_last=True) on the (samples, 1) waveform of pretssel_vocoder.py:106-113."""

    heard = 0

    def __init__(self, num_mel_bins=80, waveform_scale=1.0, channel_last=False, standardize=False, device=None, dtype=None):
        assert num_mel_bins == 80 and waveform_scale == 2**15 and channel_last and standardize is False

    def __call__(self, data):
        w = data["waveform"]
        assert data["sample_rate"] == 16000 and w.dim() == 2 and w.shape[1] == 1 and w.dtype == torch.float32
        _Converter.heard = int(w.shape[0])
        return {"fbank": ss.fbank_outputs(w[:, 0].tolist()) * float(2**15)}


class _ScriptPretssel:
    def __init__(self, calls):
        self.calls = calls

    def eval(self):
        return self

    def __call__(self, unit, tgt_lang, prosody_input_seqs, durations, normalize_before):
        assert normalize_before is True and durations.dim() == 2 and durations.shape[0] == 1 and unit.dim() == 1
        assert prosody_input_seqs.shape[0] == 1 + (_Converter.heard - 400) // 160  # the fbank of everything heard reaches the vocoder
        tokens, dur = unit.tolist(), durations[0].tolist()
        self.calls.append(sx.call_record(tokens, dur, _Converter.heard, tgt_lang))
        return [torch.tensor(sx.expressive_outputs(tokens, dur, _Converter.heard)).reshape(1, 1, -1)]


class _Card:
    def __init__(self, value):
        self.value = value

    def field(self, name):
        return _Card(self.value[name])

    def as_(self, kind):
        return kind(self.value)

    def as_list(self, kind):
        return [kind(v) for v in self.value]


def _load(agents_dir: Path, name: str):
    full = f"seamless_communication.streaming.agents.{name}"
    spec = importlib.util.spec_from_file_location(full, agents_dir / f"{name}.py")
    m = importlib.util.module_from_spec(spec)
    sys.modules[full] = m
    setattr(sys.modules["seamless_communication.streaming.agents"], name, m)
    spec.loader.exec_module(m)
    return m


def _placeholder(name: str, **attrs):
    m = msg._Placeholder(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    setattr(sys.modules[parent], leaf, m)
    return m


def argparse_defaults(agents_dir: Path) -> dict:
    """flag -> default of the add_argument calls of the two agents (store_true: False; required: null)."""
    found = {}
    for name in ("pretssel_vocoder", "dual_vocoder_agent"):
        tree = ast.parse((agents_dir / f"{name}.py").read_text())
        for call in (n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "attr", "") == "add_argument"):
            kw = {k.arg: k.value for k in call.keywords}
            flag = call.args[0].value
            if "default" in kw:
                found[flag] = ast.literal_eval(kw["default"])
            elif isinstance(kw.get("action"), ast.Constant) and kw["action"].value == "store_true":
                found[flag] = False
            elif isinstance(kw.get("required"), ast.Constant) and kw["required"].value is True:
                found[flag] = None
    return found


def policy_goldens(root: Path) -> dict:
    agents_dir = root / "streaming" / "agents"
    msg._install_stand_ins()
    calls = []
    card = _Card({"sample_rate": sx.VOCODER_SAMPLE_RATE, "model_config": {"langs": sx.VOCODER_LANGS}})
    sys.modules["fairseq2.assets"].asset_store = Namespace(retrieve_card=lambda name: card)
    sys.modules["fairseq2.data.audio"].WaveformToFbankConverter = _Converter
    sys.modules["seamless_communication.models.generator.loader"].load_pretssel_vocoder_model = lambda *a, **k: _ScriptPretssel(calls)
    sys.modules["seamless_communication.models.unity"].load_gcmvn_stats = lambda name: sx.GCMVN
    _placeholder("seamless_communication.store", add_gated_assets=lambda d: None)
    _placeholder("seamless_communication.streaming.agents.silero_vad")
    _load(agents_dir, "common")
    feat = _load(agents_dir, "online_feature_extractor")
    enc = _load(agents_dir, "offline_w2v_bert_encoder")
    text = _load(agents_dir, "online_text_decoder")
    unit = _load(agents_dir, "online_unit_decoder")
    voc = _load(agents_dir, "online_vocoder")
    _load(agents_dir, "detokenizer")
    _load(agents_dir, "unity_pipeline")
    pv = _load(agents_dir, "pretssel_vocoder")
    dual = _load(agents_dir, "dual_vocoder_agent")
    s2st = _load(agents_dir, "seamless_s2st")
    voc.load_vocoder_model = lambda *a, **k: msg._ScriptVocoder()
    feat.WaveformToFbankConverter = msg.WaveformToFbankConverter  # stage 1 keeps the converter of make_streaming_goldens.py

    def expressive_args(opts, name="vocoder_pretssel"):
        args = msg.reference_args(opts)
        args.vocoder_name, args.gated_model_dir = name, None
        return args

    def pretssel_agent(args):
        agent = pv.PretsselVocoderAgent(args)
        agent.device = args.device  # simuleval's GenericAgent carries the device; the restated one does not
        return agent

    golden = {"argparse_defaults": argparse_defaults(agents_dir), "stages": [], "chain": [],
              "linear_pipeline": [c.__name__ for c in s2st.SeamlessS2STAgent.pipeline]}
    for scn in sx.stage_scenarios():
        if scn["dual"] is None:
            agent = pretssel_agent(expressive_args(scn["opts"]))
        else:
            args = msg.reference_args(scn["opts"])
            args.expressive, args.expr_vocoder_name, args.gated_model_dir = scn["dual"], "vocoder_pretssel", None
            expr_args = copy.deepcopy(args)
            expr_args.vocoder_name = args.expr_vocoder_name
            agent = dual.DualVocoderAgent(args, voc.VocoderAgent(args), pretssel_agent(expr_args))
        del calls[:]
        trace = sx.drive_stage(agent, scn, feat.FeatureStates(), calls, simul.SpeechSegment, simul.TextSegment, simul.EmptySegment)
        golden["stages"].append(dict(name=scn["name"], trace=trace))

    tok = ss.ScriptTokenizer()
    config = Namespace(num_decoder_layers=ss.LAYERS)
    for scn in sx.chain_scenarios():
        args = expressive_args(scn["opts"])
        seed = scn["seed"]
        unity_model = Namespace(encode_speech=lambda seqs, mask, seed=seed: (ss.encoder_outputs(seed, seqs[0]), mask))
        unit_tok = UnitTokenizer(ss.NUM_UNITS, ["eng", "fra", "deu"], "base_v2")
        modules = [feat.OnlineFeatureExtractorAgent(args), enc.OfflineWav2VecBertEncoderAgent(unity_model, Namespace(fbank_stride=2), tok, args),
                   text.UnitYMMATextDecoderAgent(ss.ScriptMonotonicDecoder(seed), config, tok, args),
                   unit.NARUnitYUnitDecoderAgent(ss.ScriptT2U(seed), unit_tok, args), pretssel_agent(args)]
        assert [type(m).__name__ for m in modules] == golden["linear_pipeline"]
        chain = object.__new__(s2st.SeamlessS2STAgent)  # __init__ loads checkpoints; the agents are built above
        simul.AgentPipeline.__init__(chain, modules)
        del calls[:]
        golden["chain"].append(sx.drive_chain(chain, scn, calls, simul.SpeechSegment))

    # the scenarios do reach what they are about
    flat = [r for s in golden["stages"] for r in s["trace"]] + [r for t in golden["chain"] for r in t]
    spoke = sum(len(r["calls"]) for r in flat)
    silent = sum(1 for r in flat if not r["empty"] and r.get("sample_rate") == sx.VOCODER_SAMPLE_RATE and r["content"] == [] and not r["calls"])
    restarts = sum(sx.chain_restarts(t) for t in golden["chain"])
    print(f"{len(golden['stages'])} stage scenarios, {len(golden['chain'])} chain scenarios: {spoke} vocoder calls, {silent} written segments "
          f"without content, {restarts} chain restarts between two chunks")
    assert spoke > 40 and silent > 5 and restarts > 0
    return golden


# ------------------------------------------------------------------------------------------------------------ 2. waveforms
def _forget_stand_ins() -> None:
    for name in [n for n in sys.modules if n.split(".")[0] in ("fairseq2", "simuleval", "seamless_communication")]:
        del sys.modules[name]


def waveform_goldens(root: Path) -> dict:
    _forget_stand_ins()
    import _pretssel_stub

    _pretssel_stub.install(root)
    from make_pretssel_goldens import build
    from oracle import fbank as ofb
    from seamless_communication.models.generator import vocoder as ref
    from seamless_communication_amd import synthetic as syn
    from seamless_communication_amd.config import pretssel_config
    from tests import pretssel_oracle as oracle

    card = yaml.safe_load((root / "cards/vocoder_pretssel.yaml").read_text())
    cfg = pretssel_config(ARCH)
    langs, stats = card["model_config"]["langs"][:cfg.num_langs], card["model_config"]["gcmvn_stats"]
    w = cfg.waveform
    over = dict(upsample_rates=list(w.upsample_rates), upsample_kernel_sizes=list(w.upsample_kernel_sizes), upsample_initial_channel=w.upsample_initial_channel,
                resblock_kernel_sizes=list(w.resblock_kernel_sizes), resblock_dilation_sizes=[list(d) for d in w.resblock_dilation_sizes], dimension=w.dimension,
                n_filters=w.n_filters, ratios=list(w.ratios), kernel_size=w.kernel_size, last_kernel_size=w.kernel_size,
                residual_kernel_size=w.residual_kernel_size)
    shim = types.SimpleNamespace(PretsselEncoderFrontend=ref.PretsselEncoderFrontend, PretsselDecoderFrontend=ref.PretsselDecoderFrontend,
                                 PretsselVocoder=lambda **kw: ref.PretsselVocoder(**{**kw, **over}))
    m = build(shim, cfg, langs, stats)
    sd = {**syn.make_pretssel_state_dict(cfg, SEED), **syn.make_pretssel_wave_state_dict(cfg, SEED)}
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys), res
    mean, std = torch.tensor(stats["mean"], dtype=torch.float32), torch.tensor(stats["std"], dtype=torch.float32)
    g = torch.Generator().manual_seed(UNIT_SEED)
    units = [torch.randint(0, 6, (n,), generator=g) * 37 + 11 for n in CHUNK_UNITS]  # six distinct units: runs of equal ones occur

    got = {}
    inner = m.gcmvn_denormalize
    m.gcmvn_denormalize = lambda x: got.__setitem__("mel", inner(x).clone()) or got["mel"].clone()
    m.encoder_frontend.prosody_encoder.register_forward_hook(lambda mod, a, out: got.__setitem__("pros", out.clone()))
    for wave_seed in range(7, 60):
        heard = syn.synthetic_waveform(wave_seed, max(HEARD_SECONDS)).numpy().astype(np.float32)
        arrs, figs = {"heard": heard}, []
        for i, (u, sec) in enumerate(zip(units, HEARD_SECONDS)):
            n = int(round(sec * 16000))
            feats = (torch.from_numpy(np.asarray(ofb.fbank_raw(heard[:n]), dtype=np.float32)) - mean) / std  # gcmvn_normalize, :73-75
            tokens, dur = torch.unique_consecutive(u + 4, return_counts=True)  # :92-97
            dur = dur * 2
            with torch.inference_mode():
                wav = m(tokens, tgt_lang=langs[TGT_LANG], prosody_input_seqs=feats, durations=dur.unsqueeze(0), normalize_before=True)
            wav = wav[0][0][0]
            frames = int(dur.sum())
            assert wav.numel() == frames * w.hop and got["mel"].shape == (1, frames, cfg.mel_dim)
            tk, tl, du = tokens.unsqueeze(0), torch.tensor([tokens.numel()]), dur.unsqueeze(0)
            pr = {}
            o64, _ = oracle.pretssel_mel(sd, cfg, tk, tl, du, TGT_LANG, got["pros"], stats["mean"], stats["std"], torch.float64, pr)
            o32, _ = oracle.pretssel_mel(sd, cfg, tk, tl, du, TGT_LANG, got["pros"], stats["mean"], stats["std"], torch.float32)
            figs.append(dict(units=int(u.numel()), heard_samples=n, prosody_frames=int(feats.shape[0]), frames=frames, peak=float(wav.abs().max()),
                             vuv_margin=float(pr["vuv"][0, :tl[0]].abs().min()), oracle_fp32_gap_mel=float((o32[0, :frames] - got["mel"][0]).abs().max()),
                             oracle_f64_gap_mel=float((o64[0, :frames] - got["mel"][0]).abs().max())))
            arrs.update({f"units{i}": u.numpy().astype(np.int32), f"tokens{i}": tokens.numpy().astype(np.int32), f"durations{i}": dur.numpy().astype(np.int32),
                         f"pros{i}": got["pros"][0].numpy(), f"mel{i}": got["mel"][0].numpy(), f"wav{i}": wav.numpy()})
        print("source seed", wave_seed, figs)
        if all(f["vuv_margin"] >= VUV_MARGIN for f in figs):
            break
    else:
        raise SystemExit("no source seed keeps the voiced logits clear of zero")
    assert all(f["peak"] >= 0.3 for f in figs), figs  # the 2e-3 bar of the GPU test means something
    meta = dict(arch=ARCH, seed=SEED, unit_seed=UNIT_SEED, wave_seed=wave_seed, tgt_lang=TGT_LANG, langs=langs, gcmvn_stats=stats, sample_rate=card["sample_rate"],
                chunks=figs)
    arrs["meta"] = np.array(json.dumps(meta))
    return arrs


def main() -> None:
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    root = Path(sys.argv[1])
    golden = policy_goldens(root)
    out = HERE / "seamless_streaming_policy_ref.json"
    out.write_text(json.dumps(golden, separators=(",", ":")))
    print(f"wrote {out} ({out.stat().st_size} bytes)")
    arrs = waveform_goldens(root)
    out = HERE / "seamless_streaming_ref.npz"
    np.savez_compressed(out, **arrs)
    print(f"wrote {out} ({out.stat().st_size} bytes)")
    assert out.stat().st_size < 200_000


if __name__ == "__main__":
    main()
