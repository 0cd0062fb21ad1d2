"""Mints tests/golden/pretssel_wave_ref.npz and pretssel_wave_ref.json.

The real PretsselVocoder is built as make_pretssel_goldens.build builds it (arch ``24khz``; for ``small`` with this project's
``small`` waveform geometry in place of the builder's), loaded with the seeded synthetic weights of BOTH halves
(``make_pretssel_state_dict`` + ``make_pretssel_wave_state_dict``; the only keys the module may miss are the BatchNorm counters,
and none may be unexpected), and the WAVEFORM HALF of its forward is EXECUTED in fp32: the statements of
``PretsselVocoder.forward`` from ``wavs = []`` on are cut out of the reference file and run, unchanged, on recorded mel inputs,
one item per call as the reference's loop does.

  small  items of 1, 7, 33 and 40 frames: the waveform and the outputs of conv_post (the HiFi-GAN), both LSTMs and the decoder's
         last residual block;
  24khz  items of 40, 7 and 1 frames: the waveform.

Also recorded: the mel inputs, the sorted key list with shapes of the waveform half, the largest gap of the fp32 oracle
(tests/pretssel_wave_oracle.py, exact weights) to every recorded stage (``oracle_fp32_gap``: the CPU test's bar is 8 x that), the
float64 oracle's gap with the weights the library holds (folded, fp16), and the liveness figures, ASSERTED here for every item:
max |wav| >= 0.3, max |0.8 h| >= 0.1, LSTM gate pre-activations within +-12.

    python tests/golden/make_pretssel_wave_goldens.py <reference tree>/src/seamless_communication
"""
from __future__ import annotations

import ast
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch
import yaml

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent.parent))
import _pretssel_stub  # noqa: E402
from make_pretssel_goldens import build  # noqa: E402
from seamless_communication_amd.config import pretssel_config  # noqa: E402
from seamless_communication_amd.synthetic import make_pretssel_state_dict, make_pretssel_wave_state_dict  # noqa: E402
from tests.pretssel_wave_oracle import wave_oracle  # noqa: E402

SEED = {"small": 3, "24khz": 3}
MEL_SEED = {"small": 21, "24khz": 22}
FRAMES = {"small": [1, 7, 33, 40], "24khz": [40, 7, 1]}
STAGES = ("hifi", "lstm_enc", "lstm_dec", "dec", "wav")


def waveform_half(ref_root):
    """The statements of PretsselVocoder.forward from ``wavs = []`` on, compiled from the reference file into
    f(self, x, durations, normalize_before) -> wavs."""
    src = (ref_root / "models/generator/vocoder.py").read_text()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "PretsselVocoder")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "forward")
    start = next((i for i, st in enumerate(fn.body) if isinstance(st, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "wavs" for t in st.targets)), None)
    if start is None:
        raise SystemExit("forward() no longer assigns `wavs`: the waveform half cannot be cut out")
    fn.body = fn.body[start:]
    fn.name = "waveform_half"
    fn.decorator_list, fn.returns = [], None
    fn.args = ast.arguments(posonlyargs=[], args=[ast.arg(arg=a) for a in ("self", "x", "durations", "normalize_before")], kwonlyargs=[], kw_defaults=[],
                            defaults=[])
    mod = ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[]))
    import torch.nn.functional as F

    from seamless_communication.models.generator import vocoder as ref

    ns = {"torch": torch, "F": F, "LRELU_SLOPE": ref.LRELU_SLOPE}
    exec(compile(mod, "reference forward(), waveform half", "exec"), ns)
    return ns["waveform_half"]


def mels_of(arch):
    g = torch.Generator().manual_seed(MEL_SEED[arch])
    return [torch.randn(f, 80, generator=g) * 2 - 4 for f in FRAMES[arch]]


def main() -> None:
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    root = Path(sys.argv[1])
    _pretssel_stub.install(root)
    from seamless_communication.models.generator import vocoder as ref

    half = waveform_half(root)
    card = yaml.safe_load((root / "cards/vocoder_pretssel.yaml").read_text())
    langs, stats = card["model_config"]["langs"], card["model_config"]["gcmvn_stats"]
    arrs = {}
    meta = {"seed": SEED, "mel_seed": MEL_SEED, "frames": FRAMES, "keys": {}, "missing_keys": {}, "oracle_fp32_gap": {}, "library_weights_gap": {}, "liveness": {},
            "lengths": {}}
    for arch in FRAMES:
        cfg = pretssel_config(arch)
        w = cfg.waveform
        over = dict(upsample_rates=list(w.upsample_rates), upsample_kernel_sizes=list(w.upsample_kernel_sizes), upsample_initial_channel=w.upsample_initial_channel,
                    resblock_kernel_sizes=list(w.resblock_kernel_sizes), resblock_dilation_sizes=[list(d) for d in w.resblock_dilation_sizes], dimension=w.dimension,
                    n_filters=w.n_filters, ratios=list(w.ratios), kernel_size=w.kernel_size, last_kernel_size=w.kernel_size,
                    residual_kernel_size=w.residual_kernel_size)
        shim = types.SimpleNamespace(PretsselEncoderFrontend=ref.PretsselEncoderFrontend, PretsselDecoderFrontend=ref.PretsselDecoderFrontend,
                                     PretsselVocoder=lambda **kw: ref.PretsselVocoder(**{**kw, **over}))
        m = build(shim, cfg, langs[:cfg.num_langs], stats)
        wsd = make_pretssel_wave_state_dict(cfg, SEED[arch])
        res = m.load_state_dict({**make_pretssel_state_dict(cfg, SEED[arch]), **wsd}, strict=False)
        assert not res.unexpected_keys, res.unexpected_keys
        assert all(k.endswith("num_batches_tracked") for k in res.missing_keys), res.missing_keys  # strict apart from the counters
        meta["missing_keys"][arch] = sorted(res.missing_keys)
        wave = tuple(f"layers.{i}." for i in range(cfg.post_layers, 400)) + ("mean", "scale")
        meta["keys"][arch] = {k: list(v.shape) for k, v in sorted(m.state_dict().items()) if k.startswith(wave)}
        ix = w.layer_index(cfg.post_layers)
        st = ix["stream"]
        got = {}
        hooks = [m.layers[ix["conv_post"]].register_forward_hook(lambda mod, a, out: got.__setitem__("hifi", out.reshape(-1).clone())),
                 m.layers[st[13]].register_forward_hook(lambda mod, a, out: got.__setitem__("lstm_enc", out[0].t().clone())),
                 m.layers[st[17]].register_forward_hook(lambda mod, a, out: got.__setitem__("lstm_dec", out[0].t().clone())),
                 m.layers[st[29]].register_forward_hook(lambda mod, a, out: got.__setitem__("dec", out[0].t().clone())),
                 m.layers[st[31]].register_forward_hook(lambda mod, a, out: got.__setitem__("h", out.reshape(-1).clone()))]
        gaps, lib_gaps, live, lens = {k: 0.0 for k in STAGES}, {k: 0.0 for k in STAGES}, [], []
        for i, mel in enumerate(mels_of(arch)):
            T = mel.shape[0]
            with torch.inference_mode():
                wavs = half(m, mel.unsqueeze(0).clone(), torch.tensor([[T]]), True)
            assert len(wavs) == 1 and wavs[0].numel() == T * w.hop, (arch, T, wavs[0].shape)
            got["wav"] = wavs[0].reshape(-1).clone()
            n, steps, dec = w.lengths(T)
            assert got["lstm_enc"].shape[0] == steps and got["dec"].shape[0] == dec and got["hifi"].numel() == n, (arch, T, got["lstm_enc"].shape, got["dec"].shape)
            lens.append([n, steps, dec])
            arrs[f"{arch}.mel{i}"] = mel.numpy()
            for k in STAGES if arch == "small" else ("wav",):
                arrs[f"{arch}.{k}{i}"] = got[k].numpy()
            o32 = wave_oracle(cfg, wsd, mel, torch.float32, fp16_weights=False)
            o64 = wave_oracle(cfg, wsd, mel, torch.float64, fp16_weights=True)
            for k in STAGES:
                gaps[k] = max(gaps[k], float((o32[k] - got[k]).abs().max()))
                lib_gaps[k] = max(lib_gaps[k], float((o64[k] - got[k].double()).abs().max()))
            fig = {"frames": T, "max_wav": float(got["wav"].abs().max()), "max_08h": float(0.8 * got["h"][:n].abs().max()), "gate_peak": float(o64["gate_peak"])}
            print(arch, fig)
            assert fig["max_wav"] >= 0.3 and fig["max_08h"] >= 0.1 and fig["gate_peak"] <= 12.0, fig
            live.append(fig)
        for h in hooks:
            h.remove()
        print(arch, "fp32 oracle vs executed reference", gaps)
        print(arch, "float64 oracle with the library's weights vs executed reference", lib_gaps)
        meta["oracle_fp32_gap"][arch], meta["library_weights_gap"][arch], meta["liveness"][arch], meta["lengths"][arch] = gaps, lib_gaps, live, lens
    np.savez_compressed(HERE / "pretssel_wave_ref.npz", **arrs)
    size = (HERE / "pretssel_wave_ref.npz").stat().st_size
    print("pretssel_wave_ref.npz", size, "bytes")
    assert size < (1 << 20)
    meta["arrays"] = {k: list(v.shape) for k, v in sorted(arrs.items())}
    (HERE / "pretssel_wave_ref.json").write_text(json.dumps(meta, indent=1) + "\n")


if __name__ == "__main__":
    main()
