"""GPU: the expressive streaming chain's device side (HipStreamingBackend.speak_expressive and the prosody history behind it) at
arch ``small``, and the chain itself on the tiny synthetic streaming model.

  * the frame history, built feed by feed, against ONE fbank of everything heard: equal bits;
  * three successive chunks against the executed reference PretsselVocoder (tests/golden/seamless_streaming_ref.npz, minted by
    tests/golden/make_seamless_streaming_goldens.py): waveforms within 2e-3 absolute, the standing waveform bar (WAV_BAR of
    test_pretssel_wave_model_gpu.py); the mel within ``BAR * e32 + gap`` as in test_pretssel_gpu.py;
  * the same script twice, and a chunk against the same tokens and durations sent straight through HipPretssel.mel and
    HipPretsselWave.wave: equal bits;
  * SeamlessS2STAgent over 2 s of audio; the unsupported-language and over-limit paths;
  * arch ``16khz``: 7 frames against the float64 restatement (its last upsampling stage is k = 4, stride 2).

Measured errors go to seamless_streaming_report.txt."""
import json
import logging
from pathlib import Path

import numpy as np
import pytest
import torch

from seamless_communication_amd import synthetic as syn
from seamless_communication_amd.config import pretssel_config
from tests import common
from tests import pretssel_oracle as oracle
from tests.pretssel_wave_oracle import wave_oracle

pytestmark = pytest.mark.gpu
WAV_BAR = 2e-3
BAR = 16.0
GOLD = Path(__file__).resolve().parent / "golden" / "seamless_streaming_ref.npz"


def _log(report_dir, name, **kw):
    line = name + " " + " ".join(f"{k}={v}" for k, v in kw.items())
    print(line)
    with open(report_dir / "seamless_streaming_report.txt", "a") as f:
        f.write(line + "\n")


def _err(a, b):
    return float((a.double().cpu() - b.double()).abs().max())


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from seamless_communication_amd.inference import PretsselGenerator
    from seamless_communication_amd.streaming import HipStreamingBackend

    z = np.load(GOLD)
    meta = json.loads(str(z["meta"]))
    cfg, _, _, tt, _ = common.tiny_bundle()
    hip = common.make_hip_streaming()
    card = {"name": "small", "model_arch": meta["arch"], "checkpoint": f"synthetic-full://{meta['seed']}", "sample_rate": meta["sample_rate"],
            "model_config": {"langs": meta["langs"], "gcmvn_stats": meta["gcmvn_stats"]}}
    gen = PretsselGenerator(card)
    return dict(z=z, meta=meta, cfg=cfg, tt=tt, hip=hip, gen=gen, backend=HipStreamingBackend(hip, cfg, pretssel_generator=gen))


def _whole_fbank(hip, heard):
    wav = torch.from_numpy(np.ascontiguousarray(heard, dtype=np.float32)).cuda().unsqueeze(0)
    fb, frames = hip.fbank(wav, [wav.shape[1]], standardize=False, pad_to_multiple=1)
    return fb[0, : int(frames[0])]


def test_history_equals_one_fbank_of_everything_heard(env):
    """Feeds that end below one window, exactly on it, one sample past it, and across many frames: after each the history holds
    the bits of a single fbank over the concatenation."""
    be, hip = env["backend"], env["hip"]
    src = syn.synthetic_waveform(3, 0.8).numpy().astype(np.float32)
    be.reset_expressive()
    hist, n = be.prosody_history, 0
    for feed, frames in zip((1, 399, 400, 401, 5000, 5120), (0, 1, 3, 6, 37, 69)):
        n += feed
        got = hist.extend_to(src[:n])
        assert hist.count == frames == got.shape[0], (n, hist.count)
        if frames:
            assert torch.equal(got, _whole_fbank(hip, src[:n])), n
    again = hist.extend_to(src[:n])  # nothing new: nothing computed, the same rows
    assert again.data_ptr() == got.data_ptr() and torch.equal(again, _whole_fbank(hip, src[:n]))
    with pytest.raises(ValueError, match="reset_expressive"):
        hist.extend_to(src[: n - 200])  # the source shrank without a reset
    be.reset_expressive()
    assert hist.count == 0 and hist.frames.shape[0] == 0


def _script(env, capture=None):
    """The recorded script: three chunks against a growing heard source.  -> the waveforms (and the mels through `capture`)."""
    z, meta, be, gen = env["z"], env["meta"], env["backend"], env["gen"]
    lang = meta["langs"][meta["tgt_lang"]]
    inner = gen.wave_model.wave
    if capture is not None:
        gen.wave_model.wave = lambda mel, flens, **kw: (capture.append(mel.clone()), inner(mel, flens, **kw))[1]
    try:
        be.reset_expressive()
        return [be.speak_expressive(z["heard"][: c["heard_samples"]], z[f"units{i}"].tolist(), lang).cpu() for i, c in enumerate(meta["chunks"])]
    finally:
        gen.wave_model.wave = inner


def test_chunks_match_the_executed_reference(env, report_dir):
    z, meta, be, gen, hip = env["z"], env["meta"], env["backend"], env["gen"], env["hip"]
    cfg = pretssel_config(meta["arch"])
    assert [c["units"] for c in meta["chunks"]] == [1, 6, 17] and [c["heard_samples"] for c in meta["chunks"]] == [5120, 10240, 15360]
    sd = syn.make_pretssel_state_dict(cfg, meta["seed"])
    st = meta["gcmvn_stats"]
    mean, std = torch.tensor(st["mean"], dtype=torch.float64), torch.tensor(st["std"], dtype=torch.float64)
    mels = []
    wavs = _script(env, mels)
    assert be.prosody_history.count == meta["chunks"][-1]["prosody_frames"]
    assert torch.equal(be.prosody_history.frames, _whole_fbank(hip, z["heard"]))
    figures = []
    for i, c in enumerate(meta["chunks"]):
        tk, du = z[f"tokens{i}"][None], z[f"durations{i}"][None]
        tl, pros = np.array([tk.shape[1]]), torch.from_numpy(z[f"pros{i}"])[None]
        r64, fl = oracle.pretssel_mel(sd, cfg, tk, tl, du, meta["tgt_lang"], pros, mean, std, torch.float64)
        r32, _ = oracle.pretssel_mel(sd, cfg, tk, tl, du, meta["tgt_lang"], pros, mean, std, torch.float32)
        L = c["frames"]
        assert int(fl[0]) == L and tuple(mels[i].shape) == (1, L, 80) and wavs[i].numel() == L * cfg.waveform.hop
        e32, gap = _err(r32[0, :L], r64[0, :L]), c["oracle_fp32_gap_mel"]
        e_mel = _err(mels[i][0], torch.from_numpy(z[f"mel{i}"]))
        e_wav = _err(wavs[i], torch.from_numpy(z[f"wav{i}"]))
        _log(report_dir, f"seamless streaming chunk {i} units={c['units']} heard={c['heard_samples']}", mel=f"{e_mel:.3e}", mel_bar=f"{BAR * e32 + gap:.3e}",
             wav=f"{e_wav:.3e}", wav_bar=WAV_BAR, peak=f"{c['peak']:.3f}")
        figures.append((i, e_mel, BAR * e32 + gap, e_wav))
    for i, e_mel, mel_bar, e_wav in figures:
        assert torch.isfinite(wavs[i]).all()
        assert e_mel <= mel_bar, (i, e_mel, mel_bar)
        assert e_wav <= WAV_BAR, (i, e_wav)


def test_same_script_same_bits_and_the_stage_adds_nothing(env):
    z, meta, gen, hip = env["z"], env["meta"], env["gen"], env["hip"]
    first, second = _script(env), _script(env)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    # the last chunk by hand: prosody from ONE fbank of the whole source, the recorded tokens and durations
    i = len(meta["chunks"]) - 1
    pros = gen.prosody_encoder.model.encode(_whole_fbank(hip, z["heard"]).unsqueeze(0), None, gen.gcmvn_mean, gen.gcmvn_std)
    tk, du = z[f"tokens{i}"][None], z[f"durations{i}"][None]
    mel, flens = gen.model.mel(tk, [tk.shape[1]], du, meta["tgt_lang"], pros)
    assert torch.equal(gen.wave_model.wave(mel, flens)[0].cpu(), first[i])


def _chain_args(lang):
    from seamless_communication_amd.streaming import default_args

    # a threshold of 0 never listens for the policy's sake: what is written depends on the arg-max ids alone
    return default_args(tgt_lang=lang, decision_threshold=0.0, min_unit_chunk_size=20, min_starting_wait_w2vbert=48, max_len_a=0, max_len_b=30)


def test_full_chain_on_the_synthetic_streaming_model(env, report_dir, caplog):
    from seamless_communication_amd.streaming import HipStreamingBackend, SeamlessS2STAgent

    be, tt, gen, meta = env["backend"], env["tt"], env["gen"], env["meta"]
    lang, other = meta["langs"][meta["tgt_lang"]], "fra"
    assert other not in gen.langs
    hop = gen.cfg.waveform.hop
    wav = common.waves((2.0,))[0]
    calls = []
    inner = be.speak_expressive
    be.speak_expressive = lambda heard, units, l: (calls.append((len(heard), len(units), be.prosody_history.count)), inner(heard, units, l))[1]
    try:
        outs = common.run_stream(SeamlessS2STAgent(be, tt, _chain_args(lang)), wav, tgt_lang=lang)
        spoken = [o for o in outs if len(o.content)]
        assert len(spoken) == len(calls) >= 2 and outs[-1].finished and not any(o.finished for o in outs[:-1])
        for o, (heard, units, _) in zip(spoken, calls):
            assert o.sample_rate == meta["sample_rate"] and o.tgt_lang == lang and o.data_type == "speech"
            assert len(o.content) == 2 * units * hop and np.isfinite(np.asarray(o.content)).all()
        # an early stop starts the chain over: the heard source of a later call is shorter, and so was the history it found
        assert any(b[0] < a[0] and b[2] == 0 for a, b in zip(calls, calls[1:])), calls
        _log(report_dir, "seamless streaming chain 2 s", calls=calls)
        # a language the vocoder does not list: a warning, written segments without content, no device call
        del calls[:]
        with caplog.at_level(logging.WARNING):
            outs = common.run_stream(SeamlessS2STAgent(be, tt, _chain_args(other)), wav, tgt_lang=other)
        assert f"{other} not supported" in caplog.text and not calls
        assert len(outs) >= 1 and all(o.content == [] and o.sample_rate == meta["sample_rate"] and o.tgt_lang == other for o in outs) and outs[-1].finished
    finally:
        be.speak_expressive = inner
    # past the prosody encoder's limit: refused by name before anything runs, the history untouched
    from seamless_communication_amd.streaming.backend import PE_MAX_FRAMES

    be.reset_expressive()
    be.speak_expressive(wav[:5120], [3, 3, 4], lang)
    count = be.prosody_history.count
    with pytest.raises(ValueError, match=f"PE_MAX_FRAMES = {PE_MAX_FRAMES}"):
        be.speak_expressive(np.zeros(400 + 160 * PE_MAX_FRAMES, dtype=np.float32), [3], lang)
    assert PE_MAX_FRAMES == 4096 and be.prosody_history.count == count
    with pytest.raises(ValueError, match="not one of"):
        be.speak_expressive(wav[:5120], [3], other)
    # a backend without the vocoder refuses the chain by name
    with pytest.raises(ValueError, match="without a PretsselGenerator"):
        SeamlessS2STAgent(HipStreamingBackend(env["hip"], env["cfg"]), tt, _chain_args(lang))


def test_16khz_waveform_at_7_frames_against_float64(report_dir):
    """The dual chain speaks at 16 kHz next to the plain vocoder.  Tokens and durations of 7 frames through HipPretssel.mel, the
    waveform of that mel against the float64 restatement with the library's weights."""
    from seamless_communication_amd.inference import PretsselGenerator

    cfg = pretssel_config("16khz")
    assert cfg.waveform.upsample_rates[-1] == 2 and cfg.waveform.upsample_kernel_sizes[-1] == 4
    mean, std = (torch.arange(80) * 0.01 - 4).tolist(), (torch.arange(80) * 0.005 + 2).tolist()
    langs = [f"l{i}" for i in range(cfg.num_langs)]
    gen = PretsselGenerator({"name": "t", "model_arch": "16khz", "checkpoint": "synthetic-full://3", "sample_rate": 16000,
                             "model_config": {"langs": langs, "gcmvn_stats": {"mean": mean, "std": std}}})
    try:
        assert gen.output_sample_rate == 16000
        fb = torch.randn(1, 50, 80, generator=torch.Generator().manual_seed(1)).cuda()
        pros = gen.prosody_encoder.model.encode(fb, None, None, None)
        mel, flens = gen.model.mel(np.array([[9, 5, 7]]), [3], np.array([[2, 4, 1]]), 2, pros)
        assert flens.tolist() == [7]
        wav = gen.wave_model.wave(mel, flens)[0].cpu()
        o = wave_oracle(cfg, syn.make_pretssel_wave_state_dict(cfg, 3), mel[0, :7].cpu(), torch.float64)
        e = _err(wav, o["wav"])
        _log(report_dir, "seamless streaming 16khz T=7", wav=f"{e:.3e}", wav_bar=WAV_BAR, peak=f"{float(o['wav'].abs().max()):.3f}")
        assert wav.numel() == 7 * cfg.waveform.hop == 7 * 160 and torch.isfinite(wav).all()
        assert e <= WAV_BAR, e
    finally:
        gen.wave_model.close()
        gen.model.close()
        gen.prosody_encoder.model.close()
