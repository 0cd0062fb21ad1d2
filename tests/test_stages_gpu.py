"""Stage-level parity of the HIP path (through the C ABI) against the CPU oracle
on a tiny seeded model: fbank, speech encoder, greedy text generation, teacher
forced decoding, NAR T2U, vocoder, and the whole S2ST chain.

Bars: token / unit / duration ids bit-exact; floating-point tensors within the
tolerance written in each test.
"""
import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu


def _log(report_dir, name, **kw):
    with open(report_dir / "stages_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    return cfg, tt, ct, common.make_oracle(), common.make_hip()


def test_fbank_matches_oracle(env, report_dir):
    cfg, tt, ct, orc, hip = env
    ws = common.waves((2.0, 1.37, 0.5))
    fb_ref, lens_ref = orc.collate_fbank(ws)
    wav, ns = common.pad_waves(ws)
    fb, frames = hip.fbank(torch.from_numpy(wav).cuda(), ns)
    assert frames.tolist() == lens_ref.tolist()
    assert tuple(fb.shape) == tuple(fb_ref.shape)
    err = float((fb.cpu() - fb_ref).abs().max())
    _log(report_dir, "fbank", err=err)
    assert err < 2e-3  # log-mel, standardised (fp32 FFT vs float64 FFT)


def test_fbank_raw_unstandardized(env, report_dir):
    from oracle import fbank as ofb

    cfg, tt, ct, orc, hip = env
    ws = common.waves((1.0,))
    wav, ns = common.pad_waves(ws)
    fb, frames = hip.fbank(torch.from_numpy(wav).cuda(), ns, standardize=False, pad_to_multiple=1)
    ref = ofb.fbank_raw(ws[0])
    err = float(np.abs(fb.cpu().numpy()[0, : ref.shape[0]] - ref).max())
    _log(report_dir, "fbank_raw", err=err)
    assert err < 2e-3


def test_encoder_matches_oracle(env, report_dir):
    from oracle import unity as ou

    cfg, tt, ct, orc, hip = env
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37)))
    ref, ref_lens = ou.encode_speech(orc.P, cfg, fb, lens)
    out, out_lens = hip.encode_speech(fb.cuda().contiguous(), lens.tolist())
    assert out_lens.tolist() == ref_lens.tolist()
    errs = []
    for b in range(fb.shape[0]):
        n = int(ref_lens[b])
        errs.append(float((out[b, :n].cpu() - ref[b, :n]).abs().max()))
    _log(report_dir, "encoder", errs=errs, ref_absmax=float(ref.abs().max()))
    assert max(errs) < 2e-4


def test_greedy_text_ids_bit_exact(env, report_dir):
    cfg, tt, ct, orc, hip = env
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37)))
    seqs, enc, enc_lens, margins = orc.s2tt(fb, lens, "fra", (1, 200), 20)
    prefix = tt.target_prefix("fra")
    for use_graph in (False, True):
        ids, out_lens, scores, hidden = hip.generate_text(
            enc.cuda().contiguous(), enc_lens.tolist(), prefix, soft_max_seq_len=(1, 200), hard_max_seq_len=20,
            use_graph=use_graph,
        )
        got = [ids[b, : out_lens[b]].tolist() for b in range(len(seqs))]
        _log(report_dir, "greedy", use_graph=use_graph, got=got, ref=seqs, min_margin=min(min(m) for m in margins))
        assert got == seqs


# The encoder's length limit (4096 fbank frames): 40 s is 3998 frames, 1999 attention positions (63 key tiles, 16 query
# workgroups per head), next to a 3.1 s item.  start = 1 picks waveforms whose greedy decode keeps every top-2 logit
# margin of the oracle above 1e-3, so that exact ids are a fair bar.
LONG = (40.0, 3.1)
LONG_START = 1


def test_encoder_matches_oracle_at_40s(env, report_dir):
    """fbank, then the encoder at T = 1999: Shaw attention, the fused GLU / depthwise conv / LayerNorm kernels."""
    from oracle import unity as ou

    cfg, tt, ct, orc, hip = env
    ws = common.waves(LONG, start=LONG_START)
    fb, lens = orc.collate_fbank(ws)
    wav, ns = common.pad_waves(ws)
    fb_hip, frames = hip.fbank(torch.from_numpy(wav).cuda(), ns)
    assert frames.tolist() == lens.tolist() and max(frames.tolist()) > 3990
    assert tuple(fb_hip.shape) == tuple(fb.shape)
    fb_err = float((fb_hip.cpu() - fb).abs().max())
    ref, ref_lens = ou.encode_speech(orc.P, cfg, fb, lens)
    out, out_lens = hip.encode_speech(fb.cuda().contiguous(), lens.tolist())
    assert out_lens.tolist() == ref_lens.tolist()
    errs = []
    for b in range(fb.shape[0]):
        n = int(ref_lens[b])
        errs.append(float((out[b, :n].cpu() - ref[b, :n]).abs().max()))
    _log(report_dir, "encoder_40s", frames=frames.tolist(), fbank_err=fb_err, errs=errs, ref_absmax=float(ref.abs().max()))
    assert fb_err < 2e-3  # as test_fbank_matches_oracle
    assert max(errs) < 2e-4


def test_greedy_text_ids_bit_exact_at_40s(env, report_dir):
    cfg, tt, ct, orc, hip = env
    fb, lens = orc.collate_fbank(common.waves(LONG, start=LONG_START))
    seqs, enc, enc_lens, margins = orc.s2tt(fb, lens, "fra", (1, 200), 20)
    min_margin = min(min(m) for m in margins)
    assert min_margin > 1e-3, min_margin
    prefix = tt.target_prefix("fra")
    for use_graph in (False, True):
        ids, out_lens, scores, hidden = hip.generate_text(
            enc.cuda().contiguous(), enc_lens.tolist(), prefix, soft_max_seq_len=(1, 200), hard_max_seq_len=20,
            use_graph=use_graph,
        )
        got = [ids[b, : out_lens[b]].tolist() for b in range(len(seqs))]
        _log(report_dir, "greedy_40s", use_graph=use_graph, got=got, ref=seqs, min_margin=min_margin)
        assert got == seqs


def test_generated_hidden_equals_teacher_forced_pass(env, report_dir):
    from oracle import unity as ou

    cfg, tt, ct, orc, hip = env
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37)))
    seqs, enc, enc_lens, _ = orc.s2tt(fb, lens, "fra", (1, 200), 16)
    ids, out_lens, _, hidden = hip.generate_text(enc.cuda().contiguous(), enc_lens.tolist(), tt.target_prefix("fra"),
                                                 hard_max_seq_len=16)
    L = max(len(s) for s in seqs)
    text = torch.full((len(seqs), L), cfg.pad_idx, dtype=torch.int64)
    for i, s in enumerate(seqs):
        text[i, : len(s)] = torch.tensor(s)
    text = text[:, :-1]
    tl = torch.tensor([len(s) - 1 for s in seqs])
    ref = ou.decode_text(orc.P, cfg, text, tl, enc, enc_lens, orc.pos_table)
    errs = [float((hidden[b, : tl[b]].cpu() - ref[b, : tl[b]]).abs().max()) for b in range(len(seqs))]
    _log(report_dir, "hidden_capture", errs=errs)
    assert max(errs) < 2e-4


def test_teacher_forced_decode_matches_oracle(env, report_dir):
    from oracle import unity as ou

    cfg, tt, ct, orc, hip = env
    fb, lens = orc.collate_fbank(common.waves((1.0, 0.8)))
    enc, enc_lens = ou.encode_speech(orc.P, cfg, fb, lens)
    tl = [11, 7]
    text = common.random_text_seqs(cfg, tt, 2, tl, seed=3)
    ref = ou.decode_text(orc.P, cfg, torch.from_numpy(text), torch.tensor(tl), enc, enc_lens, orc.pos_table)
    hid = hip.decode_text(enc.cuda().contiguous(), enc_lens.tolist(), text)
    errs = [float((hid[b, : tl[b]].cpu() - ref[b, : tl[b]]).abs().max()) for b in range(2)]
    _log(report_dir, "decode_forced", errs=errs)
    assert max(errs) < 2e-4


def test_t2u_units_and_durations_bit_exact(env, report_dir):
    from oracle import unity as ou

    cfg, tt, ct, orc, hip = env
    fb, lens = orc.collate_fbank(common.waves((1.0, 0.8)))
    enc, enc_lens = ou.encode_speech(orc.P, cfg, fb, lens)
    tl = [12, 8]
    text = common.random_text_seqs(cfg, tt, 2, tl, seed=5)
    dec = ou.decode_text(orc.P, cfg, torch.from_numpy(text), torch.tensor(tl), enc, enc_lens, orc.pos_table)
    ref_units, aux = ou.t2u_nar(orc.P, cfg, dec, torch.tensor(tl), torch.from_numpy(text.copy()), tt, ct, 1.0)
    units, ulens, dur, cids, clens = hip.t2u_nar(dec.cuda().contiguous(), text, tl, 1.0)
    _log(report_dir, "t2u", unit_lens=ulens.tolist(), ref_unit_lens=aux["unit_lens"].tolist(),
         n_mismatch=int((units != ref_units.numpy()).sum()) if units.shape == tuple(ref_units.shape) else -1)
    assert clens.tolist() == aux["char_seq_lens"].tolist()
    assert cids.tolist() == aux["char_seqs"].tolist()
    assert dur.tolist() == aux["durations"].tolist()
    assert ulens.tolist() == aux["unit_lens"].tolist()
    assert units.tolist() == ref_units.tolist()


def test_vocoder_waveform(env, report_dir):
    from oracle import vocoder as ov

    cfg, tt, ct, orc, hip = env
    rng = np.random.RandomState(0)
    units = rng.randint(0, cfg.vocoder.num_embeddings, size=(2, 37)).astype(np.int64)
    lang_idx, spkr_idx = ov.resolve_lang_spkr(orc.lang_spkr_idx_map, ["fra", "fra"], [-1, 3])
    ref = ov.vocode(orc.vocoder_sd, cfg.vocoder, torch.from_numpy(units), lang_idx, spkr_idx)
    wav = hip.vocode(units, lang_idx, spkr_idx)
    assert tuple(wav.shape) == tuple(ref.shape)
    err = float((wav.cpu() - ref).abs().max())
    _log(report_dir, "vocoder", err=err, ref_absmax=float(ref.abs().max()))
    # fp16 rounding of the weight-norm-folded weights: stated tolerance 2e-3 absolute on [-1,1] audio
    assert err < 2e-3


def test_s2st_end_to_end(env, report_dir):
    cfg, tt, ct, orc, hip = env
    ws = common.waves((2.0, 1.37))
    fb_ref, lens_ref = orc.collate_fbank(ws)
    seqs, speech_units, wavs, units_ref, aux = orc.s2st(fb_ref, lens_ref, "fra", (1, 200), 14)
    wav, ns = common.pad_waves(ws)
    fb, frames = hip.fbank(torch.from_numpy(wav).cuda(), ns)
    enc, enc_lens = hip.encode_speech(fb, frames.tolist())
    ids, out_lens, _, hidden = hip.generate_text(enc, enc_lens.tolist(), tt.target_prefix("fra"), hard_max_seq_len=14)
    got = [ids[b, : out_lens[b]].tolist() for b in range(len(seqs))]
    assert got == seqs
    text = ids[:, :-1].copy()
    units, ulens, dur, cids, clens = hip.t2u_nar(hidden, text, (out_lens - 1).tolist(), 1.0)
    _log(report_dir, "e2e", text=got, unit_lens=ulens.tolist(), ref_unit_lens=aux["unit_lens"].tolist())
    assert dur.tolist() == aux["durations"].tolist()
    assert units.tolist() == units_ref.tolist()


def test_forked_handles_concurrent_microbatches_match_single_batch(env, report_dir):
    """sc_fork: two handles on the same weights, driven from two host threads on their own HIP
    streams, must reproduce bit for bit what the parent handle computes for the same two slices one
    after the other.  (Slices, not single utterances, are the unit of comparison: like the reference,
    the adaptor's strided convolution reads the positions behind a shorter item's end
    (adaptor_block.py:255-276 applies no padding mask before the convolutions), so an item's result
    depends on how far its batch is padded.)"""
    from concurrent.futures import ThreadPoolExecutor

    cfg, tt, ct, orc, hip = env
    ws = common.waves((2.0, 1.37, 1.0, 1.8))
    wav, ns = common.pad_waves(ws)
    wav_dev = torch.from_numpy(wav).cuda()

    def run(model, lo, hi):
        fb, frames = model.fbank(wav_dev[lo:hi].contiguous(), ns[lo:hi])
        enc, enc_lens = model.encode_speech(fb, frames.tolist())
        ids, out_lens, _, hidden = model.generate_text(enc, enc_lens.tolist(), tt.target_prefix("fra"), hard_max_seq_len=12)
        units, ulens, dur, _, _ = model.t2u_nar(hidden, ids[:, :-1].copy(), (out_lens - 1).tolist(), 1.0)
        return [ids[b, : out_lens[b]].tolist() for b in range(hi - lo)], [units[b, : ulens[b]].tolist() for b in range(hi - lo)]

    ref_text, ref_units = [], []
    for lo, hi in ((0, 2), (2, 4)):  # the same slices, sequentially, on the parent handle
        t, u = run(hip, lo, hi)
        ref_text += t
        ref_units += u
    child = hip.fork()
    try:
        tc, uc = run(child, 2, 4)  # the fork alone
        assert tc == ref_text[2:] and uc == ref_units[2:]
        for _ in range(3):
            with ThreadPoolExecutor(2) as ex:
                f0 = ex.submit(run, hip, 0, 2)
                f1 = ex.submit(run, child, 2, 4)
                (t0, u0), (t1, u1) = f0.result(), f1.result()
            assert t0 + t1 == ref_text
            assert u0 + u1 == ref_units
    finally:
        child.close()
    _log(report_dir, "fork", text=ref_text)


@pytest.mark.parametrize("beam,hard_max,min_len", [(2, 12, 1), (5, 14, 1), (5, 10, 6), (3, 9, 1)])
def test_beam_search_ids_match_oracle(env, report_dir, beam, hard_max, min_len):
    """beam_size > 1 (the API default is 5): best hypothesis per utterance, ids exact, against
    oracle.beam_search_generate on the SAME encoder output; three utterances of different lengths so that
    the searches finish at different steps."""
    from oracle import unity as ou

    cfg, tt, ct, orc, hip = env
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37, 0.9)))
    enc, enc_lens = hip.encode_speech(fb.cuda(), lens.tolist())
    prefix = tt.target_prefix("fra")
    want, every = ou.beam_search_generate(orc.P, cfg, enc.cpu(), torch.from_numpy(enc_lens.astype(np.int64)), prefix, beam,
                                          hard_max_seq_len=hard_max, min_seq_len=min_len, pos_table=orc.pos_table,
                                          return_all=True)
    ids, out_lens, scores, hidden = hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=beam, hard_max_seq_len=hard_max,
                                                      min_seq_len=min_len)
    got = [ids[b, : out_lens[b]].tolist() for b in range(len(want))]
    _log(report_dir, "beam", beam=beam, got=got, want=want, scores=scores.tolist(),
         ref_scores=[[round(f[0], 5) for f in e] for e in every])
    assert got == want
    for b in range(len(want)):
        assert abs(float(scores[b]) - every[b][0][0]) < 2e-4
    # decoder outputs of the chosen hypotheses = the teacher-forced pass over them (generator.py:281-299)
    L = max(len(s) for s in want) - 1
    toks = np.full((len(want), L), cfg.pad_idx, dtype=np.int32)
    for b, s in enumerate(want):
        toks[b, : len(s) - 1] = s[:-1]
    forced = hip.decode_text(enc, enc_lens.tolist(), toks)
    for b, s in enumerate(want):
        err = float((hidden[b, : len(s) - 1] - forced[b, : len(s) - 1]).abs().max())
        assert err < 1e-5, err


@pytest.mark.parametrize("beam,opts", [(5, dict(unk_penalty=0.75)), (5, dict(unk_penalty=-5.0)), (5, dict(len_penalty=0.6)),
                                        (5, dict(len_penalty=1.3)), (5, dict(normalize_scores=False)), (8, {})])
def test_beam_search_options_match_oracle(env, report_dir, beam, opts):
    """The search options the other GPU tests leave at their defaults (the device kernels hold their own copy of each rule:
    UNK penalty in the candidate search, length penalty and normalisation in the candidate walk) and the largest beam: ids
    exact, best score within 2e-4, against oracle.beam_search_generate on the SAME encoder output."""
    from oracle import unity as ou

    cfg, tt, ct, orc, hip = env
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37, 0.9)))
    enc, enc_lens = hip.encode_speech(fb.cuda(), lens.tolist())
    prefix = tt.target_prefix("fra")
    want, every = ou.beam_search_generate(orc.P, cfg, enc.cpu(), torch.from_numpy(enc_lens.astype(np.int64)), prefix, beam,
                                          hard_max_seq_len=12, pos_table=orc.pos_table, return_all=True, **opts)
    ids, out_lens, scores, _ = hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=beam, hard_max_seq_len=12, want_hidden=False,
                                                 **opts)
    got = [ids[b, : out_lens[b]].tolist() for b in range(len(want))]
    _log(report_dir, "beam_opts", beam=beam, opts=opts, got=got, scores=scores.tolist(), ref_scores=[round(e[0][0], 5) for e in every])
    assert got == want
    for b in range(len(want)):
        assert abs(float(scores[b]) - every[b][0][0]) < 2e-4
    if opts.get("unk_penalty", 0) < 0:  # the rule is really exercised: UNK made it into a finished hypothesis
        assert any(cfg.unk_idx in seq[len(prefix):] for e in every for _, seq in e)


def test_beam_size_above_eight_fails_cleanly(env):
    """beam_size 9: the library refuses it (SC_CHECK, an error status, no crash; the handle stays usable) and so does
    Translator.predict (its own range check)."""
    from seamless_communication_amd._lib import SeamlessHipError
    from seamless_communication_amd.inference import SequenceGeneratorOptions, Translator
    from seamless_communication_amd.inference.translator import DEFAULT_CARDS

    cfg, tt, ct, orc, hip = env
    fb, lens = orc.collate_fbank(common.waves((1.2,)))
    enc, enc_lens = hip.encode_speech(fb.cuda(), lens.tolist())
    prefix = tt.target_prefix("fra")
    with pytest.raises(SeamlessHipError, match="beam_size 9 > 8"):
        hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=9, hard_max_seq_len=8, want_hidden=False)
    ids, out_lens, _, _ = hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=8, hard_max_seq_len=8, want_hidden=False)
    assert 1 <= int(out_lens[0]) <= 8
    card = dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="tiny_v2")
    tr = Translator(card, dict(DEFAULT_CARDS["vocoder_v2"]), device=torch.device("cuda", 0))
    src = {"seqs": fb.cuda(), "seq_lens": lens, "is_ragged": False}
    with pytest.raises(ValueError, match="beam_size"):
        tr.predict(src, "S2TT", "fra", text_generation_opts=SequenceGeneratorOptions(beam_size=9, hard_max_seq_len=8))


@pytest.mark.parametrize("n_utt,beam", [(16, 5), (27, 4)])
def test_beam_search_wide_step_matches_oracle(env, report_dir, n_utt, beam):
    """More than 64 live rows (the API default beam 5 at the benchmark batch is 64 x 5 = 320): the decoder step cuts every
    product into row groups, the beams of an utterance share its encoder K / V, the logits come from the LDS-staged
    projection kernel in row groups.  Ids of every utterance against oracle.beam_search_generate."""
    from oracle import unity as ou

    cfg, tt, ct, orc, hip = env
    secs = [0.9 + 0.11 * (i % 9) for i in range(n_utt)]
    fb, lens = orc.collate_fbank(common.waves(secs))
    enc, enc_lens = hip.encode_speech(fb.cuda(), lens.tolist())
    prefix = tt.target_prefix("fra")
    want = ou.beam_search_generate(orc.P, cfg, enc.cpu(), torch.from_numpy(enc_lens.astype(np.int64)), prefix, beam, hard_max_seq_len=11,
                                   pos_table=orc.pos_table)
    ids, out_lens, scores, hidden = hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=beam, hard_max_seq_len=11)
    got = [ids[b, : out_lens[b]].tolist() for b in range(n_utt)]
    bad = [b for b in range(n_utt) if got[b] != want[b]]
    _log(report_dir, "beam_wide", n_utt=n_utt, beam=beam, rows=n_utt * beam, mismatching=bad)
    assert not bad, (bad, [got[b] for b in bad], [want[b] for b in bad])


def test_beam_search_graph_replay_equals_eager_launching(env):
    """use_graph=True (the step of run_generate_beam replayed from its captured graph) and use_graph=False (the same launches
    made one by one) return the same ids, lengths, scores and decoder outputs, bit for bit, at the smallest utterance count
    whose 5-beam step runs on the wide row-group chain (family 4: 13 utterances = 65 live rows on the tiny model)."""
    cfg, tt, ct, orc, hip = env
    n_utt = next(n for n in range(1, 104) if int(hip.lib.sc_decoder_step_family(hip.handle, n * 5, 1)) == 4)
    print(f"family 4 from {n_utt} utterances x 5 beams")
    fb, lens = orc.collate_fbank(common.waves([0.9 + 0.11 * (i % 9) for i in range(n_utt)]))
    enc, enc_lens = hip.encode_speech(fb.cuda(), lens.tolist())
    prefix = tt.target_prefix("fra")
    eager, graph = (hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=5, hard_max_seq_len=11, use_graph=g) for g in (False, True))
    for a, b in zip(eager[:3], graph[:3]):
        assert np.array_equal(a, b)
    assert torch.equal(eager[3], graph[3])


def test_beam_size_one_equals_greedy(env):
    from oracle import unity as ou

    cfg, tt, ct, orc, hip = env
    fb, lens = orc.collate_fbank(common.waves((1.2,)))
    enc, enc_lens = hip.encode_speech(fb.cuda(), lens.tolist())
    prefix = tt.target_prefix("fra")
    a = ou.beam_search_generate(orc.P, cfg, enc.cpu(), torch.from_numpy(enc_lens.astype(np.int64)), prefix, 1, hard_max_seq_len=11,
                                pos_table=orc.pos_table)
    b = ou.greedy_generate(orc.P, cfg, enc.cpu(), torch.from_numpy(enc_lens.astype(np.int64)), prefix, hard_max_seq_len=11,
                           pos_table=orc.pos_table)
    ids, out_lens, _, _ = hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=1, hard_max_seq_len=11)
    assert a == b == [ids[0, : out_lens[0]].tolist()]


@pytest.mark.parametrize("beam,ngram,hard_max", [(1, 2, 14), (1, 1, 9), (4, 2, 14), (5, 3, 16), (3, 1, 10)])
def test_ngram_block_step_processor_matches_oracle(env, report_dir, beam, ngram, hard_max):
    """SequenceGeneratorOptions.step_processor = NGramRepeatBlockProcessor(G) (cli/m4t/predict/predict.py:172-175):
    ids exact against the oracle's beam search with the same processor, for greedy (beam 1, which leaves the
    graph-captured step for the host-driven loop) and beam search; the unconstrained tiny model repeats itself,
    so the processor changes the result."""
    from oracle import unity as ou

    cfg, tt, ct, orc, hip = env
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37, 0.9)))
    enc, enc_lens = hip.encode_speech(fb.cuda(), lens.tolist())
    prefix = tt.target_prefix("fra")
    el = torch.from_numpy(enc_lens.astype(np.int64))
    want, every = ou.beam_search_generate(orc.P, cfg, enc.cpu(), el, prefix, beam, hard_max_seq_len=hard_max, pos_table=orc.pos_table,
                                          return_all=True, no_repeat_ngram_size=ngram)
    plain = ou.beam_search_generate(orc.P, cfg, enc.cpu(), el, prefix, beam, hard_max_seq_len=hard_max, pos_table=orc.pos_table)
    ids, out_lens, scores, hidden = hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=beam, hard_max_seq_len=hard_max,
                                                      no_repeat_ngram_size=ngram)
    got = [ids[b, : out_lens[b]].tolist() for b in range(len(want))]
    _log(report_dir, "ngram_block", beam=beam, ngram=ngram, got=got, want=want, unconstrained=plain)
    assert got == want
    for b in range(len(want)):
        assert abs(float(scores[b]) - every[b][0][0]) < 2e-4
    L = max(len(s) for s in want) - 1
    toks = np.full((len(want), L), cfg.pad_idx, dtype=np.int32)
    for b, s in enumerate(want):
        toks[b, : len(s) - 1] = s[:-1]
    forced = hip.decode_text(enc, enc_lens.tolist(), toks)
    for b, s in enumerate(want):
        assert float((hidden[b, : len(s) - 1] - forced[b, : len(s) - 1]).abs().max()) < 1e-5


def test_translator_accepts_ngram_step_processor():
    """Translator.predict with text_generation_opts.step_processor set (the reference CLI's
    --text_generation_ngram_blocking): same text ids as the stage-level call; other processors are refused."""
    from seamless_communication_amd.inference import NGramRepeatBlockProcessor, SequenceGeneratorOptions

    from seamless_communication_amd.inference import Translator
    from seamless_communication_amd.inference.translator import DEFAULT_CARDS

    card = dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="tiny_v2")
    tr = Translator(card, None, device=torch.device("cuda", 0), output_modality=None)
    wav = torch.from_numpy(common.waves((1.5,))[0])
    opts = SequenceGeneratorOptions(beam_size=3, soft_max_seq_len=(0, 12), step_processor=NGramRepeatBlockProcessor(2))
    tr.predict(wav, "S2TT", "fra", text_generation_opts=opts)
    blocked = tr.last_text_ids[0]
    tr.predict(wav, "S2TT", "fra", text_generation_opts=SequenceGeneratorOptions(beam_size=3, soft_max_seq_len=(0, 12)))
    plain = tr.last_text_ids[0]
    grams = [tuple(blocked[i : i + 2]) for i in range(len(blocked) - 1)]
    body = grams[:-1] if len(blocked) == 12 else grams
    assert len(body) == len(set(body)), blocked
    assert blocked != plain or len(set(grams)) == len(grams)
    with pytest.raises(NotImplementedError):
        tr.predict(wav, "S2TT", "fra", text_generation_opts=SequenceGeneratorOptions(beam_size=1, step_processor=object()))


def test_ragged_vocoder_and_bucketed_t2u_match_the_padded_batch(env, report_dir):
    """Length buckets (sc_vocode_ragged; the bucketed NAR decoder inside sc_t2u_nar): every kept sample / unit equals the
    padded batch's.  Items of very different lengths, so that several buckets form; the padded batch is the reference
    semantics (translator.py:407-419: the vocoder runs on the padded unit matrix, the trim is proportional)."""
    from oracle import vocoder as ov

    cfg, tt, ct, orc, hip = env
    rng = np.random.RandomState(5)
    lens = [230, 40, 7, 228, 100, 1, 64, 229]
    T = max(lens)
    units = np.full((len(lens), T), cfg.unit_pad_idx, dtype=np.int32)
    for i, l in enumerate(lens):
        units[i, :l] = rng.randint(2, cfg.vocoder.num_embeddings, size=l)
    lang_idx, spkr_idx = ov.resolve_lang_spkr(orc.lang_spkr_idx_map, ["fra"] * len(lens), [-1] * len(lens))
    full = hip.vocode(units, lang_idx, spkr_idx)
    rag = hip.vocode(units, lang_idx, spkr_idx, lens)
    pad = hip.last_padding()
    hop = full.shape[-1] // T
    errs = [float((full[i, :, : l * hop] - rag[i, :, : l * hop]).abs().max()) for i, l in enumerate(lens)]
    _log(report_dir, "ragged_vocoder", errs=errs, rows_computed=pad["vocoder_rows_computed"], rows_padded=len(lens) * T)
    assert max(errs) == 0.0  # the same kernels on the same window: bit-identical where it is kept
    assert pad["vocoder_rows_computed"] < 0.75 * len(lens) * T
    # the buckets run on side chains (own stream + scratch pool each, model_t2u.hip: run_vocode): repeated calls must not
    # differ by a bit - a block handed to two chains at once or a missing join would show up here
    for _ in range(4):
        again = hip.vocode(units, lang_idx, spkr_idx, lens)
        assert all(torch.equal(again[i, :, : l * hop], rag[i, :, : l * hop]) for i, l in enumerate(lens))
    # NAR decoder: ids of a ragged batch equal the ids of each item run alone (one bucket each)
    ws = common.waves((2.0, 0.6, 1.3, 0.4))
    fb, flens = orc.collate_fbank(ws)
    seqs, enc, enc_lens, _ = orc.s2tt(fb, flens, "fra", (1, 200), 14)
    ids, out_lens, _, hidden = hip.generate_text(enc.cuda().contiguous(), enc_lens.tolist(), tt.target_prefix("fra"), hard_max_seq_len=14)
    u_all, ul_all, _, _, _ = hip.t2u_nar(hidden, ids[:, :-1].copy(), (out_lens - 1).tolist(), 1.0)
    pad = hip.last_padding()
    for b in range(len(ws)):
        u1, ul1, _, _, _ = hip.t2u_nar(hidden[b : b + 1].contiguous(), ids[b : b + 1, :-1].copy(), [int(out_lens[b]) - 1], 1.0)
        assert int(ul1[0]) == int(ul_all[b]) and u1[0, : ul1[0]].tolist() == u_all[b, : ul_all[b]].tolist()
    assert pad["t2u_rows_computed"] <= pad["t2u_rows_padded"]


def test_soft_length_rule_uses_the_source_length(env):
    """fairseq2 computes int(a * source_len + b) from the sequences the generator is called with (fbank frames for
    speech, inference/generator.py:261-263); sc_gen_opts.source_len carries that, 0 falls back to the encoder length."""
    import ctypes as C

    cfg, tt, ct, orc, hip = env
    for source_len, s_enc, want in ((0, 13, min(13 + 5, 200)), (100, 13, min(100 + 5, 200)), (1000, 13, 200)):
        o = hip._gen_opts(1, (1, 5), 200, 1, 0.0, True, source_len=source_len)
        assert hip.lib.sc_text_max_len(hip.handle, C.byref(o), s_enc) == min(want, cfg.text_max_seq_len)


def test_sc_s2st_one_call_equals_the_staged_calls(env):
    """sc_s2st (the fused convenience entry of SURVEY section 8b) returns what the four staged calls return."""
    from oracle import vocoder as ov

    cfg, tt, ct, orc, hip = env
    ws = common.waves((1.6, 0.9, 1.2))
    wav, ns = common.pad_waves(ws)
    fb, frames = hip.fbank(torch.from_numpy(wav).cuda(), ns)
    prefix = tt.target_prefix("fra")
    lang_idx, spkr_idx = ov.resolve_lang_spkr(orc.lang_spkr_idx_map, ["fra"] * 3, [-1] * 3)
    enc, enc_lens = hip.encode_speech(fb, frames.tolist())
    ids, out_lens, _, hidden = hip.generate_text(enc, enc_lens.tolist(), prefix, hard_max_seq_len=14, source_len=fb.shape[1])
    units, ulens, _, _, _ = hip.t2u_nar(hidden, ids[:, :-1].copy(), (out_lens - 1).tolist(), 1.0)
    wav_ref = hip.vocode(units, lang_idx, spkr_idx, ulens)
    ids2, tl2, units2, ul2, wav2, su = hip.s2st(fb, frames.tolist(), prefix, lang_idx, spkr_idx, unit_cap=units.shape[1] + 7, hard_max_seq_len=14)
    assert su == units.shape[1] and ids2.tolist() == ids.tolist() and tl2.tolist() == out_lens.tolist() and ul2.tolist() == ulens.tolist()
    assert units2[:, :su].tolist() == units.tolist() and (units2[:, su:] == cfg.unit_pad_idx).all()
    for b in range(3):
        k = int(ulens[b]) * hip.hop
        assert torch.equal(wav2[b, :, :k], wav_ref[b, :, :k])
    with pytest.raises(Exception, match="unit_cap"):
        hip.s2st(fb, frames.tolist(), prefix, lang_idx, spkr_idx, unit_cap=3, hard_max_seq_len=14)
