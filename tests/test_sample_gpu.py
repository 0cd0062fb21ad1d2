"""GPU: sampled text generation (csrc/model_sample.hip, sc_generate_text_sampled, Translator.sample / predict with a sampler) on
the tiny models (V = 1200).

Post-hoc verification: every returned sequence goes through the existing teacher-forced pass (sc_decode_text), the tied
projection gives float64 logits per position, and tests/sample_oracle.py is re-run step by step with the same (seed, stream,
gen, position): every token must pass the acceptance rule of tests/test_sample_kernel_gpu.py, at most 2 % of the steps may
need its tolerance clause (asserted on the oracle side), and step_lprobs / scores must agree within 2e-4 - the bar the beam
search's scores have against the float64 oracle (tests/test_banned_gpu.py): the logits of the step loop and of the
teacher-forced pass come from different kernels."""
import numpy as np
import pytest
import torch

from tests import common
from tests import sample_oracle as so

pytestmark = pytest.mark.gpu

HARD_MAX = 14


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    orc, hip = common.make_oracle(), common.make_hip()
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37, 0.9)))
    enc, enc_lens = hip.encode_speech(fb.cuda(), lens.tolist())
    W = sd["final_proj.weight"].half().double()  # the tied projection as the library stores it
    return {"cfg": cfg, "tt": tt, "hip": hip, "enc": enc, "enc_lens": enc_lens.tolist(), "W": W, "prefix": tt.target_prefix("fra")}


def sample(env, rows=None, **kw):
    enc, lens = env["enc"], env["enc_lens"]
    if rows is not None:
        enc, lens = enc[rows].contiguous(), [lens[r] for r in rows]
    kw.setdefault("hard_max_seq_len", HARD_MAX)
    return env["hip"].generate_text_sampled(enc, lens, env["prefix"], **kw)


def posthoc(env, out, *, seed, streams, T, top_k, top_p, rows=None, min_seq_len=1, unk_penalty=0.0, max_len=HARD_MAX):
    """Re-runs the oracle over every returned hypothesis.  -> (steps, steps near a boundary, steps through the tolerance)."""
    ids, lens, scores, slp, _ = out
    hip, W, P = env["hip"], env["W"], len(env["prefix"])
    enc, enc_lens = env["enc"], env["enc_lens"]
    if rows is not None:
        enc, enc_lens = enc[rows].contiguous(), [enc_lens[r] for r in rows]
    n, G, _ = ids.shape
    steps = near = used = 0
    found = [[] for _ in range(n)]
    for g in range(G):
        L = int(lens[:, g].max()) - 1
        toks = np.full((n, L), env["cfg"].pad_idx, dtype=np.int32)
        for u in range(n):
            toks[u, : lens[u, g] - 1] = ids[u, g, : lens[u, g] - 1]
        hidden = hip.decode_text(enc, enc_lens, toks).cpu().double()
        for u in range(n):
            x = (hidden[u] @ W.T).numpy().astype(np.float32)  # row p: the logits behind position p
            last = int(lens[u, g]) - 1
            echo = 0.0  # prompt echo: the log-probabilities of the prompt tokens under the temperature, no rule
            for p in range(P - 1):
                y = np.float64(np.float32(x[p, ids[u, g, p + 1]]) * (np.float32(1.0) / np.float32(T)))
                echo += float(y - so.row_values(x[p], T)[1])
            assert (slp[u, g, :P] == 0.0).all()
            # the hypotheses come back sorted by score, so the hypothesis number of slot g is not known: one of them must
            # explain every step of the sequence
            fits = {}
            for gen in range(G):
                refs = [so.sample_row(x[p], T, top_k, top_p, seed, streams[u], gen, p + 1, no_eos=p < min_seq_len,
                                      force_eos=p == max_len - 2, unk_penalty=unk_penalty) for p in range(P - 1, last)]
                verdicts = [so.judge(ref, int(ids[u, g, P + i])) for i, ref in enumerate(refs)]
                if all(v is not None for v in verdicts):
                    fits[gen] = (refs, verdicts)
            assert fits, (u, g, ids[u, g, : lens[u, g]].tolist())
            found[u].append(set(fits))
            refs, verdicts = next(iter(fits.values()))
            steps += len(refs)
            near += sum(so.near_boundary(ref) for ref in refs)
            used += sum(v == "near" for v in verdicts)
            total = echo
            for i, ref in enumerate(refs):
                v = float(ref["v"][ids[u, g, P + i]])
                assert abs(float(slp[u, g, P + i]) - v) < 2e-4, (u, g, i)
                total += v
            want = total / float(last)
            assert abs(float(scores[u, g]) - want) < 2e-4 * (1 + abs(want)), (u, g, float(scores[u, g]), want)
    for u in range(n):  # distinct sequences of an utterance come from distinct hypothesis numbers
        distinct = len({tuple(ids[u, g, : lens[u, g]]) for g in range(G)})
        assert len(set().union(*found[u])) >= distinct, (u, found[u])
    return steps, near, used


def test_top_k_1_is_the_greedy_hypothesis(env):
    hip, enc, lens, prefix = env["hip"], env["enc"], env["enc_lens"], env["prefix"]
    ids, out_lens, scores, slp, _ = sample(env, num_gens=3, top_k=1, seed=5)
    g_ids, g_lens, _, _ = hip.generate_text(enc, lens, prefix, beam_size=1, hard_max_seq_len=HARD_MAX, want_hidden=False)
    # the host-driven loop of the beam search at beam_size 1 (an n-gram size above every length blocks nothing)
    _, _, h_scores, _ = hip.generate_text(enc, lens, prefix, beam_size=1, hard_max_seq_len=HARD_MAX, want_hidden=False,
                                          no_repeat_ngram_size=HARD_MAX + 1)
    worst = 0.0
    for u in range(3):
        for g in range(3):
            assert out_lens[u, g] == g_lens[u] and ids[u, g, : g_lens[u]].tolist() == g_ids[u, : g_lens[u]].tolist()
            d = abs(float(scores[u, g]) - float(h_scores[u]))
            worst = max(worst, d / (1 + abs(float(h_scores[u]))))
    print(f"top_k=1 score against the host-driven loop: worst relative difference {worst:.3e}")
    assert worst <= 1e-5


def test_sampled_run_verifies_post_hoc(env):
    kw = dict(num_gens=4, top_p=0.9, temperature=0.8, seed=20240901)
    out = sample(env, **kw)
    again = sample(env, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(out[:4], again[:4])), "the same call twice"
    other = sample(env, **{**kw, "seed": 7})
    assert not np.array_equal(out[0], other[0])
    ids, lens, scores, slp, _ = out
    for u in range(3):
        s = scores[u].tolist()
        assert s == sorted(s, reverse=True), s
        for g in range(4):
            row = ids[u, g].tolist()
            assert so.PAD not in row[: lens[u, g]] and row[lens[u, g] - 1] == so.EOS and all(t == so.PAD for t in row[lens[u, g]:])
    steps, near, used = posthoc(env, out, seed=20240901, streams=[0, 1, 2], T=0.8, top_k=0, top_p=0.9)
    print(f"post-hoc: {steps} steps, {near} near a boundary, {used} through the tolerance clause")
    assert steps > 40 and near <= 0.02 * steps and used <= 0.02 * steps


def test_graph_replay_equals_eager_launching(env):
    """use_graph=True (the step replayed from its captured graph) and use_graph=False (the same launches made one by one)
    return the same ids, lengths, scores and step log-probabilities, bit for bit: 2 utterances x 3 hypotheses."""
    kw = dict(rows=[0, 1], num_gens=3, top_p=0.9, temperature=0.8, seed=20240901)
    eager, graph = sample(env, use_graph=False, **kw), sample(env, use_graph=True, **kw)
    assert eager[0].shape[:2] == (2, 3)
    for a, b in zip(eager[:4], graph[:4]):
        assert np.array_equal(a, b)


def test_streams_make_an_utterance_independent_of_its_batch(env):
    kw = dict(num_gens=4, top_p=0.9, temperature=0.8, seed=11)
    batch = sample(env, streams=[7, 8, 9], **kw)
    steps, near, used = posthoc(env, batch, seed=11, streams=[7, 8, 9], T=0.8, top_k=0, top_p=0.9)
    assert near <= 0.02 * steps and used <= 0.02 * steps
    for u in range(3):  # one utterance per call, the same stream id: verified by the oracle, not by the bits of the logits
        alone = sample(env, rows=[u], streams=[7 + u], **kw)
        s1, n1, u1 = posthoc(env, alone, seed=11, streams=[7 + u], T=0.8, top_k=0, top_p=0.9, rows=[u])
        steps, near, used = steps + s1, near + n1, used + u1
    assert near <= 0.02 * steps and used <= 0.02 * steps  # over all steps of the four calls
    assert not np.array_equal(batch[0], sample(env, streams=[17, 18, 19], **kw)[0])


def test_rules_inside_the_loop(env):
    P = len(env["prefix"])
    ids, lens, _, _, _ = sample(env, num_gens=4, top_p=1.0, seed=3, min_seq_len=8)
    for u in range(3):
        for g in range(4):
            assert so.EOS not in ids[u, g, 1:9].tolist(), "EOS before min_seq_len"
    ids, lens, _, _, _ = sample(env, num_gens=4, top_p=1.0, seed=3, hard_max_seq_len=6)
    assert (lens <= 6).all() and all(ids[u, g, lens[u, g] - 1] == so.EOS for u in range(3) for g in range(4))
    assert (lens == 6).any(), "no row reached the length limit: the forced EOS was not exercised"
    plain = sample(env, num_gens=4, top_k=3, seed=9)[0]
    banned = [[int(t)] for t in {int(plain[u, 0, P]) for u in range(3)}] + [[int(plain[0, 1, P + 1]), int(plain[0, 1, P + 2])]]
    ids, lens, _, _, _ = sample(env, num_gens=4, top_k=3, seed=9, no_repeat_ngram_size=2, banned_seqs=banned)
    single = {b[0] for b in banned if len(b) == 1}
    for u in range(3):
        for g in range(4):
            hyp = ids[u, g, : lens[u, g]].tolist()
            body = hyp[:-1] if len(hyp) == HARD_MAX else hyp  # (the forced-EOS step applies no processor)
            grams = list(zip(body, body[1:]))
            assert len(set(grams)) == len(grams), hyp
            assert not single & set(body[P:]) and tuple(banned[-1]) not in set(zip(body[P - 1:], body[P:])), hyp
            assert so.PAD not in hyp


def test_invalid_options_are_refused_before_device_work(env):
    from seamless_communication_amd._lib import SeamlessHipError

    for bad in (dict(num_gens=0), dict(num_gens=65), dict(num_gens=-3), dict(temperature=0.0),
                dict(temperature=float("inf")), dict(temperature=float("nan")), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5),
                dict(banned_seqs=[[5, 100000]])):
        with pytest.raises(SeamlessHipError, match="status -1"):
            sample(env, **bad)
    with pytest.raises(ValueError):
        sample(env, streams=[1, 2])
    assert sample(env, top_k=1)[1].min() > len(env["prefix"])  # the handle stays usable


def _translator(vocoder):
    from seamless_communication_amd.inference import Translator
    from seamless_communication_amd.inference.translator import DEFAULT_CARDS

    return Translator(dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="tiny_v2"), dict(DEFAULT_CARDS["vocoder_v2"]) if vocoder else None,
                      device=torch.device("cuda", 0))


def test_translator_sample_and_predict_with_a_sampler():
    from seamless_communication_amd.inference import SampledHypothesis, SequenceGeneratorOptions, TopKSampler, TopPSampler

    tr = _translator(True)
    wav = torch.from_numpy(common.waves((1.5,))[0])
    opts = SequenceGeneratorOptions(beam_size=5, hard_max_seq_len=12)  # (sampled rows of the tiny model seldom draw EOS: a hard limit)
    hyps = tr.sample(wav, "S2TT", "fra", sampler=TopPSampler(0.9), num_gens=4, temperature=0.8, seed=3, text_generation_opts=opts)
    assert len(hyps) == 1 and len(hyps[0]) == 4 and all(isinstance(h, SampledHypothesis) for h in hyps[0])
    assert [h.score for h in hyps[0]] == sorted((h.score for h in hyps[0]), reverse=True)
    for h in hyps[0]:
        assert h.text == tr.text_tokenizer.decode(h.token_ids) and len(h.step_lprobs) == len(h.token_ids) and h.token_ids[-1] == so.EOS
    assert hyps == tr.sample(wav, "S2TT", "fra", sampler=TopPSampler(0.9), num_gens=4, temperature=0.8, seed=3, text_generation_opts=opts)
    assert len(tr.sample("hello there", "T2TT", "fra", "eng", sampler=TopKSampler(3), num_gens=2, text_generation_opts=opts)[0]) == 2
    with pytest.raises(ValueError, match="predict"):
        tr.sample(wav, "S2ST", "fra", sampler=TopKSampler(3))
    with pytest.raises(ValueError):
        tr.sample(wav, "S2TT", "fra", sampler=TopKSampler(3), num_gens=0)
    # predict without a sampler: the options the sampler reads are inert
    base_t, base_s = tr.predict(wav, "S2ST", "fra", text_generation_opts=opts, duration_factor=0.1)
    base_ids = list(tr.last_text_ids[0])
    same_t, same_s = tr.predict(wav, "S2ST", "fra", duration_factor=0.1,
                                text_generation_opts=SequenceGeneratorOptions(beam_size=5, hard_max_seq_len=12, temperature=0.3, seed=99))
    assert same_t == base_t and same_s.units == base_s.units and torch.equal(same_s.audio_wavs[0], base_s.audio_wavs[0])
    # predict with a sampler: one sampled text feeds T2U and the vocoder
    sopts = SequenceGeneratorOptions(beam_size=5, hard_max_seq_len=12, sampler=TopKSampler(4), temperature=1.3, seed=21)
    texts, speech = tr.predict(wav, "S2ST", "fra", text_generation_opts=sopts, duration_factor=0.1)
    ids = list(tr.last_text_ids[0])
    assert ids != base_ids and texts == [tr.text_tokenizer.decode(ids)]
    assert len(speech.units[0]) > 0 and speech.audio_wavs[0].shape[-1] > 0 and torch.isfinite(speech.audio_wavs[0]).all()
    again_t, again_s = tr.predict(wav, "S2ST", "fra", text_generation_opts=sopts, duration_factor=0.1)
    assert again_t == texts and again_s.units == speech.units
    want = tr.sample(wav, "S2TT", "fra", sampler=TopKSampler(4), temperature=1.3, seed=21, text_generation_opts=sopts)[0][0]
    assert want.token_ids == ids
