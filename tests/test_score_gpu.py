"""Teacher-forced scoring at stage level: sc_score_text (runtime.HipS2STModel.score_text), Translator.score and
finetune_eval_loss on the tiny models - against the float64 head on the device's own decoder output (kernel bars of
tests/test_score_kernel_gpu.py), against the full CPU oracle, item-alone vs ragged batch, forked handles, and against
what greedy generation reports for the same sequences."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import common
from tests import score_oracle as so

pytestmark = pytest.mark.gpu

HIDDEN_TOL = 2e-4  # tests/test_stages_gpu.py: teacher-forced hidden against the oracle, stepwise against batched
LENS = (2, 3, 17, 20)  # whole sequences (prompt ... </s>): the shortest allowed, one body token, a middle one, s_text


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@functools.lru_cache(maxsize=None)
def model(kind):
    """(cfg, state dict, tokenizer, HIP handle) of a tiny model: v2, v1 (enc_variant / t2u_variant 1), expressive (GELU
    decoder), text (v2 with the NLLB text encoder)."""
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from seamless_communication_amd import cards, synthetic as syn
    from seamless_communication_amd.config import tiny_expressive_config, tiny_v1_config
    from seamless_communication_amd.runtime import HipS2STModel
    from seamless_communication_amd.tokenizer import NllbTextTokenizer

    if kind == "v2":
        cfg, sd, _, tt, _ = common.tiny_bundle()
        return cfg, sd, tt, common.make_hip()
    if kind == "text":
        cfg, sd, _, tt, _ = common.tiny_bundle_text()
        return cfg, sd, tt, common.make_hip_text()
    cfg = tiny_v1_config() if kind == "v1" else tiny_expressive_config()
    sd = syn.make_unity_state_dict(cfg, syn.DEFAULT_SEED)
    tt = NllbTextTokenizer(cfg.text_vocab_size, cards.TEXT_LANGS)
    return cfg, sd, tt, HipS2STModel(cfg, sd, None, device=0)


def sequences(cfg, tt, lens=LENS, seed=5):
    """Whole sequences </s> __fra__ w.. </s>, pad filled."""
    rng = np.random.RandomState(seed)
    out = np.full((len(lens), max(lens)), cfg.pad_idx, dtype=np.int32)
    for b, n in enumerate(lens):
        row = [cfg.eos_idx, tt.lang_token_idx("fra")] + rng.randint(4, cfg.text_vocab_size - 110, size=max(n - 3, 0)).tolist() + [cfg.eos_idx]
        out[b, :n] = row[:n] if n > 2 else row[:2]
    return out, np.asarray(lens, dtype=np.int32)


def encoder_output(kind, cfg, hip, n):
    """d_enc of n items, ragged: the speech encoder (v2), the text encoder (text), or - the scoring stage takes any
    encoder output - seeded values of encoder-output scale (v1, expressive)."""
    if kind == "v2":
        orc = common.make_oracle()
        fb, lens = orc.collate_fbank(common.waves((2.0, 1.37, 0.9, 1.1)[:n]))
        enc, enc_lens = hip.encode_speech(fb.cuda().contiguous(), lens.tolist())
        return enc, enc_lens.tolist()
    if kind == "text":
        src_lens = [9, 4, 6, 7][:n]
        rng = np.random.RandomState(11)
        src = rng.randint(4, cfg.text_vocab_size - 110, size=(n, max(src_lens))).astype(np.int32)
        return hip.encode_text(src, src_lens), src_lens
    g = torch.Generator().manual_seed(17)
    return torch.randn(n, 12, cfg.model_dim, generator=g).cuda().contiguous(), [12, 7, 9, 5][:n]


def head_ref(lib, hidden, w16, tokens, tok_lens):
    """float64 head on the given hidden states (n, s-1, M): per valid row the reference statistics, the parent product's
    error e and the (b, p) it belongs to."""
    rows = [(b, p) for b in range(len(tok_lens)) for p in range(int(tok_lens[b]) - 1)]
    x = torch.stack([hidden[b, p] for b, p in rows]).float().cpu()
    target = np.asarray([tokens[b, p + 1] for b, p in rows], dtype=np.int32)
    ref = so.score_ref(x, w16, None, target)
    M, K = x.shape
    N = w16.shape[0]
    xd, wd = x.cuda(), w16.cuda().contiguous()
    y = torch.full((M, N), float("nan"), device="cuda")
    torch.cuda.synchronize()
    assert lib.sc_op_linear_presplit(P(xd), P(wd), None, None, P(y), None, None, M, N, K, 0, 1.0) == 0, lib.sc_last_error().decode()
    e = (y.cpu().double() - ref["logits"]).abs().amax(dim=1)
    return rows, ref, e


def packed(arr, rows):
    return torch.as_tensor(np.asarray([arr[b, p] for b, p in rows]))


@pytest.mark.parametrize("kind", ["v2", "v1", "expressive", "text"])
def test_score_text_against_float64_head_on_device_hidden(kind):
    """Every model the handle can hold, both encoder-output sources: d_dec_hidden equals sc_decode_text's output to the bit,
    and the scores equal the float64 head on that hidden inside the kernel bars; padded positions hold 0 / -1."""
    cfg, sd, tt, hip = model(kind)
    tokens, tok_lens = sequences(cfg, tt)
    enc, enc_lens = encoder_output(kind, cfg, hip, len(tok_lens))
    res = hip.score_text(enc, enc_lens, tokens, tok_lens, want_sum=True, want_top1=True, want_hidden=True)
    hidden = hip.decode_text(enc, enc_lens, tokens[:, :-1])
    assert torch.equal(res["hidden"], hidden)
    w16 = sd["final_proj.weight"].half()
    rows, ref, e = head_ref(hip.lib, hidden, w16, tokens, tok_lens)
    V = cfg.text_vocab_size
    bar = so.bars(ref, e, hip.lib.sc_op_score_record_cols(V), V)
    lp, sl, t1 = packed(res["tok_lprob"], rows).double(), packed(res["sum_lprob"], rows).double(), packed(res["top1"], rows).numpy()
    err_lp, err_sl = (lp - ref["lprob"]).abs(), (sl - ref["sum_lprob"]).abs() / V
    print(f"score_text[{kind}] lprob err {float(err_lp.max()):.3e} (bar {float(bar['lprob'].max()):.3e}) sum_lprob/V err {float(err_sl.max()):.3e} "
          f"(bar {float(bar['sum_lprob_mean'].max()):.3e}) e {float(e.max()):.3e}")
    assert (err_lp <= bar["lprob"]).all() and (err_sl <= bar["sum_lprob_mean"]).all()
    assert (lp <= 0).all()
    sure = (ref["margin"] > 2 * e).numpy()
    assert np.array_equal(t1[sure], ref["top1"][sure])
    for b, n in enumerate(tok_lens):
        assert (res["tok_lprob"][b, n - 1:] == 0).all() and (res["sum_lprob"][b, n - 1:] == 0).all() and (res["top1"][b, n - 1:] == -1).all()
        assert (res["top1"][b, : n - 1] >= 0).all()


def test_score_text_against_the_oracle():
    """The full CPU oracle (oracle.unity.decode_text, then the float64 head).  Bar: the decoder output may differ by the
    teacher-forced tolerance of tests/test_stages_gpu.py (2e-4) in every element, a logit then by that times the L1 norm of
    its final_proj row, and a log-probability (a difference of two 1-Lipschitz functions of the logits) by twice that."""
    from oracle import unity as ou

    cfg, sd, tt, hip = model("v2")
    orc = common.make_oracle()
    tokens, tok_lens = sequences(cfg, tt)
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37, 0.9, 1.1)))
    with torch.inference_mode():
        enc, enc_lens = ou.encode_speech(orc.P, cfg, fb, lens)
        hid = ou.decode_text(orc.P, cfg, torch.from_numpy(tokens[:, :-1]).long(), torch.from_numpy(tok_lens - 1).long(), enc, enc_lens, orc.pos_table)
    W = orc.P["final_proj.weight"]
    bar = 2 * HIDDEN_TOL * float(W.double().abs().sum(dim=1).max())
    res = hip.score_text(enc.cuda().contiguous(), enc_lens.tolist(), tokens, tok_lens, want_sum=True)
    rows = [(b, p) for b in range(len(tok_lens)) for p in range(int(tok_lens[b]) - 1)]
    x = torch.stack([hid[b, p] for b, p in rows])
    ref = so.score_ref(x, W, None, np.asarray([tokens[b, p + 1] for b, p in rows]))
    err = (packed(res["tok_lprob"], rows).double() - ref["lprob"]).abs()
    err_s = (packed(res["sum_lprob"], rows).double() - ref["sum_lprob"]).abs() / cfg.text_vocab_size
    print(f"score_text vs oracle: lprob err {float(err.max()):.3e} sum_lprob/V err {float(err_s.max()):.3e} bar {bar:.3e}")
    assert float(err.max()) <= bar and float(err_s.max()) <= bar


def test_ragged_batch_equals_items_alone_and_forked_handle():
    """Lengths 2, 3, 17 and s_text in one batch: each item's scores equal, to the bit, its scores when scored alone (at
    its own length and encoder length); a forked handle gives the same bits.  That needs a decoder pass whose rows do not
    see the row count, so below 65 rows d_dec_hidden is the tiled products' and not sc_decode_text's skinny products':
    the two agree to fp32 re-association (1e-5, the bar tests/test_stages_gpu.py sets between the stepwise and the
    batched pass of one hypothesis)."""
    cfg, sd, tt, hip = model("v2")
    tokens, tok_lens = sequences(cfg, tt)
    enc, enc_lens = encoder_output("v2", cfg, hip, len(tok_lens))
    kw = dict(want_sum=True, want_top1=True)
    res = hip.score_text(enc, enc_lens, tokens, tok_lens, **kw)
    for b, n in enumerate(tok_lens):
        s_enc = int(enc_lens[b])
        alone = hip.score_text(enc[b:b + 1, :s_enc].contiguous(), [s_enc], tokens[b:b + 1, :n], [n], want_hidden=True, **kw)
        skinny = hip.decode_text(enc[b:b + 1, :s_enc].contiguous(), [s_enc], tokens[b:b + 1, : n - 1])
        assert float((alone["hidden"] - skinny).abs().max()) < 1e-5
        for k in ("tok_lprob", "sum_lprob", "top1"):
            assert np.array_equal(alone[k][0].view(np.int32), res[k][b, : n - 1].view(np.int32)), (b, k)
    fork = hip.fork()
    try:
        res_f = fork.score_text(enc, enc_lens, tokens, tok_lens, **kw)
    finally:
        fork.close()
    for k in ("tok_lprob", "sum_lprob", "top1"):
        assert np.array_equal(res_f[k].view(np.int32), res[k].view(np.int32)), k


def test_scores_agree_with_greedy_generation():
    """The greedy hypotheses of sc_generate_text_capture, scored: step_lprob agrees with tok_lprob within the stepwise-vs-
    batched tolerance (2e-4 on the hidden, times the largest L1 norm of a final_proj row, twice: as against the oracle) at
    the positions whose chosen token is not EOS (the step rules - no PAD, forced EOS at the length limit - do not touch
    those), and top1 reproduces the hypothesis wherever the oracle's greedy margin exceeds that tolerance."""
    cfg, sd, tt, hip = model("v2")
    orc = common.make_oracle()
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37)))
    seqs, enc, enc_lens, margins = orc.s2tt(fb, lens, "fra", (1, 200), 20)
    encd = enc.cuda().contiguous()
    ids, out_lens, _, _, step_lprob, _ = hip.generate_text_capture(encd, enc_lens.tolist(), tt.target_prefix("fra"), hard_max_seq_len=20)
    assert [ids[b, : out_lens[b]].tolist() for b in range(len(seqs))] == seqs
    tol = 2 * HIDDEN_TOL * float(sd["final_proj.weight"].double().abs().sum(dim=1).max())
    s_text = int(out_lens.max())
    tokens = np.where(np.arange(s_text)[None] < out_lens[:, None], ids[:, :s_text], cfg.pad_idx).astype(np.int32)
    res = hip.score_text(encd, enc_lens.tolist(), tokens, out_lens, want_top1=True)
    checked = 0
    for b, seq in enumerate(seqs):
        assert step_lprob[b, 0] == 0.0  # fed </s>, "chose" the prompt's language token
        for p in range(1, len(seq) - 1):  # fed position p chose seq[p + 1]; margins[b][p - 1] is that step's
            if seq[p + 1] != cfg.eos_idx:
                assert abs(float(step_lprob[b, p]) - float(res["tok_lprob"][b, p])) <= tol, (b, p)
                checked += 1
                if margins[b][p - 1] > tol:
                    assert res["top1"][b, p] == seq[p + 1], (b, p)
    assert checked >= 8


@functools.lru_cache(maxsize=1)
def translator():
    from seamless_communication_amd.inference import Translator
    from seamless_communication_amd.inference.translator import DEFAULT_CARDS

    card = dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="tiny_v2")
    return Translator(card, None, device=torch.device("cuda", 0))


def test_translator_score_speech_and_text_strings_and_ids():
    """Translator.score: a target as a string and as the ids the tokenizer gives are the same call; `score` leaves the
    language-token position out; a single input with several targets scores each against it; token_lprobs equal
    score_text's on the same sequences."""
    tr = translator()
    tt = tr.text_tokenizer
    wav = torch.from_numpy(common.waves((1.5,))[0])
    texts = ["ab cd", "hello there"]
    by_text = tr.score(wav, "s2tt", "fra", texts)
    body = [tt.encode_pieces(t) for t in texts]
    by_ids = tr.score(wav, "S2TT", "fra", body)
    whole = tr.score(wav, "asr", "fra", [tt.target_prefix("fra") + b + [tt.vocab_info.eos_idx] for b in body])
    for a, b, c, ids in zip(by_text, by_ids, whole, body):
        assert a.token_ids == b.token_ids == c.token_ids == [tt.lang_token_idx("fra")] + ids + [tt.vocab_info.eos_idx]
        assert a.token_lprobs == b.token_lprobs == c.token_lprobs and len(a.top1) == len(a.token_ids)
        assert all(x <= 0 for x in a.token_lprobs)
        assert a.score == pytest.approx(float(np.sum(np.float64(a.token_lprobs[1:]))), abs=1e-9)
        assert a.score_normalized == pytest.approx(a.score / (len(a.token_ids) - 1), abs=1e-12)
    one = tr.score(wav, "s2tt", "fra", texts[1])
    assert one[0].token_lprobs == by_text[1].token_lprobs  # scored alone: the same bits
    # text input
    t2 = tr.score("ab cd ef", "t2tt", "fra", ["ab cd", body[1]], src_lang="eng")
    assert [s.token_ids for s in t2] == [s.token_ids for s in by_text]
    assert all(x <= 0 for s in t2 for x in s.token_lprobs) and t2[0].token_lprobs != by_text[0].token_lprobs
    with pytest.raises(ValueError):
        tr.score("ab cd ef", "t2tt", "fra", ["ab cd"])  # src_lang missing, as predict


@pytest.mark.parametrize("ls", [0.0, 0.2])
def test_finetune_eval_loss_against_materialised_logits(ls):
    """finetune_eval_loss over two batches against the float64 restatement on materialised logits: the device's decoder
    output through the float64 head, log_softmax, the fairseq2 0.2 label-smoothed nll_loss formula with the language
    position dropped and pads ignored, divided by sum(target_lengths - 1).  Bar per token: the lprob bar of the kernel
    tests for smoothing 0 (an average of per-token errors), the same for the smoothed term's eps * sum_lprob."""
    from seamless_communication_amd.scoring import finetune_eval_loss

    tr = translator()
    cfg, tt, hip = tr.cfg, tr.text_tokenizer, tr.model
    w16 = common.tiny_bundle()[1]["final_proj.weight"].half()
    orc = common.make_oracle()
    batches, num, den, tol_sum = [], 0.0, 0, 0.0
    for k, (secs, lens) in enumerate((((2.0, 1.37), (9, 5)), ((0.9,), (12,)))):
        fb, flens = orc.collate_fbank(common.waves(secs))
        tokens, tok_lens = sequences(cfg, tt, lens, seed=20 + k)
        batch = dict(src_tokens=fb, src_lengths=flens, prev_output_tokens=torch.from_numpy(tokens[:, :-1]).long(),
                     target_tokens=torch.from_numpy(tokens[:, 1:]).long(), target_lengths=torch.from_numpy(tok_lens - 1).long())
        batches.append(batch)
        enc, enc_lens = hip.encode_speech(fb.cuda().contiguous(), flens.tolist())
        hidden = hip.decode_text(enc, enc_lens.tolist(), tokens[:, :-1])
        logits = torch.nn.functional.linear(hidden.cpu().double(), w16.double())
        num += so.smoothed_loss_ref(logits, batch["target_tokens"], cfg.pad_idx, ls)
        den += int((tok_lens - 2).sum())
        rows, ref, e = head_ref(hip.lib, hidden, w16, tokens, tok_lens)
        V = cfg.text_vocab_size
        bar = so.bars(ref, e, hip.lib.sc_op_score_record_cols(V), V)
        tol_sum += float(bar["lprob"].sum()) + ls * float(bar["sum_lprob_mean"].sum()) * V / (V - 1)
    got = finetune_eval_loss(tr, batches, label_smoothing=ls)
    want = num / den
    print(f"finetune_eval_loss ls={ls}: got {got:.9f} want {want:.9f} diff {abs(got - want):.3e} bar {tol_sum / den:.3e}")
    assert abs(got - want) <= tol_sum / den
