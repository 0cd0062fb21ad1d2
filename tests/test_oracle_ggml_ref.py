"""Pins the CPU oracle (oracle/unity.py) against the reference's OWN native restatement of the
fairseq2 modules, executed: ggml/examples/unity/fairseq2.cpp compiled from /root/reference by
oracle/build_ref.sh (oracle/_ref/libggml_ref.so) and driven with the tiny synthetic checkpoint.  Its answers are recorded
in tests/golden/compiled_ref_calls.npz (tests/ref_replay.py), so the module runs without the library.

What this pins: LayerNorm / Linear / FFN (ReLU, SiLU), multi-head attention
(scaling, head split, causal mask), the pre-LN encoder layer + encoder stack (a12), the decoder layer and
teacher-forced decoder stack (a9, a11), the embedding frontend (a9), the adaptor layer (a7), and the
sequence generator's step rules + KV-cached incremental decoding end to end (a8, a10): greedy ids, and every
hypothesis (ids and scores) of beam search with beam sizes 2-5 (f3).

Tolerances: LayerNorm / Linear / ReLU-FFN 2e-4 abs on O(1) values (different accumulation order);
anything through ggml's SiLU or soft-max 3e-3 abs, because the reference's ggml evaluates exp() and SiLU
through fp16 lookup tables (ggml/src/ggml.c `ggml_table_exp_f16`, `ggml_table_silu_f16`) - the reference's own
ggml-vs-fairseq2 tests use tolerances of that order (ggml/test_unity_cpp.py); token ids exact.
"""
import math

import numpy as np
import pytest
import torch

from oracle import unity as ou
from tests import common
from tests import ref_replay as ggml_ref

ATOL = 2e-4
ATOL_TABLE = 3e-3  # paths through ggml's fp16 exp / SiLU tables


@pytest.fixture(scope="module")
def env():
    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    P = ou.Params(sd)
    ref = ggml_ref.GgmlRef(tensor_mem_mb=128)
    keep = ("text_decoder.", "t2u_model.encoder.", "speech_encoder.adaptor_layers.", "speech_encoder.inner.layers.0.ffn",
            "speech_encoder.inner.layers.0.layer_norm", "final_proj.")
    sub = {k: v for k, v in sd.items() if k.startswith(keep)}
    ref.add_state_dict(sub)
    ref.configure(sub, num_heads=cfg.num_heads, norm_order=ggml_ref.NORM_ORDER_PRE)
    # embedding frontend the way ggml_convert.py exports it: scale baked in, sinusoidal table stored
    pos = ou.sinusoidal_table(cfg.text_max_seq_len, cfg.model_dim, 1)
    ref.add_tensor("text_decoder_frontend.embed.weight", P["text_decoder_frontend.embed.weight"] * math.sqrt(cfg.model_dim))
    ref.add_tensor("text_decoder_frontend.pos_encoder", pos)
    for i, lang in enumerate(("__fra__", "__deu__")):
        ref.add_token(lang, tt.lang_token_idx(lang.strip("_")))
    ref.add_token("<unk>", cfg.unk_idx)
    yield cfg, sd, P, ref, tt, pos
    ref.close()


def _x(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_layer_norm_and_linear(env):
    cfg, sd, P, ref, tt, pos = env
    x = _x((1, 9, cfg.model_dim), 1) * 3 + 0.5
    pre = "text_decoder.layers.0.self_attn_layer_norm"
    assert torch.allclose(ref.forward("LayerNorm", pre, x), P.layer_norm(x, pre), atol=1e-5)
    pre = "text_decoder.layers.0.ffn.inner_proj"
    assert torch.allclose(ref.forward("Linear", pre, x), P.linear(x, pre), atol=1e-4)


def test_ffn_relu_and_silu(env):
    cfg, sd, P, ref, tt, pos = env
    x = _x((1, 7, cfg.model_dim), 2)
    got = ref.forward("StandardFeedForwardNetwork", "text_decoder.layers.1.ffn", x)
    assert torch.allclose(got, ou.ffn(P, "text_decoder.layers.1.ffn", x, "relu"), atol=ATOL)
    got = ref.forward("SiluFeedForwardNetwork", "speech_encoder.inner.layers.0.ffn1", x)
    assert torch.allclose(got, ou.ffn(P, "speech_encoder.inner.layers.0.ffn1", x, "silu"), atol=ATOL_TABLE)


@pytest.mark.parametrize("causal", [False, True])
def test_multihead_attention_self(env, causal):
    cfg, sd, P, ref, tt, pos = env
    x = _x((1, 11, cfg.model_dim), 3)
    pre = "text_decoder.layers.0.self_attn"
    got = ref.forward("MultiheadAttention", pre, x, causal=causal)
    want = ou.mha(P, pre, x, x, cfg.num_heads, causal=causal)
    assert torch.allclose(got, want, atol=ATOL_TABLE), float((got - want).abs().max())


def test_multihead_attention_cross(env):
    cfg, sd, P, ref, tt, pos = env
    x, enc = _x((1, 5, cfg.model_dim), 4), _x((1, 13, cfg.model_dim), 5)
    pre = "text_decoder.layers.1.encoder_decoder_attn"
    got = ref.forward("MultiheadAttention", pre, x, y=enc)
    assert torch.allclose(got, ou.mha(P, pre, x, enc, cfg.num_heads), atol=ATOL)


def test_t2u_encoder_layer_and_stack(env):
    """StandardTransformerEncoderLayer (pre-LN) x2 + final LayerNorm == the T2U encoder of oracle.t2u_nar."""
    cfg, sd, P, ref, tt, pos = env
    x = _x((1, 10, cfg.model_dim), 6)
    pre = "t2u_model.encoder.layers.0"
    h = P.layer_norm(x, pre + ".self_attn_layer_norm")
    want = x + ou.mha(P, pre + ".self_attn", h, h, cfg.num_heads)
    want = want + ou.ffn(P, pre + ".ffn", P.layer_norm(want, pre + ".ffn_layer_norm"), "relu")
    got = ref.forward("StandardTransformerEncoderLayer", pre, x)
    assert torch.allclose(got, want, atol=ATOL_TABLE)
    got = ref.forward("StandardTransformerEncoder", "t2u_model.encoder", x)
    want = ou.t2u_encoder(P, cfg, x, None)
    assert torch.allclose(got, want, atol=ATOL_TABLE), float((got - want).abs().max())


def test_decoder_layer_and_teacher_forced_stack(env):
    cfg, sd, P, ref, tt, pos = env
    x, enc = _x((1, 8, cfg.model_dim), 7), _x((1, 12, cfg.model_dim), 8)
    got = ref.forward("StandardTransformerDecoderLayer", "text_decoder.layers.0", x, y=enc)
    want = ou.decoder_layer(P, cfg, "text_decoder.layers.0", x, enc, None)
    assert torch.allclose(got, want, atol=ATOL_TABLE), float((got - want).abs().max())
    got = ref.forward("StandardTransformerDecoder", "text_decoder", x, y=enc)
    want = x
    for i in range(cfg.dec_layers):
        want = ou.decoder_layer(P, cfg, f"text_decoder.layers.{i}", want, enc, None)
    want = P.layer_norm(want, "text_decoder.layer_norm")
    assert torch.allclose(got, want, atol=ATOL_TABLE), float((got - want).abs().max())


def test_embedding_frontend(env):
    cfg, sd, P, ref, tt, pos = env
    toks = [3, 260, 17, 1, 999, 4]
    got = ref.embed("text_decoder_frontend", toks, cfg.model_dim)
    want = ou.embed_text(P, cfg, torch.tensor([toks]), 0, pos)[0]
    assert torch.allclose(got, want, atol=1e-5)


def test_adaptor_layer(env):
    """UnitYTransformerAdaptorLayer (a7): strided GLU convolutions on both branches, MHA, FFN."""
    cfg, sd, P, ref, tt, pos = env
    assert (cfg.adaptor_kernel_size, cfg.adaptor_stride) == (8, 8)  # hard-coded in fairseq2.cpp:817,824
    x = _x((1, 99, cfg.model_dim), 9)
    got = ref.forward("StandardConformerEncoderAdaptorLayer", "speech_encoder.adaptor_layers.0", x)
    want, lens = ou.adaptor_layer(P, cfg, "speech_encoder.adaptor_layers.0", x, torch.tensor([99]))
    assert got.shape[-2] == int(lens[0]) == want.shape[1]
    assert torch.allclose(got.reshape(want.shape), want, atol=ATOL_TABLE), float((got.reshape(want.shape) - want).abs().max())


def _craft_natural_eos(cfg, P, enc, prefix, pos, stop_after):
    """Synthetic weights never emit EOS on their own, and the reference's C++ generator loses its
    `_tweak_lprobs` edits (forced EOS at max_len-2, PAD/min-length masks, UNK penalty) when it is executed:
    fairseq2.cpp:1517-1539 re-runs the whole step graph after the tweak, which overwrites the in-place
    log-softmax buffer with plain soft-max probabilities (observed here: positive "lprobs", no hypothesis is
    ever finalised at the length limit).  Arg-max over probabilities equals arg-max over log-probabilities, so
    the greedy path itself is intact; to compare it end to end the EOS row of final_proj is set so that EOS
    wins on its own at step `stop_after` and not before."""
    import copy

    base = ou.greedy_generate(P, cfg, enc, torch.tensor([enc.shape[1]]), prefix, hard_max_seq_len=stop_after + 8, pos_table=pos)[0]
    dec = ou.IncrementalDecoder(P, cfg, enc, torch.tensor([enc.shape[1]]), pos)
    dec(torch.tensor([base[:1]]))
    hs = [dec(torch.tensor([[t]]))[0, -1] for t in base[1 : stop_after + 1]]  # decoder outputs that predict base[2:...]
    W = P["final_proj.weight"].clone()
    best = [float((W @ h).max()) for h in hs]
    # minimum-norm EOS row with prescribed logits: far below the winner before `stop_after`, above it there
    H = torch.stack(hs).double()
    target = torch.tensor([b - 6.0 for b in best[:-1]] + [best[-1] + 4.0], dtype=torch.float64)
    W[cfg.eos_idx] = (torch.linalg.pinv(H) @ target).float()
    eos_logits = [float(W[cfg.eos_idx] @ h) for h in hs]
    ok = all(e < b - 0.5 for e, b in zip(eos_logits[:-1], best[:-1])) and eos_logits[-1] > best[-1] + 1.0
    P2 = copy.copy(P)
    P2.sd = dict(P.sd)
    P2.sd["final_proj.weight"] = W
    return ok, P2, W


@pytest.mark.parametrize("seed,s_enc", [(11, 9), (12, 20), (13, 5), (14, 31)])
def test_generate_sequence_greedy_ids_match_oracle(env, seed, s_enc):
    """The reference's generate_sequence with beam_size=1 (prompt bootstrap, KV-cached incremental decoding,
    tied projection, arg-max feedback, EOS finalisation) against oracle.greedy_generate, ids exact."""
    cfg, sd, P, ref, tt, pos = env
    enc = _x((1, s_enc, cfg.model_dim), seed)
    prefix = tt.target_prefix("fra")
    crafted = [(_craft_natural_eos(cfg, P, enc, prefix, pos, stop), stop) for stop in (7, 5, 9, 4)]
    (ok, P2, W), stop = next((c for c in crafted if c[0][0]), crafted[0])
    assert ok, "could not craft an EOS row that wins at exactly one step"
    want, margins = ou.greedy_generate(P2, cfg, enc, torch.tensor([s_enc]), prefix, hard_max_seq_len=64, pos_table=pos,
                                       return_margins=True)
    assert want[0][-1] == cfg.eos_idx and len(want[0]) == stop + 2
    assert min(margins[0]) > 1e-3, "degenerate test case: near-tie between the two best tokens"
    ref2 = ggml_ref.GgmlRef(tensor_mem_mb=64)
    try:
        sub = {k: v for k, v in sd.items() if k.startswith("text_decoder.")}
        ref2.add_state_dict(sub)
        ref2.configure(sub, num_heads=cfg.num_heads)
        ref2.add_tensor("final_proj.weight", W)
        ref2.add_tensor("text_decoder_frontend.embed.weight", P["text_decoder_frontend.embed.weight"] * math.sqrt(cfg.model_dim))
        ref2.add_tensor("text_decoder_frontend.pos_encoder", pos)
        ref2.add_token("__fra__", tt.lang_token_idx("fra"))
        ref2.add_token("<unk>", cfg.unk_idx)
        ids, score, steps = ref2.generate(enc[0], prefix, beam_size=1, hard_max_seq_len=64, pad_idx=cfg.pad_idx,
                                          unk_idx=cfg.unk_idx, bos_idx=cfg.bos_idx, eos_idx=cfg.eos_idx)
    finally:
        ref2.close()
    assert ids == want[0], (ids, want[0])
    assert ids[:2] == list(prefix)


def _decoder_ref(cfg, sd, P, W, tt, pos):
    ref2 = ggml_ref.GgmlRef(tensor_mem_mb=64)
    sub = {k: v for k, v in sd.items() if k.startswith("text_decoder.")}
    ref2.add_state_dict(sub)
    ref2.configure(sub, num_heads=cfg.num_heads)
    ref2.add_tensor("final_proj.weight", W)
    ref2.add_tensor("text_decoder_frontend.embed.weight", P["text_decoder_frontend.embed.weight"] * math.sqrt(cfg.model_dim))
    ref2.add_tensor("text_decoder_frontend.pos_encoder", pos)
    ref2.add_token("__fra__", tt.lang_token_idx("fra"))
    ref2.add_token("<unk>", cfg.unk_idx)
    return ref2


@pytest.mark.parametrize("seed,s_enc,stop", [(11, 9, 7), (12, 20, 5), (13, 5, 9), (14, 31, 7)])
def test_generate_sequence_beam_search_matches_oracle(env, seed, s_enc, stop):
    """Beam search with beam_size > 1: the reference's compiled generate_sequence against oracle.beam_search_generate run
    with `compiled_port_rules=True` (the two places where the port as compiled departs from fairseq2 - soft-max
    probabilities instead of log-probabilities after the re-run of the step graph, EOS finalised at any rank - are switched
    on in the oracle; see its docstring).  Everything else is the code the product is checked against: prompt bootstrap and
    its cumulative log-probabilities, first step from beam 0 only, best 2 x beam candidates over (beam, token), refill of the
    live beams, re-order of sequences / scores / KV cache, score / (step+1)^len_penalty, stop at `beam` finished hypotheses,
    final sort.  Every finished hypothesis is compared: ids exact, scores to 2e-4 (ggml's fp16 exp table)."""
    cfg, sd, P, ref, tt, pos = env
    enc = _x((1, s_enc, cfg.model_dim), seed)
    prefix = tt.target_prefix("fra")
    ok, P2, W = _craft_natural_eos(cfg, P, enc, prefix, pos, stop)
    kw = dict(hard_max_seq_len=40, pad_idx=cfg.pad_idx, unk_idx=cfg.unk_idx, bos_idx=cfg.bos_idx, eos_idx=cfg.eos_idx)
    ref2 = _decoder_ref(cfg, sd, P, W, tt, pos)
    compared = 0
    try:
        for beam, len_penalty, normalize in ((2, 1.0, True), (3, 1.0, True), (5, 1.0, True), (4, 0.6, True), (3, 1.0, False)):
            got = ref2.generate_all(enc[0], prefix, beam, len_penalty=len_penalty, normalize_scores=normalize, **kw)
            _, every = ou.beam_search_generate(P2, cfg, enc, torch.tensor([s_enc]), prefix, beam, hard_max_seq_len=40,
                                               len_penalty=len_penalty, normalize_scores=normalize, pos_table=pos,
                                               return_all=True, compiled_port_rules=True)
            want = every[0]
            assert [g[1] for g in got] == [w[1] for w in want], (beam, got, want)
            for (gs, _), (ws, _) in zip(got, want):
                assert abs(gs - ws) < 2e-4 * max(1.0, abs(ws)), (beam, gs, ws)
            compared += len(want)
    finally:
        ref2.close()
    # (14, 31, 7): most beams run into the length limit, which the port as compiled does not close with a forced EOS
    assert compared >= (5 if seed != 14 else 2)


def test_step_rules_equal_compiled_tweak_lprobs():
    """`_tweak_lprobs` (fairseq2.cpp:1269-1305) called directly on random log-probabilities against oracle.tweak_lprobs
    (the function both oracle searches apply every step): every combination of before / at the minimum length, before /
    at the last step the length limit allows, with and without UNK penalty, beams 1-5, EOS at the first, a middle and the
    last vocabulary index.  Exact: the rules only overwrite with -inf and subtract one constant."""
    g = torch.Generator().manual_seed(4)
    n = 0
    for beam in (1, 2, 5):
        for V, pad, unk, eos in ((17, 0, 1, 3), (9, 1, 3, 0), (12, 0, 1, 11), (300, 5, 7, 150)):
            for max_len in (4, 9, 30):
                for step_nr in sorted({1, 2, 3, max_len - 3, max_len - 2}):
                    if step_nr < 1 or step_nr > max_len - 2:
                        continue
                    for min_seq_len in (1, 3, max_len):
                        for unk_penalty in (0.0, 0.75, -1.5):
                            lp = torch.log_softmax(torch.randn(beam, V, generator=g), dim=-1)
                            got = ggml_ref.tweak_lprobs(lp, step_nr, max_len, min_seq_len, unk_penalty, pad, unk, eos)
                            want = ou.tweak_lprobs(lp.clone(), step_nr, max_len, min_seq_len, unk_penalty, pad, unk, eos)
                            assert torch.equal(got, want), (beam, V, max_len, step_nr, min_seq_len, unk_penalty)
                            n += 1
    assert n > 1000


def test_length_rule_executed_on_the_compiled_reference(env):
    """`_determine_max_seq_len` (fairseq2.cpp:1097-1105) observed through generate_sequence: the EOS row is crafted so that
    the greedy hypothesis has exactly 9 tokens; the compiled reference returns it when the limit oracle.max_seq_len_rule
    computes is 9 and returns nothing when it is 8 (the port as compiled has no forced EOS at the limit), for the soft rule
    int(a * S_enc) + b, the hard limit and the a <= 0 case."""
    cfg, sd, P, ref, tt, pos = env
    s_enc = 9
    enc = _x((1, s_enc, cfg.model_dim), 11)
    prefix = tt.target_prefix("fra")
    ok, P2, W = _craft_natural_eos(cfg, P, enc, prefix, pos, 7)
    assert ok
    want = ou.greedy_generate(P2, cfg, enc, torch.tensor([s_enc]), prefix, hard_max_seq_len=64, pos_table=pos)[0]
    assert len(want) == 9
    kw = dict(pad_idx=cfg.pad_idx, unk_idx=cfg.unk_idx, bos_idx=cfg.bos_idx, eos_idx=cfg.eos_idx)
    ref2 = _decoder_ref(cfg, sd, P, W, tt, pos)
    try:
        for soft, hard in (((0.5, 5), 64), ((1, 0), 64), ((1, 200), 9), ((0, 3), 9), ((0.99, 1), 64), ((2.0, 200), 9)):
            limit = ou.max_seq_len_rule(soft[0], soft[1], hard, s_enc)
            assert limit == 9, (soft, hard, limit)
            ids, _, _ = ref2.generate(enc[0], prefix, beam_size=1, soft_max_seq_len=soft, hard_max_seq_len=hard, **kw)
            assert ids == want, (soft, hard)
        for soft, hard in (((0.5, 4), 64), ((1, 200), 8), ((0, 3), 8), ((0.88, 1), 64)):
            assert ou.max_seq_len_rule(soft[0], soft[1], hard, s_enc) == 8, (soft, hard)
            with pytest.raises(RuntimeError, match="no hypothesis"):
                ref2.generate(enc[0], prefix, beam_size=1, soft_max_seq_len=soft, hard_max_seq_len=hard, **kw)
    finally:
        ref2.close()


def test_length_rule_matches_reference_source():
    """max_len = min(hard, int(a * S_enc) + b), prompt included: restated from fairseq2.cpp:1097-1105
    (`_determine_max_seq_len`); fixed expectations next to the executed check above."""
    assert ou.max_seq_len_rule(1, 200, 1024, 63) == 263
    assert ou.max_seq_len_rule(0.5, 4, 200, 6) == 7
    assert ou.max_seq_len_rule(0, 4, 200, 6) == 200
    assert ou.max_seq_len_rule(1, 200, 42, 63) == 42


def test_text_encoder_frontend_and_stack():
    """Text-input tasks (T2TT / T2ST): UnitYModel.encode_text = the shared embedding frontend + the NLLB pre-LN encoder
    stack (models/unity/model.py:138-151) == oracle.encode_text, via the reference's TransformerEmbeddingFrontend_forward
    and StandardTransformerEncoder_forward."""
    cfg, sd, vsd, tt, ct = common.tiny_bundle_text()
    P = ou.Params(sd)
    ref = ggml_ref.GgmlRef(tensor_mem_mb=64)
    try:
        sub = {k: v for k, v in sd.items() if k.startswith("text_encoder.")}
        assert len(sub) == cfg.text_enc_layers * 16 + 2
        ref.add_state_dict(sub)
        ref.configure(sub, num_heads=cfg.num_heads, norm_order=ggml_ref.NORM_ORDER_PRE)
        pos = ou.sinusoidal_table(cfg.text_max_seq_len, cfg.model_dim, 1)
        ref.add_tensor("text_encoder_frontend.embed.weight", P["text_encoder_frontend.embed.weight"] * math.sqrt(cfg.model_dim))
        ref.add_tensor("text_encoder_frontend.pos_encoder", pos)
        toks = tt.create_encoder(task="translation", lang="eng", mode="source")("hello there, my friend").tolist()
        x = ref.embed("text_encoder_frontend", toks, cfg.model_dim)
        got = ref.forward("StandardTransformerEncoder", "text_encoder", x[None])
        want = ou.encode_text(P, cfg, torch.tensor([toks]), None, pos)
        assert torch.allclose(got, want, atol=ATOL_TABLE), float((got - want).abs().max())
    finally:
        ref.close()
