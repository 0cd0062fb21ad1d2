"""Kernel-level parity of the decoder-step kernels in their decode-engine and beam modes, of the engine's bookkeeping
(csrc/k_engine.hip) and of the greedy bookkeeping (csrc/k_misc.hip: step_update, row_swap) against plain float64 / list
restatements, through the C ABI (sc_op_dstep_attention_ex, sc_op_engine_*, sc_op_dstep3_*_ex, sc_op_step_update,
sc_op_row_swap: the launchers the model calls).

Bars (none of them measured on a GPU for this module): attention output 2e-5 absolute at unit-scale inputs and appended K / V
rows 1e-5 (tests/test_dstep_gpu.py); log-probability of the vocabulary projection 1e-4 and LayerNorm output 2e-5
(tests/test_dstep3_gpu.py, tests/test_dstep_gpu.py).  The attention bar was set with at most 200 keys: a float32 torch
restatement of the same soft-max over 1024 unit-scale keys (16 heads, 24 rows, seeds 0..4) stays within 2.9e-7 of float64 on the
CPU, far below half the bar, so the 1023-key cases keep it.  Integer outputs are compared exactly; every buffer a kernel may
not touch holds a sentinel (NaN / a recognisable int) before the call and is compared bit for bit after it.

Every engine / beam attention case is additionally compared BIT FOR BIT with the plain kernel (sc_op_dstep_attention, pinned
against float64 in tests/test_dstep_gpu.py) on the same rows gathered into plain order at one common position per call.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

PAD, UNK, EOS = 0, 1, 3
NAN = float("nan")
TOL_ATTN, TOL_KV, TOL_LPROB, TOL_LN, MIN_GAP = 2e-5, 1e-5, 1e-4, 2e-5, 1e-3
EDGE_POS = [0, 1, 62, 63, 64, 65, 127, 128, 129, 255, 256, 511, 1022, 1023]
ENGINE_MAX_PREFIX = 12   # kernels.h
ROWSWAP_MAX_PAIRS = 64   # kernels.h


def _log(report_dir, name, **kw):
    with open(report_dir / "engine_kernels_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def ints(x):
    return torch.as_tensor(x, dtype=torch.int32)


def bits_equal(a, b):
    """same shape and the same 32-bit patterns (NaN sentinels included)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def attend(q, k, v, heads):
    """float64 single-query attention: q [M], k / v [L][M] -> [M]"""
    L = k.shape[0]
    qh, kh, vh = q.view(heads, 1, 64), k.view(L, heads, 64).transpose(0, 1), v.view(L, heads, 64).transpose(0, 1)
    w = torch.softmax((qh @ kh.transpose(-1, -2)) * 0.125, -1)
    return (w @ vh).reshape(heads * 64)


def slot_tables(nb, n_states, n_lanes, live, seed):
    """Three different permutations: slot s -> row state rid[s] -> lane[s].  Behind `live`: {0, 0} / lane 0, as
    engine_set_slots_kernel writes them; row state 0 and lane 0 are held by LIVE slots (not slot 0)."""
    g = torch.Generator().manual_seed(seed)
    rid = torch.randperm(n_states, generator=g)[:nb].tolist()
    lane = torch.randperm(n_lanes, generator=g)[:nb].tolist()
    if live > 1:  # row state 0 / lane 0 live in the last live slot / the one before
        for tab, s in ((rid, live - 1), (lane, max(live - 2, 0))):
            if 0 in tab:
                tab[tab.index(0)] = tab[s]
            tab[s] = 0
    if n_states > nb and live >= 1 and max(rid[:live]) < nb:
        rid[0] = max(set(range(n_states)) - set(rid))
    return rid, lane


# --------------------------------------------------------------------------------------------------------------------- #
# 1. attention: engine and beam modes
# --------------------------------------------------------------------------------------------------------------------- #
def ref_engine_self(proj, bias, kc_in, vc_in, rid, lane, pos, live, heads):
    """float64 restatement.  Slot s appends its new key / value row at [lane[s]][pos[s]] and attends over keys 0 .. pos[s] of
    that lane.  -> (out [live][M], new key rows [live][M], new value rows [live][M])"""
    M = heads * 64
    qkv = proj.double().sum(0) + bias.double()
    out, kn, vn = [], [], []
    for s in range(live):
        q, k1, v1 = qkv[s, :M], qkv[s, M: 2 * M], qkv[s, 2 * M:]
        p, ln = pos[s], lane[s]
        k = torch.cat([kc_in[ln, :p].double(), k1[None]])
        v = torch.cat([vc_in[ln, :p].double(), v1[None]])
        out.append(attend(q, k, v, heads))
        kn.append(k1)
        vn.append(v1)
    return torch.stack(out), torch.stack(kn), torch.stack(vn)


ENGINE_SELF_CASES = [
    # name, nb, heads, row states, lanes, cap, positions (None: drawn from a few values around the 64-key trips), live, S
    ("edges_cap1024", 24, 16, 40, 24, 1024, EDGE_POS + [1023, 700, 64, 63, 1, 0, 300, 129, 128, 1022], 24, 2),
    ("edges_cap1024_live17", 24, 16, 40, 24, 1024, EDGE_POS + [5, 900, 64], 17, 2),
    ("bench_geometry", 256, 16, 320, 256, 136, None, 256, 2),
    ("bench_geometry_live201", 256, 16, 320, 256, 136, None, 201, 3),
    ("one_slot", 1, 16, 5, 3, 136, [129], 1, 2),
    ("nb64", 64, 16, 80, 64, 136, None, 64, 2),
    ("nb65", 65, 16, 80, 65, 136, None, 60, 1),
    ("heads2", 24, 2, 40, 24, 200, None, 20, 2),
]


@pytest.mark.parametrize("name,nb,heads,n_states,n_lanes,cap,positions,live,S", ENGINE_SELF_CASES, ids=[c[0] for c in ENGINE_SELF_CASES])
def test_engine_self_attention(lib, report_dir, name, nb, heads, n_states, n_lanes, cap, positions, live, S):
    """dattn_kernel<false, false, true>: per-slot row state, position and K / V lane; `live` slots of nb."""
    seed = nb * 131 + heads * 7 + cap + live
    g = torch.Generator().manual_seed(seed)
    M = heads * 64
    rid, lane = slot_tables(nb, n_states, n_lanes, live, seed)
    if positions is None:
        pool = [0, 1, 62, 63, 64, 65, 127, 128, 129, cap - 2, cap - 1, 17]
        positions = [pool[int(i)] for i in torch.randint(0, len(pool), (nb,), generator=g)]
    pos = (positions * (nb // len(positions) + 1))[:nb]
    if live > 1 and pos[max(live - 2, 0)] == 0:
        pos[max(live - 2, 0)] = 64  # the live holder of lane 0 has real keys at row 0: a dead slot's {0, 0} / lane 0 would overwrite them
    if name == "edges_cap1024":
        assert set(EDGE_POS) <= set(pos[:live])
    if nb > 1 and live > 1:
        assert any(len({s, rid[s], lane[s]}) == 3 for s in range(live)) and (n_states <= nb or max(rid[:live]) >= nb)
    proj = torch.randn(S, nb, 3 * M, generator=g)
    bias = torch.randn(3 * M, generator=g) * 0.1
    kc_in = torch.randn(n_lanes, cap, M, generator=g)
    vc_in = torch.randn(n_lanes, cap, M, generator=g)
    held = torch.zeros(n_lanes, dtype=torch.bool)
    for s in range(live):  # uninitialised memory from the slot's own position on; lanes nobody holds: everywhere
        kc_in[lane[s], pos[s]:] = NAN
        vc_in[lane[s], pos[s]:] = NAN
        held[lane[s]] = True
    kc_in[~held] = NAN
    vc_in[~held] = NAN
    rp = [[rid[s], pos[s]] if s < live else [0, 0] for s in range(nb)]
    ln = [lane[s] if s < live else 0 for s in range(nb)]
    ref, kn, vn = ref_engine_self(proj[:, :live], bias, kc_in, vc_in, rid, lane, pos, live, heads)

    d_k, d_v = dev(kc_in), dev(vc_in)
    out = torch.full((nb, M), 123.0, device="cuda")
    check(lib, lib.sc_op_dstep_attention_ex(P(dev(proj)), S, P(dev(bias)), P(d_k), P(d_v), cap, n_lanes, 0, P(None), 0, nb, heads,
                                            P(dev(ints(rp))), P(dev(ints(ln))), P(None), P(None), 1, P(dev(ints([live]))), P(out)))
    out, got_k, got_v = out.cpu(), d_k.cpu(), d_v.cpu()
    assert not torch.isnan(out[:live]).any() and torch.isnan(out[live:]).all(), "a dead slot's output planes were written / a live one's not"
    err = float((out[:live].double() - ref).abs().max())
    idx_l, idx_p = torch.tensor(lane[:live]), torch.tensor(pos[:live])
    ek = float((got_k[idx_l, idx_p].double() - kn).abs().max())
    ev = float((got_v[idx_l, idx_p].double() - vn).abs().max())
    exp_k, exp_v = kc_in.clone(), vc_in.clone()
    exp_k[idx_l, idx_p] = got_k[idx_l, idx_p]
    exp_v[idx_l, idx_p] = got_v[idx_l, idx_p]
    untouched = bits_equal(got_k, exp_k) and bits_equal(got_v, exp_v)
    # the plain kernel on the rows of one position, gathered into plain order (<= 64 rows a call): same bits
    same, calls = True, 0
    for p in sorted(set(pos[:live])):
        slots_p = [s for s in range(live) if pos[s] == p]
        for c0 in range(0, len(slots_p), 64):
            ss = slots_p[c0: c0 + 64]
            pk, pv = dev(kc_in[[lane[s] for s in ss]]), dev(vc_in[[lane[s] for s in ss]])
            po = torch.full((len(ss), M), NAN, device="cuda")
            check(lib, lib.sc_op_dstep_attention(P(dev(proj[:, ss].contiguous())), S, P(dev(bias)), P(pk), P(pv), cap, p, P(None), 0, len(ss), heads, P(po)))
            calls += 1
            same &= bits_equal(po.cpu(), out[ss]) and bits_equal(pk.cpu()[:, p], got_k[[lane[s] for s in ss], p])
            same &= bits_equal(pv.cpu()[:, p], got_v[[lane[s] for s in ss], p])
    _log(report_dir, "engine_self_attention", case=name, nb=nb, heads=heads, cap=cap, live=live, max_pos=max(pos[:live]), err=err, bar=TOL_ATTN,
         ek=ek, ev=ev, bar_kv=TOL_KV, plain_calls=calls, plain_bits=same, cache_untouched=untouched)
    assert err < TOL_ATTN and ek < TOL_KV and ev < TOL_KV, (err, ek, ev)
    assert untouched, "a cache element outside the appended rows changed"
    assert same, "engine mode and the plain kernel differ in bits"


@pytest.mark.parametrize("nb,heads,n_states,s_enc,live,S", [(24, 16, 40, 70, 24, 1), (24, 16, 40, 70, 13, 4), (256, 16, 320, 65, 201, 1), (65, 16, 80, 64, 65, 2),
                                                            (24, 2, 40, 13, 20, 1)])
def test_engine_cross_attention(lib, report_dir, nb, heads, n_states, s_enc, live, S):
    """dattn_kernel<true, false, true>: encoder K / V and their lengths by row state, q and the output by slot."""
    seed = nb * 17 + heads + s_enc + live
    g = torch.Generator().manual_seed(seed)
    M = heads * 64
    rid, _ = slot_tables(nb, n_states, n_states, live, seed)
    edge = [1, 63, 64, 65, s_enc]
    lens = [min(edge[r % 5], s_enc) if r % 3 else 1 + (r * 7) % s_enc for r in range(n_states)]
    for i, s in enumerate(range(min(live, 5))):
        lens[rid[s]] = min(edge[i], s_enc)
    proj = torch.randn(S, nb, M, generator=g)
    bias = torch.randn(M, generator=g) * 0.1
    kv = torch.randn(n_states, s_enc, 2 * M, generator=g)
    kv_in = kv.clone()
    used = set(rid[:live])
    for r in range(n_states):
        kv_in[r, lens[r] if r in used else 0:] = NAN
    q = proj.double().sum(0) + bias.double()
    ref = torch.stack([attend(q[s], kv[rid[s], : lens[rid[s]], :M].double(), kv[rid[s], : lens[rid[s]], M:].double(), heads) for s in range(live)])
    rp = [[rid[s], 5 + s % 5] if s < live else [0, 0] for s in range(nb)]  # the position is not the cross-attention's business
    d_kv = dev(kv_in)
    out = torch.full((nb, M), 123.0, device="cuda")
    check(lib, lib.sc_op_dstep_attention_ex(P(dev(proj)), S, P(dev(bias)), P(d_kv), P(None), s_enc, n_states, 0, P(dev(ints(lens))), 1, nb, heads,
                                            P(dev(ints(rp))), P(None), P(None), P(None), 1, P(dev(ints([live]))), P(out)))
    out = out.cpu()
    assert not torch.isnan(out[:live]).any() and torch.isnan(out[live:]).all()
    err = float((out[:live].double() - ref).abs().max())
    assert bits_equal(d_kv.cpu(), kv_in), "cross-attention wrote to the encoder K / V"
    same = True
    for c0 in range(0, live, 64):
        ss = list(range(c0, min(live, c0 + 64)))
        po = torch.full((len(ss), M), NAN, device="cuda")
        check(lib, lib.sc_op_dstep_attention(P(dev(proj[:, ss].contiguous())), S, P(dev(bias)), P(dev(kv_in[[rid[s] for s in ss]])), P(None), s_enc, 0,
                                             P(dev(ints([lens[rid[s]] for s in ss]))), 1, len(ss), heads, P(po)))
        same &= bits_equal(po.cpu(), out[ss])
    _log(report_dir, "engine_cross_attention", nb=nb, heads=heads, s_enc=s_enc, live=live, err=err, bar=TOL_ATTN, plain_bits=same)
    assert err < TOL_ATTN, err
    assert same, "engine mode and the plain kernel differ in bits"


def beam_anc_table(n_utt, beams, cap, pos, shared, g):
    """anc[b][j]: keys 0 .. shared-1 of every beam of an utterance live in its beam 0's cache row (a shared prefix), later
    keys in a random beam's row of the same utterance, key `pos` in the row itself (a row appends at its own cache row)."""
    nb = n_utt * beams
    anc = torch.full((nb, cap), -1, dtype=torch.int32)
    for b in range(nb):
        u = b // beams
        anc[b, :shared] = u * beams
        anc[b, shared: pos] = u * beams + torch.randint(0, beams, (max(pos - shared, 0),), generator=g).int()
        anc[b, pos] = b
    return anc


@pytest.mark.parametrize("n_utt,beams,heads,cap,pos,S", [(3, 4, 16, 80, 70, 2), (5, 5, 16, 140, 129, 1), (2, 4, 2, 80, 64, 2), (16, 4, 16, 72, 65, 3)])
def test_beam_self_attention_reads_through_the_ancestor_table(lib, report_dir, n_utt, beams, heads, cap, pos, S):
    """dattn_kernel<false, true, false>: key j of row b lives in cache row anc[b][j] (32-bit byte offsets)."""
    g = torch.Generator().manual_seed(n_utt * 100 + beams * 10 + heads + pos)
    nb, M = n_utt * beams, heads * 64
    anc = beam_anc_table(n_utt, beams, cap, pos, 30, g)
    assert any(int(anc[b, j]) != b for b in range(nb) for j in (0, pos - 1))
    proj = torch.randn(S, nb, 3 * M, generator=g)
    bias = torch.randn(3 * M, generator=g) * 0.1
    kc_in = torch.randn(nb, cap, M, generator=g)
    vc_in = torch.randn(nb, cap, M, generator=g)
    kc_in[:, pos:] = NAN
    vc_in[:, pos:] = NAN
    jj = torch.arange(pos)
    gk = torch.stack([kc_in[anc[b, :pos].long(), jj] for b in range(nb)])  # [nb][pos][M]: the keys each row sees
    gv = torch.stack([vc_in[anc[b, :pos].long(), jj] for b in range(nb)])
    qkv = proj.double().sum(0) + bias.double()
    ref = torch.stack([attend(qkv[b, :M], torch.cat([gk[b].double(), qkv[b, None, M: 2 * M]]), torch.cat([gv[b].double(), qkv[b, None, 2 * M:]]), heads)
                       for b in range(nb)])
    d_k, d_v = dev(kc_in), dev(vc_in)
    out = torch.full((nb, M), NAN, device="cuda")
    check(lib, lib.sc_op_dstep_attention_ex(P(dev(proj)), S, P(dev(bias)), P(d_k), P(d_v), cap, nb, pos, P(None), 0, nb, heads, P(None), P(None),
                                            P(dev(anc)), P(None), 1, P(None), P(out)))
    out, got_k, got_v = out.cpu(), d_k.cpu(), d_v.cpu()
    err = float((out.double() - ref).abs().max())
    ek = float((got_k[:, pos].double() - qkv[:, M: 2 * M]).abs().max())
    ev = float((got_v[:, pos].double() - qkv[:, 2 * M:]).abs().max())
    exp_k, exp_v = kc_in.clone(), vc_in.clone()
    exp_k[:, pos], exp_v[:, pos] = got_k[:, pos], got_v[:, pos]
    assert bits_equal(got_k, exp_k) and bits_equal(got_v, exp_v), "a cache element outside the appended rows changed"
    same = True
    for c0 in range(0, nb, 64):
        c1 = min(nb, c0 + 64)
        pk, pv = torch.full((c1 - c0, cap, M), NAN), torch.full((c1 - c0, cap, M), NAN)
        pk[:, :pos], pv[:, :pos] = gk[c0:c1], gv[c0:c1]
        po = torch.full((c1 - c0, M), NAN, device="cuda")
        check(lib, lib.sc_op_dstep_attention(P(dev(proj[:, c0:c1].contiguous())), S, P(dev(bias)), P(dev(pk)), P(dev(pv)), cap, pos, P(None), 0, c1 - c0,
                                             heads, P(po)))
        same &= bits_equal(po.cpu(), out[c0:c1])
    _log(report_dir, "beam_self_attention", n_utt=n_utt, beams=beams, heads=heads, pos=pos, err=err, bar=TOL_ATTN, ek=ek, ev=ev, bar_kv=TOL_KV,
         plain_bits=same)
    assert err < TOL_ATTN and ek < TOL_KV and ev < TOL_KV, (err, ek, ev)
    assert same, "beam mode and the plain kernel differ in bits"


def test_beam_self_attention_byte_offsets_past_2_gib(lib, report_dir):
    """The ancestor-table loads address the caches by 32-bit BYTE offsets.  The launcher admits caches below 4 GiB; this case
    uses 48 rows x 12000 positions x 1024 floats = 2.2 GiB per cache (4.4 GiB for K and V, the device memory the full-size
    model tests hold; a pair just under 4 GiB each would double it), so that the rows from 43 up lie past 2^31 bytes, where a
    signed offset would go wrong.  Only positions 0 .. pos are ever valid; the rest is NaN and must stay NaN."""
    n_utt, beams, heads, cap, pos, S = 12, 4, 16, 12000, 200, 1
    g = torch.Generator().manual_seed(4321)
    nb, M = n_utt * beams, heads * 64
    assert (nb - 1) * cap * M * 4 > 2 ** 31 and nb * cap * M * 4 < 2 ** 32
    anc = beam_anc_table(n_utt, beams, cap, pos, 30, g)
    anc[:, 30:pos] = torch.where(torch.rand(nb, pos - 30, generator=g) < 0.5, ints(nb - 1 - (torch.arange(nb) % beams))[:, None].expand(nb, pos - 30),
                                 anc[:, 30:pos])  # half of the later keys from the LAST utterance's rows: the far end of the cache
    head_k = torch.randn(nb, pos, M, generator=g)
    head_v = torch.randn(nb, pos, M, generator=g)
    proj = torch.randn(S, nb, 3 * M, generator=g)
    d_k = torch.full((nb, cap, M), NAN, device="cuda")
    d_v = torch.full((nb, cap, M), NAN, device="cuda")
    d_k[:, :pos] = head_k.cuda()
    d_v[:, :pos] = head_v.cuda()
    jj = torch.arange(pos)
    qkv = proj.double().sum(0)
    ref = torch.stack([attend(qkv[b, :M], torch.cat([head_k[anc[b, :pos].long(), jj].double(), qkv[b, None, M: 2 * M]]),
                              torch.cat([head_v[anc[b, :pos].long(), jj].double(), qkv[b, None, 2 * M:]]), heads) for b in range(nb)])
    out = torch.full((nb, M), NAN, device="cuda")
    check(lib, lib.sc_op_dstep_attention_ex(P(dev(proj)), S, P(None), P(d_k), P(d_v), cap, nb, pos, P(None), 0, nb, heads, P(None), P(None),
                                            P(dev(anc)), P(None), 1, P(None), P(out)))
    err = float((out.cpu().double() - ref).abs().max())
    ek = float((d_k[:, pos].cpu().double() - qkv[:, M: 2 * M]).abs().max())
    clean = bits_equal(d_k[:, :pos].cpu(), head_k) and bits_equal(d_v[:, :pos].cpu(), head_v)
    clean &= bool(torch.isnan(d_k[:, pos + 1:]).all()) and bool(torch.isnan(d_v[:, pos + 1:]).all())
    del d_k, d_v
    _log(report_dir, "beam_self_attention_large", cache_gib=round(nb * cap * M * 4 / 2 ** 30, 2), launcher_limit_gib=4, err=err, bar=TOL_ATTN, ek=ek,
         cache_untouched=clean)
    assert err < TOL_ATTN and ek < TOL_KV and clean, (err, ek, clean)


@pytest.mark.parametrize("n_utt,beams,heads,s_enc,items,S", [(5, 4, 16, 70, None, 1), (5, 4, 16, 70, [6, 2, 0, 5, 3], 1), (16, 5, 16, 65, None, 2),
                                                             (3, 4, 2, 13, [2, 0, 1], 1)])
def test_beam_cross_attention_shares_the_utterances_encoder_rows(lib, report_dir, n_utt, beams, heads, s_enc, items, S):
    """kv_row_div = beams: the beams of an utterance read one encoder K / V row - cache row b / beams, or kv_item[b / beams]
    (a permuted item table, as after slot compaction).  kv_lens stays per live row."""
    g = torch.Generator().manual_seed(n_utt * 13 + beams + s_enc + (7 if items else 0))
    nb, M = n_utt * beams, heads * 64
    n_items = max(items) + 1 if items else n_utt
    item = items if items else list(range(n_utt))
    edge = [1, 63, 64, 65, s_enc]
    item_len = [min(edge[i % 5], s_enc) for i in range(n_items)]
    lens = [item_len[item[b // beams]] for b in range(nb)]
    proj = torch.randn(S, nb, M, generator=g)
    bias = torch.randn(M, generator=g) * 0.1
    kv = torch.randn(n_items, s_enc, 2 * M, generator=g)
    kv_in = kv.clone()
    for i in range(n_items):
        kv_in[i, item_len[i] if i in item else 0:] = NAN
    q = proj.double().sum(0) + bias.double()
    ref = torch.stack([attend(q[b], kv[item[b // beams], : lens[b], :M].double(), kv[item[b // beams], : lens[b], M:].double(), heads) for b in range(nb)])
    out = torch.full((nb, M), NAN, device="cuda")
    check(lib, lib.sc_op_dstep_attention_ex(P(dev(proj)), S, P(dev(bias)), P(dev(kv_in)), P(None), s_enc, n_items, 0, P(dev(ints(lens))), 1, nb, heads,
                                            P(None), P(None), P(None), P(dev(ints(items)) if items else None), beams, P(None), P(out)))
    out = out.cpu()
    err = float((out.double() - ref).abs().max())
    same = True
    for c0 in range(0, nb, 64):
        bb = list(range(c0, min(nb, c0 + 64)))
        po = torch.full((len(bb), M), NAN, device="cuda")
        check(lib, lib.sc_op_dstep_attention(P(dev(proj[:, bb].contiguous())), S, P(dev(bias)), P(dev(kv_in[[item[b // beams] for b in bb]])), P(None), s_enc,
                                             0, P(dev(ints([lens[b] for b in bb]))), 1, len(bb), heads, P(po)))
        same &= bits_equal(po.cpu(), out[bb])
    _log(report_dir, "beam_cross_attention", n_utt=n_utt, beams=beams, heads=heads, s_enc=s_enc, kv_item=bool(items), err=err, bar=TOL_ATTN, plain_bits=same)
    assert err < TOL_ATTN, err
    assert same, "beam mode and the plain kernel differ in bits"


# --------------------------------------------------------------------------------------------------------------------- #
# 2. vocabulary projection with per-slot rules + engine_finalize_kernel
# --------------------------------------------------------------------------------------------------------------------- #
MIN_EOS_STEP, UNK_PENALTY, BOOST = 5, 20.0, 12.0
KINDS = ["echo", "last_prompt", "no_eos", "forced", "pad_top", "unk_top", "finished", "eos_now", "plain"]
SENT = -7777


def pick(logits, pos, limit):
    """float64 restatement of the step rules for one row (tests/test_dstep3_gpu.py::test_vocab3_fused_argmax, with the row's own
    position and limit) -> (token, log-probability, gap between the best and the second-best admissible logit)."""
    lse = torch.logsumexp(logits, 0)
    if pos == limit - 2:  # forced EOS: scored with its raw logit
        return EOS, float(logits[EOS] - lse), float("inf")
    t = logits.clone()
    t[UNK] -= UNK_PENALTY
    t[PAD] = -float("inf")
    if pos < MIN_EOS_STEP:
        t[EOS] = -float("inf")
    top = torch.topk(t, 2)
    tok = int(torch.nonzero(t == top.values[0])[0])  # lowest index among equal values
    return tok, float(top.values[0] - lse), float(top.values[0] - top.values[1])


def ref_step_close(logits, st, rp, live, cap):
    """Expected EngineRows after engine_finalize_kernel; st = dict of lists (one entry per row state), rp [slots][2].
    -> (state after, expected score increments {row state: lprob}, smallest gap)"""
    out = {k: (v.clone() if torch.is_tensor(v) else list(v)) for k, v in st.items()}
    rp = [list(x) for x in rp]
    inc, gap = {}, float("inf")
    for s in range(live):
        r, pos = rp[s]
        if st["finished"][r]:
            out["tok"][r] = PAD
            continue
        if pos + 1 < st["prefix_len"][r]:
            tok = int(st["hist"][r, pos + 1])
        else:
            tok, lp, gp = pick(logits[s], pos, st["limit"][r])
            gap = min(gap, gp)
            inc[r] = lp
            out["hist"][r, pos + 1] = tok
            if tok == EOS:
                out["finished"][r] = 1
                out["out_len"][r] = pos + 2
        out["tok"][r] = tok
        out["pos"][r] = pos + 1
        rp[s][1] = pos + 1
    return out, rp, inc, gap


_VOCAB_CACHE = {}
# seeds of x / W per shape for which every scored row of every case below has a float64 gap >= MIN_GAP between its two best
# admissible logits (found on the CPU; the tests assert the gap themselves)
SEEDS = {(256, 256102, 1024): 1, (65, 256102, 1024): 0, (160, 10082, 1024): 0, (24, 1200, 128): 0, (64, 256102, 1024): 0, (33, 10082, 1024): 0}


def vocab_case(M, N, K, tie=None):
    """x [M][K], W [N][K] fp16 and the float64 logits; rows of kind no_eos / eos_now / pad_top / unk_top get BOOST times the
    EOS / PAD / UNK row of W added to x so that that logit is the raw arg-max.  tie = (a, b): column b of W a copy of column a
    and every row boosted along it."""
    key = (M, N, K, tie)
    if key not in _VOCAB_CACHE:
        _VOCAB_CACHE.clear()
        g = torch.Generator().manual_seed(SEEDS[(M, N, K)])
        x = torch.randn(M, K, generator=g)
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
        if tie:
            w[tie[1]] = w[tie[0]]
        for m in range(M):
            kind = KINDS[m % len(KINDS)]
            col = tie[0] if tie else {"no_eos": EOS, "eos_now": EOS, "pad_top": PAD, "unk_top": UNK}.get(kind)
            if col is not None:
                x[m] += BOOST * w[col].float() / float(w[col].float().norm()) ** 2
        logits = x.double() @ w.double().t()
        if tie:
            logits[:, tie[1]] = logits[:, tie[0]]  # identical columns: equal bit for bit whatever order the reference's BLAS sums in
        _VOCAB_CACHE[key] = (x, w, logits)
    return _VOCAB_CACHE[key]


def engine_state(M, n_states, cap, live, seed, N):
    """Row states of every kind (KINDS, by slot) at different positions with their own limits; sentinels elsewhere."""
    g = torch.Generator().manual_seed(seed)
    rid, _ = slot_tables(M, n_states, n_states, live, seed)
    st = {k: [SENT] * n_states for k in ("tok", "pos", "finished", "out_len", "limit", "prefix_len")}
    st["hist"] = torch.full((n_states, cap), SENT, dtype=torch.int32)
    st["score"] = (torch.rand(n_states, generator=g) * 6 - 3)
    st["finished"] = [1 if r % 2 else 0 for r in range(n_states)]  # rows outside the live slots: nobody may read or change them
    rp = []
    for s in range(M):
        if s >= live:
            rp.append([0, 0])
            continue
        r, kind = rid[s], KINDS[s % len(KINDS)]
        pos = {"no_eos": 1 + s % (MIN_EOS_STEP - 1), "echo": s % 7, "last_prompt": 1 + s % 6}.get(kind, MIN_EOS_STEP + (s * 5) % (cap - MIN_EOS_STEP - 2))
        st["pos"][r], st["tok"][r], st["finished"][r], st["out_len"][r] = pos, 4 + s, int(kind == "finished"), cap
        st["limit"][r] = pos + 2 if kind == "forced" else pos + 3 + s % 4
        st["prefix_len"][r] = {"echo": pos + 2 + s % 3, "last_prompt": pos + 1}.get(kind, 1 + min(pos, s % 3))
        st["hist"][r, : pos + 1] = 4 + torch.randint(0, N - 4, (pos + 1,), generator=g).int()
        if kind == "echo":
            st["hist"][r, pos + 1] = 4 + (s * 37) % (N - 4)
        rp.append([r, pos])
    return st, rp


def run_step_close(lib, x, w, M, N, K, st, rp, live, n_states, cap):
    d = {k: dev(ints(st[k])) for k in ("tok", "pos", "finished", "out_len", "limit", "prefix_len")}
    d_hist, d_score, d_rp = dev(st["hist"]), dev(st["score"].clone()), dev(ints(rp))
    check(lib, lib.sc_op_engine_step_close(P(dev(x)), P(dev(w)), M, N, K, MIN_EOS_STEP, PAD, EOS, UNK, UNK_PENALTY, P(d_rp), P(dev(ints([live]))), n_states,
                                           cap, P(d["tok"]), P(d["pos"]), P(d["finished"]), P(d["out_len"]), P(d["limit"]), P(d["prefix_len"]), P(d_score),
                                           P(d_hist)))
    got = {k: v.cpu().tolist() for k, v in d.items()}
    got["hist"], got["score"] = d_hist.cpu(), d_score.cpu()
    return got, d_rp.cpu().tolist()


def compare_state(got, got_rp, want, want_rp, st, inc):
    for k in ("tok", "pos", "finished", "out_len", "limit", "prefix_len"):
        assert got[k] == want[k], (k, [(r, a, b) for r, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:8])
    assert torch.equal(got["hist"], want["hist"]), torch.nonzero(got["hist"] != want["hist"])[:8].tolist()
    assert got_rp == want_rp
    err = 0.0
    for r in range(len(st["tok"])):
        if r in inc:
            err = max(err, abs((float(got["score"][r]) - float(st["score"][r])) - inc[r]))
        else:
            assert bits_equal(got["score"][r: r + 1], st["score"][r: r + 1]), f"row state {r}: score changed without a scored token"
    return err


@pytest.mark.parametrize("M,N,K", [(256, 256102, 1024), (65, 256102, 1024), (160, 10082, 1024), (24, 1200, 128)])
@pytest.mark.parametrize("all_live", [True, False])
def test_engine_step_close(lib, report_dir, M, N, K, all_live):
    """launch_vocab3 with the per-slot step rules + engine_finalize_kernel; rows of every kind in one call."""
    live = M if all_live else M - max(3, M // 5)
    n_states, cap = M + M // 4 + 3, 48
    x, w, logits = vocab_case(M, N, K)
    st, rp = engine_state(M, n_states, cap, live, M + N + live, N)
    kinds = {KINDS[s % len(KINDS)] for s in range(live)}
    assert kinds == set(KINDS) and len({st["limit"][rp[s][0]] for s in range(live) if KINDS[s % len(KINDS)] == "forced"}) >= 2
    want, want_rp, inc, gap = ref_step_close(logits, st, rp, live, cap)
    assert gap >= MIN_GAP, f"float64 gap {gap} between the two best admissible logits: pick another seed"
    for s in range(live):  # the premises of the kinds, by the float64 logits
        kind, r = KINDS[s % len(KINDS)], rp[s][0]
        raw = int(logits[s].argmax())
        assert raw == {"no_eos": EOS, "eos_now": EOS, "pad_top": PAD, "unk_top": UNK}.get(kind, raw), (s, kind, raw)
        if kind in ("no_eos", "pad_top", "unk_top"):
            assert want["tok"][r] not in (EOS, PAD, UNK)
        if kind in ("eos_now", "forced"):
            assert want["tok"][r] == EOS and want["finished"][r] == 1 and want["out_len"][r] == rp[s][1] + 2
    got, got_rp = run_step_close(lib, x, w, M, N, K, st, rp, live, n_states, cap)
    err = compare_state(got, got_rp, want, want_rp, st, inc)
    _log(report_dir, "engine_step_close", M=M, N=N, K=K, live=live, scored=len(inc), min_gap=gap, lprob_err=err, bar=TOL_LPROB)
    assert err < TOL_LPROB, err


@pytest.mark.parametrize("M,N,K,tie", [(65, 256102, 1024, (5000, 200000)), (65, 256102, 1024, (7000, 7001)), (24, 1200, 128, (40, 1100)), (160, 10082, 1024, (31, 32))])
def test_engine_step_close_exact_tie_takes_the_lower_index(lib, report_dir, M, N, K, tie):
    """Two identical columns of W: their logits are equal bit for bit, in different tile groups / tiles / lanes."""
    n_states, cap = M + 5, 48
    x, w, logits = vocab_case(M, N, K, tie)
    st, rp = engine_state(M, n_states, cap, M, M + N, N)
    for s in range(M):  # every row chooses freely: past the prompt and the EOS mask, away from its limit, unfinished
        r = rp[s][0]
        st["prefix_len"][r], st["finished"][r], st["limit"][r] = 1, 0, rp[s][1] + 9
        top = torch.topk(logits[s], 3).values
        assert float(top[0]) == float(top[1]) == float(logits[s, tie[0]]) and float(top[1] - top[2]) >= MIN_GAP
    want, want_rp, inc, _ = ref_step_close(logits, st, rp, M, cap)
    assert all(want["tok"][rp[s][0]] == tie[0] for s in range(M))
    got, got_rp = run_step_close(lib, x, w, M, N, K, st, rp, M, n_states, cap)
    err = compare_state(got, got_rp, want, want_rp, st, inc)
    _log(report_dir, "engine_step_close_tie", M=M, N=N, tie=tie, lprob_err=err, bar=TOL_LPROB)
    assert err < TOL_LPROB


@pytest.mark.parametrize("M,N,K", [(64, 256102, 1024), (33, 10082, 1024), (24, 1200, 128)])
@pytest.mark.parametrize("forced", [False, True])
def test_engine_step_close_equals_the_scalar_step_projection(lib, report_dir, M, N, K, forced):
    """Up to 64 rows, all at one position with one limit: tokens and log-probabilities of sc_op_dstep3_argmax, bit for bit."""
    step, cap = 6, 12
    x, w, _ = vocab_case(M, N, K)
    st = {"tok": [9] * M, "pos": [step] * M, "finished": [0] * M, "out_len": [cap] * M, "limit": [step + 2 if forced else cap] * M, "prefix_len": [1] * M,
          "hist": torch.full((M, cap), SENT, dtype=torch.int32), "score": torch.zeros(M)}
    rp = [[s, step] for s in range(M)]
    got, _ = run_step_close(lib, x, w, M, N, K, st, rp, M, M, cap)
    idx = torch.full((M,), SENT, dtype=torch.int32, device="cuda")
    lp = torch.full((M,), NAN, device="cuda")
    check(lib, lib.sc_op_dstep3_argmax(P(dev(x)), P(dev(w)), M, N, K, step, MIN_EOS_STEP, step if forced else -1, PAD, EOS, UNK, UNK_PENALTY, P(idx), P(lp)))
    assert got["tok"] == idx.cpu().tolist() == got["hist"][:, step + 1].tolist()
    assert bits_equal(got["score"], lp.cpu())
    _log(report_dir, "engine_step_close_vs_scalar", M=M, N=N, forced=forced, equal_bits=True)


# --------------------------------------------------------------------------------------------------------------------- #
# 3. engine bookkeeping, slot modes of embed / capture
# --------------------------------------------------------------------------------------------------------------------- #
def test_engine_admit(lib, report_dir):
    n_states, cap, n = 20, 300, ENGINE_MAX_PREFIX  # cap > 256 and not a multiple of it: the history loop's second, partial pass
    g = torch.Generator().manual_seed(5)
    rids = torch.randperm(n_states, generator=g)[:n].tolist()
    recs = torch.full((n, 4 + ENGINE_MAX_PREFIX), SENT, dtype=torch.int32)
    for i, r in enumerate(rids):
        plen = i + 1
        recs[i, :4] = ints([r, 40 + 3 * i, plen, 7 + i])
        recs[i, 4: 4 + plen] = 100 * (i + 1) + torch.arange(plen).int()
    names = ("tok", "pos", "finished", "out_len", "limit", "prefix_len", "enc_lens")
    d = {k: dev(torch.full((n_states,), SENT + j, dtype=torch.int32)) for j, k in enumerate(names)}
    score0 = torch.rand(n_states, generator=g) + 1
    d_score, d_hist = dev(score0.clone()), dev(torch.full((n_states, cap), SENT, dtype=torch.int32))
    check(lib, lib.sc_op_engine_admit(P(dev(recs)), n, n_states, cap, PAD, *[P(d[k]) for k in names], P(d_score), P(d_hist)))
    want = {k: [SENT + j] * n_states for j, k in enumerate(names)}
    w_hist, w_score = torch.full((n_states, cap), SENT, dtype=torch.int32), score0.clone()
    for i, r in enumerate(rids):
        _, limit, plen, enc_len = recs[i, :4].tolist()
        want["tok"][r], want["pos"][r], want["finished"][r], want["out_len"][r] = int(recs[i, 4]), 0, 0, limit
        want["limit"][r], want["prefix_len"][r], want["enc_lens"][r] = limit, plen, enc_len
        w_hist[r] = PAD
        w_hist[r, :plen] = recs[i, 4: 4 + plen]
        w_score[r] = 0.0
    for k in names:
        assert d[k].cpu().tolist() == want[k], k
    assert torch.equal(d_hist.cpu(), w_hist) and bits_equal(d_score.cpu(), w_score)
    _log(report_dir, "engine_admit", records=n, cap=cap, exact=True)


@pytest.mark.parametrize("slots", [24, 256, 300])
@pytest.mark.parametrize("n_live", [0, 1, -1])
def test_engine_set_slots(lib, report_dir, slots, n_live):
    n_live = slots if n_live < 0 else n_live
    n_states = slots + 40
    g = torch.Generator().manual_seed(slots + n_live)
    rids = torch.randperm(n_states, generator=g)[:slots].int()
    lanes = torch.randperm(slots, generator=g).int()
    pos = torch.randint(0, 1000, (n_states,), generator=g).int()
    d_rp, d_lane = dev(torch.full((slots + 2, 2), SENT, dtype=torch.int32)), dev(torch.full((slots + 2,), SENT, dtype=torch.int32))
    d_rows = dev(ints([SENT, SENT]))
    check(lib, lib.sc_op_engine_set_slots(P(dev(torch.cat([rids, lanes]))), n_live, slots, n_states, P(d_rp), P(d_lane), P(dev(pos)), P(d_rows)))
    w_rp = [[int(rids[s]), int(pos[rids[s]])] if s < n_live else [0, 0] for s in range(slots)] + [[SENT, SENT]] * 2
    w_lane = [int(lanes[s]) if s < n_live else 0 for s in range(slots)] + [SENT] * 2
    assert d_rp.cpu().tolist() == w_rp and d_lane.cpu().tolist() == w_lane and d_rows.cpu().tolist() == [n_live, SENT]
    _log(report_dir, "engine_set_slots", slots=slots, n_live=n_live, exact=True)


def test_engine_retire(lib, report_dir):
    n_states, cap, M, n = 26, 40, 64, 20  # 39 hidden rows per row state: more than the launch's 16 row chunks
    g = torch.Generator().manual_seed(11)
    rids = torch.randperm(n_states, generator=g)[:n].tolist()
    out_len = torch.randint(3, cap, (n_states,), generator=g).int()
    out_len[rids[0]], out_len[rids[1]], out_len[rids[2]] = 2, cap, cap  # EOS alone: no valid row; the longest hypothesis
    dst_rows = [int(out_len[r]) - 1 + d for r, d in zip(rids, [5, 0, 12, -2, 3, -1, 0, 7, -3, 2, 1, -5, 4, 0, -1, 6, 2, -2, 9, 0])]
    dst_rows = [max(0, x) for x in dst_rows]
    null = {4, 9}
    score = torch.randn(n_states, generator=g)
    hist = torch.randint(0, 5000, (n_states, cap), generator=g).int()
    hidden = torch.randn(n_states, cap - 1, M, generator=g)
    dsts = [None if i in null else dev(torch.full((dst_rows[i] + 2, M), NAN)) for i in range(n)]
    h_dst = (C.c_void_p * n)(*[d.data_ptr() if d is not None else None for d in dsts])
    h_rid, h_rows = np.asarray(rids, dtype=np.int32), np.asarray(dst_rows, dtype=np.int32)
    d_stage = dev(torch.full((n + 1, 2 + cap), SENT, dtype=torch.int32))
    check(lib, lib.sc_op_engine_retire(h_rid.ctypes.data, h_rows.ctypes.data, C.cast(h_dst, C.c_void_p), n, n_states, cap, M, P(dev(out_len)), P(dev(score)),
                                       P(dev(hist)), P(dev(hidden)), P(d_stage)))
    stage = d_stage.cpu()
    assert stage[n].tolist() == [SENT] * (2 + cap)
    for i, r in enumerate(rids):
        assert int(stage[i, 0]) == int(out_len[r]) and int(stage[i, 1]) == int(score[r: r + 1].view(torch.int32)) and stage[i, 2:].tolist() == hist[r].tolist()
        if dsts[i] is None:
            continue
        got, valid = dsts[i].cpu(), min(int(out_len[r]) - 1, dst_rows[i], cap - 1)
        want = torch.full((dst_rows[i] + 2, M), NAN)
        want[:valid] = hidden[r, :valid]
        want[valid: dst_rows[i]] = 0.0  # exact zeros behind the hypothesis, nothing past dst_rows
        assert bits_equal(got, want), (i, r, valid, dst_rows[i])
    assert any(d < int(out_len[r]) - 1 for r, d in zip(rids, dst_rows)) and any(d > int(out_len[r]) - 1 for r, d in zip(rids, dst_rows))
    _log(report_dir, "engine_retire", records=n, cap=cap, exact=True)


@pytest.mark.parametrize("rows,C_,live,slot_mode", [(24, 1024, 17, True), (24, 128, 24, True), (65, 1024, 40, True), (24, 1024, 24, False)])
def test_embed3_slot_mode(lib, report_dir, rows, C_, live, slot_mode):
    """x = embed[tok] * scale + pos_table[pos]: slot s takes the token of row state slot_rp[s].x and the position slot_rp[s].y.
    The kernel's expression is one fp32 multiply and one fp32 add (or one fused multiply-add): two roundings of at most half
    an ulp each, of the product and of the sum.  Bar: one fp32 ulp at the larger of |product| and |sum|, against float64."""
    n_states, n_pos, vocab, scale = rows + 16, 1024, 500, math.sqrt(C_)
    g = torch.Generator().manual_seed(rows + C_ + live)
    rid, _ = slot_tables(rows, n_states, n_states, live, rows + C_)
    tok = torch.randint(0, vocab, (n_states,), generator=g).int()
    embed = (torch.randn(vocab, C_, generator=g) * 0.05).half()
    table = torch.randn(n_pos, C_, generator=g)
    pos = [EDGE_POS[s % len(EDGE_POS)] for s in range(rows)]
    rp = [[rid[s], pos[s]] if s < live else [0, 0] for s in range(rows)]
    x = torch.full((rows, C_), 5.0, device="cuda")
    check(lib, lib.sc_op_dstep3_embed_ex(P(dev(tok)), P(dev(embed)), scale, P(dev(table)), 129, P(dev(ints(rp))) if slot_mode else P(None),
                                         P(dev(ints([live]))) if slot_mode else P(None), rows, C_, n_states, n_pos, vocab, P(x)))
    x = x.cpu()
    n = live if slot_mode else rows
    src = [(rid[s], pos[s]) if slot_mode else (s, 129) for s in range(n)]
    prod = torch.stack([embed[int(tok[r])].double() * float(np.float32(scale)) for r, _ in src])
    ref = prod + torch.stack([table[p].double() for _, p in src])
    ulp = torch.from_numpy(np.spacing(np.maximum(prod.abs().numpy(), ref.abs().numpy()).astype(np.float32))).double()
    worst = float(((x[:n].double() - ref).abs() / ulp).max())
    assert torch.isnan(x[n:]).all(), "a slot behind the live rows was embedded"
    _log(report_dir, "embed3_slot_mode", rows=rows, C=C_, live=live, slot_mode=slot_mode, err_ulp=worst, bar_ulp=1.0)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("rows,C_,live,slot_mode", [(24, 1024, 17, True), (24, 128, 24, True), (65, 1024, 40, True), (24, 1024, 24, False)])
def test_reduce3_capture_slot_mode(lib, report_dir, rows, C_, live, slot_mode):
    """The captured decoder output of slot s lands at hidden[row state][position]; nothing for position >= cap - 1."""
    n_states, cap, S = rows + 16, 12, 2
    g = torch.Generator().manual_seed(rows * 3 + C_ + live)
    rid, _ = slot_tables(rows, n_states, n_states, live, rows + C_ + 1)
    pos = [[0, 10, 11, 12, 5, 300][s % 6] for s in range(rows)]  # 10 = the last captured position, 11 = cap - 1 and beyond: not captured
    rp = [[rid[s], pos[s]] if s < live else [0, 0] for s in range(rows)]
    partial = torch.randn(S, rows, C_, generator=g)
    bias, x0 = torch.randn(C_, generator=g) * 0.1, torch.randn(rows, C_, generator=g)
    gam, bet = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g) * 0.1
    xr = x0.double() + partial.double().sum(0) + bias.double()
    hr = F.layer_norm(xr, (C_,), gam.double(), bet.double(), 1e-5)
    d_x, d_h = dev(x0.clone()), dev(torch.full((rows, C_), NAN))
    d_hid = dev(torch.full((n_states, cap - 1, C_), NAN))
    scalar_pos = 7
    check(lib, lib.sc_op_dstep3_reduce_capture_ex(P(dev(partial)), S, P(dev(bias)), P(d_x), P(dev(gam)), P(dev(bet)), P(d_h), P(d_hid), (cap - 1) * C_, cap - 1,
                                                  scalar_pos, P(dev(ints(rp))) if slot_mode else P(None), P(dev(ints([live]))) if slot_mode else P(None), rows,
                                                  C_, n_states))
    x, h, hid = d_x.cpu(), d_h.cpu(), d_hid.cpu()
    n = live if slot_mode else rows
    ex, eh = float((x[:n].double() - xr[:n]).abs().max()), float((h[:n].double() - hr[:n]).abs().max())
    assert bits_equal(x[n:], x0[n:]) and torch.isnan(h[n:]).all(), "a slot behind the live rows was reduced"
    want = torch.full((n_states, cap - 1, C_), NAN)
    for s in range(n):
        r, p = (rid[s], pos[s]) if slot_mode else (s, scalar_pos)
        if p < cap - 1:
            want[r, p] = h[s]  # the very row the kernel wrote as d_h
    assert bits_equal(hid, want), "captured rows: wrong owner / position, or a row written that may not be"
    _log(report_dir, "reduce3_capture", rows=rows, C=C_, live=live, slot_mode=slot_mode, err_x=ex, err_h=eh, bar=TOL_LN)
    assert ex < 1e-5 and eh < TOL_LN, (ex, eh)


# --------------------------------------------------------------------------------------------------------------------- #
# 4. greedy bookkeeping
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("nb", [1, 40, 300])
@pytest.mark.parametrize("mode", ["mixed", "all_done", "no_score"])
def test_step_update(lib, report_dir, nb, mode):
    pos, ld = 6, 10
    g = torch.Generator().manual_seed(nb)
    tok = torch.randint(4, 900, (nb,), generator=g).int()
    tok[::3] = EOS
    fin = (torch.arange(nb) % 4 == 1).int()
    if mode == "all_done":
        fin[tok != EOS] = 1
    lprob, score = -torch.rand(nb, generator=g), torch.randn(nb, generator=g)
    out_len = torch.full((nb,), 99, dtype=torch.int32)
    d_tok, d_hist, d_fin, d_len = dev(tok.clone()), dev(torch.full((nb, ld), SENT, dtype=torch.int32)), dev(fin.clone()), dev(out_len.clone())
    d_score, d_flag = dev(score.clone()), dev(ints([0, SENT]))
    check(lib, lib.sc_op_step_update(P(d_tok), P(d_hist), ld, P(d_fin), P(d_len), P(dev(lprob)), P(None) if mode == "no_score" else P(d_score), nb, pos, PAD,
                                     EOS, P(d_flag)))
    w_tok, w_fin, w_len, w_score, goes_on = tok.tolist(), fin.tolist(), out_len.tolist(), score.clone(), 0
    for b in range(nb):
        if fin[b]:
            w_tok[b] = PAD
        else:
            if mode != "no_score":
                w_score[b] = score[b] + lprob[b]  # one fp32 addition
            if w_tok[b] == EOS:
                w_fin[b], w_len[b] = 1, pos + 2
            else:
                goes_on = 1
    w_hist = torch.full((nb, ld), SENT, dtype=torch.int32)
    w_hist[:, pos + 1] = ints(w_tok)
    assert d_tok.cpu().tolist() == w_tok and d_fin.cpu().tolist() == w_fin and d_len.cpu().tolist() == w_len
    assert torch.equal(d_hist.cpu(), w_hist) and bits_equal(d_score.cpu(), w_score) and d_flag.cpu().tolist() == [goes_on, SENT]
    assert goes_on == (0 if mode == "all_done" else int(any(not f and t != EOS for f, t in zip(fin.tolist(), tok.tolist()))))
    _log(report_dir, "step_update", nb=nb, mode=mode, exact=True)


@pytest.mark.parametrize("pairs,layers,filled,with_hidden", [(1, 1, 0, True), (ROWSWAP_MAX_PAIRS, 1, 1, True), (5, 24, 12, True), (5, 24, 5, False),
                                                            (ROWSWAP_MAX_PAIRS, 24, 12, False), (3, 1, 12, True)])
def test_row_swap(lib, report_dir, pairs, layers, filled, with_hidden):
    """Self K / V rows 0 .. filled-1 and the whole encoder K / V go src -> dst, the small state and the history are exchanged,
    the captured outputs are exchanged up to min(filled, cap - 1); rows in no pair and K / V rows behind `filled` keep theirs."""
    M, cap, s_enc = 64, 12, 5
    n_rows = 2 * pairs + 3
    g = torch.Generator().manual_seed(pairs * 100 + layers + filled)
    perm = torch.randperm(n_rows, generator=g).tolist()
    src, dst = perm[:pairs], perm[pairs: 2 * pairs]
    k, v = torch.randn(layers, n_rows, cap, M, generator=g), torch.randn(layers, n_rows, cap, M, generator=g)
    k[:, :, filled:], v[:, :, filled:] = NAN, NAN  # rows behind `filled` are uninitialised memory
    cross = torch.randn(layers, n_rows, s_enc, 2 * M, generator=g)
    names = ("tok", "finished", "out_len", "enc_lens")
    st = {n_: torch.randint(0, 1000, (n_rows,), generator=g).int() for n_ in names}
    lprob, score = torch.randn(n_rows, generator=g), torch.randn(n_rows, generator=g)
    hist = torch.randint(0, 1000, (n_rows, cap), generator=g).int()
    hidden = torch.randn(n_rows, cap - 1, M, generator=g)
    d_k, d_v, d_c = dev(k), dev(v), dev(cross)
    d = {n_: dev(st[n_].clone()) for n_ in names}
    d_lp, d_sc, d_hist, d_hid = dev(lprob.clone()), dev(score.clone()), dev(hist.clone()), dev(hidden.clone())
    h_src, h_dst = np.asarray(src, dtype=np.int32), np.asarray(dst, dtype=np.int32)
    check(lib, lib.sc_op_row_swap(P(d_k), P(d_v), P(d_c), layers, pairs, h_src.ctypes.data, h_dst.ctypes.data, n_rows, M, cap, s_enc, filled, *[P(d[n_]) for n_ in names],
                                  P(d_lp), P(d_sc), P(d_hist), P(d_hid) if with_hidden else P(None)))
    w_k, w_v, w_c = k.clone(), v.clone(), cross.clone()
    w = {n_: st[n_].clone() for n_ in names}
    w_lp, w_sc, w_hist, w_hid = lprob.clone(), score.clone(), hist.clone(), hidden.clone()
    hf = min(filled, cap - 1)
    for s_, d_ in zip(src, dst):
        w_k[:, d_, :filled], w_v[:, d_, :filled], w_c[:, d_] = k[:, s_, :filled], v[:, s_, :filled], cross[:, s_]
        for t in list(w.values()) + [w_lp, w_sc, w_hist]:
            t[[s_, d_]] = t[[d_, s_]]
        if with_hidden:
            w_hid[s_, :hf], w_hid[d_, :hf] = hidden[d_, :hf], hidden[s_, :hf]
    assert bits_equal(d_k.cpu(), w_k) and bits_equal(d_v.cpu(), w_v) and bits_equal(d_c.cpu(), w_c)
    for n_ in names:
        assert torch.equal(d[n_].cpu(), w[n_]), n_
    assert bits_equal(d_lp.cpu(), w_lp) and bits_equal(d_sc.cpu(), w_sc) and torch.equal(d_hist.cpu(), w_hist) and bits_equal(d_hid.cpu(), w_hid)
    _log(report_dir, "row_swap", pairs=pairs, layers=layers, filled=filled, hidden=with_hidden, exact=True)


