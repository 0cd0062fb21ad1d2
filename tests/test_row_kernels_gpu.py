"""The row kernels between the products (k_norm.hip, k_misc.hip) by themselves, through the sc_op_* hooks of
csrc/api_ops.hip: LayerNorm in its three launch forms, the NAR T2U / vocoder front-end glue, the duration rule, the
packed-item tables and the v1 Conformer glue.

References are numpy float64; numpy float32 where the kernel's result is determined bit for bit (copies, single adds,
products with a power of two, the reference's `(x + PE) - x` cancellation).  Where a tolerance is needed it is not a
constant: the float32 CPU restatement (torch) is measured against float64 on the same inputs, and the kernel may be 4x
that far away (another summation order).  Each test appends the figures to row_kernels_report.txt.

Every `run_*` function below is one hook call on numpy arrays: outputs are pre-filled with a sentinel, the whole buffer
(padding columns included) comes back."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
SENT = f32(-7777.0)         # what a kernel must leave alone
SENT_H = np.float16(-77.0)
SENT_I = np.int32(-777)
ACT_NONE, ACT_RELU, ACT_SILU, ACT_GELU = 0, 1, 2, 4  # enum Act, kernels.h
U23 = 2.0 ** -23


def _log(report_dir, name, **kw):
    with open(report_dir / "row_kernels_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def _d(a):
    return None if a is None else dev(torch.from_numpy(np.ascontiguousarray(a)))


def _out(shape, fill, dtype):
    return dev(torch.from_numpy(np.full(shape, fill, dtype=dtype)))


def _np(t):
    return None if t is None else t.cpu().numpy()


def _i32(a):
    return np.asarray(a, dtype=np.int32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# --------------------------------------------------------------------------------------------------------------------- #
# one hook call each
# --------------------------------------------------------------------------------------------------------------------- #
def run_layernorm(lib, x, g, b, C, act=ACT_NONE, mode="plain", ldy=None, ldh=None, lens=None, tpb=1):
    """x [rows][ldx] -> (y [rows][ldy] | None, hi [rows][ldh] | None, lo | None); mode plain | split | both"""
    rows, ldx = x.shape
    ldy, ldh = ldy or C, ldh or C
    y = _out((rows, ldy), SENT, f32) if mode != "split" else None
    hi = _out((rows, ldh), SENT_H, np.float16) if mode != "plain" else None
    lo = _out((rows, ldh), SENT_H, np.float16) if mode != "plain" else None
    check(lib, lib.sc_op_layernorm_ex(P(_d(x)), ldx, P(_d(g)), P(_d(b)), P(y), ldy, P(hi), P(lo), ldh, rows, C, act,
                                      P(_d(None if lens is None else _i32(lens))), tpb))
    return _np(y), _np(hi), _np(lo)


def run_layernorm2(lib, x, ga, ba, gb, bb):
    rows, C = x.shape
    y, hi, lo = _out((rows, C), SENT, f32), _out((rows, C), SENT_H, np.float16), _out((rows, C), SENT_H, np.float16)
    check(lib, lib.sc_op_layernorm2(P(_d(x)), P(_d(ga)), P(_d(ba)), P(_d(gb)), P(_d(bb)), P(y), P(hi), P(lo), rows, C, 1))
    return _np(y), _np(hi), _np(lo)


def run_gather_rows(lib, src, idx, C, ldd, add=None, rows_per_item=1):
    rows = len(idx)
    dst = _out((rows, ldd), SENT, f32)
    check(lib, lib.sc_op_gather_rows(P(_d(src)), src.shape[1], P(_d(_i32(idx))), P(_d(add)), 0 if add is None else add.shape[1],
                                     rows_per_item, P(dst), ldd, rows, C))
    return _np(dst)


def run_embed_tokens(lib, tok, emb, scale, pe, pos, tpb, ldo):
    rows, M = len(tok), emb.shape[1]
    out = _out((rows, ldo), SENT, f32)
    check(lib, lib.sc_op_embed_tokens(P(_d(_i32(tok))), rows, P(_d(emb)), M, float(scale), P(_d(pe)),
                                      P(_d(None if pos is None else _i32([pos, -1, -1, -1]))), tpb, P(out), ldo))
    return _np(out)


def run_char_embed_add(lib, seqs, M, ids, emb, pe, tpb, alpha, scale):
    d = _d(seqs)
    check(lib, lib.sc_op_char_embed_add(P(d), seqs.shape[1], P(_d(_i32(ids))), P(_d(emb)), P(_d(pe)), tpb, float(alpha), float(scale),
                                        seqs.shape[0], M))
    return _np(d)


def run_pos_add(lib, seqs, M, pe, tpb, row_t, alpha):
    d = _d(seqs)
    check(lib, lib.sc_op_pos_add(P(d), seqs.shape[1], P(_d(pe)), tpb, P(_d(None if row_t is None else _i32(row_t))), float(alpha),
                                 seqs.shape[0], M))
    return _np(d)


def run_durations(lib, h, H, w, b, tpb, lens, factor, min_dur):
    rows = h.shape[0]
    out = _out((rows,), SENT_I, np.int32)
    check(lib, lib.sc_op_durations(P(_d(h)), h.shape[1], P(_d(w)), P(_d(b)), rows, H, tpb, P(_d(None if lens is None else _i32(lens))),
                                   float(factor), min_dur, P(out)))
    return _np(out)


def run_vocoder_embed(lib, units, nb, T, dic, lang, lang_idx, spkr, spkr_idx, item_off):
    rows = len(units)
    E, Lg, Sp = dic.shape[1], lang.shape[1], spkr.shape[1]
    out = _out((rows + 1, Lg + E + Sp), SENT, f32)  # one row more than the kernel owns
    check(lib, lib.sc_op_vocoder_embed(P(_d(_i32(units))), nb, T, P(_d(dic)), E, P(_d(lang)), Lg, P(_d(_i32(lang_idx))), P(_d(spkr)), Sp,
                                       P(_d(_i32(spkr_idx))), P(out), P(_d(None if item_off is None else _i32(item_off))), rows))
    return _np(out)


def run_item_row_pos(lib, item_off, mul, rows):
    out = _out((rows + 1, 2), SENT_I, np.int32)
    check(lib, lib.sc_op_item_row_pos(P(_d(_i32(item_off))), len(item_off) - 1, mul, rows, P(out)))
    return _np(out)


def run_scatter_items(lib, src, item_off, item_of, mul, longest, n_dst, stride):
    dst = _out((n_dst, stride), SENT, f32)
    check(lib, lib.sc_op_scatter_items(P(_d(src)), P(_d(_i32(item_off))), P(_d(_i32(item_of))), len(item_of), mul, longest, stride, P(dst)))
    return _np(dst)


def run_glu_dwconv_ex(lib, x, w, lens, left, bn):
    nb, T, C2 = x.shape
    C, K = C2 // 2, w.shape[1]
    y = _out((nb, T, C), SENT, f32)
    g, b, mu, var = bn if bn is not None else (None,) * 4
    check(lib, lib.sc_op_glu_dwconv_ex(P(_d(x)), P(_d(w)), P(y), nb, T, C, K, P(_d(None if lens is None else _i32(lens))), left, P(_d(g)),
                                       P(_d(b)), P(_d(mu)), P(_d(var))))
    return _np(y)


def run_glu_dwconv(lib, x, w, lens):
    nb, T, C2 = x.shape
    y = _out((nb, T, C2 // 2), SENT, f32)
    check(lib, lib.sc_op_glu_dwconv(P(_d(x)), P(_d(w)), P(y), nb, T, C2 // 2, w.shape[1], P(_d(None if lens is None else _i32(lens)))))
    return _np(y)


def run_relpos_table(lib, S, M):
    out = _out((2 * S, M), SENT, f32)  # one row more than the table
    check(lib, lib.sc_op_relpos_table(S, M, P(out)))
    return _np(out)


# --------------------------------------------------------------------------------------------------------------------- #
# LayerNorm
# --------------------------------------------------------------------------------------------------------------------- #
_erf = np.frompyfunc(math.erf, 1, 1)


def act64(v, act):
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_SILU:
        return v / (1.0 + np.exp(-v))
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)).astype(f64))
    return v


def layernorm64(x, g, b, act=ACT_NONE):
    x = x.astype(f64)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return act64((x - mean) / np.sqrt(var + 1e-5) * g.astype(f64) + b.astype(f64), act)


def layernorm32(x, g, b, act=ACT_NONE):
    """the float32 CPU restatement whose own error sets the bar"""
    y = F.layer_norm(torch.from_numpy(x), (x.shape[-1],), torch.from_numpy(g), torch.from_numpy(b), 1e-5)
    y = {ACT_NONE: lambda t: t, ACT_RELU: F.relu, ACT_SILU: F.silu, ACT_GELU: F.gelu}[act](y)
    return y.numpy()


LN_C = [4, 252, 256, 260, 1024, 1028, 4096]  # layernorm_kernel<1> up to 256, <4> up to 1024, <16> above; 260: a float4 tail
LN_ROWS = [1, 3, 4, 5, 9]                    # four rows per workgroup
# exactly summable in float32 at every C here, so the mean is the constant itself and the row must come out as beta
LN_CONSTANTS = [0.0, 1.5, -7.0, 1000.0, 0.25, -0.5, 3.0, 64.0, -1000.0]
LN_FAMILIES = ("randn", "mean1e3", "const")
LN_ACTS = (ACT_NONE, ACT_RELU, ACT_SILU, ACT_GELU)


def ln_family(family, rows, C, rng):
    if family == "randn":
        return (rng.standard_normal((rows, C)) * 3 + 0.5).astype(f32)
    if family == "mean1e3":
        return (rng.standard_normal((rows, C)) + 1e3).astype(f32)
    return np.repeat(np.asarray(LN_CONSTANTS[:rows], dtype=f32)[:, None], C, axis=1)


def ln_params(C, rng):
    return (rng.random(C) + 0.5).astype(f32), (rng.standard_normal(C) * 0.1).astype(f32)


@functools.lru_cache(maxsize=None)
def ln_values_case(C):
    """gamma, beta and the rows of each family at every row count, with the float64 result and float32 torch's error per
    (family, act): computed once, read by every test that needs them"""
    rng = np.random.default_rng(1000 + C)
    g, b = ln_params(C, rng)
    xs = {family: [ln_family(family, rows, C, rng) for rows in LN_ROWS] for family in LN_FAMILIES}
    refs = {(f, a): [layernorm64(x, g, b, a) for x in xs[f]] for f in LN_FAMILIES for a in LN_ACTS}
    err32 = {k: max(float(np.abs(layernorm32(x, g, b, k[1]) - r).max()) for x, r in zip(xs[k[0]], r_)) for k, r_ in refs.items()}
    return g, b, xs, refs, err32


def ln_err32(family, C, act):
    """The float32 CPU error the kernel is judged against.  randn / mean1e3: the worst over the 22 rows of this C.  const:
    the rows come out as act(beta) whatever the constant, C distinct values per width (four at C = 4), so the worst is taken
    over the seven widths together; without an activation it is 0 at every width."""
    if family == "const":
        return max(ln_values_case(c)[4][family, act] for c in LN_C)
    return ln_values_case(C)[4][family, act]


@pytest.mark.parametrize("C", LN_C)
def test_layernorm_values_against_float64(lib, report_dir, C):
    """Every template switch point, the 4-rows-per-workgroup tail and every activation, on three input families.  The bound
    is 4x the worst error of float32 torch on the same rows (ln_err32); the constant rows have an exact float32 mean, so
    without an activation torch gives beta exactly and so must the kernel."""
    g, b, xs, refs, _ = ln_values_case(C)
    for family in LN_FAMILIES:
        for act in LN_ACTS:
            err32 = ln_err32(family, C, act)
            err = 0.0
            for x, r in zip(xs[family], refs[family, act]):
                y, _, _ = run_layernorm(lib, x, g, b, C, act)
                assert np.isfinite(y).all(), (family, act, x.shape)
                err = max(err, float(np.abs(y - r).max()))
            _log(report_dir, "layernorm_values", C=C, family=family, act=act, kernel_err=f"{err:.3e}", f32_cpu_err=f"{err32:.3e}",
                 bound=f"{4 * err32:.3e}")
            assert err <= 4 * err32, (family, act, err, err32)
            assert family != "const" or act != ACT_NONE or err32 == 0.0  # beta itself


def _ln_case(C, rows, seed):
    rng = np.random.default_rng(seed)
    g, b = ln_params(C, rng)
    return ln_family("randn", rows, C, rng), g, b


def _padded(x, ld, fill=np.nan):
    out = np.full((x.shape[0], ld), fill, dtype=x.dtype)
    out[:, : x.shape[1]] = x
    return out


@pytest.mark.parametrize("C", [4, 260, 1028, 4096])
@pytest.mark.parametrize("mode", ["plain", "split", "both"])
def test_layernorm_strides(lib, report_dir, C, mode):
    """ldx = C + 4 (NaN behind the row: a load one float4 too far shows), ldy = C + 8, ldh = C + 12: the result is the
    contiguous one bit for bit and the columns behind C keep what they held."""
    x, g, b = _ln_case(C, 5, 2000 + C)
    want = run_layernorm(lib, x, g, b, C, ACT_SILU, mode)
    got = run_layernorm(lib, _padded(x, C + 4), g, b, C, ACT_SILU, mode, ldy=C + 8, ldh=C + 12)
    for w, o, sent in zip(want, got, (SENT, SENT_H, SENT_H)):
        assert (w is None) == (o is None)
        if w is not None:
            assert same_bits(o[:, :C], w)
            assert (o[:, C:] == sent).all()
    _log(report_dir, "layernorm_strides", C=C, mode=mode, mismatches=0)


@pytest.mark.parametrize("C", LN_C)
@pytest.mark.parametrize("act", [ACT_NONE, ACT_GELU])
def test_layernorm_planes_are_the_split_of_the_rows(lib, report_dir, C, act):
    """hi = half(y), lo = half(y - float(hi)) of the plain launch's y, bit for bit (k_norm.hip: two round-to-nearest-even
    conversions, the difference exact in float32); `both` gives the same planes and the same y."""
    x, g, b = _ln_case(C, 5, 3000 + C)
    y, _, _ = run_layernorm(lib, x, g, b, C, act)
    hi = y.astype(np.float16)
    lo = (y - hi.astype(f32)).astype(np.float16)
    _, shi, slo = run_layernorm(lib, x, g, b, C, act, "split")
    by, bhi, blo = run_layernorm(lib, x, g, b, C, act, "both")
    assert same_bits(shi, hi) and same_bits(slo, lo)
    assert same_bits(bhi, hi) and same_bits(blo, lo) and same_bits(by, y)
    worst = float(np.abs(hi.astype(f64) + lo.astype(f64) - y).max())
    _log(report_dir, "layernorm_planes", C=C, act=act, mismatches=0, split_residual=f"{worst:.3e}")


@pytest.mark.parametrize("C", [256, 260, 1028])
def test_layernorm_length_mask(lib, report_dir, C):
    """lens = [7, 0, 3] at 7 rows per item.  plain: masked rows +0, live rows as without a mask; split: masked planes +0;
    both: masked planes +0 while the fp32 rows hold the LayerNorm of every row.  NaN in the masked input rows (plain, split)
    reaches nothing."""
    tpb, lens = 7, [7, 0, 3]
    x, g, b = _ln_case(C, 3 * tpb, 4000 + C)
    live = np.concatenate([np.arange(tpb) < n for n in lens])
    y0, _, _ = run_layernorm(lib, x, g, b, C)
    _, hi0, lo0 = run_layernorm(lib, x, g, b, C, mode="split")
    xn = x.copy()
    xn[~live] = np.nan
    y, _, _ = run_layernorm(lib, xn, g, b, C, lens=lens, tpb=tpb)
    assert same_bits(y[live], y0[live]) and same_bits(y[~live], np.zeros_like(y[~live]))
    _, hi, lo = run_layernorm(lib, xn, g, b, C, mode="split", lens=lens, tpb=tpb)
    for p, p0 in ((hi, hi0), (lo, lo0)):
        assert same_bits(p[live], p0[live]) and same_bits(p[~live], np.zeros_like(p[~live]))
    by, bhi, blo = run_layernorm(lib, x, g, b, C, mode="both", lens=lens, tpb=tpb)
    assert same_bits(by, y0)
    for p, p0 in ((bhi, hi0), (blo, lo0)):
        assert same_bits(p[live], p0[live]) and same_bits(p[~live], np.zeros_like(p[~live]))
    _log(report_dir, "layernorm_length_mask", C=C, live_rows=int(live.sum()), mismatches=0)


@pytest.mark.parametrize("C", [256, 1024])
def test_layernorm2_against_float64(lib, report_dir, C):
    """layernorm2_kernel by itself: y = LN_a(x) and the planes of LN_b(y), each against float64 with the bound of the
    values test (float32 torch through the same two steps, x4)."""
    rng = np.random.default_rng(5000 + C)
    x = ln_family("randn", 5, C, rng)
    ga, ba = ln_params(C, rng)
    gb, bb = ln_params(C, rng)
    y64 = layernorm64(x, ga, ba)
    z64 = layernorm64(y64, gb, bb)
    y32 = layernorm32(x, ga, ba)
    e32_y, e32_z = float(np.abs(y32 - y64).max()), float(np.abs(layernorm32(y32, gb, bb) - z64).max())
    y, hi, lo = run_layernorm2(lib, x, ga, ba, gb, bb)
    e_y, e_z = float(np.abs(y - y64).max()), float(np.abs(hi.astype(f64) + lo.astype(f64) - z64).max())
    _log(report_dir, "layernorm2", C=C, kernel_err_y=f"{e_y:.3e}", f32_cpu_err_y=f"{e32_y:.3e}", kernel_err_planes=f"{e_z:.3e}",
         f32_cpu_err_planes=f"{e32_z:.3e}")
    assert e_y <= 4 * e32_y and e_z <= 4 * e32_z


# --------------------------------------------------------------------------------------------------------------------- #
# gathers and embeddings
# --------------------------------------------------------------------------------------------------------------------- #
GATHER_IDX = [0, 5, -1, 2, 2, 5, -1, 0, 3, 1]  # repeats, -1, the first and the last source row; two items of five rows


@pytest.mark.parametrize("C", [4, 80, 1024, 1028])
def test_gather_rows_is_a_bit_copy(lib, report_dir, C):
    rng = np.random.default_rng(6000 + C)
    src = _padded(rng.standard_normal((6, C)).astype(f32), C + 4)
    got = run_gather_rows(lib, src, GATHER_IDX, C, C + 8)
    want = np.stack([src[i, :C] if i >= 0 else np.zeros(C, f32) for i in GATHER_IDX])
    assert same_bits(got[:, :C], want) and (got[:, C:] == SENT).all()
    _log(report_dir, "gather_rows", C=C, mismatches=0)


@pytest.mark.parametrize("C", [4, 80, 1024, 1028])
@pytest.mark.parametrize("rows_per_item", [1, 5])
def test_gather_rows_add(lib, report_dir, C, rows_per_item):
    """dst[r] = src[idx[r]] + add[r // rows_per_item]: one float32 add; a -1 row is +0, not the item's vector"""
    rng = np.random.default_rng(6100 + C)
    src = _padded(rng.standard_normal((6, C)).astype(f32), C + 4)
    add = _padded(rng.standard_normal((len(GATHER_IDX) // rows_per_item, C)).astype(f32), C + 4)
    got = run_gather_rows(lib, src, GATHER_IDX, C, C + 8, add, rows_per_item)
    want = np.stack([src[i, :C] + add[r // rows_per_item, :C] if i >= 0 else np.zeros(C, f32) for r, i in enumerate(GATHER_IDX)])
    assert same_bits(got[:, :C], want) and (got[:, C:] == SENT).all()
    _log(report_dir, "gather_rows_add", C=C, rows_per_item=rows_per_item, mismatches=0)


EMBED_POS = [(0, 0), (0, 3), (0, None), (5, None), (10, None), (5, 2)]  # (t_per_batch, device position | none); 10 = rows


@pytest.mark.parametrize("M", [8, 256, 260])
def test_embed_tokens(lib, report_dir, M):
    """out[r] = E[tok[r]] * scale + PE[pos + r % t_per_batch].  scale 16: the product is exact, so fused or not the result
    is numpy float32's bit for bit.  scale sqrt(512): |got - ref64| <= 2^-23 (|e scale| + |pe|), one rounding if the
    multiply-add is fused, two if not."""
    rng = np.random.default_rng(7000 + M)
    V, rows = 11, 10
    tok = [0, V - 1, 3, 3, 7, V - 1, 0, 5, 1, 9]
    emb = rng.standard_normal((V, M)).astype(np.float16)
    pe = rng.uniform(-1, 1, (rows + 4, M)).astype(f32)
    worst = 0.0
    for tpb, pos in EMBED_POS:
        t = (pos or 0) + (np.arange(rows) % tpb if tpb else 0) + np.zeros(rows, dtype=int)
        e, p = emb[tok].astype(f32), pe[t]
        got = run_embed_tokens(lib, tok, emb, 16.0, pe, pos, tpb, M + 4)
        assert same_bits(got[:, :M], e * f32(16.0) + p) and (got[:, M:] == SENT).all(), (tpb, pos)
        scale = f32(math.sqrt(512.0))
        got = run_embed_tokens(lib, tok, emb, scale, pe, pos, tpb, M + 4)
        es = e.astype(f64) * f64(scale)
        ratio = np.abs(got[:, :M] - (es + p)) / (U23 * (np.abs(es) + np.abs(p)))
        worst = max(worst, float(ratio.max()))
        assert (got[:, M:] == SENT).all()
    _log(report_dir, "embed_tokens", M=M, scale16_mismatches=0, sqrt512_err_over_bound=f"{worst:.3f}")
    assert worst <= 1.0


def _pos_inputs(M, rng, n_items=3, tpb=5):
    """|x| up to 1e3 against |PE| <= 1: float32 (x + PE) - x is not PE"""
    rows = n_items * tpb
    x = (rng.uniform(-1, 1, (rows, M)) * 10.0 ** rng.uniform(-1, 3, (rows, M))).astype(f32)
    pe = rng.uniform(-1, 1, (tpb + 3, M)).astype(f32)
    assert ((x + pe[np.arange(rows) % tpb]) - x != pe[np.arange(rows) % tpb]).mean() > 0.5
    return x, pe


@pytest.mark.parametrize("M", [8, 256, 260])
@pytest.mark.parametrize("by_row", [False, True])
def test_pos_add_keeps_the_cancellation(lib, report_dir, M, by_row):
    """x += alpha * ((x + PE[t]) - x) with t = row % t_per_batch (pos_add) or t = row_t[row] (pos_add_rows).  alpha 1 and
    0.5: every step is a single float32 operation or an exact product, so the result is numpy float32's bit for bit and
    x + alpha * PE would not pass.  alpha 0.3: 2^-23 (|x| + |alpha t|) around float64 on the float32 t."""
    rng = np.random.default_rng(8000 + M)
    x, pe = _pos_inputs(M, rng)
    rows, tpb = x.shape[0], 5
    row_t = [0, len(pe) - 1, 3, 3, 1, 6, 0, 2, len(pe) - 1, 4, 5, 7, 1, 0, 2] if by_row else None
    p = pe[np.asarray(row_t) if by_row else np.arange(rows) % tpb]
    t = (x + p) - x
    xin = _padded(x, M + 4, SENT)
    for alpha in (1.0, 0.5):
        got = run_pos_add(lib, xin, M, pe, tpb, row_t, alpha)
        assert same_bits(got[:, :M], x + f32(alpha) * t) and (got[:, M:] == SENT).all(), alpha
        # the simplified form is another result on these inputs (not at alpha 1: x + ((x + PE) - x) is fl(x + PE) itself)
        assert alpha == 1.0 or not same_bits(got[:, :M], x + f32(alpha) * p)
    a = f64(f32(0.3))
    got = run_pos_add(lib, xin, M, pe, tpb, row_t, 0.3)
    ratio = np.abs(got[:, :M] - (x.astype(f64) + a * t)) / (U23 * (np.abs(x) + np.abs(a * t)))
    _log(report_dir, "pos_add_rows" if by_row else "pos_add", M=M, exact_alpha_mismatches=0, alpha03_err_over_bound=f"{float(ratio.max()):.3f}")
    assert ratio.max() <= 1.0 and (got[:, M:] == SENT).all()


@pytest.mark.parametrize("M", [8, 256, 260])
def test_char_embed_add(lib, report_dir, M):
    """pos = alpha * ((x + PE[t]) - x); pos += E[id] * scale; x += pos, t = row % t_per_batch, in the reference's order"""
    rng = np.random.default_rng(9000 + M)
    x, pe = _pos_inputs(M, rng)
    rows, tpb, V = x.shape[0], 5, 9
    ids = [0, V - 1, 4, 4, 2, 7, 0, 1, V - 1, 3, 5, 6, 8, 0, 2]
    emb = rng.standard_normal((V, M)).astype(np.float16)
    e, p = emb[ids].astype(f32), pe[np.arange(rows) % tpb]
    t = (x + p) - x
    xin = _padded(x, M + 4, SENT)
    for alpha in (1.0, 0.5):
        got = run_char_embed_add(lib, xin, M, ids, emb, pe, tpb, alpha, 16.0)
        assert same_bits(got[:, :M], x + (f32(alpha) * t + e * f32(16.0))) and (got[:, M:] == SENT).all(), alpha
        assert not same_bits(got[:, :M], x + (f32(alpha) * p + e * f32(16.0)))
    a = f64(f32(0.3))
    got = run_char_embed_add(lib, xin, M, ids, emb, pe, tpb, 0.3, 16.0)
    es = e.astype(f64) * 16.0
    ratio = np.abs(got[:, :M] - (x.astype(f64) + (a * t + es))) / (U23 * (np.abs(x) + np.abs(a * t) + np.abs(es)))
    _log(report_dir, "char_embed_add", M=M, exact_alpha_mismatches=0, alpha03_err_over_bound=f"{float(ratio.max()):.3f}")
    assert ratio.max() <= 1.0 and (got[:, M:] == SENT).all()


# --------------------------------------------------------------------------------------------------------------------- #
# durations
# --------------------------------------------------------------------------------------------------------------------- #
DUR_CAP = 1000000


def durations64(x, factor, min_dur):
    """clamp(round_half_even((exp(x) - 1) * factor), min_dur), capped like the kernel"""
    with np.errstate(over="ignore"):
        r = np.rint((np.exp(x.astype(f64)) - 1.0) * factor)
    return np.minimum(np.maximum(r, min_dur), DUR_CAP).astype(np.int64)


def duration_inputs(H, rows, rng):
    """h [rows][H + 4], w [H], b [1] in float32 with x = h.w + b spread over [-1, 3]; returns x and the bound e_x in float64"""
    w = (rng.standard_normal(H) * 0.5 / math.sqrt(H)).astype(f32)
    b = np.asarray([0.75], dtype=f32)
    h = rng.standard_normal((rows, H))
    target = rng.uniform(-1.0, 3.0, rows)
    h += ((target - (h @ w.astype(f64) + f64(b[0]))) / (w.astype(f64) @ w.astype(f64)))[:, None] * w.astype(f64)
    h = h.astype(f32)
    hw = h.astype(f64) * w.astype(f64)
    x = hw.sum(-1) + f64(b[0])
    assert (x > -1.01).all() and (x < 3.01).all()
    return _padded(h, H + 4), w, b, x, 2.0 ** -21 * (np.abs(hw).sum(-1) + abs(f64(b[0])))


def duration_cases(H):
    """(h, w, b, x, e_x, t_per_batch, lens, live mask) over rows {1, 5, 8}, with lens = [full, 0, 2] and without lens"""
    rng = np.random.default_rng(10000 + H)
    for t in (1, 5, 8):
        for lens in ([t, 0, min(2, t)], None):
            rows = 3 * t if lens else t
            live = np.concatenate([np.arange(t) < n for n in lens]) if lens else np.ones(rows, dtype=bool)
            h, w, b, x, e_x = duration_inputs(H, rows, rng)
            h[~live] = np.nan  # a padded row may hold anything
            yield h, w, b, x, e_x, t, lens, live


def duration_counted(x, e_x, factor, min_dur):
    """rows on which the float64 rule gives one integer over [x - e_x, x + e_x]: the fp32 dot product and expf stay inside"""
    d = durations64(x, factor, min_dur)
    return d, (durations64(x - e_x, factor, min_dur) == d) & (durations64(x + e_x, factor, min_dur) == d)


@pytest.mark.parametrize("H", [64, 256, 260])
def test_durations_grid(lib, report_dir, H):
    live_rows = left_out = 0
    for h, w, b, x, e_x, tpb, lens, live in duration_cases(H):
        for factor in (1.0, 0.5, 2.0):
            for min_dur in (0, 1):
                want, counted = duration_counted(x, e_x, factor, min_dur)
                got = run_durations(lib, h, H, w, b, tpb, lens, factor, min_dur)
                assert (got[~live] == 0).all(), (tpb, lens, factor, min_dur)
                ok = live & counted
                assert np.array_equal(got[ok], want[ok]), (tpb, lens, factor, min_dur, got, want)
                live_rows += int(live.sum())
                left_out += int((live & ~counted).sum())
    _log(report_dir, "durations_grid", H=H, live_rows=live_rows, left_out=left_out, share_left_out=f"{left_out / live_rows:.4f}", mismatches=0)
    assert left_out <= 0.1 * live_rows


@pytest.mark.parametrize("min_dur", [0, 1])
def test_durations_fixed_rows(lib, report_dir, min_dur):
    """x about -5 -> min_dur; x = 0 exactly -> max(0, min_dur); x = 20 -> the cap; x = 50 (exp(x) is finite but past 2^63,
    where a float -> integer conversion is no longer defined) -> the cap; x = 100 (expf overflows) -> the cap; masked rows
    holding NaN -> 0"""
    H, tpb = 64, 7
    rng = np.random.default_rng(11000)
    w = (rng.standard_normal(H) * 0.5 / math.sqrt(H)).astype(f32)
    unit = w.astype(f64) / (w.astype(f64) @ w.astype(f64))
    xs = [-5.0, 0.0, 20.0, 50.0, 100.0]
    h = np.stack([v * unit for v in xs] + [np.full(H, np.nan)] * 2).astype(f32)
    x = (h[:5].astype(f64) * w.astype(f64)).sum(-1)
    assert np.abs(x - xs).max() < 1e-3 and x[1] == 0
    got = run_durations(lib, _padded(h, H + 4), H, w, np.zeros(1, f32), tpb, [5], 1.0, min_dur)
    _log(report_dir, "durations_fixed_rows", min_dur=min_dur, got=got.tolist())
    assert got.tolist() == [min_dur, max(0, min_dur), DUR_CAP, DUR_CAP, DUR_CAP, 0, 0]


@pytest.mark.parametrize("factor,want", [(0.5, 0), (1.5, -2), (2.5, -2), (3.5, -4)])
def test_durations_round_an_exact_tie_to_even(lib, report_dir, factor, want):
    """x = -100: exp(x) - 1 is -1 in float32 and in float64 alike, so (exp(x) - 1) * factor is the tie -factor exactly, at
    x +- e_x too.  Under a floor of -5 the rounding shows: half to even, not half away from zero (the grid cannot tell the
    two apart: a tie there is a row the rule leaves out)."""
    H = 64
    rng = np.random.default_rng(11500)
    w = (rng.standard_normal(H) * 0.5 / math.sqrt(H)).astype(f32)
    h = (-100.0 * w.astype(f64) / (w.astype(f64) @ w.astype(f64))).astype(f32)[None, :]
    x = (h.astype(f64) * w.astype(f64)).sum(-1)
    ref, counted = duration_counted(x, 2.0 ** -21 * np.abs(h.astype(f64) * w.astype(f64)).sum(-1), factor, -5)
    assert counted.all() and ref.tolist() == [want]
    got = run_durations(lib, _padded(h, H + 4), H, w, np.zeros(1, f32), 1, None, factor, -5)
    _log(report_dir, "durations_tie", factor=factor, got=got.tolist(), want=want)
    assert got.tolist() == [want]


# --------------------------------------------------------------------------------------------------------------------- #
# packed-item tables
# --------------------------------------------------------------------------------------------------------------------- #
ITEM_OFFS = [[0, 3, 3, 10, 11], [0, 7]]  # an empty item between live ones and a one-row item last; a single item


@pytest.mark.parametrize("item_off", ITEM_OFFS)
@pytest.mark.parametrize("mul", [1, 320])
def test_item_row_pos(lib, report_dir, item_off, mul):
    rows = item_off[-1] * mul
    want = np.full((rows + 1, 2), SENT_I, dtype=np.int32)
    for i in range(len(item_off) - 1):
        n = (item_off[i + 1] - item_off[i]) * mul
        for t in range(n):
            want[item_off[i] * mul + t] = (t, n)
    got = run_item_row_pos(lib, item_off, mul, rows)
    assert np.array_equal(got, want)
    _log(report_dir, "item_row_pos", items=len(item_off) - 1, mul=mul, rows=rows, mismatches=0)


@pytest.mark.parametrize("item_off", ITEM_OFFS)
@pytest.mark.parametrize("mul", [1, 320])
def test_scatter_items(lib, report_dir, item_off, mul):
    """packed rows -> the caller's padded rows: item i lands in row item_of[i], nothing behind its length is written and an
    empty item writes nothing"""
    n = len(item_off) - 1
    rng = np.random.default_rng(12000 + mul + n)
    src = rng.standard_normal(item_off[-1] * mul).astype(f32)
    item_of = [2, 0, 4, 1] if n == 4 else [1]  # destination row 3 (row 0 for a single item) belongs to nobody
    longest = max(item_off[i + 1] - item_off[i] for i in range(n)) * mul
    stride = longest + 8
    want = np.full((n + 1, stride), SENT, dtype=f32)
    for i in range(n):
        seg = src[item_off[i] * mul: item_off[i + 1] * mul]
        want[item_of[i], : len(seg)] = seg
    got = run_scatter_items(lib, src, item_off, item_of, mul, longest, n + 1, stride)
    assert same_bits(got, want)
    _log(report_dir, "scatter_items", items=n, mul=mul, mismatches=0)


@pytest.mark.parametrize("Lg,E,Sp", [(4, 12, 6), (0, 1280, 0)])
@pytest.mark.parametrize("layout", ["padded", "packed", "packed_single"])
def test_vocoder_embed(lib, report_dir, Lg, E, Sp, layout):
    """row = [lang[lang_idx[item]] | dict[unit] | spkr[spkr_idx[item]]] as exact fp16 -> fp32 values; the language and the
    speaker rows go by item (an empty packed item owns no row), not by row"""
    rng = np.random.default_rng(13000 + E)
    V = 13
    if layout == "padded":
        nb, T, item_off = 3, 5, None
        item_of_row = np.repeat(np.arange(nb), T)
    else:
        off = ITEM_OFFS[0] if layout == "packed" else ITEM_OFFS[1]
        nb, T, item_off = len(off) - 1, 0, off
        item_of_row = np.concatenate([np.full(off[i + 1] - off[i], i) for i in range(nb)])
    rows = len(item_of_row)
    units = rng.integers(0, V, rows)
    units[0], units[-1] = V - 1, 0
    dic = rng.standard_normal((V, E)).astype(np.float16)
    lang = rng.standard_normal((5, Lg)).astype(np.float16) if Lg else np.zeros((1, 0), np.float16)
    spkr = rng.standard_normal((6, Sp)).astype(np.float16) if Sp else np.zeros((1, 0), np.float16)
    lang_idx = [4, 0, 2, 1][:nb] if Lg else [0] * nb
    spkr_idx = [1, 5, 0, 3][:nb] if Sp else [0] * nb
    want = np.full((rows + 1, Lg + E + Sp), SENT, dtype=f32)
    for r in range(rows):
        i = item_of_row[r]
        want[r] = np.concatenate([lang[lang_idx[i]], dic[units[r]], spkr[spkr_idx[i]]]).astype(f32)
    got = run_vocoder_embed(lib, units, nb, T, dic, lang, lang_idx, spkr, spkr_idx, item_off)  # a zero-width table is never read
    assert same_bits(got, want)
    _log(report_dir, "vocoder_embed", Lg=Lg, E=E, Sp=Sp, layout=layout, rows=rows, mismatches=0)


# --------------------------------------------------------------------------------------------------------------------- #
# v1 Conformer glue
# --------------------------------------------------------------------------------------------------------------------- #
def glu_dwconv64(x, w, lens, left, bn):
    """GLU -> rows behind an item's length zero -> depthwise conv with `left` taps before the output row -> BatchNorm (inference)
    -> SiLU, in float64"""
    nb, T, C2 = x.shape
    C, K = C2 // 2, w.shape[1]
    x, w = x.astype(f64), w.astype(f64)
    gl = x[..., :C] / (1.0 + np.exp(-x[..., C:]))
    if lens is not None:
        for i, n in enumerate(lens):
            gl[i, n:] = 0
    pad = np.zeros((nb, T + K - 1, C))
    pad[:, left: left + T] = gl
    y = sum(pad[:, j: j + T] * w[:, j] for j in range(K))
    if bn is not None:
        g, b, mu, var = (v.astype(f64) for v in bn)
        y = (y - mu) / np.sqrt(var + 1e-5) * g + b
        y = y / (1.0 + np.exp(-y))
    return y


def glu_dwconv32(x, w, lens, left, bn):
    """the same in float32 on the CPU (torch): its error against float64 sets the bar"""
    C, K = w.shape
    gl = F.glu(torch.from_numpy(x), dim=-1)
    if lens is not None:
        for i, n in enumerate(lens):
            gl[i, n:] = 0
    y = F.conv1d(F.pad(gl.transpose(1, 2), (left, K - 1 - left)), torch.from_numpy(w).unsqueeze(1), groups=C)
    if bn is not None:
        g, b, mu, var = (torch.from_numpy(v) for v in bn)
        y = F.silu(F.batch_norm(y, mu, var, g, b, False, 0.0, 1e-5))
    return y.transpose(1, 2).numpy()


GLU_T = (1, 15, 16, 17, 40)  # around the 16-row tile of glu_dwconv_kernel<31, 16>


def glu_dwconv_inputs(K, C, T, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, T, 2 * C)).astype(f32)
    w = (rng.standard_normal((C, K)) * 0.2).astype(f32)
    bn = ((rng.random(C) + 0.5).astype(f32), (rng.standard_normal(C) * 0.1).astype(f32), (rng.standard_normal(C) * 0.1).astype(f32),
          (rng.random(C) + 0.5).astype(f32))
    return x, w, bn, [T, (T + 1) // 2]


@pytest.mark.parametrize("K", [31, 5])   # glu_dwconv_kernel<31, 16> and the generic kernel
@pytest.mark.parametrize("C", [64, 260])
def test_glu_dwconv_centred_batchnorm_silu(lib, report_dir, K, C):
    """The v1 module's middle: left = K / 2, BatchNorm folded by bn_fold_kernel, SiLU.  T around the 16-row tile; an item cut
    short by lens; and once without lens.  Bound: 4x the float32 CPU restatement's worst error over these inputs."""
    cases = []
    for T in GLU_T:
        x, w, bn, lens = glu_dwconv_inputs(K, C, T, 14000 + 100 * K + C + T)
        for ln in (lens, None) if T == 17 else (lens,):
            ref = glu_dwconv64(x, w, ln, K // 2, bn)
            cases.append((T, x, w, bn, ln, ref, float(np.abs(glu_dwconv32(x, w, ln, K // 2, bn) - ref).max())))
    err32 = max(c[-1] for c in cases)  # over every T: T = 1 alone is 2 x C values to take a worst error from
    for T, x, w, bn, ln, ref, e32 in cases:
        got = run_glu_dwconv_ex(lib, x, w, ln, K // 2, bn)
        e = float(np.abs(got - ref).max())
        _log(report_dir, "glu_dwconv_centred", K=K, C=C, T=T, lens=ln, kernel_err=f"{e:.3e}", f32_cpu_err_here=f"{e32:.3e}",
             f32_cpu_err=f"{err32:.3e}", bound=f"{4 * err32:.3e}")
        assert np.isfinite(got).all() and e <= 4 * err32, (T, ln, e, err32)


@pytest.mark.parametrize("K", [31, 5])
@pytest.mark.parametrize("C", [64, 260])
def test_glu_dwconv_ex_causal_equals_the_v2_hook(lib, report_dir, K, C):
    """left = K - 1 without BatchNorm is sc_op_glu_dwconv bit for bit, and both are the float64 causal convolution to the
    bound above"""
    cases = []
    for T in GLU_T:
        x, w, _, lens = glu_dwconv_inputs(K, C, T, 15000 + 100 * K + C + T)
        ref = glu_dwconv64(x, w, lens, K - 1, None)
        cases.append((T, x, w, lens, ref, float(np.abs(glu_dwconv32(x, w, lens, K - 1, None) - ref).max())))
    err32 = max(c[-1] for c in cases)
    for T, x, w, lens, ref, e32 in cases:
        got = run_glu_dwconv_ex(lib, x, w, lens, K - 1, None)
        assert same_bits(got, run_glu_dwconv(lib, x, w, lens)), T
        assert same_bits(got, run_glu_dwconv_ex(lib, x, w, lens, -1, None)), T
        e = float(np.abs(got - ref).max())
        _log(report_dir, "glu_dwconv_causal", K=K, C=C, T=T, mismatches=0, kernel_err=f"{e:.3e}", f32_cpu_err_here=f"{e32:.3e}",
             f32_cpu_err=f"{err32:.3e}", bound=f"{4 * err32:.3e}")
        assert e <= 4 * err32, (T, e, err32)


def relpos64(S, M):
    """oracle/unity.py rel_pos_table in float64: row t = position (S - 1) - t, sin at the even columns, cos at the odd ones"""
    pos = np.arange(S - 1, -S, -1, dtype=f64)[:, None]
    div = np.exp(np.arange(0, M, 2, dtype=f64) * -(math.log(10000.0) / M))
    out = np.zeros((2 * S - 1, M))
    out[:, 0::2] = np.sin(pos * div)
    out[:, 1::2] = np.cos(pos * div)
    return out, np.repeat(np.abs(pos), M, axis=1)


@pytest.mark.parametrize("S", [1, 2, 129])
@pytest.mark.parametrize("M", [8, 1024])
def test_relpos_table(lib, report_dir, S, M):
    """|got - ref64| <= 2^-22 |pos| + 2^-22: the fp32 frequency and argument, then sinf / cosf.  The float64 table is tied to
    the oracle's float32 one by the same bound."""
    from oracle.unity import rel_pos_table

    ref, pos = relpos64(S, M)
    bound = 2.0 ** -22 * pos + 2.0 ** -22
    assert (np.abs(rel_pos_table(S, M).numpy() - ref) <= bound).all()
    got = run_relpos_table(lib, S, M)
    assert (got[2 * S - 1:] == SENT).all()
    got = got[: 2 * S - 1]
    ratio = float((np.abs(got - ref) / bound).max())
    _log(report_dir, "relpos_table", S=S, M=M, err=f"{float(np.abs(got - ref).max()):.3e}", err_over_bound=f"{ratio:.3f}")
    assert ratio <= 1.0
    # the shape of the table: the middle row is position 0, row 0 is +(S - 1), sin and cos interleave
    assert (got[S - 1, 0::2] == 0).all() and (got[S - 1, 1::2] == 1).all()
    if S > 1:
        assert abs(got[S - 2, 0] - math.sin(1.0)) <= 2.0 ** -21 and abs(got[S - 2, 1] - math.cos(1.0)) <= 2.0 ** -21
        assert got[S - 2, 0] > 0 > got[S, 0] and got[S - 2, 1] == got[S, 1]
        assert (got[0, 0::2] == -got[-1, 0::2]).all() and (got[0, 1::2] == got[-1, 1::2]).all()
