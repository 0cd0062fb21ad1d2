"""GPU: the fp16-split attention kernel (k_attn.hip: attn_mfma16_kernel) in every mode the model ships, called through
sc_op_attention_ex with the operand layouts of its callers, against float64 references computed one (item, head) at a
time (oracle/unity.py: mha for the plain and Shaw modes, mha_relpos for the Transformer-XL mode).

What the kernel-level test of test_ops_gpu.py does not reach: interleaved q / k / v rows ([rows][3M], the self-attention
of every caller) and the cross-attention strides (ldq = M, ldk = ldv = 2M); the result as two fp16 planes (v2 encoder,
NAR T2U decoder); packed varlen rows (NAR T2U decoder); Transformer-XL relative positions (v1 encoder); the edges of
the 32-key tiles and 128-query workgroups; the online soft-max rescale and its skip; and sequences up to the encoder's
length limit (4096 fbank frames = 2048 positions).

Every output buffer is NaN before the call and has a row stride of heads * 64 + 16 plus guard rows after the last row;
the gap columns and guard rows must still hold NaN afterwards.  Key / value rows behind an item's length are NaN too:
the kernel must never read them.  Bars: 2e-5 absolute on unit-variance inputs (test_attention's bar) and, per (item,
head), 1e-4 relative to max |reference|; the planes and the packed layout are bit-exact against the fp32-output and
padded runs of the same inputs.  Logits of standard deviation ~900 (q, k and v times 30) are beyond what fp32 scores
resolve to 1e-4; there the kernel must stay within twice the error of plain fp32 PyTorch (test_large_logits_fp32_class).
Every measured error is appended to attention_report.txt in the report directory (conftest.py: report_dir).
"""
import ctypes as C

import pytest
import torch

from oracle import unity as ou
from tests.test_ops_gpu import check, lib  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

HD = 64
PAD = 16  # extra columns of every output row: must stay NaN
GUARD = 3  # NaN rows behind the last output row
ABS_BAR = 2e-5  # unit-variance inputs (test_ops_gpu.py::test_attention)
REL_BAR = 1e-4  # per (item, head), relative to max |reference|
NAN = float("nan")


def _log(report_dir, name, **kw):
    with open(report_dir / "attention_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


# ------------------------------------------------------------------------------------------------------------------ #
# problems: host tensors q [nb][Sq][H][64], k / v [nb][Skv][H][64] (fp32) and the mode's extra operands
# ------------------------------------------------------------------------------------------------------------------ #
class Problem:
    def __init__(self, nb, H, Sq, Skv, lens=None, causal=False, mode=0, left=0, right=0, qk_scale=1.0, v_scale=1.0,
                 pattern=None, seed=0):
        g = torch.Generator().manual_seed(seed * 7919 + nb * 1009 + H * 101 + Sq * 13 + Skv)
        self.nb, self.H, self.Sq, self.Skv, self.M = nb, H, Sq, Skv, H * HD
        self.lens, self.causal, self.mode, self.left, self.right = lens, causal, mode, left, right
        self.q = torch.randn(nb, Sq, H, HD, generator=g)
        self.k = torch.randn(nb, Skv, H, HD, generator=g)
        self.v = torch.randn(nb, Skv, H, HD, generator=g)
        if pattern is not None:
            # a shared direction d in every query; the keys carry t_j * d, so the logits follow t_j along the keys
            d = torch.randn(HD, generator=g)
            d = d / d.norm()
            if pattern in ("rise", "fall"):
                t = torch.linspace(-8.0, 8.0, Skv) if pattern == "rise" else torch.linspace(8.0, -8.0, Skv)
                self.q = 0.3 * self.q + 4.0 * d
                self.k = 0.3 * self.k + t[None, :, None, None] * d
            elif pattern == "spike":
                # one key per item, the last valid one (in the last tile), about 12 logits above the others
                self.q = 0.5 * self.q + 3.0 * d
                for n in range(nb):
                    self.k[n, self._len(n) - 1] = 32.0 * d
            else:
                raise ValueError(pattern)
        self.q, self.k, self.v = self.q * qk_scale, self.k * qk_scale, self.v * v_scale
        self.rel = self.rp = self.u = self.vb = None
        if mode == 1:  # Shaw relative keys [left + 1 + right][64], shared by the heads
            self.rel = torch.randn(left + 1 + right, HD, generator=g) * 0.3
        elif mode == 2:  # Transformer-XL: r_proj(position table) [2S-1][M], u / v biases [M]
            assert Sq == Skv
            r_proj = torch.randn(self.M, self.M, generator=g) / self.M ** 0.5
            self.rp = ou.rel_pos_table(Skv, self.M) @ r_proj.T
            self.u = torch.randn(self.M, generator=g) * 0.5
            self.vb = torch.randn(self.M, generator=g) * 0.5

    def _len(self, n):
        return self.Skv if self.lens is None else min(self.lens[n], self.Skv)

    def ref_head(self, n, h, dt=torch.float64):
        """[Sq][64] of item n, head h, computed in `dt` (float64: the reference; float32: what plain fp32 arithmetic
        makes of the same inputs)."""
        q = self.q[n, :, h].to(dt)
        k = self.k[n, : self._len(n), h].to(dt)  # keys behind the length do not exist (their rows are NaN)
        v = self.v[n, : self._len(n), h].to(dt)
        Sq, L, shift = self.Sq, k.shape[0], self.Skv - self.Sq
        i = torch.arange(Sq)[:, None]
        j = torch.arange(L)[None, :]
        if self.mode == 2:  # mha_relpos: ((q + u).k_j + (q + v).r[S - 1 + j - i]) / 8
            hs = slice(h * HD, (h + 1) * HD)
            r = self.rp[:, hs].to(dt)
            w = (q + self.u[hs].to(dt)) @ k.T
            w = w + torch.gather((q + self.vb[hs].to(dt)) @ r.T, 1, (self.Skv - 1 + j - i).expand(Sq, L))
        else:  # mha: q.k_j (+ q.rel[clamp(j - i', -left, right) + left], i' = i + Skv - Sq) / 8
            w = q @ k.T
            if self.mode == 1:
                idx = (j - (i + shift)).clamp(-self.left, self.right) + self.left
                w = w + torch.gather(q @ self.rel.to(dt).T, 1, idx.expand(Sq, L))
        w = w * HD ** -0.5
        if self.causal:
            w = w.masked_fill(j > i + shift, float("-inf"))
        return torch.softmax(w, -1) @ v


# ------------------------------------------------------------------------------------------------------------------ #
# layouts and the call
# ------------------------------------------------------------------------------------------------------------------ #
def _ptr(t, elems=0):
    return C.c_void_p(t.data_ptr() + elems * t.element_size()) if t is not None else C.c_void_p(0)


def _nan_behind_lens(pb, x):
    """Copy of k / v with the rows behind each item's length set to NaN."""
    x = x.clone()
    if pb.lens is not None:
        for n in range(pb.nb):
            x[n, pb._len(n):] = NAN
    return x


def _inputs(pb, layout):
    """Device operands as the callers lay them out.  'self': one [rows][3M] buffer, q | k | v (attention_self, the
    encoders, the T2U decoders); 'cross': q [rows][M] and k | v [rows][2M] (model_decoder.hip's encoder-decoder
    attention); 'packed': [sum of lengths][3M], item n at row row_off[n], then NaN guard rows."""
    M, nb = pb.M, pb.nb
    k, v = _nan_behind_lens(pb, pb.k), _nan_behind_lens(pb, pb.v)
    if layout == "cross":
        qb = pb.q.reshape(nb * pb.Sq, M).cuda()
        kvb = torch.cat([k.reshape(nb * pb.Skv, M), v.reshape(nb * pb.Skv, M)], 1).cuda()
        return (qb, 0, M), (kvb, 0, 2 * M), (kvb, M, 2 * M)
    assert pb.Sq == pb.Skv
    wide = torch.cat([pb.q.reshape(nb, pb.Sq, M), k.reshape(nb, pb.Skv, M), v.reshape(nb, pb.Skv, M)], 2)
    if layout == "packed":
        wide = torch.cat([wide[n, : pb._len(n)] for n in range(nb)] + [torch.full((40, 3 * M), NAN)], 0)
    else:
        wide = wide.reshape(nb * pb.Sq, 3 * M)
    wide = wide.cuda()
    return (wide, 0, 3 * M), (wide, M, 3 * M), (wide, 2 * M, 3 * M)


def _run(lib, pb, layout, planes=False, packed_rows=None):
    """One sc_op_attention_ex call.  Returns the output buffer(s) on the host: fp32 [rows + GUARD][M + PAD], or the
    (hi, lo) fp16 planes of that shape."""
    M, nb = pb.M, pb.nb
    (qb, qo, ldq), (kb, ko, ldk), (vb, vo, ldv) = _inputs(pb, layout)
    rows = packed_rows if layout == "packed" else nb * pb.Sq
    ld = M + PAD
    d_lens = torch.tensor(pb.lens, dtype=torch.int32).cuda() if pb.lens is not None else None
    d_row_off = None
    if layout == "packed":
        offs = [0]
        for n in range(nb - 1):
            offs.append(offs[-1] + pb._len(n))
        d_row_off = torch.tensor(offs, dtype=torch.int32).cuda()
    d_rel = pb.rel.cuda() if pb.rel is not None else None
    d_rp = d_u = d_v = None
    rp_ld = 0
    if pb.mode == 2:
        rp_ld = M + 8  # a row stride wider than the table: the gap columns are NaN and must not be read
        d_rp = torch.full((2 * pb.Skv - 1, rp_ld), NAN)
        d_rp[:, :M] = pb.rp
        d_rp, d_u, d_v = d_rp.cuda(), pb.u.cuda(), pb.vb.cuda()
    out = hi = lo = None
    if planes:
        hi = torch.full((rows + GUARD, ld), NAN, dtype=torch.float16, device="cuda")
        lo = torch.full((rows + GUARD, ld), NAN, dtype=torch.float16, device="cuda")
    else:
        out = torch.full((rows + GUARD, ld), NAN, device="cuda")
    check(lib, lib.sc_op_attention_ex(
        _ptr(qb, qo), _ptr(kb, ko), _ptr(vb, vo), _ptr(out), nb, pb.H, pb.Sq, pb.Skv, ldq, ldk, ldv,
        0 if planes else ld, _ptr(d_lens), int(pb.causal), _ptr(d_rel), pb.left, pb.right, _ptr(d_row_off),
        _ptr(d_rp), rp_ld, _ptr(d_u), _ptr(d_v), _ptr(hi), _ptr(lo), ld if planes else 0))
    if planes:
        return hi.cpu(), lo.cpu()
    return out.cpu()


def _assert_guards(buf, rows, M):
    assert torch.isnan(buf[:, M:].float()).all(), "a gap column behind heads * 64 was written"
    assert torch.isnan(buf[rows:].float()).all(), "a guard row behind the last output row was written"
    assert not torch.isnan(buf[:rows, :M].float()).any(), "an output element was not written (or is NaN)"


def _errors(pb, got, row_of, packed=False, dt=torch.float64):
    """Largest absolute and relative (to max |reference|) error over the (item, head) pairs of `got` [rows][M + PAD]
    (row_of(n) = first row of item n); got=None measures ref_head(dt) instead."""
    worst_abs = worst_rel = 0.0
    for n in range(pb.nb):
        nq = pb._len(n) if packed else pb.Sq
        for h in range(pb.H):
            ref = pb.ref_head(n, h)[:nq]
            if got is None:
                o = pb.ref_head(n, h, dt)[:nq].double()
            else:
                o = got[row_of(n): row_of(n) + nq, h * HD: (h + 1) * HD].double()
            e = float((o - ref).abs().max())
            worst_abs, worst_rel = max(worst_abs, e), max(worst_rel, e / max(float(ref.abs().max()), 1e-30))
    return worst_abs, worst_rel


def _compare(report_dir, group, pb, got, row_of, bar_abs=True, **tag):
    """Checks every (item, head) of `got` against the float64 reference; logs the largest errors first."""
    err, rel = _errors(pb, got, row_of, tag.get("layout") == "packed")
    _log(report_dir, group, nb=pb.nb, H=pb.H, Sq=pb.Sq, Skv=pb.Skv, lens=pb.lens, causal=pb.causal, mode=pb.mode,
         left=pb.left, right=pb.right, **tag, err=f"{err:.3e}", rel=f"{rel:.3e}")
    if bar_abs:
        assert err < ABS_BAR, (group, err)
    assert rel < REL_BAR, (group, rel)


def _check(lib, report_dir, group, pb, layout, planes=False, bar_abs=True, **tag):
    rows = pb.nb * pb.Sq
    got = _run(lib, pb, layout, planes)
    if planes:
        hi, lo = got
        _assert_guards(hi, rows, pb.M)
        _assert_guards(lo, rows, pb.M)
        got = hi.double() + lo.double()
    else:
        _assert_guards(got, rows, pb.M)
    _compare(report_dir, group, pb, got, lambda n: n * pb.Sq, bar_abs, layout=layout, planes=planes, **tag)
    return got


# ------------------------------------------------------------------------------------------------------------------ #
# 1. layouts
# ------------------------------------------------------------------------------------------------------------------ #
LAYOUT_CASES = [
    # interleaved [rows][3M] q | k | v with padded items: self_attention (layers.hip)
    ("self", dict(nb=3, H=5, Sq=200, Skv=200, lens=[200, 77, 129])),
    # encoder-decoder attention (model_decoder.hip): Sq != Skv, ldq = M, ldk = ldv = 2M, encoder lengths
    ("cross", dict(nb=3, H=4, Sq=37, Skv=301, lens=[301, 150, 7])),
    # ... with more text positions than encoder frames
    ("cross", dict(nb=2, H=2, Sq=150, Skv=20, lens=[20, 9])),
    # teacher-forced decoder self-attention: causal, no kv_lens, S up to the default hard_max_seq_len (M = 1024)
    ("self", dict(nb=1, H=16, Sq=1024, Skv=1024, causal=True)),
    ("self", dict(nb=2, H=3, Sq=257, Skv=257, causal=True)),
    # causal with Skv > Sq: key j visible iff j <= i + (Skv - Sq); with and without key lengths
    ("cross", dict(nb=2, H=2, Sq=100, Skv=230, causal=True)),
    ("cross", dict(nb=2, H=4, Sq=61, Skv=230, causal=True, lens=[230, 180])),
]


@pytest.mark.parametrize("layout,kw", LAYOUT_CASES)
def test_layouts(lib, report_dir, layout, kw):
    _check(lib, report_dir, "layouts", Problem(**kw), layout)


# ------------------------------------------------------------------------------------------------------------------ #
# 2. edges of the 32-key tiles (MKV) and 128-query workgroups (MQ); nb * heads = 0 mod 8 runs the XCD re-mapping of
# the workgroup ids (k_attn.hip, attn_mfma16_kernel), any other value skips it
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("H", [8, 3])  # nb * H = 56 (re-mapped) / 21 (plain order)
def test_tile_edges_kv_lens(lib, report_dir, H):
    # one item per length: a single key, one short of / exactly / one past one and four key tiles, inside Skv = 160
    pb = Problem(nb=7, H=H, Sq=160, Skv=160, lens=[1, 31, 32, 33, 127, 128, 129])
    _check(lib, report_dir, "tile_edges", pb, "self", bh=pb.nb * H)


@pytest.mark.parametrize("S", [1, 127, 128, 129, 257])
@pytest.mark.parametrize("nb,H", [(2, 4), (1, 3)])  # nb * H = 8 (re-mapped) / 3 (plain order)
def test_tile_edges_queries(lib, report_dir, S, nb, H):
    # one query / one short of, exactly, one past one workgroup of 128 queries / two workgroups and one query
    lens = None if nb == 1 else [S, max(1, S - 40)]
    _check(lib, report_dir, "tile_edges", Problem(nb=nb, H=H, Sq=S, Skv=S, lens=lens), "self", bh=nb * H)


# ------------------------------------------------------------------------------------------------------------------ #
# 3. online soft-max
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("pattern", [
    "rise",   # logits rise along the keys: the running maximum moves at every tile, O is rescaled every time
    "fall",   # logits fall: the maximum of the first tile holds, alpha == 1 and the ballot skips the rescale
    "spike",  # one key in the last tile dominates: the last tile rescales everything before it by ~exp(-12)
])
def test_online_softmax_patterns(lib, report_dir, pattern):
    pb = Problem(nb=2, H=4, Sq=300, Skv=300, lens=[300, 290], pattern=pattern)
    _check(lib, report_dir, "softmax", pb, "self", pattern=pattern)


@pytest.mark.parametrize("scale", [1e-2, 1.0, 30.0])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_online_softmax_magnitudes(lib, report_dir, scale, mode):
    """Logits and values scaled by `scale` (q and k by sqrt(scale), v by scale): near-uniform weights and values whose
    fp16 lo halves are subnormal (1e-2) to near one-hot weights over logits of standard deviation ~30 and outputs up to
    ~100 (30).  Relative bar per (item, head); the absolute bar where the inputs have unit variance."""
    kw = dict(left=64, right=8) if mode == 1 else {}
    pb = Problem(nb=2, H=4, Sq=300, Skv=300, lens=[300, 170], mode=mode, qk_scale=scale ** 0.5, v_scale=scale, **kw)
    _check(lib, report_dir, "magnitude", pb, "self", bar_abs=scale == 1.0, scale=scale)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_large_logits_fp32_class(lib, report_dir, mode):
    """q, k and v each scaled by 30: logits of standard deviation ~900.  fp32 holds a logit near 2^11 to 2^-13, and
    where the two largest logits of a query nearly tie, that much moves the output by ~1e-4 of its magnitude whatever
    the arithmetic: plain fp32 PyTorch misses the 1e-4 relative bar on these inputs (up to 1.8e-4).  Bar: the kernel's
    largest relative error is at most twice that of fp32 PyTorch on the same inputs."""
    kw = dict(left=64, right=8) if mode == 1 else {}
    pb = Problem(nb=2, H=4, Sq=300, Skv=300, lens=[300, 170], mode=mode, qk_scale=30.0, v_scale=30.0, **kw)
    got = _run(lib, pb, "self")
    _assert_guards(got, pb.nb * pb.Sq, pb.M)
    err, rel = _errors(pb, got, lambda n: n * pb.Sq)
    err32, rel32 = _errors(pb, None, None, dt=torch.float32)
    _log(report_dir, "large_logits", mode=mode, err=f"{err:.3e}", rel=f"{rel:.3e}", fp32_torch_rel=f"{rel32:.3e}")
    assert rel <= 2 * rel32, (rel, rel32)


# ------------------------------------------------------------------------------------------------------------------ #
# 4. Shaw relative keys (mode 1, v2 encoder): per 32 x 32 block of a wave the kernel takes one of three branches: the
# whole key tile left of the clamp window (one q.R value: the leftmost relative key), the whole tile right of it (the
# rightmost), or the per-key gather (mixed).  S >= 300 reaches all three for both windows; S = 33 only the mixed one.
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("left,right", [(64, 8), (8, 40)])  # config.py's window and an asymmetric one
@pytest.mark.parametrize("layout,kw", [
    ("self", dict(nb=2, H=4, Sq=499, Skv=499, lens=[499, 310])),  # nb * H = 8: re-mapped
    ("self", dict(nb=3, H=3, Sq=300, Skv=300, lens=[300, 33, 129])),  # 9: plain order
    ("self", dict(nb=1, H=2, Sq=33, Skv=33)),
    ("cross", dict(nb=2, H=2, Sq=100, Skv=260, lens=[260, 200])),  # query i at position i + 160
])
def test_shaw(lib, report_dir, left, right, layout, kw):
    _check(lib, report_dir, "shaw", Problem(mode=1, left=left, right=right, **kw), layout)


# ------------------------------------------------------------------------------------------------------------------ #
# 5. Transformer-XL relative positions (mode 2, v1 encoder): the per-wave window of 64 table rows around key - query
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("S", [1, 33, 129, 304, 1000])
@pytest.mark.parametrize("nb,H", [(2, 4), (3, 3)])  # nb * H = 8 (re-mapped) / 9 (plain order)
def test_relpos(lib, report_dir, S, nb, H):
    lens = [S, max(1, (2 * S) // 3), max(1, S // 5)][:nb]
    _check(lib, report_dir, "relpos", Problem(nb=nb, H=H, Sq=S, Skv=S, lens=lens, mode=2), "self", bh=nb * H)


# ------------------------------------------------------------------------------------------------------------------ #
# 6. the result as fp16 planes (hi, lo) instead of fp32: same arithmetic, so bit-exact against the fp32 result
# ------------------------------------------------------------------------------------------------------------------ #
def _split(out):
    """(hi, lo) of fp32 values as the kernel's epilogue forms them: hi = fp16(x), lo = fp16(x - float(hi)), both
    rounded to nearest-even."""
    hi = out.half()
    lo = (out - hi.float()).half()
    return hi, lo


def _assert_planes_equal(hi, lo, out, rows, M):
    want_hi, want_lo = _split(out[:rows, :M])
    assert torch.equal(hi[:rows, :M].view(torch.int16), want_hi.view(torch.int16)), "hi plane != fp16(out)"
    assert torch.equal(lo[:rows, :M].view(torch.int16), want_lo.view(torch.int16)), "lo plane != fp16(out - hi)"


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_planes_bit_exact(lib, report_dir, mode):
    kw = dict(left=64, right=8) if mode == 1 else {}
    pb = Problem(nb=2, H=4, Sq=300, Skv=300, lens=[300, 170], mode=mode, **kw)
    out = _check(lib, report_dir, "planes", pb, "self", planes=False)
    hi, lo = _run(lib, pb, "self", planes=True)
    rows = pb.nb * pb.Sq
    _assert_guards(hi, rows, pb.M)
    _assert_guards(lo, rows, pb.M)
    _assert_planes_equal(hi, lo, out.float(), rows, pb.M)
    _compare(report_dir, "planes", pb, hi.double() + lo.double(), lambda n: n * pb.Sq, layout="self", planes=True)


# ------------------------------------------------------------------------------------------------------------------ #
# 7. packed varlen rows (NAR T2U decoder): item n at rows row_off[n] .. + len[n], no padding between items
# ------------------------------------------------------------------------------------------------------------------ #
PACKED_LENS = [1, 127, 128, 129, 500, 33]


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("H", [4, 3])  # nb * H = 24 (re-mapped) / 18 (plain order)
def test_packed_rows(lib, report_dir, H, planes):
    S = max(PACKED_LENS)
    pb = Problem(nb=len(PACKED_LENS), H=H, Sq=S, Skv=S, lens=PACKED_LENS)
    R = sum(PACKED_LENS)
    offs = [sum(PACKED_LENS[:n]) for n in range(pb.nb)]
    packed = _run(lib, pb, "packed", planes, packed_rows=R)
    padded = _run(lib, pb, "self", planes)
    for buf_p, buf_q in (zip(packed, padded) if planes else [(packed, padded)]):
        _assert_guards(buf_p, R, pb.M)  # nothing behind the last item's last row
        for n, l in enumerate(PACKED_LENS):  # bit for bit the valid rows of the padded run
            a = buf_p[offs[n]: offs[n] + l, : pb.M]
            b = buf_q[n * S: n * S + l, : pb.M]
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16),
                               b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16)), (n, l)
    got = packed[0].double() + packed[1].double() if planes else packed
    _compare(report_dir, "packed", pb, got, lambda n: offs[n], layout="packed", planes=planes)


# ------------------------------------------------------------------------------------------------------------------ #
# 8. long inputs: the encoder's limit of 4096 fbank frames = 2048 positions, 64 key tiles and 16 query workgroups;
# one item padded
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("S", [2047, 2048])
@pytest.mark.parametrize("mode", [1, 2])
def test_long(lib, report_dir, mode, S):
    kw = dict(left=64, right=8) if mode == 1 else {}
    pb = Problem(nb=2, H=16, Sq=S, Skv=S, lens=[S, 1500], mode=mode, **kw)
    _check(lib, report_dir, "long", pb, "self")


# ------------------------------------------------------------------------------------------------------------------ #
# 9. rejected arguments: non-zero status, an error text, nothing launched (the output stays NaN)
# ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("what", ["row_off_without_kv_lens", "rp_table_causal", "rp_table_cross", "shaw_97_positions"])
def test_rejected_arguments(lib, what):
    nb, H, S = 2, 2, 40
    M = H * HD
    Sq, Skv = (20, S) if what == "rp_table_cross" else (S, S)
    q = torch.randn(nb * S, 3 * M).cuda()
    out = torch.full((nb * Sq + GUARD, M + PAD), NAN, device="cuda")
    lens = torch.tensor([S, 30], dtype=torch.int32).cuda()
    row_off = torch.tensor([0, S], dtype=torch.int32).cuda()
    rp = torch.randn(2 * S - 1, M).cuda()
    bias = torch.randn(M).cuda()
    rel = torch.randn(98, HD).cuda()
    a = dict(lens=None, causal=0, rel=None, left=0, right=0, row_off=None, rp=None, u=None, v=None)
    if what == "row_off_without_kv_lens":
        a.update(row_off=row_off)
    elif what == "rp_table_causal":
        a.update(lens=lens, causal=1, rp=rp, u=bias, v=bias)
    elif what == "rp_table_cross":
        a.update(lens=lens, rp=rp, u=bias, v=bias)
    else:
        a.update(lens=lens, rel=rel, left=64, right=32)
    st = lib.sc_op_attention_ex(
        _ptr(q), _ptr(q, M), _ptr(q, 2 * M), _ptr(out), nb, H, Sq, Skv, 3 * M, 3 * M, 3 * M, M + PAD, _ptr(a["lens"]),
        a["causal"], _ptr(a["rel"]), a["left"], a["right"], _ptr(a["row_off"]), _ptr(a["rp"]), M, _ptr(a["u"]),
        _ptr(a["v"]), None, None, 0)
    assert st != 0
    assert b"attention" in lib.sc_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a rejected call wrote its output"
