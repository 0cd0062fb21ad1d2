"""GPU: the cross-attention rows of a whole teacher-forced pass (k_xattn.hip: xattn_rows_kernel) by themselves, through
sc_op_xattn_rows, at shapes the tiny model does not reach.

Reference: softmax(q . k / 8) summed over the heads in float64 numpy on the same fp32 inputs (standard normal).  Bar 1e-5
absolute - the project's bar for this quantity through the whole decoder (tests/test_transcriber_gpu.py: tol_x); the kernel
alone has to sit inside it.  (Its own error: a score is a 64-term fp32 fmaf chain of products of size ~1, scaled by 1/8 -
about 64 * 2^-24 / 8 = 5e-7 at the worst - times p (1 - p) <= 1/4 per head, plus a few ulps of expf and of the row sum per
probability <= 1; 16 heads stay below 1e-5.)

Shapes cross the kernel's tiles: QT query rows per workgroup, KC key rows per LDS chunk.  Outputs start as NaN: the kernel
writes its own zeros."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
QT, KC = 16, 64  # the kernel's query tile and key chunk (test_tile_constants pins them to the library's)
BAR = 1e-5


def _log(report_dir, name, **kw):
    with open(report_dir / "transcriber_align_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def _hp(a):
    return C.c_void_p(a.ctypes.data)


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _reference(q, k, enc_lens, tok_lens, heads):
    """q (n, S1, H * 64), k (n, s_enc, H * 64) fp32 -> (n, S1, s_enc) float64"""
    n, S1, _ = q.shape
    s_enc = k.shape[1]
    q64 = q.astype(np.float64).reshape(n, S1, heads, 64)
    k64 = k.astype(np.float64).reshape(n, s_enc, heads, 64)
    out = np.zeros((n, S1, s_enc))
    for b in range(n):
        el, live = int(enc_lens[b]), int(tok_lens[b]) - 1
        s = np.einsum("phd,jhd->hpj", q64[b, :live], k64[b, :el]) / 8.0
        s = np.exp(s - s.max(axis=-1, keepdims=True))
        out[b, :live, :el] = (s / s.sum(axis=-1, keepdims=True)).sum(axis=0)
    return out


def _run(lib, q, k, enc_lens, tok_lens, heads, pad_rows=0, pad_keys=0):
    """q (n, S1, M), k (n, s_enc, M) numpy -> xattn (n, S1 + pad_rows, s_enc + pad_keys) numpy.  The keys are handed over as the
    model holds them (row stride 2 M, the value half NaN); the padding rows of q and k are NaN and must not be read into a
    live result."""
    n, S1, M = q.shape
    s_enc = k.shape[1]
    qq = np.full((n, S1 + pad_rows, M), np.nan, dtype=np.float32)
    qq[:, :S1] = q
    kv = np.full((n, s_enc + pad_keys, 2 * M), np.nan, dtype=np.float32)
    kv[:, :s_enc, :M] = k
    out = dev(torch.full((n, S1 + pad_rows, s_enc + pad_keys), float("nan")))
    el, tl = _i32(enc_lens), _i32(tok_lens)  # named: the arrays must outlive the call that takes their addresses
    check(lib, lib.sc_op_xattn_rows(P(dev(torch.from_numpy(qq))), M, P(dev(torch.from_numpy(kv))), 2 * M, n, S1 + pad_rows, s_enc + pad_keys, heads,
                                    _hp(el), _hp(tl), P(out)))
    return out.cpu().numpy()


def _lens(S1, s_enc):
    """three items: full; keys below s_enc and odd (no multiple of 4, 16 or 64) with a ragged text; a single live row"""
    odd = max(1, s_enc - 1 if (s_enc - 1) % 2 else s_enc - 2)
    return [s_enc, odd, max(1, s_enc // 3)], [S1 + 1, max(2, S1 // 2 + 2), 2]


def test_tile_constants(lib):
    assert (lib.sc_op_xattn_rows_tile(0), lib.sc_op_xattn_rows_tile(1)) == (QT, KC)


@pytest.mark.parametrize("heads", [1, 2, 16])
@pytest.mark.parametrize("S1", [1, QT - 1, QT, QT + 1])
@pytest.mark.parametrize("s_enc", [1, KC - 1, KC, KC + 1, 2 * KC + 1])
def test_rows_against_float64(lib, report_dir, heads, S1, s_enc):
    rng = np.random.default_rng(1000 * heads + 100 * S1 + s_enc)
    n, M = 3, heads * 64
    q = rng.standard_normal((n, S1, M)).astype(np.float32)
    k = rng.standard_normal((n, s_enc, M)).astype(np.float32)
    enc_lens, tok_lens = _lens(S1, s_enc)
    want = _reference(q, k, enc_lens, tok_lens, heads)
    got = _run(lib, q, k, enc_lens, tok_lens, heads)
    assert np.isfinite(got).all()
    err = float(np.abs(got - want).max())
    sums = 0.0
    for b in range(n):
        el, live = enc_lens[b], tok_lens[b] - 1
        assert not got[b, :, el:].any(), "keys behind the encoder length must be exact zeros"
        assert not got[b, live:].any(), "rows behind the last target must be exact zeros"
        sums = max(sums, float(np.abs(got[b, :live].astype(np.float64).sum(axis=1) - heads).max()))
    print(f"xattn_rows heads={heads} S1={S1} s_enc={s_enc}: max_err={err:.3e} row_sum_err={sums:.3e}")
    _log(report_dir, "xattn_rows_kernel", heads=heads, S1=S1, s_enc=s_enc, max_err=f"{err:.3e}", row_sum_err=f"{sums:.3e}")
    assert err < BAR, err
    assert sums < 1e-5, sums


@pytest.mark.parametrize("heads,S1,s_enc", [(2, QT + 1, KC + 1), (16, 3, 2 * KC + 1), (1, QT, KC - 1)])
def test_an_items_rows_do_not_depend_on_the_batch_or_the_padding(lib, heads, S1, s_enc):
    rng = np.random.default_rng(7 + heads)
    n, M = 3, heads * 64
    q = rng.standard_normal((n, S1, M)).astype(np.float32)
    k = rng.standard_normal((n, s_enc, M)).astype(np.float32)
    enc_lens, tok_lens = _lens(S1, s_enc)
    got = _run(lib, q, k, enc_lens, tok_lens, heads)
    for b in range(n):
        alone = _run(lib, q[b : b + 1], k[b : b + 1], enc_lens[b : b + 1], tok_lens[b : b + 1], heads)
        assert np.array_equal(alone[0].view(np.int32), got[b].view(np.int32)), b
        # a larger padded S1 and s_enc (another grid, another output stride); the padding holds NaN
        wide = _run(lib, q[b : b + 1], k[b : b + 1], enc_lens[b : b + 1], tok_lens[b : b + 1], heads, pad_rows=QT + 3, pad_keys=KC + 7)
        assert np.array_equal(wide[0, :S1, :s_enc].view(np.int32), got[b].view(np.int32)), b
        assert not wide[0, S1:].any() and not wide[0, :, s_enc:].any()


def test_unsupported_geometry_and_lengths_fail_before_any_launch(lib):
    q = dev(torch.zeros(1, 2, 17 * 64))
    out = dev(torch.zeros(1, 2, 4))
    one, two, long_text, long_enc = _i32([4]), _i32([3]), _i32([4]), _i32([5])
    assert lib.sc_op_xattn_rows(P(q), 17 * 64, P(q), 17 * 64, 1, 2, 4, 17, _hp(one), _hp(two), P(out)) != 0
    assert b"heads" in lib.sc_last_error()
    assert lib.sc_op_xattn_rows(P(q), 64, P(q), 64, 1, 2, 4, 1, _hp(one), _hp(long_text), P(out)) != 0
    assert b"tok_lens[0]=4" in lib.sc_last_error()
    assert lib.sc_op_xattn_rows(P(q), 64, P(q), 64, 1, 2, 4, 1, _hp(long_enc), _hp(two), P(out)) != 0
    assert b"enc_lens[0]=5" in lib.sc_last_error()
    assert lib.sc_op_xattn_rows(P(q), 64, P(q), 64, 1, 2, 4, 1, _hp(one), _hp(two), None) != 0
    assert b"null" in lib.sc_last_error()
