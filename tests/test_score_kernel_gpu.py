"""The fused vocabulary projection + log-softmax (k_gemm_ps.hip, SCORE epilogue + score_finish_kernel) through its hook
sc_op_linear_presplit_score, against the float64 restatement of tests/score_oracle.py.

Error bars.  Per row, e = max_j |sc_op_linear_presplit - float64| on the same inputs: the error of the PARENT's product,
whose accumulators the scoring epilogue reads (same MFMA order, same bits).  c = columns per record, r = records per row.
  * lse = log sum_j exp v_j is 1-Lipschitz in the max norm of v, so the product's error moves it by at most e.  In fp32 the
    kernel then sums c exponentials sequentially inside a record (relative error <= c u, u = 2^-24, of a positive sum), folds
    r records (<= r u more) and takes a handful of correctly-rounded-to-a-few-ulp steps (expf, the rescale, logf, max + log:
    the 8); a relative error d of the sum is an absolute error d of its log, and the final addition rounds at |lse| u:
        |lse - ref| <= e + (c + r + 8) u max(1, |lse|)
  * lprob_target = (v_t - max) - log(sum): v_t carries another e:
        |lprob_target - ref| <= 2 e + (c + r + 8) u max(1, |lse|)
  * sum_lprob / N = mean_j v_j - lse: the mean is summed in the same c + r steps, relative to mean |v|:
        |sum_lprob / N - ref / N| <= e + (c + r + 8) u max(1, |lse|) + (c + r) u mean|v|
  * top1 equals the float64 arg-max wherever the float64 top-2 margin exceeds 2 e.
Errors observed on the MI355X are listed in DESIGN.md (section 7, teacher-forced scoring)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import score_oracle as so

pytestmark = pytest.mark.gpu

M_FULL = 300
KS = (32, 128, 1024)
NS = (33, 256, 257, 1200, 4100)  # a tail inside a wave's range, an exact tile edge, one past it, the tiny vocabulary, many tiles
MS = (1, 63, 65, 300)
ROW_EQUAL, ROW_DOMINANT, ROW_NAN = 5, 9, 17  # ROW_NAN only where a test asks for it


@pytest.fixture(scope="module")
def lib():
    from seamless_communication_amd import _lib

    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return _lib.load_library()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def check(lib, st):
    assert st == 0, lib.sc_last_error().decode()


def boundary_targets(N):
    cand = [0, N - 1, 31, 32, 33, 127, 128, 129, 255, 256, 257, -1]
    return [c for c in cand if c < N]


@functools.lru_cache(maxsize=None)
def case(K, N, with_bias=False):
    """Inputs and float64 reference of one (K, N) at 300 rows, computed once; every smaller M is a prefix of it."""
    g = torch.Generator().manual_seed(1000 * K + N)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
    x = torch.randn(M_FULL, K, generator=g)
    bias = torch.randn(N, generator=g) * 0.5 if with_bias else None
    raw = x.double() @ w.double().T
    # a ladder of scales; every fourth row is scaled so that its largest |logit| is 80 (no max subtraction: exp overflows)
    scale = torch.tensor([0.5, 2.0, 6.0, 0.0])[torch.arange(M_FULL) % 4]
    hot = scale == 0.0
    scale = torch.where(hot, (80.0 / raw.abs().amax(dim=1)).float(), scale)
    x = x * scale[:, None]
    x[ROW_EQUAL] = 0.0  # all logits equal (0): lse = log N, top1 = 0
    # one logit dominant by 40: x along the longest weight row j (w_i.w_j <= |w_i||w_j| < |w_j|^2)
    j = int(w.double().norm(dim=1).argmax())
    d = w[j].double() @ w.double().T
    gap = float(d[j] - torch.cat([d[:j], d[j + 1:]]).max())
    assert gap > 0
    x[ROW_DOMINANT] = (w[j].double() * (40.0 / gap)).float()
    bt = boundary_targets(N)
    tg = torch.Generator().manual_seed(7 * K + N)
    target = torch.randint(0, N, (M_FULL,), generator=tg).numpy().astype(np.int32)
    target[20:20 + len(bt)] = bt
    target[ROW_DOMINANT] = j
    target[ROW_EQUAL] = N - 1
    ref = so.score_ref(x, w, bias, target)
    return {"x": x, "w": w, "bias": bias, "target": target, "ref": ref, "dominant": j}


def run_score(lib, x, w, bias, target, group_rows=0):
    M, K = x.shape
    N = w.shape[0]
    xd, wd = x.contiguous().cuda(), w.contiguous().cuda()
    bd = bias.cuda() if bias is not None else None
    td = torch.as_tensor(np.asarray(target, dtype=np.int32)).cuda()
    lp = torch.full((M,), 7.0, device="cuda")
    sl = torch.full((M,), 7.0, device="cuda")
    lse = torch.full((M,), 7.0, device="cuda")
    t1 = torch.full((M,), -7, device="cuda", dtype=torch.int32)
    torch.cuda.synchronize()
    if group_rows:
        check(lib, lib.sc_op_linear_presplit_score_grouped(P(xd), P(wd), P(bd), P(td), P(lp), P(sl), P(lse), P(t1), M, N, K, group_rows))
    else:
        check(lib, lib.sc_op_linear_presplit_score(P(xd), P(wd), P(bd), P(td), P(lp), P(sl), P(lse), P(t1), M, N, K))
    return {"lprob": lp.cpu(), "sum_lprob": sl.cpu(), "lse": lse.cpu(), "top1": t1.cpu().numpy()}


def product_error(lib, x, w, bias, ref):
    """e per row: the parent's product (sc_op_linear_presplit, fp32 logits written out) against float64."""
    M, K = x.shape
    N = w.shape[0]
    xd, wd = x.contiguous().cuda(), w.contiguous().cuda()
    bd = bias.cuda() if bias is not None else None
    y = torch.full((M, N), float("nan"), device="cuda")
    torch.cuda.synchronize()
    check(lib, lib.sc_op_linear_presplit(P(xd), P(wd), P(bd), None, P(y), None, None, M, N, K, 0, 1.0))
    return (y.cpu().double() - ref["logits"][:M]).abs().amax(dim=1)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.int32), np.asarray(b[k]).view(np.int32)) for k in ("lprob", "sum_lprob", "lse", "top1"))


def assert_within(lib, got, c, M, N, e, report=None):
    ref = {k: v[:M] for k, v in c["ref"].items()}
    cols = lib.sc_op_score_record_cols(N)
    assert cols in (32, 64, 128)
    bar = so.bars(ref, e, cols, N)
    err = {
        "lse": (got["lse"].double() - ref["lse"]).abs(),
        "lprob": (got["lprob"].double() - ref["lprob"]).abs(),
        "sum_lprob_mean": (got["sum_lprob"].double() - ref["sum_lprob"]).abs() / N,
    }
    for k in err:
        worst = float((err[k] / bar[k]).max())
        print(f"score_kernel M={M} N={N} K={c['x'].shape[1]} {k}: max err {float(err[k].max()):.3e} max bar {float(bar[k].max()):.3e} worst err/bar {worst:.3f}")
        assert (err[k] <= bar[k]).all(), (k, worst)
    # sign: a log-probability
    assert (got["lprob"] <= 0).all()
    # arg-max wherever float64 separates the two best by more than the product's error
    sure = ref["margin"] > 2 * e
    assert np.array_equal(got["top1"][sure.numpy()], ref["top1"][sure.numpy()])
    assert ((got["top1"] >= 0) & (got["top1"] < N)).all()
    return float(sure.double().mean())


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_score_against_float64(lib, K, N):
    """Every (K, N) at M = 1, 63, 65 and 300 (prefixes of one 300-row input, one float64 reference): lse, lprob_target and
    sum_lprob / N inside their bars, lprob_target <= 0, top1 equal wherever float64 separates the two best columns by more
    than 2 e, and the rows below M = 300 carry the bits of the 300-row call (a row does not see the rest of the launch)."""
    c = case(K, N)
    full = None
    for M in sorted(MS, reverse=True):
        x = c["x"][:M]
        got = run_score(lib, x, c["w"], None, c["target"][:M])
        e = product_error(lib, x, c["w"], None, c["ref"])
        share = assert_within(lib, got, c, M, N, e)
        if M == M_FULL:
            full = got
            # the inputs separate the two best columns in at least 95 % of the rows (float64, checked here on the CPU side)
            assert share >= 0.95, share
            # all-equal row: lse = v + log N with v = 0, the lowest column wins
            assert abs(float(got["lse"][ROW_EQUAL]) - math.log(N)) <= (lib.sc_op_score_record_cols(N) + 16) * so.U24 * max(1.0, math.log(N))
            assert got["top1"][ROW_EQUAL] == 0
            # one logit dominant by 40: every other exponential is below 2^-57, the sum is 1.0 and its log 0.0
            assert float(got["lprob"][ROW_DOMINANT]) == 0.0
            assert got["top1"][ROW_DOMINANT] == c["dominant"]
            # rows scaled to |logit| = 80 stay finite
            assert torch.isfinite(got["lse"]).all() and torch.isfinite(got["sum_lprob"]).all()
        else:
            assert same_bits(got, {k: v[:M] for k, v in full.items()})


@pytest.mark.parametrize("N", NS)
def test_score_row_independence(lib, N):
    """The 300-row call and 300 one-row calls give the same bits in all four outputs; so does a call cut into row groups
    (groups of 128: three groups, the last one partial; groups of 7)."""
    K = 128
    c = case(K, N)
    full = run_score(lib, c["x"], c["w"], None, c["target"])
    for m in range(M_FULL):
        one = run_score(lib, c["x"][m:m + 1], c["w"], None, c["target"][m:m + 1])
        assert same_bits(one, {k: v[m:m + 1] for k, v in full.items()}), m
    for g in (128, 7):
        assert same_bits(run_score(lib, c["x"], c["w"], None, c["target"], group_rows=g), full), g


@pytest.mark.parametrize("N", (257, 4100))
def test_score_nan_row_stays_in_its_row(lib, N):
    """A NaN in one row of x: that row's lse / lprob_target / sum_lprob are NaN, its top1 lies inside [0, N), and every
    other row keeps the bits of the clean call."""
    K = 128
    c = case(K, N)
    clean = run_score(lib, c["x"][:65], c["w"], None, c["target"][:65])
    x = c["x"][:65].clone()
    x[ROW_NAN, 3] = float("nan")
    got = run_score(lib, x, c["w"], None, c["target"][:65])
    for k in ("lse", "lprob", "sum_lprob"):
        assert math.isnan(float(got[k][ROW_NAN])), k
    assert 0 <= got["top1"][ROW_NAN] < N
    keep = np.arange(65) != ROW_NAN
    assert same_bits({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in clean.items()})


@pytest.mark.parametrize("N", (33, 1200))
def test_score_bias_and_no_target(lib, N):
    """A bias is honoured as the arg-max epilogue honours it; target -1 gives lprob_target 0."""
    K, M = 128, 65
    c = case(K, N, True)
    x = c["x"][:M]
    got = run_score(lib, x, c["w"], c["bias"], c["target"][:M])
    e = product_error(lib, x, c["w"], c["bias"], c["ref"])
    assert_within(lib, got, c, M, N, e)
    none = np.flatnonzero(c["target"][:M] < 0)
    assert len(none) and (got["lprob"][none] == 0).all()
