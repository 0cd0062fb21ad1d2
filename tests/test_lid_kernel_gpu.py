"""The candidate-set log-softmax of the vocabulary product (k_gemm_ps.hip: gemm_cand_kernel + cand_finish_kernel) through its
hook sc_op_score_candidates: against the target form of the same product (sc_op_linear_presplit_score, bit for bit) and
against the float64 restatement of tests/score_oracle.py inside the bars of tests/test_score_kernel_gpu.py.

Shapes.  K = 64, rows 1, 33 and 70 (prefixes of one 70-row input).  N = 2 * cols + 5 with cols = sc_op_score_record_cols(N)
has one solution, N = 69 (cols 32, the 64 x 64 tile): two full records and a tail of five columns.  69 columns cannot hold a
run of 100 or a list of 512, so the same construction is repeated where the other two tile shapes start: N = 645 (128 x 128
tile, cols 64, ten records and a tail of five) and N = 1029 (256 x 256 tile, cols 128, eight records and a tail of five,
two tile columns).  Every N takes every list that fits in it; N = 69 takes all of its 69 columns in place of the two long
lists.

Per N the target form is run ONCE on 70 * N rows (row m * N + t = input row m with target t; a row's results depend on that
row alone, tests/test_score_kernel_gpu.py::test_score_row_independence): the table tgt[m][t] every list is compared with."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import score_oracle as so

pytestmark = pytest.mark.gpu

K = 64
M_FULL = 70
MS = (1, 33, 70)
NS = (69, 645, 1029)
ROW_NAN = 17


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


def cand_lists(N, cols):
    """name -> strictly ascending columns."""
    out = {"first": [0], "last": [N - 1], "straddle": [cols - 1, cols]}
    if N >= 2 * cols + 5 and N > 100:
        out["run100"] = list(range(cols - 37, cols + 63))  # 37 columns of record 0, all or most of record 1 (and of record 2 at cols 32)
    if N >= 512:
        g = np.random.default_rng(N)
        inner = np.sort(g.choice(np.arange(1, N - 1), 510, replace=False))  # both ends of the row and 510 columns between them
        out["list512"] = [0] + [int(p) for p in inner] + [N - 1]
    else:
        out["all"] = list(range(N))
    for v in out.values():
        assert 1 <= len(v) <= 512 and all(b > a for a, b in zip(v, v[1:])) and v[0] >= 0 and v[-1] < N
    return out


@functools.lru_cache(maxsize=None)
def case(N):
    """Inputs and float64 reference of one N at 70 rows, computed once; rows 1 and 33 are prefixes of it."""
    g = torch.Generator().manual_seed(4242 + N)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
    x = torch.randn(M_FULL, K, generator=g)
    x = x * torch.tensor([1.0, 3.0, 6.0])[torch.arange(M_FULL) % 3][:, None]  # a ladder of logit scales
    bias = torch.randn(N, generator=g) * 0.5
    ref = so.score_ref(x, w, bias, np.full(M_FULL, -1, dtype=np.int32))
    ref["lsm"] = torch.log_softmax(ref["logits"], dim=-1)
    return {"x": x, "w": w, "bias": bias, "ref": ref}


def run_cand(lib, x, w, bias, cand):
    M, N, L = x.shape[0], w.shape[0], len(cand)
    xd, wd = x.contiguous().cuda(), w.contiguous().cuda()
    bd = bias.cuda() if bias is not None else None
    hc = np.ascontiguousarray(cand, dtype=np.int32)
    lp = torch.full((M, L), 7.0, device="cuda")
    best = torch.full((M,), -7, device="cuda", dtype=torch.int32)
    torch.cuda.synchronize()
    check(lib, lib.sc_op_score_candidates(P(xd), P(wd), P(bd), hc.ctypes.data_as(C.c_void_p), L, P(lp), P(best), M, N, x.shape[1]))
    return lp.cpu(), best.cpu().numpy()


def target_form(lib, x, w, bias, N):
    """lprob of sc_op_linear_presplit_score for every (row, target column): (M, N) float32."""
    M = x.shape[0]
    xr = x.repeat_interleave(N, dim=0).contiguous().cuda()
    wd = w.contiguous().cuda()
    bd = bias.cuda() if bias is not None else None
    td = torch.arange(N, dtype=torch.int32).repeat(M).cuda()
    lp = torch.full((M * N,), 7.0, device="cuda")
    torch.cuda.synchronize()
    check(lib, lib.sc_op_linear_presplit_score(P(xr), P(wd), P(bd), P(td), P(lp), None, None, None, M * N, N, x.shape[1]))
    return lp.cpu().view(M, N)


_tables = {}


def tables(lib, N):
    """Per N, once: the target form's table on the 70 rows, and e = the parent product's error per row against float64."""
    if N not in _tables:
        c = case(N)
        y = torch.full((M_FULL, N), float("nan"), device="cuda")
        xd, wd, bd = c["x"].contiguous().cuda(), c["w"].contiguous().cuda(), c["bias"].cuda()
        torch.cuda.synchronize()
        check(lib, lib.sc_op_linear_presplit(P(xd), P(wd), P(bd), None, P(y), None, None, M_FULL, N, K, 0, 1.0))
        e = (y.cpu().double() - c["ref"]["logits"]).abs().amax(dim=1)
        _tables[N] = (target_form(lib, c["x"], c["w"], c["bias"], N), e)
    return _tables[N]


def bits(t):
    return np.asarray(t).view(np.int32)


@pytest.mark.parametrize("N", NS)
def test_candidates_equal_the_target_form_and_float64(lib, N):
    """(a) lprob[:, j] carries the bits of the target form with target cand[j]; (b) it lies inside the project's bar around
    float64; (c) best is the float64 arg-max among the candidates, and every row of every list separates its two best
    candidates by more than 2 e (asserted: no row is excused)."""
    cols = lib.sc_op_score_record_cols(N)
    assert N == {69: 2, 645: 10, 1029: 8}[N] * cols + 5
    c = case(N)
    tgt, e = tables(lib, N)
    bar = so.bars(c["ref"], e, cols, N)["lprob"]
    for name, cand in cand_lists(N, cols).items():
        ci = torch.as_tensor(cand, dtype=torch.int64)
        ref_lp = c["ref"]["lsm"][:, ci]
        ref_v = c["ref"]["logits"][:, ci]
        ref_best = np.argmax(ref_v.numpy(), axis=1)
        if len(cand) > 1:
            top2 = torch.topk(ref_v, 2, dim=1).values
            margin = top2[:, 0] - top2[:, 1]
            assert (margin > 2 * e).all(), (name, float((margin - 2 * e).min()))
        for M in MS:
            lp, best = run_cand(lib, c["x"][:M], c["w"], c["bias"], cand)
            assert np.array_equal(bits(lp), bits(tgt[:M][:, ci])), (name, M)
            err = (lp.double() - ref_lp[:M]).abs()
            print(f"lid_kernel N={N} {name} M={M}: lprob max err {float(err.max()):.3e} max bar {float(bar[:M].max()):.3e} "
                  f"worst err/bar {float((err / bar[:M, None]).max()):.3f}")
            assert (err <= bar[:M, None]).all(), (name, M)
            assert (lp <= 0).all()
            assert np.array_equal(best, ref_best[:M]), (name, M)


def test_candidates_equal_the_target_form_with_many_records(lib):
    """N = 2000 * 128 + 5 (about the full-size vocabulary): 2001 records per row, so a lane of the finish kernels folds 31 or 32
    of them - the two finish kernels must round that sum alike (with at most 64 records every lane holds one term and a fused
    multiply-add cannot show).  16 candidates spread over the row; the target form runs on 70 * 16 rows."""
    N = 2000 * 128 + 5
    assert lib.sc_op_score_record_cols(N) == 128
    g = torch.Generator().manual_seed(99)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
    x = torch.randn(M_FULL, K, generator=g) * torch.tensor([1.0, 3.0, 6.0])[torch.arange(M_FULL) % 3][:, None]
    cand = sorted({0, 127, 128, N - 1} | {int(c) for c in torch.randint(0, N, (12,), generator=g)})
    L = len(cand)
    lp, best = run_cand(lib, x, w, None, cand)
    xr = x.repeat_interleave(L, dim=0).contiguous().cuda()
    td = torch.as_tensor(cand, dtype=torch.int32).repeat(M_FULL).cuda()
    wd = w.cuda()
    tl = torch.full((M_FULL * L,), 7.0, device="cuda")
    torch.cuda.synchronize()
    check(lib, lib.sc_op_linear_presplit_score(P(xr), P(wd), None, P(td), P(tl), None, None, None, M_FULL * L, N, K))
    assert np.array_equal(bits(lp), bits(tl.cpu().view(M_FULL, L)))
    ref_v = (x.double() @ w.double().T)[:, cand]
    top2 = torch.topk(ref_v, 2, dim=1).values
    sure = ((top2[:, 0] - top2[:, 1]) > 1e-3).numpy()  # far above the product's error at K = 64 (e < 1e-5 in the cases above)
    assert sure.mean() > 0.9 and np.array_equal(best[sure], np.argmax(ref_v.numpy(), axis=1)[sure])


@pytest.mark.parametrize("N", (69, 1029))
def test_candidates_nan_row_stays_in_its_row(lib, N):
    """(d) A NaN in one row of x: that row's log-probabilities are NaN and its best is 0; every other row keeps its bits."""
    cols = lib.sc_op_score_record_cols(N)
    c = case(N)
    lists = cand_lists(N, cols)
    cand = lists.get("list512", lists.get("all"))
    clean_lp, clean_best = run_cand(lib, c["x"][:33], c["w"], c["bias"], cand)
    x = c["x"][:33].clone()
    x[ROW_NAN, 3] = float("nan")
    lp, best = run_cand(lib, x, c["w"], c["bias"], cand)
    assert torch.isnan(lp[ROW_NAN]).all() and best[ROW_NAN] == 0
    keep = np.arange(33) != ROW_NAN
    assert np.array_equal(bits(lp)[keep], bits(clean_lp)[keep]) and np.array_equal(best[keep], clean_best[keep])
    assert ((best >= 0) & (best < len(cand))).all()


@pytest.mark.parametrize("N", NS)
def test_equal_candidates_choose_the_lower_index(lib, N):
    """(e) Two candidates with the same weight row and bias have the same value in every row: the lower j wins - as a pair on
    its own (in two records, so two waves write them), and as the largest two of a longer list (x along that weight row)."""
    cols = lib.sc_op_score_record_cols(N)
    c = case(N)
    c1, c2 = cols - 1, cols + 3
    w, bias = c["w"].clone(), c["bias"].clone()
    w[c2], bias[c2] = w[c1], bias[c1]
    lp, best = run_cand(lib, c["x"], w, bias, [c1, c2])
    assert np.array_equal(bits(lp[:, 0]), bits(lp[:, 1])) and (best == 0).all()
    # the pair dominant: x = s * w[c1] makes column c1 (= c2) the largest by far (|w_i . w_c1| < |w_c1|^2 for i != c1, checked)
    d = w.double() @ w[c1].double()
    rest = torch.cat([d[:c1], d[c1 + 1:c2], d[c2 + 1:]])
    gap = float(d[c1] - rest.max())
    assert gap > 0
    s = (8.0 + float(bias.abs().max()) * 2) / gap
    x = (w[c1].double() * s).float()[None].repeat(M_FULL, 1) + 0.01 * c["x"]
    cand = sorted(set(range(0, N, 3)) | {c1, c2})[:512]
    assert c1 in cand and c2 in cand
    ref_v = (x.double() @ w.double().T + bias.double())[:, cand]
    assert (np.argmax(ref_v.numpy(), axis=1) == cand.index(c1)).all()
    lp, best = run_cand(lib, x, w, bias, cand)
    assert (best == cand.index(c1)).all()
    assert np.array_equal(bits(lp[:, cand.index(c1)]), bits(lp[:, cand.index(c2)]))
