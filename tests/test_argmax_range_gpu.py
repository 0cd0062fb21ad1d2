"""Row arg-max hooks on rows that are not numbers: the index a hook stores is inside the row, always.

Every row arg-max starts its running index at 0x7fffffff and no comparison with NaN is true, so a row of NaN logits (NaN
audio, or an activation beyond the finite range of the split products, DESIGN.md "Numeric range of the products") used to
leave that value as the chosen token.  Here the index is only stored - no test feeds it on into an embedding or a gather.
Which in-range index a NaN row gets is not specified; its log-probability / score is NaN, so the caller can see it.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN, NINF = float("nan"), float("-inf")


@pytest.fixture(scope="module")
def lib():
    from seamless_communication_amd import _lib

    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return _lib.load_library()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


_KEEP = []


def dev(t):
    """Device copy that stays alive until the end of the test: the raw pointer
    handed to the C ABI must not be recycled by the caching allocator."""
    d = t.contiguous().cuda()
    _KEEP.append(d)
    return d


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    _KEEP.clear()


def check(lib, st):
    assert st == 0, lib.sc_last_error().decode()


# rows 1, 4: all NaN; row 2: NaN at some positions; row 5: all -inf; the others finite
ALL_NAN, SOME_NAN, ALL_NINF = (1, 4), (2,), (5,)
FINITE = (0, 3, 6)


@pytest.mark.parametrize("with_lprob", [True, False], ids=["lprob", "plain"])
@pytest.mark.parametrize("V", [1200, 1201])
def test_argmax_rows(lib, V, with_lprob):
    """sc_op_argmax: argmax_rows_kernel (log-probability asked for, or odd V) and argmax_plain_rows_kernel."""
    rows = 7
    g = torch.Generator().manual_seed(V)
    clean = torch.randn(rows, V, generator=g) * 3
    x = clean.clone()
    for r in ALL_NAN:
        x[r] = NAN
    x[2, ::3] = NAN
    x[2, V - 1] = NAN
    x[5] = NINF

    def run(t):
        idx = torch.full((rows,), -5, dtype=torch.int32, device="cuda")
        lp = torch.full((rows,), 7.0, device="cuda") if with_lprob else None
        check(lib, lib.sc_op_argmax(P(dev(t)), rows, V, P(idx), P(lp)))
        return idx.cpu(), (lp.cpu() if with_lprob else None)

    idx, lp = run(x)
    idx0, lp0 = run(clean)
    assert ((idx >= 0) & (idx < V)).all(), idx.tolist()
    assert idx0.tolist() == clean.argmax(-1).tolist()
    for r in FINITE:
        assert int(idx[r]) == int(idx0[r])
    assert int(idx[5]) == 0  # a row of -inf: the lowest index, as before
    masked = x[2].clone()
    masked[torch.isnan(masked)] = NINF
    assert int(idx[2]) == int(masked.argmax())  # NaN never wins: the largest number does
    if with_lprob:
        assert torch.equal(lp[list(FINITE)], lp0[list(FINITE)])
        assert torch.isnan(lp[list(ALL_NAN)]).all()


def _vocab_hook(lib, name):
    if name == "skinny":
        return lambda x, w, M, N, K, idx, lp: lib.sc_op_skinny_argmax(P(x), P(w), M, N, K, 5, 0, -1, 0, 3, 1, 0.0, P(idx), P(lp))
    if name == "dstep":
        return lambda x, w, M, N, K, idx, lp: lib.sc_op_dstep_argmax(P(x), P(w), M, N, K, 5, 0, -1, 0, 3, 1, 0.0, 4, P(idx), P(lp))
    return lambda x, w, M, N, K, idx, lp: lib.sc_op_dstep3_argmax(P(x), P(w), M, N, K, 5, 0, -1, 0, 3, 1, 0.0, P(idx), P(lp))


@pytest.mark.parametrize("poison", [NAN, 70000.0], ids=["nan", "overflow"])
@pytest.mark.parametrize("name", ["skinny", "dstep", "dstep3"])
def test_fused_vocabulary_argmax(lib, name, poison):
    """Vocabulary projection with the arg-max in its epilogue + argmax_finalize_kernel (pad 0, unk 1, eos 3, step 5): a NaN
    or an overflowing element in the activation row makes every logit of the row NaN."""
    M, N, K = 5, 1200, 128
    g = torch.Generator().manual_seed(M + N + K)
    clean = torch.randn(M, K, generator=g)
    w = dev((torch.randn(N, K, generator=g) / K ** 0.5).half())
    x = clean.clone()
    x[1, 9] = poison
    x[3, 0] = poison
    hook = _vocab_hook(lib, name)

    def run(t):
        idx = torch.full((M,), -5, dtype=torch.int32, device="cuda")
        lp = torch.full((M,), 7.0, device="cuda")
        check(lib, hook(dev(t), w, M, N, K, idx, lp))
        return idx.cpu(), lp.cpu()

    idx, lp = run(x)
    idx0, lp0 = run(clean)
    assert ((idx >= 0) & (idx < N)).all(), idx.tolist()
    good = [0, 2, 4]
    assert idx[good].tolist() == idx0[good].tolist()
    assert torch.equal(lp[good], lp0[good])
    assert torch.isnan(lp[[1, 3]]).all(), lp.tolist()


@pytest.mark.parametrize("with_bias", [True, False])
def test_presplit_gemm_fused_argmax(lib, with_bias):
    """The arg-max in the epilogue of the DMA GEMM + amax_finish_kernel (the NAR T2U unit projection)."""
    M, N, K = 70, 1030, 64
    g = torch.Generator().manual_seed(M + N)
    clean = torch.randn(M, K, generator=g) * 2
    w = dev((torch.randn(N, K, generator=g) / K ** 0.5).half())
    b = dev(torch.randn(N, generator=g) * 0.1) if with_bias else None
    x = clean.clone()
    bad = [0, 33, 64, 69]  # in both row halves of the first 64-row tile, and in the ragged last one
    x[0, 5] = NAN
    x[33] = NAN
    x[64, 63] = 70000.0
    x[69, 0] = NAN

    def run(t):
        idx = torch.full((M,), -7, dtype=torch.int32, device="cuda")
        check(lib, lib.sc_op_linear_presplit_argmax(P(dev(t)), P(w), P(b), P(idx), M, N, K))
        return idx.cpu()

    idx, idx0 = run(x), run(clean)
    assert ((idx >= 0) & (idx < N)).all(), idx[bad].tolist()
    good = [r for r in range(M) if r not in bad]
    assert idx[good].tolist() == idx0[good].tolist()


def test_kmeans_units(lib):
    """sc_op_kmeans: the arg-min of the distance as the fused arg-max of x.c - |c|^2 / 2."""
    rows, C_, K = 40, 64, 300
    g = torch.Generator().manual_seed(5)
    clean = torch.randn(rows, C_, generator=g)
    cent = dev(torch.randn(C_, K, generator=g))
    x = clean.clone()
    bad = [3, 17, 39]
    x[3, 1] = NAN
    x[17] = NAN
    x[39, 63] = NAN

    def run(t):
        idx = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
        check(lib, lib.sc_op_kmeans(P(dev(t)), P(cent), rows, C_, K, P(idx)))
        return idx.cpu()

    idx, idx0 = run(x), run(clean)
    assert ((idx >= 0) & (idx < K)).all(), idx[bad].tolist()
    good = [r for r in range(rows) if r not in bad]
    assert idx[good].tolist() == idx0[good].tolist()


def test_engine_step_close(lib):
    """launch_vocab3 with the per-slot step rules + engine_finalize_kernel at the smallest shape of its own test: slots
    whose activation row holds a NaN get a token inside the vocabulary and a NaN score; the rows of every other slot end
    as in a launch without the NaN.  engine_finalize writes `hist` by position, not by token."""
    from tests import test_engine_kernels_gpu as eng

    M, N, K = 24, 1200, 128
    n_states, cap = M + M // 4 + 3, 48
    x, w, _ = eng.vocab_case(M, N, K)
    st, rp = eng.engine_state(M, n_states, cap, M, M + N + M, N)
    bad_slots = [s for s in range(M) if eng.KINDS[s % len(eng.KINDS)] in ("plain", "no_eos", "unk_top")]
    assert len(bad_slots) >= 6
    xp = x.clone()
    for s in bad_slots:
        xp[s, s % K] = NAN
    got, got_rp = eng.run_step_close(lib, xp, w, M, N, K, st, rp, M, n_states, cap)
    ref, ref_rp = eng.run_step_close(lib, x, w, M, N, K, st, rp, M, n_states, cap)
    bad_rows = {rp[s][0] for s in bad_slots}
    assert got_rp == ref_rp  # positions advance alike
    for s in range(M):
        r = rp[s][0]
        pos = rp[s][1]
        if r in bad_rows:
            assert 0 <= got["tok"][r] < N, (s, got["tok"][r])
            assert 0 <= int(got["hist"][r, pos + 1]) < N
            assert torch.isnan(got["score"][r])
        else:
            for k in ("tok", "pos", "finished", "out_len", "limit", "prefix_len"):
                assert got[k][r] == ref[k][r], (k, s)
            assert torch.equal(got["hist"][r], ref["hist"][r])
            assert torch.equal(got["score"][r], ref["score"][r])
