"""The range of the split-fp16 products on the device: every product family against tests/split_model.py (the exact
hi + lo planes in float64 times the weights) over a ladder of row scales 2^-24 .. 2^15, over a ladder of weight scales
down into the fp16 subnormals, and with one row poisoned by an overflowing or NaN element.

Against the model only the kernel's fp32 summation is left, so the bar is the one the family's unit-scale test asserts,
here per row (max abs error of the row / max abs value of the row) and at every scale.  The per-scale error against the
true float64 product - the measured counterpart of the table in DESIGN.md, "Numeric range of the products" - goes to
range_report.txt in the report directory.
"""
import ctypes as C

import pytest
import torch

from tests import split_model as sm

pytestmark = pytest.mark.gpu


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


def _log(report_dir, name, **kw):
    with open(report_dir / "range_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


# --------------------------------------------------------------------------------------------------------------------- #
# the product hooks: run(lib, x [M, K] fp32, w [N, K] fp16, bias [N] or None, act) -> dict of host tensors, "y" [M, N] first
# --------------------------------------------------------------------------------------------------------------------- #
def _run_product(lib, case, x, w, bias=None, act=0):
    name, M, N, K, _, extra = case
    dx, dw = dev(x), dev(w)
    db = dev(bias) if bias is not None else None
    y = _nan(M, N)
    out = {}
    if name in ("linear_general", "linear_fast"):
        check(lib, lib.sc_op_force_general_gemm(1 if name == "linear_general" else 0))
        try:
            check(lib, lib.sc_op_linear(P(dx), P(dw), P(db), P(None), P(y), M, N, K, act, 1.0, 1, 0))
        finally:
            check(lib, lib.sc_op_force_general_gemm(0))
    elif name == "gemv":
        check(lib, lib.sc_op_linear(P(dx), P(dw), P(db), P(None), P(y), M, N, K, act, 1.0, 1, 1))
    elif name == "presplit":
        yh, yl = _nan(M, N, dtype=torch.float16), _nan(M, N, dtype=torch.float16)
        check(lib, lib.sc_op_linear_presplit(P(dx), P(dw), P(db), P(None), P(y), P(yh), P(yl), M, N, K, act, 1.0))
        out["hi"], out["lo"] = yh.cpu(), yl.cpu()
    elif name == "skinny":
        check(lib, lib.sc_op_skinny_linear(P(dx), P(dw), P(db), P(None), P(y), M, N, K, act, 1.0))
    elif name in ("skinny_res_ln", "dstep_res_ln"):
        # x_inout starts at zero, gamma = 1, beta = 0: x_inout = product + bias, h = LayerNorm(x_inout)
        fn = lib.sc_op_skinny_res_ln if name == "skinny_res_ln" else lib.sc_op_dstep_res_ln
        y.zero_()
        h = _nan(M, N)
        zb = db if db is not None else dev(torch.zeros(N))
        check(lib, fn(P(dx), P(dw), P(zb), P(y), P(dev(torch.ones(N))), P(dev(torch.zeros(N))), P(h), M, N, K, extra["splits"]))
        out["h"] = h.cpu()
    elif name == "dstep_planes":
        zb = db if db is not None else dev(torch.zeros(N))
        check(lib, lib.sc_op_dstep_linear_planes(P(dx), P(dw), P(zb), P(y), M, N, K, act))
    elif name == "dstep3_resid":
        zb = db if db is not None else dev(torch.zeros(N))
        check(lib, lib.sc_op_dstep3_gemv(1, P(dx), P(dw), P(zb), P(None), P(None), P(dev(torch.zeros(M, N))), P(y), P(None), M, N, K, 0, 16, 0))
    elif name == "dstep3_partial":
        zb = db if db is not None else dev(torch.zeros(N))
        check(lib, lib.sc_op_dstep3_gemv(3, P(dx), P(dw), P(zb), P(None), P(None), P(dev(torch.zeros(M, N))), P(y), P(None), M, N, K, 0, 0,
                                         extra["shape"]))
    elif name in ("dstep3_ln_rows", "dstep3_ln_planes"):
        ga, be = sm.ln_params(case)
        zb = db if db is not None else dev(torch.zeros(N))
        mode = 0 if name == "dstep3_ln_rows" else 2
        check(lib, lib.sc_op_dstep3_gemv(mode, P(dx), P(dw), P(zb), P(dev(ga)), P(dev(be)), P(None), P(y), P(None), M, N, K, act,
                                         extra.get("rg", 16), extra.get("shape", 0)))
    else:
        raise AssertionError(name)
    return {"y": y.cpu(), **out}


# activations each hook's epilogue takes (0 none, 1 ReLU, 2 SiLU, 3 tanh)
_ACTS = {"linear_general": (0, 1, 2, 3), "linear_fast": (0, 1, 2, 3), "gemv": (0, 1, 2, 3), "presplit": (0, 1, 2, 3), "skinny": (0, 1, 2, 3),
         "skinny_res_ln": (0,), "dstep_res_ln": (0,), "dstep_planes": (0, 1), "dstep3_resid": (0,), "dstep3_partial": (0,), "dstep3_ln_rows": (0,), "dstep3_ln_planes": (0, 1)}


def _per_scale(rel, es):
    """{exponent (or 'edge'): largest entry of rel over the rows of that scale}"""
    d = {}
    for r, e in zip(rel.tolist(), es):
        k = "edge" if e is None else e
        d[k] = max(d.get(k, 0.0), r)
    return {k: f"{v:.1e}" for k, v in d.items()}


def _planes_quantum(case):
    # A hook that hands its result on as fp16 planes returns hi + lo: the value to 2^-22 relative, and no finer than the
    # smallest fp16 subnormal, 2^-24 (the lo plane of a small value is subnormal or zero).  One such step is allowed on top
    # of the bar for these hooks, since the kernel's fp32 value and the model's may round to different sides.
    return 2.0 ** -24 if case[5].get("planes") else 0.0


def _mfma(case, x, w):
    # the MFMA's treatment of subnormal fp16 operands (sm.mfma_subnormal_allowance); the fp32 FMA kernel has none
    return 0.0 if case[5].get("exact") else sm.mfma_subnormal_allowance(sm.split_input(case, x), w)


@pytest.mark.parametrize("case", sm.PRODUCT_CASES, ids=sm.case_id)
def test_row_scale_ladder(lib, report_dir, case):
    """Measured on the MI355X: every family meets its bar against the model on every row down to 2^-16 (2.7e-6 at 2^-20); on the 2^-24 rows
    (hi itself a subnormal of one or two quanta) the products are 1e-5 .. 2.5e-5 of the row's maximum off the model, the
    same in every family - the MFMA's alignment of subnormal operands, not a kernel's split.  The bar is
    therefore asserted with sm.mfma_subnormal_allowance on top, which is zero wherever no operand is subnormal."""
    name, M, N, K, bar, extra = case
    if "tile" in extra:
        assert lib.sc_op_pretssel_postnet_tile(M, N) == extra["tile"]
    x, es, w = sm.product_inputs(case)
    true = sm.case_true(case, x, w)
    model = sm.case_model(case, x, w)
    out = _run_product(lib, case, x, w)
    y = out["y"]
    err = (y.double() - model).abs()
    allowed = bar * model.abs().amax(dim=1, keepdim=True) + _planes_quantum(case) + _mfma(case, x, w)
    rel = sm.rel_rows(y, model)
    _log(report_dir, "row_ladder", case=sm.case_id(case), worst_vs_model=f"{float(rel.max()):.2e}", vs_model=_per_scale(rel, es),
         vs_float64=_per_scale(sm.rel_rows(y, true), es))
    assert torch.isfinite(y).all()
    bad = (err > allowed).any(dim=1).nonzero().flatten().tolist()
    assert not bad, [(r, es[r], float(rel[r])) for r in bad]
    if "hi" in out:  # the epilogue's split planes, down into the fp16 subnormals on the small rows
        hi = y.half()
        assert torch.equal(out["hi"], hi)
        assert torch.equal(out["lo"], (y - hi.float()).half())
        assert float(out["hi"].float().abs()[out["hi"] != 0].min()) < 2.0 ** -14  # subnormal outputs did occur
    if extra.get("planes"):
        assert torch.equal(sm.planes_sum(y), y.double())  # the result is a sum of two fp16 planes


@pytest.mark.parametrize("case", sm.WEIGHT_LADDER_CASES, ids=sm.case_id)
def test_weight_scale_ladder(lib, report_dir, case):
    """Weight row n scaled by 2^-{0, 6, 10, 14, 18}: whole output columns come from subnormal fp16 weights."""
    name, M, N, K, bar, extra = case
    x, es, w = sm.product_inputs(case, weight_ladder=True)
    assert int(((w != 0) & (w.float().abs() < 2.0 ** -14)).sum()) > N * K // 5  # two of five weight rows are subnormal
    model = sm.case_model(case, x, w)
    y = _run_product(lib, case, x, w)["y"]
    err = (y.double() - model).abs()
    allowed = bar * model.abs().amax(dim=0, keepdim=True) + _planes_quantum(case) + _mfma(case, x, w)
    rel = sm.rel_cols(y, model)
    ws = [sm.WEIGHT_LADDER[n % len(sm.WEIGHT_LADDER)] for n in range(N)]
    _log(report_dir, "weight_ladder", case=sm.case_id(case), worst_vs_model=f"{float(rel.max()):.2e}", vs_model=_per_scale(rel, ws),
         vs_float64=_per_scale(sm.rel_cols(y, sm.case_true(case, x, w)), ws))
    bad = (err > allowed).any(dim=0).nonzero().flatten().tolist()
    assert not bad, [(n, ws[n], float(rel[n])) for n in bad]


@pytest.mark.parametrize("case", sm.WEIGHT_LADDER_SMALL_CASES, ids=sm.case_id)
def test_weight_scale_ladder_three_rows(lib, report_dir, case):
    """The M = 3 shapes under the weight ladder, every element against bar * sum_k |a_k| |w_k| (split_model.py:
    WEIGHT_LADDER_SMALL_CASES)."""
    name, M, N, K, bar, extra = case
    x, es, w = sm.product_inputs(case, weight_ladder=True)
    model = sm.case_model(case, x, w)
    y = _run_product(lib, case, x, w)["y"]
    err = (y.double() - model).abs()
    scale = sm.abs_products(case, x, w)
    _log(report_dir, "weight_ladder_3rows", case=sm.case_id(case), worst_of_abs_products=f"{float((err / scale).max()):.2e}")
    assert (err <= bar * scale + _mfma(case, x, w)).all(), float((err / scale).max())


# --------------------------------------------------------------------------------------------------------------------- #
# convolutions
# --------------------------------------------------------------------------------------------------------------------- #
def _pack(lib, w):
    cout, cin, k = w.shape
    wp = torch.zeros(cout, (cin * k + 31) // 32 * 32, dtype=torch.float16, device="cuda")
    check(lib, lib.sc_op_pack_conv_weight(P(dev(w)), P(wp), cout, cin, k))
    _KEEP.append(wp)
    return wp


def _run_conv(lib, hook, case, x, wp, bias, act=0):
    nb, T, cin, cout, k, stride, pad, dil, in_act, lens = case
    t_out = (T + 2 * pad - dil * (k - 1) - 1) // stride + 1
    y = _nan(nb, t_out, cout)
    d_lens = dev(torch.tensor(lens, dtype=torch.int32)) if lens is not None else None
    if hook == "conv1d":
        check(lib, lib.sc_op_conv1d(P(dev(x)), P(wp), P(dev(bias)), P(None), P(y), nb, T, cin, cout, k, stride, pad, dil, P(d_lens), in_act, act))
        return {"y": y.cpu()}
    # the presplit hook takes planes of x as it is: the input activation and the length mask are applied here, in fp32
    xin = x.clone()
    if lens is not None:
        for i, n in enumerate(lens):
            xin[i, n:] = 0
    xin = sm.in_activation(xin, in_act)
    yh, yl = _nan(nb, t_out, cout, dtype=torch.float16), _nan(nb, t_out, cout, dtype=torch.float16)
    check(lib, lib.sc_op_conv1d_presplit(P(dev(xin)), P(wp), P(dev(bias)), P(None), P(y), P(yh), P(yl), nb, T, cin, cout, k, pad, dil, P(None), act))
    return {"y": y.cpu(), "hi": yh.cpu(), "lo": yl.cpu()}


_CONV_RUNS = [("conv1d", c) for c in sm.CONV_CASES] + [("conv1d_presplit", c) for c in sm.CONV_CASES if c[5] == 1]
_conv_id = lambda v: v if isinstance(v, str) else f"T{v[1]}-{v[2]}to{v[3]}-k{v[4]}"


@pytest.mark.parametrize("hook,case", _CONV_RUNS, ids=_conv_id)
def test_conv_row_scale_ladder(lib, report_dir, hook, case):
    """The ladder over the (item, time) rows of the input; an output row sums the rows within tap reach."""
    nb, T, cin, cout, k, stride, pad, dil, in_act, lens = case
    x, es, w = sm.conv_inputs(case)
    bias = torch.zeros(cout)
    model = sm.conv1d(x, w, None, stride, pad, dil, in_act, lens)
    xt = x.clone()
    if lens is not None:
        for i, n in enumerate(lens):
            xt[i, n:] = 0
    true = torch.nn.functional.conv1d(sm.in_activation(xt, in_act).double().transpose(1, 2), w.double(), None, stride=stride, padding=pad,
                                      dilation=dil).transpose(1, 2)
    out = _run_conv(lib, hook, case, x, _pack(lib, w), bias)
    y = out["y"]
    rel = sm.rel_rows(y, model).flatten()
    rel_true = sm.rel_rows(y, true).flatten()
    _log(report_dir, "conv_ladder", hook=hook, case=_conv_id(case), worst_vs_model=f"{float(rel.max()):.2e}",
         worst_vs_float64=f"{float(rel_true[torch.isfinite(rel_true)].max()):.2e}")
    assert torch.isfinite(y).all()
    assert float(rel.max()) <= 3e-6, float(rel.max())
    if "hi" in out:
        hi = y.half()
        assert torch.equal(out["hi"], hi)
        assert torch.equal(out["lo"], (y - hi.float()).half())


@pytest.mark.parametrize("general", [1, 0], ids=["general", "fast"])
def test_conv_transpose_row_scale_ladder(lib, report_dir, general):
    """sc_op_conv_transpose1d folds the weight norm on the device and rounds the folded weights to fp16 once (2^-11 per
    weight): its own test's bar, 1e-3, here per output row."""
    nb, T, cin, cout, k, s = 3, 77, 32, 16, 8, 4
    g = torch.Generator().manual_seed(T + cin + k)
    x, es = sm.ladder_rows(nb * T, cin, g)
    x = x.reshape(nb, T, cin)
    v = (torch.randn(cin, cout, k, generator=g) / (cin * k) ** 0.5).half()
    gg = (torch.rand(cin, 1, 1, generator=g) + 0.5).half()
    pad = (k - s) // 2
    wn = gg.double() * v.double() / v.double().reshape(cin, -1).norm(dim=1).reshape(cin, 1, 1)
    model = torch.nn.functional.conv_transpose1d(sm.planes_sum(sm.in_activation(x, 1)).transpose(1, 2), wn, None, stride=s, padding=pad).transpose(1, 2)
    y = _nan(nb, T * s, cout)
    check(lib, lib.sc_op_force_general_gemm(general))
    try:
        check(lib, lib.sc_op_conv_transpose1d(P(dev(x)), P(dev(v)), P(dev(gg)), P(dev(torch.zeros(cout))), P(y), nb, T, cin, cout, k, s, pad, 1))
    finally:
        check(lib, lib.sc_op_force_general_gemm(0))
    rel = sm.rel_rows(y.cpu(), model)
    _log(report_dir, "conv_transpose_ladder", general=general, worst_vs_model=f"{float(rel.max()):.2e}")
    assert torch.isfinite(y).all()
    assert float(rel.max()) <= 1e-3, float(rel.max())


def _resblock_model(x, w1, b1, w2, b2, k, dil, single):
    """x + conv2(split(lrelu(fp32(conv1(split(lrelu(x))) + b1)))) + b2 in float64 on the planes"""
    h = sm.conv1d(x, w1, b1, 1, dil * (k - 1) // 2, dil, 1, None, single)
    return sm.conv1d(h.float(), w2, b2, 1, (k - 1) // 2, 1, 1, None, single) + x.double()


@pytest.mark.parametrize("hook,C_,k,dil,single,bar", [("pair", 32, 3, 3, 0, 3e-6), ("pair", 32, 3, 3, 1, 3e-6), ("pair_ps", 128, 3, 1, 0, 3e-6)],
                         ids=["pair", "pair_single_plane", "pair_ps"])
def test_resblock_pair_row_scale_ladder(lib, report_dir, hook, C_, k, dil, single, bar):
    """One HiFi-GAN dilation pair.  Against the model the bar is test_resblock_pair_bit_identical_to_two_convs' 3e-6; with
    a single plane the model multiplies hi only, so the plane's 2^-11 is inside the model and the same bar is left."""
    nb, T = 1, 200
    g = torch.Generator().manual_seed(T * 13 + C_ * 5 + k + dil)
    x, es = sm.ladder_rows(nb * T, C_, g)
    x = x.reshape(nb, T, C_)
    w1 = (torch.randn(C_, C_, k, generator=g) / (C_ * k) ** 0.5).half()
    w2 = (torch.randn(C_, C_, k, generator=g) / (C_ * k) ** 0.5).half()
    b1, b2 = torch.randn(C_, generator=g) * 0.1, torch.randn(C_, generator=g) * 0.1
    model = _resblock_model(x, w1, b1, w2, b2, k, dil, bool(single))
    y = _nan(nb, T, C_)
    check(lib, lib.sc_op_single_plane(single))
    try:
        if hook == "pair":
            check(lib, lib.sc_op_resblock_pair(P(dev(x)), P(_pack(lib, w1)), P(dev(b1)), P(_pack(lib, w2)), P(dev(b2)), P(y), nb, T, C_, k, dil, 0.1,
                                               P(None), P(None)))
        else:
            check(lib, lib.sc_op_resblock_pair_ps(P(dev(x)), P(_pack(lib, w1)), P(dev(b1)), P(_pack(lib, w2)), P(dev(b2)), P(y), nb, T, C_, k, dil))
    finally:
        check(lib, lib.sc_op_single_plane(0))
    rel = sm.rel_rows(y.cpu(), model).flatten()
    _log(report_dir, "resblock_ladder", hook=hook, single=single, worst_vs_model=f"{float(rel.max()):.2e}", vs_model=_per_scale(rel, es))
    assert torch.isfinite(y).all()
    assert float(rel.max()) <= bar, float(rel.max())


# --------------------------------------------------------------------------------------------------------------------- #
# one poisoned row: loud and isolated
# --------------------------------------------------------------------------------------------------------------------- #
_POISON = {"overflow": 70000.0, "nan": float("nan")}
# (the fp32 FMA kernel behind force_gemv does not split: 70000 is an ordinary value there; in front of a LayerNorm it is
# normalised away.)  The last case is mode 2 of sc_op_dstep3_gemv with the weights stationary (gemv3s_kernel: two row
# groups walked by one workgroup), which has a ReLU epilogue of its own.
_STATIONARY = ("dstep3_ln_planes", 28, 128, 128, 2e-6, {"ln": True, "planes": True, "rg": 16, "shape": 1 | (1 << 4)})
_POISON_CASES = [(c, p) for c in sm.PRODUCT_CASES + [_STATIONARY] if not c[5].get("big") for p in _POISON
                 if not ((c[5].get("exact") or c[5].get("ln")) and p == "overflow")]


@pytest.mark.parametrize("case,poison", _POISON_CASES, ids=lambda v: sm.case_id(v) if isinstance(v, tuple) else v)
def test_poisoned_row_is_nonfinite_and_alone(lib, case, poison):
    """One element of one row is 70000 (hi = inf, lo = -inf) or NaN: that row of the result is non-finite in every column
    and under every activation of the hook; every other row keeps the bits it has when the row is zero instead."""
    name, M, N, K, _, extra = case
    g = torch.Generator().manual_seed(M + N + K)
    x = sm.uniform(M, K, gen=g) * 2
    w = sm.ladder_weights(N, K, g)
    bias = torch.randn(N, generator=g) * 0.1
    r = 1 if M <= 3 else 5
    rest = [i for i in range(M) if i != r]
    for act in _ACTS[name]:
        xp = x.clone()
        xp[r, 7] = _POISON[poison]
        xz = x.clone()
        xz[r] = 0
        got, clean = _run_product(lib, case, xp, w, bias, act), _run_product(lib, case, xz, w, bias, act)
        for key in got:
            a, b = got[key].float(), clean[key].float()
            assert not torch.isfinite(a[r]).any(), (key, act, a[r][torch.isfinite(a[r])][:4])
            assert torch.equal(a[rest], b[rest]), (key, act)
            assert torch.isfinite(b).all()


def _reach(T_in, t_out, t0, k, stride, pad, dil):
    """output rows whose window holds input row t0"""
    return sorted({(t0 + pad - j * dil) // stride for j in range(k) if (t0 + pad - j * dil) % stride == 0 and 0 <= (t0 + pad - j * dil) // stride < t_out})


@pytest.mark.parametrize("poison", list(_POISON))
@pytest.mark.parametrize("hook,case", _CONV_RUNS, ids=_conv_id)
def test_poisoned_conv_row_reaches_its_taps_only(lib, hook, case, poison):
    """The rows within tap reach of the poisoned input row, in the same item, are non-finite in every channel (ReLU and tanh
    epilogues and the LeakyReLU input activation included); all other rows and the other items keep their bits."""
    nb, T, cin, cout, k, stride, pad, dil, in_act, lens = case
    g = torch.Generator().manual_seed(T + cin)
    x = sm.uniform(nb, T, cin, gen=g) * 2
    w = (torch.randn(cout, cin, k, generator=g) / (cin * k) ** 0.5).half()
    bias = torch.randn(cout, generator=g) * 0.1
    wp = _pack(lib, w)
    item, t0 = nb - 1, 11  # inside the shortest item of the masked case
    for act in (0, 1, 3):
        xp = x.clone()
        xp[item, t0, 3] = _POISON[poison]
        xz = x.clone()
        xz[item, t0] = 0
        got, clean = _run_conv(lib, hook, case, xp, wp, bias, act), _run_conv(lib, hook, case, xz, wp, bias, act)
        t_out = got["y"].shape[1]
        hit = torch.zeros(nb, t_out, dtype=torch.bool)
        hit[item, _reach(T, t_out, t0, k, stride, pad, dil)] = True
        assert int(hit.sum()) >= 1
        for key in got:
            a, b = got[key].float(), clean[key].float()
            assert not torch.isfinite(a[hit]).any(), (key, act)
            assert torch.equal(a[~hit], b[~hit]), (key, act)
            assert torch.isfinite(b).all()


@pytest.mark.parametrize("poison", list(_POISON))
@pytest.mark.parametrize("hook,C_,k,dil,single", [("pair", 32, 3, 3, 0), ("pair", 32, 3, 3, 1), ("pair_ps", 128, 3, 1, 0)],
                         ids=["pair", "pair_single_plane", "pair_ps"])
def test_poisoned_resblock_row(lib, hook, C_, k, dil, single, poison):
    nb, T = 2, 200
    g = torch.Generator().manual_seed(T + C_)
    x = sm.uniform(nb, T, C_, gen=g) * 2
    w1 = (torch.randn(C_, C_, k, generator=g) / (C_ * k) ** 0.5).half()
    w2 = (torch.randn(C_, C_, k, generator=g) / (C_ * k) ** 0.5).half()
    b1, b2 = dev(torch.randn(C_, generator=g) * 0.1), dev(torch.randn(C_, generator=g) * 0.1)
    p1, p2 = _pack(lib, w1), _pack(lib, w2)
    item, t0 = 1, 100
    h = (k - 1) // 2
    mid = {t0 + (j - h) * dil for j in range(k)}  # rows of the intermediate that see x[t0]
    hit = torch.zeros(nb, T, dtype=torch.bool)
    hit[item, sorted({m + j - h for m in mid for j in range(k)})] = True
    outs = []
    for poisoned in (True, False):
        xi = x.clone()
        if poisoned:
            xi[item, t0, 3] = _POISON[poison]
        else:
            xi[item, t0] = 0
        y = _nan(nb, T, C_)
        check(lib, lib.sc_op_single_plane(single))
        try:
            if hook == "pair":
                check(lib, lib.sc_op_resblock_pair(P(dev(xi)), P(p1), P(b1), P(p2), P(b2), P(y), nb, T, C_, k, dil, 0.1, P(None), P(None)))
            else:
                check(lib, lib.sc_op_resblock_pair_ps(P(dev(xi)), P(p1), P(b1), P(p2), P(b2), P(y), nb, T, C_, k, dil))
        finally:
            check(lib, lib.sc_op_single_plane(0))
        outs.append(y.cpu())
    assert not torch.isfinite(outs[0][hit]).any()
    assert torch.equal(outs[0][~hit], outs[1][~hit])
    assert torch.isfinite(outs[1]).all()


@pytest.mark.parametrize("poison", ["nan"])
def test_poisoned_seanet_resblock_row(lib, poison):
    """x + conv_{k=1}(elu(conv_{k=3}(elu(x)))) over packed items (k_seanet.hip): the three rows around the poisoned one, in
    its item, are non-finite; the rest of the item and the neighbouring item keep their bits.  The kernel multiplies in fp32
    without a split, so 70000 is an ordinary value to it: NaN only."""
    import numpy as np

    C_, lens = 32, [70, 30]
    g = torch.Generator().manual_seed(C_)
    w1 = dev((torch.randn(C_ // 2, C_, 3, generator=g) / (3 * C_) ** 0.5).half())
    w2 = dev((torch.randn(C_, C_ // 2, 1, generator=g) / (C_ // 2) ** 0.5).half())
    b1, b2 = dev(torch.randn(C_ // 2, generator=g) * 0.1), dev(torch.randn(C_, generator=g) * 0.1)
    x = sm.uniform(sum(lens), C_, gen=g) * 2
    h_lens = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    t0 = lens[0] - 1  # the last row of item 0: the first row of item 1 is next to it in memory and must not see it
    hit = torch.zeros(sum(lens), dtype=torch.bool)
    hit[t0 - 1: t0 + 1] = True
    outs = []
    for poisoned in (True, False):
        xi = x.clone()
        if poisoned:
            xi[t0, 3] = _POISON[poison]
        else:
            xi[t0] = 0
        y = _nan(sum(lens), C_)
        check(lib, lib.sc_op_seanet_resblock(P(dev(xi)), C.c_void_p(h_lens.ctypes.data), len(lens), C_, P(w1), P(b1), P(w2), P(b2), P(y)))
        outs.append(y.cpu())
    assert not torch.isfinite(outs[0][hit]).any()
    assert torch.equal(outs[0][~hit], outs[1][~hit])
    assert torch.isfinite(outs[1]).all()


@pytest.mark.parametrize("poison", list(_POISON))
def test_poisoned_ecapa_chain_row(lib, poison):
    """The fused Res2Net chain (k_ecapa.hip; conv k = 3 -> ReLU -> norm per chunk, chunk j fed x_j + y_{j-1}): an element of
    chunk 1 that is not a number spreads by one dilation step per chunk, through the ReLU, and no further; chunk 0 (passed
    through) and the other item keep their bits."""
    chunk, scale, dil, nb, T = 64, 8, 2, 2, 48
    g = torch.Generator().manual_seed(7)
    n = scale - 1
    w = dev((torch.randn(n, chunk, chunk, 3, generator=g) * (2.0 / (3 * chunk)) ** 0.5).half())
    b, ga, be = dev(0.1 * torch.randn(n, chunk, generator=g)), dev(1 + 0.1 * torch.randn(n, chunk, generator=g)), dev(0.1 * torch.randn(n, chunk, generator=g))
    x = sm.uniform(nb, T, scale * chunk, gen=g) * 2
    item, t0 = 1, 20
    hit = torch.zeros(nb, T, scale * chunk, dtype=torch.bool)
    for j in range(1, scale):
        for m in range(-j, j + 1):
            if 0 <= t0 + m * dil < T:
                hit[item, t0 + m * dil, j * chunk: (j + 1) * chunk] = True
    outs = []
    for poisoned in (True, False):
        xi = x.clone()
        if poisoned:
            xi[item, t0, chunk + 5] = _POISON[poison]
        else:
            xi[item, t0, chunk: 2 * chunk] = 0
        y = _nan(nb, T, scale * chunk)
        check(lib, lib.sc_op_ecapa_chain(P(dev(xi)), P(w), P(b), P(ga), P(be), P(y), nb, T, chunk, scale, dil))
        outs.append(y.cpu())
    assert not torch.isfinite(outs[0][hit]).any()
    assert torch.equal(outs[0][~hit], outs[1][~hit])
    assert torch.isfinite(outs[1]).all()


@pytest.mark.parametrize("poison", list(_POISON))
def test_poisoned_conv_transpose_row(lib, poison):
    """sc_op_conv_transpose1d (LeakyReLU(0.1) on the input, polyphase product): input row t0 reaches the output rows
    t0 * s - pad .. t0 * s - pad + k - 1 of its item and no other."""
    nb, T, cin, cout, k, s = 3, 77, 32, 16, 8, 4
    g = torch.Generator().manual_seed(T + cin + k)
    x = sm.uniform(nb, T, cin, gen=g) * 2
    v = dev((torch.randn(cin, cout, k, generator=g) / (cin * k) ** 0.5).half())
    gg = dev((torch.rand(cin, 1, 1, generator=g) + 0.5).half())
    b = dev(torch.randn(cout, generator=g) * 0.1)
    pad = (k - s) // 2
    item, t0 = 1, 40
    hit = torch.zeros(nb, T * s, dtype=torch.bool)
    hit[item, t0 * s - pad: t0 * s - pad + k] = True
    outs = []
    for poisoned in (True, False):
        xi = x.clone()
        if poisoned:
            xi[item, t0, 3] = _POISON[poison]
        else:
            xi[item, t0] = 0
        y = _nan(nb, T * s, cout)
        check(lib, lib.sc_op_conv_transpose1d(P(dev(xi)), P(v), P(gg), P(b), P(y), nb, T, cin, cout, k, s, pad, 1))
        outs.append(y.cpu())
    assert not torch.isfinite(outs[0][hit]).any()
    assert torch.equal(outs[0][~hit], outs[1][~hit])
    assert torch.isfinite(outs[1]).all()


# --------------------------------------------------------------------------------------------------------------------- #
# SEANet residual block and ECAPA Res2Net chain: scale ladders
# --------------------------------------------------------------------------------------------------------------------- #
BAR_FP32 = 16.0  # the bar of these kernels' own tests: this many times the error of the plain fp32 restatement


def test_seanet_resblock_row_scale_ladder(lib, report_dir):
    """k_seanet.hip multiplies in fp32 without a split: float64 is its model at every scale, and 65519 is an ordinary value.
    Per row, against 16 x the largest per-row error of the fp32 PyTorch restatement (its own test's bar)."""
    import numpy as np

    C_, lens = 32, [45, 28]
    g = torch.Generator().manual_seed(C_ + 1)
    w1 = (torch.randn(C_ // 2, C_, 3, generator=g) / (3 * C_) ** 0.5).half()
    w2 = (torch.randn(C_, C_ // 2, 1, generator=g) / (C_ // 2) ** 0.5).half()
    b1, b2 = torch.randn(C_ // 2, generator=g) * 0.1, torch.randn(C_, generator=g) * 0.1
    x, es = sm.ladder_rows(sum(lens), C_, g)
    items = list(torch.split(x, lens, 0))
    ref = torch.cat([sm.seanet_resblock(i, w1, b1, w2, b2, torch.float64) for i in items])
    ref32 = torch.cat([sm.seanet_resblock(i, w1, b1, w2, b2, torch.float32) for i in items])
    h_lens = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    y = _nan(sum(lens), C_)
    check(lib, lib.sc_op_seanet_resblock(P(dev(x)), C.c_void_p(h_lens.ctypes.data), len(lens), C_, P(dev(w1)), P(dev(b1)), P(dev(w2)), P(dev(b2)), P(y)))
    rel, rel32 = sm.rel_rows(y.cpu(), ref), sm.rel_rows(ref32, ref)
    _log(report_dir, "seanet_ladder", worst=f"{float(rel.max()):.2e}", fp32_cpu=f"{float(rel32.max()):.2e}", per_scale=_per_scale(rel, es))
    assert torch.isfinite(y).all()
    assert float(rel.max()) <= BAR_FP32 * float(rel32.max()), (float(rel.max()), float(rel32.max()))


def test_ecapa_chain_row_scale_ladder(lib, report_dir):
    """The fused Res2Net chain at the smallest chunk / scale of its own test (32, 4; dilation 2), the ladder over the
    (item, frame) rows.  Model: sm.ecapa_chain in float64 on the planes; bar: 16 x the largest error of the same chain in
    plain fp32, per (row, chunk) - chunk 0 is passed through and must be equal.  The large elements of the edge row sit
    in chunk 1, whose input is x alone (x_j + y_{j-1} of a later chunk could leave the finite range)."""
    chunk, scale, dil, nb, T = 32, 4, 2, 2, 36
    g = torch.Generator().manual_seed(41)
    n = scale - 1
    W = {"w": (torch.randn(n, chunk, chunk, 3, generator=g) * (2.0 / (3 * chunk)) ** 0.5).half(), "b": 0.1 * torch.randn(n, chunk, generator=g),
         "g": 1 + 0.1 * torch.randn(n, chunk, generator=g), "be": 0.1 * torch.randn(n, chunk, generator=g)}
    x, es = sm.ladder_rows(nb * T, scale * chunk, g)
    r = es.index(None)
    big = x[r].abs() > 60000
    vals = x[r][big].clone()
    x[r][big] = 0.5
    x[r, chunk: chunk + len(vals)] = vals
    x = x.reshape(nb, T, scale * chunk)
    model, ref32 = sm.ecapa_chain(x, W, chunk, scale, dil, torch.float64), sm.ecapa_chain(x, W, chunk, scale, dil, torch.float32)
    y = _nan(nb, T, scale * chunk)
    check(lib, lib.sc_op_ecapa_chain(P(dev(x)), P(dev(W["w"])), P(dev(W["b"])), P(dev(W["g"])), P(dev(W["be"])), P(y), nb, T, chunk, scale, dil))
    y = y.cpu()
    per = lambda t: t.reshape(nb * T, scale, chunk)[:, 1:]
    rel, rel32 = sm.rel_rows(per(y), per(model)), sm.rel_rows(per(ref32), per(model))
    _log(report_dir, "ecapa_ladder", worst=f"{float(rel.max()):.2e}", fp32_cpu=f"{float(rel32.max()):.2e}",
         per_scale=_per_scale(rel.amax(dim=1), es))
    assert torch.isfinite(y).all() and torch.isfinite(model).all()
    assert torch.equal(y[..., :chunk], x[..., :chunk])
    assert float(rel.max()) <= BAR_FP32 * float(rel32.max()), (float(rel.max()), float(rel32.max()))


# --------------------------------------------------------------------------------------------------------------------- #
# the other ReLU sites that were made to keep NaN: one NaN row through each
# --------------------------------------------------------------------------------------------------------------------- #
def test_layernorm_relu_keeps_a_nan_row(lib):
    """sc_op_layernorm with act = ReLU (k_norm.hip: act_f)"""
    rows, C_ = 7, 160
    g = torch.Generator().manual_seed(2)
    x = sm.uniform(rows, C_, gen=g) * 3
    ga, be = dev(torch.rand(C_, generator=g) + 0.5), dev(torch.randn(C_, generator=g) * 0.1)
    outs = []
    for poisoned in (True, False):
        xi = x.clone()
        xi[3, 11] = float("nan") if poisoned else 0.0
        y = _nan(rows, C_)
        check(lib, lib.sc_op_layernorm(P(dev(xi)), P(ga), P(be), P(y), rows, C_, 1))
        outs.append(y.cpu())
    rest = [r for r in range(rows) if r != 3]
    assert torch.isnan(outs[0][3]).all()
    assert torch.equal(outs[0][rest], outs[1][rest]) and torch.isfinite(outs[1]).all()
    assert (outs[1] >= 0).all() and (outs[1] == 0).any()  # the ReLU did act


@pytest.mark.parametrize("with_bias", [False, True])
def test_ecapa_relu_ln_keeps_a_nan_row(lib, with_bias):
    """ecapa_relu_ln_kernel: ReLU + LayerNorm over the channels, optionally a per-item bias in front and tanh behind"""
    rows, C_ = 2 * 19, 128
    g = torch.Generator().manual_seed(rows + C_)
    x = sm.uniform(rows, C_, gen=g) * 2
    ga, be = dev(1 + 0.1 * torch.randn(C_, generator=g)), dev(0.1 * torch.randn(C_, generator=g))
    ib = dev(torch.randn(2, C_, generator=g)) if with_bias else None
    outs = []
    for poisoned in (True, False):
        xi = x.clone()
        xi[20, 5] = float("nan") if poisoned else 0.0
        y = _nan(rows, C_)
        check(lib, lib.sc_op_ecapa_relu_ln(P(dev(xi)), P(ib), rows // 2 if with_bias else 0, P(ga), P(be), P(y), rows, C_, 3 if with_bias else 0))
        outs.append(y.cpu())
    rest = [r for r in range(rows) if r != 20]
    assert torch.isnan(outs[0][20]).all()
    assert torch.equal(outs[0][rest], outs[1][rest]) and torch.isfinite(outs[1]).all()


def test_ecapa_se_gate_keeps_a_nan_item(lib):
    """ecapa_se_gate_kernel (masked time mean, 1 x 1 product, ReLU, 1 x 1 product, sigmoid): a NaN frame inside an item's
    length makes that item's gate NaN in every channel; the other items' gates keep their bits."""
    import numpy as np

    Cc, S, T, nb = 512, 128, 40, 3
    g = torch.Generator().manual_seed(4)
    x = sm.uniform(nb, T, Cc, gen=g) + 0.3
    w1, b1 = dev((torch.randn(S, Cc, 1, generator=g) * Cc ** -0.5).half()), dev(0.1 * torch.randn(S, generator=g))
    w2, b2 = dev((torch.randn(Cc, S, 1, generator=g) * S ** -0.5).half()), dev(0.1 * torch.randn(Cc, generator=g))
    hl = np.ascontiguousarray(np.asarray([T, T - 7, 9], dtype=np.int32))
    outs = []
    for poisoned in (True, False):
        xi = x.clone()
        xi[1, 12, 100] = float("nan") if poisoned else 0.0
        gate = _nan(nb, Cc)
        check(lib, lib.sc_op_ecapa_se_gate(P(dev(xi)), nb, T, C.c_void_p(hl.ctypes.data), Cc, S, P(w1), P(b1), P(w2), P(b2), P(gate)))
        outs.append(gate.cpu())
    assert torch.isnan(outs[0][1]).all()
    assert torch.equal(outs[0][[0, 2]], outs[1][[0, 2]]) and torch.isfinite(outs[1]).all()
