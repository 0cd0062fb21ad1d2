"""Executable statement of the split-fp16 product every dense kernel of the library implements.

An fp32 activation x is split as ``hi = fp16(x)``, ``lo = fp16(x - hi)`` (round to nearest even, fp16 subnormals kept:
what ``(_Float16)`` / ``__builtin_convertvector`` do in the kernels) and both planes are multiplied by the fp16 weights
with fp32 accumulation.  The model keeps everything but the accumulation: the exact ``hi + lo`` in float64 times the
weights in float64.  Against it a kernel may differ only by its fp32 summation; against the true float64 product it also
shows what the split loses on rows of small magnitude ("Numeric range of the products").
"""
import torch
import torch.nn.functional as F

FP16_MAX_IN = 65520.0  # the smallest |x| whose fp16 rounding is infinite


def split(x):
    """(hi, lo) fp16 planes of an fp32 tensor."""
    x = x.float()
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi, lo


def planes_sum(x, single_plane=False):
    """float64 value of the planes that reach the MFMA: hi + lo, or hi alone for the single-plane products."""
    hi, lo = split(x)
    return hi.double() if single_plane else hi.double() + lo.double()


def flush_fp16_subnormals(t):
    """fp16 tensor with its subnormals replaced by zero (the accident the ladder tests exist to catch)."""
    return torch.where(t.abs().float() < 2.0 ** -14, torch.zeros_like(t), t)


def product(x, w, bias=None, single_plane=False, flush=False):
    """float64 [M, N] = (hi + lo) @ w^T (+ bias); x fp32 [M, K], w fp16 [N, K]."""
    hi, lo = split(x)
    if flush:
        hi, lo, w = flush_fp16_subnormals(hi), flush_fp16_subnormals(lo), flush_fp16_subnormals(w)
    a = hi.double() if single_plane else hi.double() + lo.double()
    y = a @ w.double().t()
    if bias is not None:
        y = y + bias.double()
    return y


def in_activation(x, in_act):
    """The input activation of the conv kernels, in fp32 like the kernels apply it before the split."""
    x = x.float()
    if in_act == 1:
        return F.leaky_relu(x, 0.1)
    if in_act == 2:
        return F.leaky_relu(x, 0.01)
    return x


def conv1d(x, w, bias=None, stride=1, pad=0, dil=1, in_act=0, lens=None, single_plane=False):
    """float64 [nb, T_out, cout]; x fp32 [nb, T, cin] (time-major like the kernels), w fp16 [cout, cin, k]."""
    x = x.float().clone()
    if lens is not None:
        for i, n in enumerate(lens):
            x[i, n:] = 0
    a = planes_sum(in_activation(x, in_act), single_plane)
    y = F.conv1d(a.transpose(1, 2), w.double(), None if bias is None else bias.double(), stride=stride, padding=pad, dilation=dil)
    return y.transpose(1, 2)


def conv_transpose1d(x, w, bias=None, stride=1, pad=0, in_act=0):
    """float64 [nb, T_out, cout]; x fp32 [nb, T, cin], w fp16 [cin, cout, k]."""
    a = planes_sum(in_activation(x, in_act))
    y = F.conv_transpose1d(a.transpose(1, 2), w.double(), None if bias is None else bias.double(), stride=stride, padding=pad)
    return y.transpose(1, 2)


def rel_rows(y, ref):
    """Per row: max |y - ref| over the row / max |ref| over the row.  A row whose reference is all zero must be equal
    (0 if it is, inf if not).  Rows are the leading dimensions, the last dimension is the row."""
    y, ref = y.double(), ref.double()
    err = (y - ref).abs().amax(dim=-1)
    mag = ref.abs().amax(dim=-1)
    zero = mag == 0
    rel = err / torch.where(zero, torch.ones_like(mag), mag)
    return torch.where(zero, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))), rel)


def rel_cols(y, ref):
    """rel_rows over the columns of a [M, N] result (the weight ladder scales whole output columns)."""
    return rel_rows(y.transpose(-1, -2), ref.transpose(-1, -2))


def uniform(*shape, gen):
    """uniform(-1, 1) in fp32 with all 24 significand bits random: drawn in float64 and rounded (torch.rand in fp32 yields
    multiples of 2^-24, which hi + lo represents exactly - the split would never be seen to round)."""
    return (torch.rand(*shape, generator=gen, dtype=torch.float64) * 2 - 1).float()


LADDER = (-24, -20, -16, -12, -8, -4, 0, 4, 8, 12, 15)
WEIGHT_LADDER = (0, -6, -10, -14, -18)


def ladder_rows(M, K, gen, exps=LADDER, edge_rows=True):
    """fp32 [M, K]: row r is uniform(-1, 1) * 2^exps[r % len]; with edge_rows the last three rows are (a) unit scale with
    +-65504 and +-65519 (the largest fp32 that still rounds to a finite fp16) at a few places, (b) all zero, (c) 2^-20
    and 2^8 elements mixed.  Returns (x, exponent per row or None for the edge rows)."""
    x = uniform(M, K, gen=gen)
    n = M - 3 if edge_rows else M
    es = [exps[r % len(exps)] for r in range(n)]
    for r, e in enumerate(es):
        x[r] *= 2.0 ** e
    if edge_rows:
        big = torch.tensor([65504.0, -65504.0, 65519.0, -65519.0])
        pos = torch.randperm(K, generator=gen)[:4]
        x[n, pos] = big
        x[n + 1] = 0
        x[n + 2] *= torch.where(torch.rand(K, generator=gen) < 0.5, 2.0 ** -20, 2.0 ** 8)
        es = es + [None, None, None]
    return x, es


def ladder_weights(N, K, gen, weight_ladder=False):
    """fp16 [N, K] = randn / sqrt(K); with weight_ladder row n is scaled by 2^WEIGHT_LADDER[n % 5], so that whole output
    columns come from subnormal fp16 weights."""
    w = torch.randn(N, K, generator=gen) / K ** 0.5
    if weight_ladder:
        w = w * torch.tensor([2.0 ** WEIGHT_LADDER[n % len(WEIGHT_LADDER)] for n in range(N)])[:, None]
    return w.half()


def mfma_subnormal_allowance(x, w, single_plane=False):
    """[M, N] absolute allowance for what the fp16 MFMA does with subnormal operands (measured on the MI355X):
    they are kept, not flushed, but the dot product is aligned on the operands' exponent FIELDS, and a subnormal's field
    says 2^-14 whatever its leading bit.  A product with a subnormal operand is therefore rounded like a value of the
    nominal size max(|a|, 2^-14) * max(|w|, 2^-14) to the 24 bits of the fp32 accumulator: an error of up to 2^-24 of
    the nominal size, of either sign, per such product.  Independent roundings add in quadrature; the allowance is 4
    times the root of the summed squares over the products of the row and column that have a subnormal operand (4 sigma
    of a bound that is itself a worst case per product).  Zero where every operand is normal or zero, so the bar itself is
    untouched at unit scale; a flushed subnormal would miss it by the whole value."""
    tiny = 2.0 ** -14
    hi, lo = split(x)
    planes = (hi,) if single_plane else (hi, lo)
    wa = w.double().abs()
    w_nom = torch.where((wa > 0) & (wa < tiny), torch.full_like(wa, tiny), wa) ** 2
    w_normal = torch.where(wa >= tiny, wa, torch.zeros_like(wa)) ** 2
    total = 0.0
    for p in planes:
        pa = p.double().abs()
        p_nom = torch.where((pa > 0) & (pa < tiny), torch.full_like(pa, tiny), pa) ** 2
        p_normal = torch.where(pa >= tiny, pa, torch.zeros_like(pa)) ** 2
        total = total + p_nom @ w_nom.t() - p_normal @ w_normal.t()
    return 4 * 2.0 ** -24 * total.clamp(min=0).sqrt()


def fp32_product(x, w):
    """The planes' product with plain fp32 PyTorch arithmetic: what is left between a kernel and `product` is fp32
    summation, and this is one fp32 summation - the bars of the ladder tests must hold for it with room to spare."""
    hi, lo = split(x)
    wt = w.float().t()
    return hi.float() @ wt + lo.float() @ wt


def fp32_conv1d(x, w, stride=1, pad=0, dil=1, in_act=0, lens=None):
    x = x.float().clone()
    if lens is not None:
        for i, n in enumerate(lens):
            x[i, n:] = 0
    hi, lo = split(in_activation(x, in_act))
    f = lambda p: F.conv1d(p.float().transpose(1, 2), w.float(), None, stride=stride, padding=pad, dilation=dil)
    return (f(hi) + f(lo)).transpose(1, 2)


# The product families of the ladder tests (tests/test_product_range_gpu.py) and their shapes: name, M, N, K, bar, extra.
# M = 28: two cycles of the ladder plus the three edge rows.  M = 3: the ladder rows -12, 0, 12.  `big`: the ladder cycles
# over all rows (the smallest M, N of test_ops_gpu.PRESPLIT_SHAPES that select the 128- and the 256-wide tile).
PRODUCT_CASES = [
    ("linear_general", 28, 96, 256, 2e-6, {}),
    ("linear_general", 28, 100, 160, 2e-6, {}),
    ("linear_fast", 28, 96, 256, 2e-6, {}),
    ("linear_fast", 28, 100, 160, 2e-6, {}),
    ("gemv", 3, 1003, 1024, 2e-6, {"exact": True}),  # fp32 FMA on x itself: the model is the float64 product
    ("presplit", 28, 96, 256, 2e-6, {}),
    ("presplit", 333, 100, 160, 2e-6, {}),
    ("presplit", 4100, 1024, 96, 2e-6, {"big": True, "tile": 128}),
    ("presplit", 15968, 1024, 96, 2e-6, {"big": True, "tile": 256}),
    ("skinny", 28, 128, 256, 2e-6, {}),
    ("skinny_res_ln", 16, 128, 1024, 2e-6, {"splits": 4}),
    ("skinny_res_ln", 3, 128, 256, 2e-6, {"splits": 0}),
    ("dstep_res_ln", 16, 128, 1024, 2e-6, {"splits": 4}),
    ("dstep_res_ln", 3, 128, 256, 2e-6, {"splits": 0}),
    ("dstep_planes", 28, 256, 128, 2e-6, {"planes": True}),
    ("dstep3_resid", 28, 128, 256, 2e-6, {}),
    ("dstep3_partial", 28, 128, 256, 2e-6, {"shape": 0}),
    ("dstep3_partial", 28, 128, 1024, 2e-6, {"shape": 2}),
    # sc_op_dstep3_gemv modes 0 and 2: the ladder is on the LayerNorm's input, the split on its output
    ("dstep3_ln_rows", 28, 128, 128, 2e-6, {"ln": True}),
    ("dstep3_ln_planes", 28, 128, 128, 2e-6, {"ln": True, "planes": True}),
]


def ln_params(case):
    """(gamma, beta) of the LayerNorm in front of a `ln` case's product"""
    K = case[3]
    gen = torch.Generator().manual_seed(77 + K)
    return torch.rand(K, generator=gen) + 0.5, torch.randn(K, generator=gen) * 0.1


def split_input(case, x, dtype=torch.float64):
    """The fp32 activations a case's kernel splits: x itself, or for the `ln` cases LayerNorm(x) (eps 1e-5) computed in
    `dtype` and rounded to fp32 (float64: the model; float32: the plain restatement)."""
    if not case[5].get("ln"):
        return x.float()
    g, b = ln_params(case)
    return F.layer_norm(x.to(dtype), (case[3],), g.to(dtype), b.to(dtype), 1e-5).float()


def case_model(case, x, w):
    """float64 model of a PRODUCT_CASES entry: the float64 product itself for the kernels that do not split (`exact`),
    else `product` on the activations the kernel splits; through the output planes where the hook returns those."""
    if case[5].get("exact"):
        return x.double() @ w.double().t()
    y = product(split_input(case, x), w)
    return planes_sum(y.float()) if case[5].get("planes") else y


def case_true(case, x, w):
    """the float64 product without any split (what the split's own loss is measured against)"""
    a = x.double()
    if case[5].get("ln"):
        g, b = ln_params(case)
        a = F.layer_norm(a, (case[3],), g.double(), b.double(), 1e-5)
    return a @ w.double().t()


def case_fp32(case, x, w):
    """the same in plain fp32 PyTorch (LayerNorm included)"""
    if case[5].get("exact"):
        return x @ w.float().t()
    return fp32_product(split_input(case, x, torch.float32), w)


def case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" + ("".join(f"-{k}{v}" for k, v in c[5].items() if k in ("splits", "shape")))


def product_inputs(case, weight_ladder=False):
    """(x fp32 [M, K], exponent per row, w fp16 [N, K]) of a PRODUCT_CASES entry, seeded by its shape.  With the weight
    ladder the metric is per column, and a column's maximum has to be taken over comparable values to be a denominator
    (a single dot product may cancel to anything): A is then uniform(-1, 1) in every row, and only the shapes of
    WEIGHT_LADDER_CASES (M >= 16) take part."""
    name, M, N, K, _, extra = case
    gen = torch.Generator().manual_seed(1000 * M + 10 * N + K + (7 if weight_ladder else 0))
    if weight_ladder:
        x, es = uniform(M, K, gen=gen), [0] * M
    elif M <= 3:
        x, es = ladder_rows(M, K, gen, exps=(-12, 0, 12), edge_rows=False)
    else:
        x, es = ladder_rows(M, K, gen, edge_rows=not extra.get("big"))
    return x, es, ladder_weights(N, K, gen, weight_ladder)


WEIGHT_LADDER_CASES = [c for c in PRODUCT_CASES if c[1] >= 16 and not c[5].get("big")]
# The M = 3 shapes (the fp32 GEMV, the res_ln hooks without split-K) under the weight ladder: no column maximum to divide
# by, so every element is held to bar * sum_k |a_k| |w_k| - the size an fp32 summation's error scales with (its worst case
# is K * 2^-24 of that sum, its typical error sqrt(K) * 2^-24 of the far smaller partial sums), and one that a flushed
# subnormal weight column (error = the whole value, about the sum / sqrt(K)) misses by orders of magnitude.
WEIGHT_LADDER_SMALL_CASES = [c for c in PRODUCT_CASES if c[1] < 16]


def abs_products(case, x, w):
    """[M, N] sum_k |a_k| |w_k| of the activations the case's kernel multiplies"""
    a = x.float() if case[5].get("exact") else split_input(case, x)
    return a.double().abs() @ w.double().abs().t()


# nb, T, cin, cout, k, stride, pad, dil, in_act, lens; the ladder runs over the (item, time) rows
CONV_CASES = [
    (2, 61, 128, 128, 7, 1, 3, 1, 0, [61, 20]),
    (1, 300, 64, 64, 11, 1, 25, 5, 1, None),
    (2, 64, 128, 256, 8, 8, 4, 1, 0, None),  # the adaptor's strided convolution: sc_op_conv1d only
]


def conv_inputs(case):
    nb, T, cin, cout, k, stride, pad, dil, in_act, lens = case
    gen = torch.Generator().manual_seed(T * 31 + cin + k)
    x, es = ladder_rows(nb * T, cin, gen)
    w = (torch.randn(cout, cin, k, generator=gen) / (cin * k) ** 0.5).half()
    return x.reshape(nb, T, cin), es, w


def ecapa_chain(x, W, chunk, scale, dil, dt):
    """The fused Res2Net chain of k_ecapa.hip on the planes: chunk 0 passes through, chunk j = LayerNorm(ReLU(conv_{k=3,
    dil}(split(x_j + y_{j-1})) + b)) (eps 1e-12, y_0 not added), y carried in fp32.  x [nb, T, scale * chunk] fp32, W: "w"
    [scale - 1, chunk, chunk, 3] fp16, "b", "g", "be" [scale - 1, chunk].  dt float64: the model; float32: the plain
    restatement the bar is measured with.  Returns [nb, T, scale * chunk] in dt."""
    outs, y = [x[..., :chunk].to(dt)], None
    for j in range(1, scale):
        inp = x[..., j * chunk:(j + 1) * chunk].float()
        if j >= 2:
            inp = inp + y
        hi, lo = split(inp)
        w = W["w"][j - 1].to(dt)
        conv = lambda p: F.conv1d(p.to(dt).transpose(1, 2), w, None, dilation=dil, padding=dil).transpose(1, 2)
        v = conv(hi.double() + lo.double()) if dt == torch.float64 else conv(hi) + conv(lo)
        v = F.relu(v + W["b"][j - 1].to(dt))
        v = F.layer_norm(v, (chunk,), W["g"][j - 1].to(dt), W["be"][j - 1].to(dt), 1e-12)
        y = v.float()
        outs.append(v)
    return torch.cat(outs, dim=-1)


def seanet_resblock(x, w1, b1, w2, b2, dt):
    """x + conv_{k=1}(elu(conv_{k=3}(elu(x)) + b1)) + b2 of one item, x [T, C]; k_seanet.hip multiplies in fp32 without a
    split, so float64 of this is its model at every scale."""
    xt = x.to(dt).t().unsqueeze(0)
    h = F.conv1d(F.elu(xt), w1.to(dt), b1.to(dt), padding=1)
    return (xt + F.conv1d(F.elu(h), w2.to(dt), b2.to(dt)))[0].t()
