"""The written numeric contract of the split-fp16 products ("Numeric range of the products") against its
executable statement (tests/split_model.py): the emulated error table, the LeakyReLU / ReLU expressions of the kernels
over the edge values, and the room the bars of tests/test_product_range_gpu.py leave to an fp32 summation."""
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from tests import split_model as sm

ROOT = Path(__file__).resolve().parent.parent
TABLE_SCALES = (12, 8, 4, 0, -4, -8, -12, -16, -20, -24)


def _emulate(scale, seed=0):
    """(exact split, fp16 subnormals flushed): largest per-row error of a 40 x 96 x 1024 product against float64."""
    M, N, K = 40, 96, 1024
    g = torch.Generator().manual_seed(seed * 100 + scale + 50)
    w = sm.ladder_weights(N, K, g)
    x = sm.uniform(M, K, gen=g) * 2.0 ** scale
    ref = x.double() @ w.double().t()
    return (float(sm.rel_rows(sm.product(x, w), ref).max()), float(sm.rel_rows(sm.product(x, w, flush=True), ref).max()))


def _recorded_table():
    text = (ROOT / "DESIGN.md").read_text()
    sec = text[text.index("| row scale 2^e | exact split | fp16 subnormals flushed |"):]
    sec = sec[:sec.index("\n\n")]  # the emulated table only: the measured tables further down have the same shape
    rows = {}
    for m in re.finditer(r"^\| (-?\d+) \| ([0-9.e+-]+) \| ([0-9.e+-]+) \|$", sec, re.M):
        rows.setdefault(int(m.group(1)), (float(m.group(2)), float(m.group(3))))
    return rows


@pytest.mark.parametrize("scale", TABLE_SCALES)
def test_emulated_table_is_the_one_in_design_md(scale):
    rec = _recorded_table()
    assert scale in rec, f"DESIGN.md has no row for scale 2^{scale}"
    got = _emulate(scale)
    print(scale, got, rec[scale])
    for g, r in zip(got, rec[scale]):
        assert r / 2 <= g <= r * 2, (scale, got, rec[scale])


def test_beyond_the_finite_range_a_row_is_nan():
    g = torch.Generator().manual_seed(3)
    w = sm.ladder_weights(8, 64, g)
    x = sm.uniform(2, 64, gen=g)
    x[1, 5] = sm.FP16_MAX_IN
    y = sm.product(x, w)
    assert torch.isfinite(y[0]).all() and torch.isnan(y[1]).all()
    x[1, 5] = torch.nextafter(torch.tensor(sm.FP16_MAX_IN), torch.tensor(0.0))  # 65519.996: still rounds to 65504
    assert torch.isfinite(sm.product(x, w)).all()


def test_rel_rows():
    ref = torch.tensor([[1.0, -4.0], [0.0, 0.0], [0.0, 0.0]])
    y = torch.tensor([[1.5, -4.0], [0.0, 0.0], [0.0, 1e-30]])
    assert sm.rel_rows(y, ref).tolist() == [0.125, 0.0, float("inf")]


def _edge_values():
    f32 = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38, 1.0, -1.0, 3.3e38, -3.3e38,
                        65504.0, -65519.0, 70000.0, -70000.0, float("inf"), float("-inf")])
    g = torch.Generator().manual_seed(11)
    sweep = (torch.rand(4096, generator=g, dtype=torch.float64) * 2 - 1).float() * 2.0 ** torch.randint(-149, 128, (4096,), generator=g).float()
    return torch.cat([f32, sweep])


@pytest.mark.parametrize("slope", [0.1, 0.01])
def test_leaky_relu_expressions_agree_on_finite_and_infinite_values(slope):
    """kernels.h: lrelu_in keeps max(x, 0) + slope * min(x, 0) - the expression the bit-identity tests were recorded with -
    and hands NaN through.  The select form x > 0 ? x : slope * x (k_resblock.hip) is compared here as well: equal as
    values everywhere (the two differ only in the sign of a zero result), which is why it was not substituted."""
    x = _edge_values()
    s = torch.tensor(slope, dtype=torch.float32)
    kept = torch.clamp(x, min=0) + s * torch.clamp(x, max=0)
    select = torch.where(x > 0, x, s * x)
    assert torch.equal(kept, select)  # value equality: -0 == +0
    assert torch.equal(F.leaky_relu(x, slope), select)
    nan = torch.tensor([float("nan")])
    assert torch.isnan(torch.where(nan != nan, nan, nan.clamp(min=0) + s * nan.clamp(max=0))).all()


def test_relu_expression_keeps_nan_and_every_finite_bit():
    """!(v <= 0) ? v : 0 against v > 0 ? v : 0: the same bits for every value that is a number (-0 -> +0 in both), NaN
    for NaN."""
    x = torch.cat([_edge_values(), torch.tensor([float("nan")])])
    old = torch.where(x > 0, x, torch.zeros_like(x))
    new = torch.where(~(x <= 0), x, torch.zeros_like(x))
    num = ~torch.isnan(x)
    assert torch.equal(old[num].view(torch.int32), new[num].view(torch.int32))
    assert torch.isnan(new[~num]).all() and not torch.isnan(old[~num]).any()


_FP32_CASES = [(c, False) for c in sm.PRODUCT_CASES] + [(c, True) for c in sm.WEIGHT_LADDER_CASES]


@pytest.mark.parametrize("case,weight_ladder", _FP32_CASES, ids=lambda v: sm.case_id(v) if isinstance(v, tuple) else ("cols" if v else "rows"))
def test_fp32_summation_stays_below_half_the_bar(case, weight_ladder):
    """Before a bar is asked of a kernel: plain fp32 PyTorch on the same planes against the model, every row (every column
    under the weight ladder)."""
    x, es, w = sm.product_inputs(case, weight_ladder)
    model = sm.product(sm.split_input(case, x), w) if not case[5].get("exact") else sm.case_model(case, x, w)
    y = sm.case_fp32(case, x, w)
    rel = sm.rel_cols(y, model) if weight_ladder else sm.rel_rows(y, model)
    assert float(rel.max()) <= case[4] / 2, float(rel.max())


@pytest.mark.parametrize("case", sm.CONV_CASES, ids=lambda c: f"T{c[1]}-{c[2]}to{c[3]}-k{c[4]}")
def test_fp32_convolution_stays_below_half_the_bar(case):
    nb, T, cin, cout, k, stride, pad, dil, in_act, lens = case
    x, es, w = sm.conv_inputs(case)
    model = sm.conv1d(x, w, None, stride, pad, dil, in_act, lens)
    rel = sm.rel_rows(sm.fp32_conv1d(x, w, stride, pad, dil, in_act, lens), model)
    assert float(rel.max()) <= 3e-6 / 2, float(rel.max())


@pytest.mark.parametrize("case", sm.WEIGHT_LADDER_SMALL_CASES, ids=sm.case_id)
def test_fp32_summation_stays_below_half_the_elementwise_bar(case):
    x, es, w = sm.product_inputs(case, weight_ladder=True)
    err = (sm.case_fp32(case, x, w).double() - sm.case_model(case, x, w)).abs()
    assert (err <= case[4] / 2 * sm.abs_products(case, x, w)).all(), float((err / sm.abs_products(case, x, w)).max())
