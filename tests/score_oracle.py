"""float64 restatements for the teacher-forced scoring tests: the vocabulary projection on the fp16-rounded weight up-cast
to double, then log_softmax / gather / sum / arg-max - what the fused kernel (k_gemm_ps.hip, SCORE epilogue) computes without
ever forming the logits - and the label-smoothed loss on materialised logits."""
import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24  # fp32 unit round-off


def score_ref(x: torch.Tensor, w_f16: torch.Tensor, bias, target) -> dict:
    """x (M, K) float, w_f16 (N, K) half, bias (N,) or None, target (M,) int (< 0: none) -> float64 statistics per row."""
    logits = F.linear(x.double(), w_f16.double(), bias.double() if bias is not None else None)
    lsm = torch.log_softmax(logits, dim=-1)
    t = torch.as_tensor(np.asarray(target), dtype=torch.int64)
    lprob = lsm.gather(1, t.clamp(min=0)[:, None])[:, 0]
    lprob = torch.where(t >= 0, lprob, torch.zeros_like(lprob))
    top2 = torch.topk(torch.nan_to_num(logits, nan=-float("inf")), min(2, logits.shape[1]), dim=1).values
    return {
        "logits": logits,
        "lse": torch.logsumexp(logits, dim=-1),
        "lprob": lprob,
        "sum_lprob": lsm.sum(dim=-1),
        "top1": np.argmax(logits.numpy(), axis=1),  # first occurrence: the lowest column among equal values
        "margin": top2[:, 0] - top2[:, -1],
        "mean_abs": logits.abs().mean(dim=-1),
    }


def bars(ref: dict, e: torch.Tensor, cols: int, n: int) -> dict:
    """The error bars of the kernel tests (tests/test_score_kernel_gpu.py has the derivation): e = per-row error of the
    parent's product against float64, cols = columns per record, n = columns."""
    c, r = cols, -(-n // cols)
    fl = (c + r + 8) * U24 * ref["lse"].abs().clamp(min=1.0)
    return {"lse": e + fl, "lprob": 2 * e + fl, "sum_lprob_mean": e + fl + (c + r) * U24 * ref["mean_abs"]}


def smoothed_loss_ref(logits: torch.Tensor, targets: torch.Tensor, pad_idx: int, label_smoothing: float, ignore_prefix_size: int = 1) -> float:
    """fairseq2 0.2 nll_loss(reduction="sum") on float64 logits (n, s, V), targets (n, s): the first `ignore_prefix_size`
    positions dropped, pad targets ignored."""
    lsm = torch.log_softmax(logits.double(), dim=-1)[:, ignore_prefix_size:]
    t = targets[:, ignore_prefix_size:].long()
    keep = t != pad_idx
    nll = -lsm.gather(2, t[..., None])[..., 0][keep].sum()
    if label_smoothing == 0.0:
        return float(nll)
    eps = label_smoothing / (logits.shape[-1] - 1)
    smooth = -lsm.sum(dim=-1)[keep].sum()
    return float((1.0 - label_smoothing - eps) * nll + eps * smooth)
