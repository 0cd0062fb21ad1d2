"""CPU restatement of the UnitY2 forced aligner (reference models/aligner/model.py), the yardstick of the device path
(sc_align): frontend + convolution stacks + distance + masked log-softmax in torch float64 on the fp16-rounded weights the
library holds, and the monotonic alignment search exactly as the reference states it - float32 log-probabilities added
into a float64 ``Q``, ties to the upper row, cells with i > j at -inf - with row 0 computed by the same sequential
recurrence (the reference sums row 0 with float32 ``sum()`` calls; tests/golden/make_aligner_goldens.py fences that
difference).  The search also returns the PATH MARGIN: the smallest |Q[i_a, j] - Q[i_b, j]| over the decisions of the
back-track, i.e. how much noise in the log-probabilities the path survives."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F


def monotonic_alignment_search(lprob, want_margin: bool = True) -> Tuple[np.ndarray, float]:
    """lprob (T_feat, T_text) float32 -> (A (T_feat,) int64: text position of every frame, path margin).  The inner loop
    over the text positions is vectorised: column 0 is Q[0, 0] = lprob[0, 0], -inf below; every later column is
    Q[i, j] = max(Q[i-1, j-1], Q[i, j-1]) + lprob[j, i] with Q[-1, .] = -inf (model.py:218-228: row 0 becomes the running sum,
    cells with i > j stay -inf).  want_margin=False skips the (T_feat, T_text) float64 margin matrix."""
    lp = np.asarray(lprob, dtype=np.float32)
    t_feat, t_text = lp.shape
    take_upper = np.zeros((t_feat, t_text), dtype=bool)  # Q[i-1, j-1] >= Q[i, j-1]: the decision at (i, j) -> column j - 1
    gap = np.zeros((t_feat, t_text), dtype=np.float64) if want_margin else None
    q = np.full(t_text, -np.inf)
    q[0] = np.float64(lp[0, 0])
    with np.errstate(invalid="ignore"):
        for j in range(1, t_feat):
            up = np.concatenate(([-np.inf], q[:-1]))
            take = up >= q
            take_upper[j] = take
            if want_margin:
                gap[j] = np.abs(up - q)  # nan where both are -inf: a tie no noise can change
            q = np.where(take, up, q) + lp[j].astype(np.float64)
    a = np.full(t_feat, t_text - 1, dtype=np.int64)
    margin = np.inf
    for j in range(t_feat - 1, 0, -1):  # model.py:231-242 (the decision between columns j and j - 1)
        i = a[j]
        if i > 0:
            if want_margin and not np.isnan(gap[j, i]):
                margin = min(margin, gap[j, i])
            if take_upper[j, i]:
                i -= 1
        a[j - 1] = i
    return a, float(margin)


def viterbi_durations(lprob, text_len: int, feat_len: int, want_margin: bool = True) -> Tuple[np.ndarray, float]:
    """viterbi_decode for one item (model.py:246-277): lprob (>= feat_len, >= text_len) -> durations (text_len,) int64."""
    a, margin = monotonic_alignment_search(np.asarray(lprob)[:feat_len, :text_len], want_margin)
    return np.bincount(a, minlength=text_len).astype(np.int64), margin


def _conv_stack(x: torch.Tensor, sd: Dict[str, torch.Tensor], prefix: str, layers: int, last_stride: int) -> torch.Tensor:
    """(T, C_in) -> (T', C): Conv1d(k=3, pad=1) + ReLU ... and a last Conv1d(k=1, stride) (model.py:99-144)."""
    x = x.t()[None]
    for i in range(layers):
        w = sd[f"{prefix}.{1 + 3 * i}.weight"].to(torch.float16).to(x.dtype)  # the library's weights are fp16
        b = sd[f"{prefix}.{1 + 3 * i}.bias"].to(torch.float32).to(x.dtype)
        last = i == layers - 1
        x = F.conv1d(x, w, b, stride=last_stride if last else 1, padding=w.shape[-1] // 2)
        if not last:
            x = F.relu(x)
    return x[0].t()


@torch.inference_mode()
def encoder_lprob(sd: Dict[str, torch.Tensor], cfg, text_emb: torch.Tensor, feat_emb: torch.Tensor,
                  dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """UnitY2AlignmentEncoder.forward up to attn_lprob for ONE item: text_emb (T_text, C), feat_emb (T_feat, F) ->
    (ceil(T_feat / reduction_factor), T_text)."""
    t = _conv_stack(text_emb.to(dtype), sd, "alignment_encoder.t_conv", cfg.num_text_layers, 1)
    f = _conv_stack(feat_emb.to(dtype), sd, "alignment_encoder.f_conv", cfg.num_feat_layers, cfg.reduction_factor)
    dist = torch.sqrt(((f[:, None, :] - t[None, :, :]) ** 2).sum(-1))
    return F.log_softmax(-cfg.temperature * dist, dim=-1)


def embed(sd: Dict[str, torch.Tensor], text_ids: Sequence[int], unit_ids: Sequence[int], dtype: torch.dtype = torch.float64):
    te = sd["alignment_frontend.embed_text.weight"].to(torch.float16).to(dtype)[torch.as_tensor(list(text_ids), dtype=torch.int64)]
    ue = sd["alignment_frontend.embed_unit.weight"].to(torch.float16).to(dtype)[torch.as_tensor(list(unit_ids), dtype=torch.int64)]
    return te, ue


def align_item(sd, cfg, text_ids: Sequence[int], unit_ids: Sequence[int], dtype: torch.dtype = torch.float64,
               want_margin: bool = True) -> Tuple[np.ndarray, np.ndarray, float]:
    """UnitY2AlignmentModel.forward for one (char ids, unit ids) pair -> (attn_lprob as float32 (T_feat', T_text), durations
    (T_text,) in reduced frames, path margin).  The search runs on the float32 values, as the reference's does
    (``.float().cpu().numpy()``)."""
    te, ue = embed(sd, text_ids, unit_ids, dtype)
    lprob = encoder_lprob(sd, cfg, te, ue, dtype)
    lp32 = lprob.to(torch.float32).numpy()
    dur, margin = viterbi_durations(lp32, lp32.shape[1], lp32.shape[0], want_margin)
    return lp32, dur, margin


def lprob_f64(sd, cfg, text_ids, unit_ids) -> np.ndarray:
    te, ue = embed(sd, text_ids, unit_ids, torch.float64)
    return encoder_lprob(sd, cfg, te, ue, torch.float64).numpy()


def random_pairs(cfg, n: int, seed: int, text_range=(8, 400), max_feat: int = 2000, num_units: Optional[int] = None):
    """Seeded (char ids, unit ids) pairs: T_text uniform in text_range, 2 - 6 units per character, capped at max_feat."""
    rng = np.random.default_rng(seed)
    num_units = num_units if num_units is not None else cfg.unit_vocab_size - 4
    pairs = []
    for _ in range(n):
        t_text = int(rng.integers(text_range[0], text_range[1] + 1))
        t_feat = int(min(max_feat, max(t_text, int(t_text * rng.uniform(2.0, 6.0)))))
        pairs.append((rng.integers(4, cfg.char_vocab_size, t_text).tolist(), (rng.integers(0, num_units, t_feat) + 4).tolist()))
    return pairs
