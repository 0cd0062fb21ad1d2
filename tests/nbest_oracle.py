"""Per-token scores of a given hypothesis, restated for tests/test_nbest_gpu.py: the hypothesis is fed token by token through
``oracle.unity.IncrementalDecoder`` (the beam search's own arithmetic, one row) and position t + 1 gets ``log_softmax`` of
the logits behind token t at token t + 1 - the prompt positions included, position 0 holds 0.  The step rules of the search
leave the value of a token that was chosen alone (they only remove others, the n-gram block is not renormalised), so this is
what ``step_scores`` must hold without a phrase boost."""
from typing import List, Sequence

import torch
import torch.nn.functional as F

from oracle import unity as ou


def step_scores(orc, cfg, enc_row: torch.Tensor, enc_len: int, tokens: Sequence[int]) -> List[float]:
    """enc_row (1, S, M) fp32 on the CPU, its valid length, the whole hypothesis (prompt, content, EOS) -> one float per token."""
    W = orc.P["final_proj.weight"]
    dec = ou.IncrementalDecoder(orc.P, cfg, enc_row, torch.tensor([int(enc_len)], dtype=torch.int64), orc.pos_table)
    out = [0.0]
    for t in range(len(tokens) - 1):
        h = dec(torch.tensor([[int(tokens[t])]], dtype=torch.int64))
        lp = torch.log_softmax(F.linear(h[0, -1], W), dim=-1)
        out.append(float(lp[int(tokens[t + 1])]))
    return out
