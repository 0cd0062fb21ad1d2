"""Forced target prefixes (sc_generate_text_prompts): the prefix material the CPU and the GPU tests share.

The five-item fixture of tests/test_lid_gpu.py (oracle_lid: WAVES, the float64 encoder output), CAP = 14, soft_max_seq_len
(1, 200): max_len = 14.  H[b] is the unconstrained greedy hypothesis of row b for __fra__ (prompt and closing EOS included).
    own prefix of row b      = content(H[b])[:k]
    foreign prefix of row b  = content(H[(b + 1) % 5])[:k]
content(h) = h[2:] without the closing EOS; a hypothesis with fewer than k content tokens is continued with its own content
tokens from the start again (a prefix must not hold EOS, and k goes up to max_len - 3 = 11), which only happens to foreign
prefixes here.  The ragged case uses the prompt lengths RAGGED_LENS = [2, 3, 5, 9, max_len - 1]: row 0 has no prefix, the last
row has only the forced EOS left.

MARGIN_BAR: the top-2 margin of the float64 oracle above which the existing id-parity tests take equal ids as a fair demand
(tests/test_stages_gpu.py: 1e-3).  A row may be left out of the comparison with the oracle only when its margin falls under
the bar at some free step, and at most one row per mode; tests/test_prefix_cpu.py asserts that on the CPU."""
import functools

import numpy as np
import torch

CAP = 14
MAX_LEN = 14
LANG = "fra"
MARGIN_BAR = 1e-3


def ragged_lens(max_len=MAX_LEN):
    return [2, 3, 5, 9, max_len - 1]


def content(h, eos_idx):
    body = list(h[2:])
    if body and body[-1] == eos_idx:
        body.pop()
    return body


def take(h, k, eos_idx):
    """The first k content tokens of hypothesis h, continued cyclically when h is shorter."""
    body = content(h, eos_idx)
    assert body or k == 0, "a hypothesis without content cannot supply a prefix"
    return [int(body[i % len(body)]) for i in range(k)]


def own_prompts(H, head, ks, eos_idx):
    return [list(head) + take(H[b], ks[b], eos_idx) for b in range(len(H))]


def foreign_prompts(H, head, ks, eos_idx):
    n = len(H)
    return [list(head) + take(H[(b + 1) % n], ks[b], eos_idx) for b in range(n)]


def pack(prompts, pad=0):
    """(rows (n, stride) int32, lens (n,) int32): the tuple form of generate_text's prefix."""
    lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
    rows = np.full((len(prompts), int(lens.max())), pad, dtype=np.int32)
    for b, p in enumerate(prompts):
        rows[b, : len(p)] = p
    return rows, lens


@functools.lru_cache(maxsize=1)
def oracle_material():
    """On the CPU, float64: H of the five rows, the ragged foreign prompts, and per row the oracle's greedy continuation of its
    prompt with the top-2 margins of the free steps."""
    from oracle import unity as ou
    from tests import common
    from tests.test_lid_gpu import oracle_lid

    o = oracle_lid()
    orc = common.make_oracle()
    cfg, tt = orc.cfg, orc.text_tok
    head = tt.target_prefix(LANG)
    src_len = 0
    with torch.inference_mode():
        H = ou.greedy_generate(orc.P, cfg, o["enc"], o["enc_lens"], head, (1, 200), CAP, pos_table=orc.pos_table, source_len=src_len)
        prompts = foreign_prompts(H, head, [l - 2 for l in ragged_lens()], cfg.eos_idx)
        greedy, margins = [], []
        for b, p in enumerate(prompts):
            s, m = ou.greedy_generate(orc.P, cfg, o["enc"][b:b + 1], o["enc_lens"][b:b + 1], p, (1, 200), CAP, pos_table=orc.pos_table,
                                      return_margins=True, source_len=src_len)
            greedy.append(s[0])
            margins.append(m[0])
    return {"H": H, "head": head, "prompts": prompts, "greedy": greedy, "margins": margins, "eos": cfg.eos_idx}


def rows_under_the_bar(margins):
    return [b for b, m in enumerate(margins) if m and min(m) < MARGIN_BAR]
