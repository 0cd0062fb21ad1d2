"""CPU restatement of what the Transcriber captures on the device (sc_generate_text_capture), from the oracle's building
blocks (oracle/unity.py): the teacher-forced decoder over known tokens, the LAST layer's encoder-decoder attention
probabilities summed over the heads (the reference's hook, inference/transcriber.py:39-57) and the log-probability of each
next token after the step rules (tweak_lprobs)."""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import unity as ou


@torch.inference_mode()
def teacher_forced_capture(P: "ou.Params", cfg, enc: torch.Tensor, enc_len: int, seq: Sequence[int], n_fed: int, max_len: int,
                           prefix_len: int = 2, min_seq_len: int = 1, unk_penalty: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
    """enc (S_enc, M) fp32 (the device's encoder output), seq: prompt + tokens (+ EOS); positions 0 .. n_fed-1 are fed.
    -> xattn (n_fed, S_enc) float64, 0 behind enc_len; lprob (n_fed,): log-probability of seq[p + 1] chosen at position p
    (0 at the prompt positions before the last)."""
    L, H, M = cfg.dec_layers, cfg.num_heads, cfg.model_dim
    D = M // H
    pos_table = ou.sinusoidal_table(cfg.text_max_seq_len, M, 1)
    tokens = torch.tensor([list(seq[:n_fed])], dtype=torch.int64)
    e = enc[None].to(torch.float32)
    e_lens = torch.tensor([enc_len])
    x = ou.embed_text(P, cfg, tokens, 0, pos_table)
    for i in range(L - 1):
        x = ou.decoder_layer(P, cfg, f"text_decoder.layers.{i}", x, e, e_lens)
    pre = f"text_decoder.layers.{L - 1}"
    h = P.layer_norm(x, pre + ".self_attn_layer_norm")
    x = x + ou.mha(P, pre + ".self_attn", h, h, H, causal=True)
    h = P.layer_norm(x, pre + ".encoder_decoder_attn_layer_norm")
    # mha's soft-max, kept: (1, H, n_fed, S_enc)
    q = P.linear(h, pre + ".encoder_decoder_attn.q_proj").view(1, n_fed, H, D).transpose(1, 2)
    k = P.linear(e, pre + ".encoder_decoder_attn.k_proj").view(1, e.shape[1], H, D).transpose(1, 2)
    w = torch.matmul(q, k.transpose(-1, -2)) * (D ** -0.5)
    w = w.masked_fill(~ou.padding_mask(e_lens, e.shape[1])[:, None, None, :], float("-inf"))
    xattn = torch.softmax(w, dim=-1).sum(dim=1)[0].double().numpy()
    x = x + ou.mha(P, pre + ".encoder_decoder_attn", h, e, H, key_lens=e_lens)
    x = x + ou.ffn(P, pre + ".ffn", P.layer_norm(x, pre + ".ffn_layer_norm"), "relu")
    hN = P.layer_norm(x, "text_decoder.layer_norm")[0]
    lprobs = torch.log_softmax(F.linear(hN, P["final_proj.weight"]), dim=-1)
    lp = np.zeros(n_fed)
    for p in range(prefix_len - 1, n_fed):
        row = ou.tweak_lprobs(lprobs[p : p + 1].clone(), p, max_len, min_seq_len, unk_penalty, cfg.pad_idx, cfg.unk_idx, cfg.eos_idx)
        lp[p] = float(row[0, seq[p + 1]]) if p + 1 < len(seq) else math.nan
    return xattn, lp
