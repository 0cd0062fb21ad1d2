"""Teacher-forced scoring: how probable the model finds GIVEN target texts.

``Translator.score`` (forced-decoding scores, n-best re-ranking, perplexity, token accuracy) and
``finetune_eval_loss`` (the S2T evaluation loss of the reference's fine-tuning trainer,
cli/m4t/finetune/trainer.py:100-125 ``UnitYFinetuneWrapper.forward`` + :155-188 ``CalcLoss``, forward only).

Both run ``sc_score_text``: the batched causal decoder pass, then the vocabulary projection with its log-softmax
statistics kept in the product's epilogue - per target position the target's log-probability, the log-probabilities
summed over the vocabulary (label smoothing's term) and the arg-max token.  No (rows, vocabulary) buffer exists.

Out of scope: the T2U unit loss (the reference implements it for the v1 autoregressive T2U only), gradients, scoring
inside beam search.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Iterable, List, Optional, Sequence, Union

import numpy as np
import torch

from .runtime import encode_source_speech


SCORE_TASKS = ("S2TT", "ASR", "T2TT")
# CalcLoss: `prefix_skip_len = 1  # language tokens to skip` (trainer.py:175), handed on as ignore_prefix_size
IGNORE_PREFIX_SIZE = 1


@dataclass
class SequenceScore:
    """One target's score.  ``token_ids``: the scored tokens ``__lang__ w1 ... </s>`` (everything behind the leading
    ``</s>`` of the prompt); ``token_lprobs[i]`` = log p(token_ids[i] | everything in front of it); ``top1[i]`` the model's
    arg-max at that position.  The language-token position is listed but NOT part of ``score`` (the reference's
    ``prefix_skip_len``): ``score`` = sum of ``token_lprobs[1:]``, ``score_normalized`` = that sum / ``len(token_ids) - 1``."""

    token_ids: List[int]
    token_lprobs: List[float]
    score: float
    score_normalized: float
    top1: List[int]


def target_sequence(text_tokenizer, tgt_lang: str, target: Union[str, Sequence[int]], max_seq_len: int) -> List[int]:
    """The whole sequence ``</s> __lang__ w1 ... </s>`` for one target, built as ``predict`` builds its prompt
    (``target_prefix``).  A string goes through the tokenizer's NLLB "target" mode.  An id list that already starts with
    the prompt is taken as it is (what ``Translator.last_text_ids`` holds), otherwise it is the text's pieces and gets
    the prompt in front; a missing final ``</s>`` is added.  Raises ValueError for an empty target, an id outside the
    vocabulary or a sequence longer than ``max_seq_len``."""
    prefix = list(text_tokenizer.target_prefix(tgt_lang))
    eos = text_tokenizer.vocab_info.eos_idx
    if isinstance(target, str):
        body = list(text_tokenizer.encode_pieces(target))
        if not body:
            raise ValueError("empty target: the text holds no token to score")
        ids = prefix + body + [eos]
    else:
        ids = [int(t) for t in target]
        if ids[: len(prefix)] != prefix:
            ids = prefix + ids
        if len(ids) == len(prefix) or ids == prefix + [eos]:
            raise ValueError("empty target: the id list holds no token to score")
        if ids[-1] != eos:
            ids.append(eos)
        size = text_tokenizer.vocab_info.size
        bad = [t for t in ids if not 0 <= t < size]
        if bad:
            raise ValueError(f"target token {bad[0]} outside the vocabulary of {size}")
    if len(ids) > max_seq_len:
        raise ValueError(f"target of {len(ids)} tokens (prompt and </s> included) exceeds text_max_seq_len={max_seq_len}")
    return ids


def pad_sequences(seqs: Sequence[Sequence[int]], pad_idx: int):
    lens = np.asarray([len(s) for s in seqs], dtype=np.int32)
    out = np.full((len(seqs), int(lens.max())), pad_idx, dtype=np.int32)
    for b, s in enumerate(seqs):
        out[b, : len(s)] = s
    return out, lens


def sequence_scores(tokens: np.ndarray, tok_lens: Sequence[int], tok_lprob: np.ndarray, top1: Optional[np.ndarray],
                    ignore_prefix_size: int = IGNORE_PREFIX_SIZE) -> List[SequenceScore]:
    """Per-item summary of sc_score_text's arrays (host side; float64 sums in position order)."""
    out = []
    for b, n in enumerate(tok_lens):
        n = int(n)
        lp = [float(x) for x in tok_lprob[b, : n - 1]]
        kept = lp[ignore_prefix_size:]
        total = float(np.sum(np.asarray(kept, dtype=np.float64))) if kept else 0.0
        out.append(SequenceScore(token_ids=[int(t) for t in tokens[b, 1:n]], token_lprobs=lp, score=total,
                                 score_normalized=total / len(kept) if kept else 0.0,
                                 top1=[int(t) for t in top1[b, : n - 1]] if top1 is not None else []))
    return out


@torch.inference_mode()
def score(self, input, task_str: str, tgt_lang: str, targets, src_lang: Optional[str] = None,
          sample_rate: int = 16000) -> List[SequenceScore]:
    """``Translator.score``: log-probabilities of ``targets`` given ``input``, teacher forced.

    ``task_str``: s2tt / asr / t2tt (the tasks with text output).  ``input``: what ``predict`` accepts - a waveform, an
    audio file, a text (``src_lang`` required), or a SequenceData dict for a batch (ragged: ``seq_lens``).  ``targets``: one
    target or a list - strings (through the model's tokenizer) or token-id lists (see :func:`target_sequence`).  One target
    per batch item; a single input with several targets scores each of them against that input (n-best re-ranking: the
    source is encoded once).  The prompt is ``predict``'s: ``</s>``, then ``__tgt_lang__``."""
    from .inference.translator import Modality

    if task_str.upper() not in SCORE_TASKS:
        raise ValueError(f"Unsupported task for scoring: {task_str} (text output only: s2tt, asr, t2tt)")
    input_modality, _ = self.get_modalities_from_task_str(task_str)
    if isinstance(targets, str) or (len(targets) > 0 and isinstance(targets[0], (int, np.integer))):
        targets = [targets]
    if len(targets) == 0:
        raise ValueError("no target to score")
    seq_ids = [target_sequence(self.text_tokenizer, tgt_lang, t, self.cfg.text_max_seq_len) for t in targets]
    tokens, tok_lens = pad_sequences(seq_ids, self.text_tokenizer.vocab_info.pad_idx)

    _, seqs, src_lens, _ = self._source_batch(input, input_modality, src_lang, sample_rate)
    if input_modality == Modality.SPEECH:
        enc, enc_lens = encode_source_speech(self.model, seqs, src_lens)
    else:
        enc, enc_lens = self.model.encode_text(seqs.cpu().numpy(), src_lens), np.asarray(src_lens, dtype=np.int32)
    n = len(seq_ids)
    if enc.shape[0] == 1 and n > 1:
        enc = enc.expand(n, -1, -1).contiguous()
        enc_lens = np.repeat(np.asarray(enc_lens), n)
    if enc.shape[0] != n:
        raise ValueError(f"{n} targets for a batch of {enc.shape[0]} inputs")
    res = self.model.score_text(enc, np.asarray(enc_lens).tolist(), tokens, tok_lens, want_top1=True)
    return sequence_scores(tokens, tok_lens, res["tok_lprob"], res["top1"])


def label_smoothed_nll(tok_lprob, sum_lprob, targets, pad_idx: int, vocab_size: int, label_smoothing: float,
                       ignore_prefix_size: int = IGNORE_PREFIX_SIZE) -> float:
    """fairseq2 0.2 ``nll_loss`` (reduction "sum") from per-position statistics instead of logits:

        loss = (1 - ls - eps) * sum(-lprob_target) + eps * sum(-sum_lprob),   eps = ls / (V - 1)

    over the positions behind the first ``ignore_prefix_size`` whose target is not ``pad_idx``.  ``tok_lprob`` /
    ``sum_lprob`` / ``targets``: (n, s).  float64 on the host.  With ``label_smoothing == 0`` this is the plain summed
    negative log-likelihood and ``sum_lprob`` may be None.  (The smoothing form is CHOSEN and UNVERIFIED: fairseq2 is not
    part of the reference tree)"""
    t = np.asarray(targets)[:, ignore_prefix_size:]
    keep = t != pad_idx
    lp = np.asarray(tok_lprob, dtype=np.float64)[:, ignore_prefix_size:]
    nll = -float(np.sum(lp[keep]))
    if label_smoothing == 0.0:
        return nll
    if sum_lprob is None:
        raise ValueError("label smoothing needs sum_lprob")
    eps = label_smoothing / (vocab_size - 1)
    smooth = -float(np.sum(np.asarray(sum_lprob, dtype=np.float64)[:, ignore_prefix_size:][keep]))
    return (1.0 - label_smoothing - eps) * nll + eps * smooth


def _field(batch: Any, name: str):
    v = batch[name] if isinstance(batch, dict) else getattr(batch, name)
    if v is None:
        raise ValueError(f"batch field '{name}' is missing")
    return v


def batch_sequences(prev_output_tokens, target_tokens, target_lengths, pad_idx: int):
    """The whole sequences behind a (prev_output_tokens, target_tokens) pair of the reference's ``SeqsBatch``
    (dataloader.py: tokens[:-1] and tokens[1:]): row b is prev[b, 0] followed by target[b, :len_b].  Raises ValueError where
    the two are not each other's shift, or a length is out of range."""
    prev = np.asarray(torch.as_tensor(prev_output_tokens).cpu(), dtype=np.int64)
    tgt = np.asarray(torch.as_tensor(target_tokens).cpu(), dtype=np.int64)
    lens = np.asarray(torch.as_tensor(target_lengths).cpu(), dtype=np.int64).reshape(-1)
    if prev.shape != tgt.shape or prev.ndim != 2 or len(lens) != prev.shape[0]:
        raise ValueError("prev_output_tokens and target_tokens must be (n, s) with one target length per row")
    n, s = tgt.shape
    if lens.min() < 1 or lens.max() > s:
        raise ValueError(f"target_lengths outside [1, {s}]")
    tokens = np.full((n, s + 1), pad_idx, dtype=np.int32)
    for b in range(n):
        L = int(lens[b])
        if not np.array_equal(prev[b, 1:L], tgt[b, : L - 1]):
            raise ValueError(f"row {b}: prev_output_tokens is not target_tokens shifted by one position")
        tokens[b, 0] = prev[b, 0]
        tokens[b, 1 : L + 1] = tgt[b, :L]
    return tokens, (lens + 1).astype(np.int32)


@torch.inference_mode()
def finetune_eval_loss(translator, batches: Iterable[Any], label_smoothing: float = 0.2) -> float:
    """The S2T loss of the reference's ``CalcLoss`` (``FinetuneMode.SPEECH_TO_TEXT``) over ``batches``, forward only -
    what ``_eval_model`` (trainer.py:339) averages: ``sum of s2t_loss / sum of s2t_numel`` with ``s2t_numel`` =
    ``sum(target_lengths - 1)``.

    A batch has the fields of the reference's ``dataloader.SeqsBatch`` (attributes or dict keys): ``src_tokens`` (fbank,
    (n, T, 80)), ``src_lengths``, ``prev_output_tokens``, ``target_tokens``, ``target_lengths``.  A ``MultimodalSeqsBatch``'s
    ``speech_to_text`` member is taken where present."""
    model, cfg = translator.model, translator.cfg
    pad = translator.text_tokenizer.vocab_info.pad_idx
    loss, numel = 0.0, 0
    for batch in batches:
        batch = getattr(batch, "speech_to_text", batch)
        fb = torch.as_tensor(_field(batch, "src_tokens")).to(translator.device, torch.float32)
        src_lens = [int(x) for x in torch.as_tensor(_field(batch, "src_lengths")).tolist()]
        if fb.shape[1] % cfg.fbank_stride:
            fb = torch.nn.functional.pad(fb, (0, 0, 0, cfg.fbank_stride - fb.shape[1] % cfg.fbank_stride))
        tokens, tok_lens = batch_sequences(_field(batch, "prev_output_tokens"), _field(batch, "target_tokens"),
                                           _field(batch, "target_lengths"), pad)
        enc, enc_lens = model.encode_speech(fb.contiguous(), src_lens)
        res = model.score_text(enc, enc_lens.tolist(), tokens, tok_lens, want_sum=label_smoothing != 0.0)
        # positions behind an item's end hold the pad token in `tokens`: they drop out as pad targets
        loss += label_smoothed_nll(res["tok_lprob"], res.get("sum_lprob"), tokens[:, 1:], pad, cfg.text_vocab_size, label_smoothing)
        numel += int(np.sum(tok_lens - 1 - IGNORE_PREFIX_SIZE))
    if numel <= 0:
        raise ValueError("no target token to average over")
    return loss / numel
