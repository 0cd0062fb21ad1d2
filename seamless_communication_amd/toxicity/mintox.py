"""MinTox pipeline (drop-in for the reference's ``toxicity/mintox.py``): where a translation holds a listed word that its
source does not, those rows are generated again with the words' token sequences banned.  The ban itself is the
``BannedSequenceProcessor`` that the HIP beam-search step applies on the device (csrc/k_beam.hip)."""
from __future__ import annotations

import logging
from typing import Any, Dict, List, Optional, Tuple

import torch
from torch import Tensor

from ..inference.generator import BannedSequenceProcessor, SequenceGeneratorOptions
from .etox_bad_word_checker import ETOXBadWordChecker

logger = logging.getLogger(__name__)

StringLike = str
SequenceData = Dict[str, Any]


def _extract_bad_words_with_batch_indices(source_texts: List[StringLike], target_texts: List[StringLike], source_lang: str,
                                          target_lang: str, bad_word_checker: ETOXBadWordChecker) -> Tuple[List[str], List[int]]:
    """-> (the variants to ban of all rows, the rows with added toxicity)."""
    words: List[str] = []
    rows: List[int] = []
    for row, (src, tgt) in enumerate(zip(source_texts, target_texts)):
        found = bad_word_checker.extract_bad_words(str(src), str(tgt), source_lang, target_lang)
        if found:
            rows.append(row)
            words += found
    return words, rows


def _replace_with_new_text_output_in_batch(original_texts: List[StringLike], indices_with_toxicity: List[int],
                                           new_texts: List[StringLike]) -> None:
    """In place: row ``indices_with_toxicity[k]`` (taken in ascending row order) becomes ``new_texts[k]``."""
    toxic = set(indices_with_toxicity)
    fresh = iter(new_texts)
    for row in range(len(original_texts)):
        if row in toxic:
            original_texts[row] = next(fresh)


def _replace_with_new_unit_output_in_batch(unit_tokenizer: Any, original_units: Tensor, indices_with_toxicity_tensor: Tensor,
                                           new_units: Tensor) -> Tensor:
    """Rows ``indices_with_toxicity_tensor`` of ``original_units`` become ``new_units``; the narrower matrix is padded on the
    right with the unit pad index.  Returns the result: ``original_units`` itself (updated in place) unless the new rows
    are wider, then a padded copy.  (The reference pads a local name in that case, so its caller keeps the OLD units;
    here the caller gets the replaced rows - INTEGRATION.md.)"""
    pad_idx = unit_tokenizer.vocab_info.pad_idx or 1
    diff = new_units.size(1) - original_units.size(1)
    if diff > 0:
        original_units = torch.nn.functional.pad(original_units, (0, diff), mode="constant", value=pad_idx)
    elif diff < 0:
        new_units = torch.nn.functional.pad(new_units, (0, -diff), mode="constant", value=pad_idx)
    original_units[indices_with_toxicity_tensor] = new_units.to(original_units.dtype)
    return original_units


def mintox_pipeline(
    model: Any,
    text_tokenizer: Any,
    unit_tokenizer: Any,
    device: Any,
    src_lang: str,
    tgt_lang: str,
    model_input: SequenceData,
    input_modality: "Modality",  # noqa: F821
    output_modality: "Modality",  # noqa: F821
    src_texts: List[StringLike],
    original_texts: List[StringLike],
    original_units: Optional[Tensor] = None,
    unit_generation_ngram_filtering: bool = False,
    text_generation_opts: Optional[SequenceGeneratorOptions] = None,
    unit_generation_opts: Optional[SequenceGeneratorOptions] = None,
    bad_word_checker: ETOXBadWordChecker = None,
    duration_factor: float = 1.0,
    prosody_encoder_input: Optional[SequenceData] = None,
    _trace: Optional[Dict[str, Any]] = None,
    forced_prefix: Any = None,
) -> Tuple[List[StringLike], Optional[Tensor]]:
    """MinTox: Mitigation at INference time of added TOXicity (reference signature; ``_trace`` and ``forced_prefix`` are this
    package's: the rows generated again keep their forced target prefix, ``Translator.predict``'s argument)."""
    from ..inference.translator import Modality, Translator

    if text_generation_opts is None:
        text_generation_opts = SequenceGeneratorOptions(beam_size=5, soft_max_seq_len=(1, 200))
    if unit_generation_opts is None:
        unit_generation_opts = SequenceGeneratorOptions(beam_size=5, soft_max_seq_len=(25, 50))

    bad_words, toxic_rows = _extract_bad_words_with_batch_indices(src_texts, original_texts, src_lang, tgt_lang, bad_word_checker)
    want_units = output_modality != Modality.TEXT
    if not toxic_rows:  # nothing added: the first output stands
        return original_texts, (original_units if want_units else None)
    logger.info("TOX src_lang=%s tgt_lang=%s added_tox=%d", src_lang, tgt_lang, len(toxic_rows))
    if _trace is not None:
        _trace["mintox_rows"] = list(toxic_rows)

    # the words as the tokenizer writes them, and as it writes them behind another symbol ("★word" without the first
    # token): a word also appears glued to punctuation, where its first piece carries no word-boundary mark
    encode = text_tokenizer.create_raw_encoder(device=device)
    words = list(set(bad_words))
    banned_seqs = [encode(w) for w in words]
    banned_seqs += [encode(f"★{w}")[1:] for w in words]
    text_generation_opts.step_processor = BannedSequenceProcessor([s for s in banned_seqs if len(s) > 0])

    rows_t = torch.tensor(toxic_rows, device=model_input["seqs"].device)
    if model_input["is_ragged"]:  # only the toxic rows are generated again
        model_input["seqs"] = torch.index_select(model_input["seqs"], 0, rows_t)
        lens = model_input["seq_lens"]
        lens = lens if isinstance(lens, Tensor) else torch.tensor(list(lens))
        model_input["seq_lens"] = torch.index_select(lens, 0, rows_t.to(lens.device))
        if isinstance(forced_prefix, tuple):  # one entry per item: those of the rows generated again
            forced_prefix = tuple(forced_prefix[r] for r in toxic_rows)
    seqs = model_input["seqs"]
    # the lengths go along whenever the input has them, as in Translator.predict's own first call (the reference builds a
    # padding mask for ragged input only; for a full-length batch the two are the same)
    padding_mask = model_input.get("seq_lens")
    new_texts, new_units = Translator.get_prediction(
        model=model, text_tokenizer=text_tokenizer, unit_tokenizer=unit_tokenizer, seqs=seqs, padding_mask=padding_mask,
        input_modality=input_modality, output_modality=output_modality, tgt_lang=tgt_lang,
        unit_generation_ngram_filtering=unit_generation_ngram_filtering, text_generation_opts=text_generation_opts,
        unit_generation_opts=unit_generation_opts, duration_factor=duration_factor, prosody_encoder_input=prosody_encoder_input,
        _trace=_trace, forced_prefix=forced_prefix,
    )
    batched = len(original_texts) > 1
    if batched:
        _replace_with_new_text_output_in_batch(original_texts, toxic_rows, new_texts)
        final_texts = original_texts
    else:
        final_texts = new_texts
    if not want_units:
        return final_texts, None
    if not batched:
        return final_texts, new_units
    assert original_units is not None and new_units is not None
    return final_texts, _replace_with_new_unit_output_in_batch(unit_tokenizer, original_units, rows_t.to(original_units.device), new_units)
