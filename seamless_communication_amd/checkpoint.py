"""Checkpoint wire format of the drop-in Translator: fairseq-keyed UnitY2 / vocoder checkpoints
(what the model cards publish) -> the fairseq2-keyed state dict the HIP library loads.

The reference does this with ``convert_unity_checkpoint`` (src/seamless_communication/models/unity/
loader.py:27-155; regex table ``_fairseq_key_map`` :179-389; ``_get_char_index_mapping`` :158-176) on
top of fairseq2's ``convert_fairseq_checkpoint`` (first matching ``re.sub`` of the key map wins), and
with ``convert_vocoder_checkpoint`` (models/vocoder/loader.py:20-36).  This module restates that for
the architectures on the MI355X hot path (``base_v2`` = X2T/S2T + NAR T2U, standard adaptor, Conformer
speech encoder) with a table organised by module family instead of one flat regex dict; the result is
pinned key-for-key and tensor-for-tensor against the reference's own functions executed from
/root/reference (tests/golden/make_checkpoint_goldens.py -> tests/test_checkpoint_conversion.py).

What the conversion does besides renaming (loader.py line numbers):
  * drops fairseq remnants (version / _float_tensor buffers, wav2vec2 ``mask_emb``, the alignment
    encoder and the character-level projection used only in training) :62-117;
  * NLLB-100 dummy row: a 256103-row ``final_proj.weight`` loses its last row :121-126;
  * one embedding table: ``text_decoder_frontend.embed.weight`` (and the text encoder's) become the
    SAME tensor as ``final_proj.weight`` :130-133, likewise the T2U unit embedding :150-153;
  * control-symbol rows permuted from fairseq's (BOS, PAD, EOS, UNK) to the tokenizer's
    (PAD, UNK, BOS, EOS) :137-139;
  * char embedding rows re-ordered from the dictionary's sorted order to the SentencePiece order
    :141-145, :158-176.
"""
from __future__ import annotations

import re
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple

import torch

FAIRSEQ2_MARKER = "speech_encoder.inner.layers.0.self_attn_layer_norm.weight"
NLLB100_FAIRSEQ_VOCAB = 256103

# fairseq module prefixes of the S2T + NAR-T2U layout (loader.py:187-192)
_PLAIN_PREFIXES = ("encoder", "target_letter_decoder", "synthesizer_encoder", "decoder")
# the expressive model's layout (loader.py:181-186, "ExpressiveUnitY model (from multi_arch codebase)"); its prosody encoder
# sits under `global_prosody.`, its prosody projection under `t2s_model.global_proj_enc.`
_EXPRESSIVE_PREFIXES = ("s2t_model.encoder", "s2t_model.decoder", "t2s_model.encoder", "t2s_model.decoder")
_ENC, _DEC, _T2U_ENC, _T2U_DEC = _PLAIN_PREFIXES
_W2V = _ENC + ".w2v_encoder.w2v_model."

# sub-keys of a fairseq transformer layer -> fairseq2 names (shared by text encoder / decoders / T2U encoder)
_XFMR_LAYER: List[Tuple[str, str]] = [
    ("self_attn.out_proj.", "self_attn.output_proj."),
    ("self_attn.", "self_attn."),
    ("self_attn_layer_norm.", "self_attn_layer_norm."),
    ("encoder_attn.out_proj.", "encoder_decoder_attn.output_proj."),
    ("encoder_attn.", "encoder_decoder_attn."),
    ("encoder_attn_layer_norm.", "encoder_decoder_attn_layer_norm."),
    ("fc1.", "ffn.inner_proj."),
    ("fc2.", "ffn.output_proj."),
    ("final_layer_norm.", "ffn_layer_norm."),
]
# sub-keys of a w2v-BERT Conformer layer
_CONFORMER_LAYER: List[Tuple[str, str]] = [
    ("conv_module.batch_norm.", "conv.batch_norm."),
    ("conv_module.layer_norm2.", "conv.layer_norm."),
    ("conv_module.depthwise_conv.", "conv.depthwise_conv."),
    ("conv_module.layer_norm.", "conv_layer_norm."),
    ("conv_module.pointwise_conv1.", "conv.pointwise_conv1."),
    ("conv_module.pointwise_conv2.", "conv.pointwise_conv2."),
    ("ffn1.layer_norm.", "ffn1_layer_norm."), ("ffn2.layer_norm.", "ffn2_layer_norm."),
    ("ffn1.w_1.", "ffn1.inner_proj."), ("ffn2.w_1.", "ffn2.inner_proj."),
    ("ffn1.w_2.", "ffn1.output_proj."), ("ffn2.w_2.", "ffn2.output_proj."),
    ("self_attn_layer_norm.", "self_attn_layer_norm."),
    ("self_attn.linear_q.", "self_attn.q_proj."), ("self_attn.linear_k.", "self_attn.k_proj."),
    ("self_attn.linear_v.", "self_attn.v_proj."), ("self_attn.linear_out.", "self_attn.output_proj."),
    ("self_attn.q_proj.", "self_attn.q_proj."), ("self_attn.k_proj.", "self_attn.k_proj."),
    ("self_attn.v_proj.", "self_attn.v_proj."),
    ("self_attn.rel_k_embedding.", "self_attn.sdpa.rel_k_embed."),
    ("self_attn.out_proj.", "self_attn.output_proj."),
    ("self_attn.linear_pos.", "self_attn.sdpa.r_proj."),
    ("self_attn.pos_bias_u", "self_attn.sdpa.u_bias"), ("self_attn.pos_bias_v", "self_attn.sdpa.v_bias"),
    ("final_layer_norm.", "layer_norm."),
]
_ADAPTOR_LAYER: List[Tuple[str, str]] = [
    ("residual_layer_norm.", "residual_layer_norm."),
    ("residual_pool.1.", "residual_conv."),
    ("attn_pool.1.", "self_attn_conv."),
    ("self_attn.out_proj.", "self_attn.output_proj."),
    ("self_attn.", "self_attn."),
    ("self_attn_layer_norm.", "self_attn_layer_norm."),
    ("fc1.", "ffn.inner_proj."), ("fc2.", "ffn.output_proj."),
    ("final_layer_norm.", "ffn_layer_norm."),
]
_NAR_DECODER_LAYER: List[Tuple[str, str]] = [
    ("self_attn.out_proj.", "self_attn.output_proj."),
    ("self_attn.", "self_attn."),
    ("self_attn_layer_norm.", "self_attn_layer_norm."),
    ("layer_norm.", "self_attn_layer_norm."),
    ("encoder_attn.out_proj.", "encoder_decoder_attn.output_proj."),
    ("encoder_attn.", "encoder_decoder_attn."),
    ("encoder_attn_layer_norm.", "encoder_decoder_attn_layer_norm."),
    ("fc1.", "ffn.inner_proj."), ("fc2.", "ffn.output_proj."),
    ("final_layer_norm.", "ffn_layer_norm."),
    ("ffn.ffn.0.", "conv1d.conv1."), ("ffn.ffn.2.", "conv1d.conv2."),
    ("ffn.layer_norm.", "conv1d_layer_norm."),
]


def _stack(src_prefix: str, dst_prefix: str, sub: Sequence[Tuple[str, str]]) -> List[Tuple[re.Pattern, str]]:
    """Rules ``<src_prefix>layers.<i>.<old>`` -> ``<dst_prefix>layers.<i>.<new>`` in table order."""
    return [(re.compile("^" + re.escape(src_prefix) + r"layers\.([0-9]+)\." + re.escape(old)), dst_prefix + r"layers.\1." + new)
            for old, new in sub]


def _plain(pairs: Sequence[Tuple[str, str]]) -> List[Tuple[re.Pattern, str]]:
    return [(re.compile("^" + re.escape(old)), new) for old, new in pairs]


def unity_v2_key_rules(expressive: bool = False) -> List[Tuple[re.Pattern, str]]:
    """Ordered rename rules for the base_v2 layout; the FIRST rule that changes a key wins, like
    fairseq2's convert_fairseq_checkpoint does with the reference's dict (insertion order).
    ``expressive``: the config has a prosody encoder (expressivity_v2) - the module prefixes of that layout, and the rules of
    loader.py:336-343 (FiLM of the NAR decoder layers, the prosody encoder, the prosody projection; the duration predictor's
    ``film.`` keys ride on its prefix rule)."""
    _ENC, _DEC, _T2U_ENC, _T2U_DEC = _EXPRESSIVE_PREFIXES if expressive else _PLAIN_PREFIXES
    _W2V = _ENC + ".w2v_encoder.w2v_model."
    rules: List[Tuple[re.Pattern, str]] = []
    # speech encoder frontend (fbank models have no feature extractor; the rules are harmless if absent)
    rules += _plain([
        (_W2V + "encoder.pos_conv.0.", "speech_encoder_frontend.pos_encoder.conv."),
        (_W2V + "layer_norm.", "speech_encoder_frontend.post_extract_layer_norm."),
        (_W2V + "post_extract_proj.", "speech_encoder_frontend.model_dim_proj."),
    ])
    rules += _stack(_W2V + "encoder.", "speech_encoder.inner.", _CONFORMER_LAYER)
    # pre-LN remnant after the Conformer blocks moves to the adaptor (loader.py:272-293, use_conformer)
    rules += _plain([
        (_W2V + "encoder.layer_norm.", "speech_encoder.inner_layer_norm."),
        (_ENC + ".adaptor.proj.0.", "speech_encoder.proj1."),
        (_ENC + ".adaptor.proj.2.", "speech_encoder.proj2."),
        (_ENC + ".adaptor.out_ln.", "speech_encoder.layer_norm."),
        ("text_encoder.embed_tokens.", "text_encoder_frontend.embed."),
    ])
    rules += _stack("text_encoder.", "text_encoder.", _XFMR_LAYER)
    rules += _plain([("text_encoder.layer_norm.", "text_encoder.layer_norm.")])
    rules += _stack(_ENC + ".adaptor.", "speech_encoder.adaptor_", _ADAPTOR_LAYER)
    # text decoder
    rules += _plain([(_DEC + ".embed_tokens.", "text_decoder_frontend.embed.")])
    rules += _stack(_DEC + ".", "text_decoder.", _XFMR_LAYER)
    rules += _plain([
        (_DEC + ".layer_norm.", "text_decoder.layer_norm."),
        (_DEC + ".output_projection.", "final_proj."),
    ])
    if expressive:
        rules += _stack(_T2U_DEC + ".", "t2u_model.decoder.", [("film.", "film.")])
        rules += _plain([("global_prosody.", "prosody_encoder_model."), ("t2s_model.global_proj_enc.", "t2u_model.prosody_proj.")])
    # T2U encoder, NAR decoder frontend, NAR decoder
    rules += _stack(_T2U_ENC + ".", "t2u_model.encoder.", _XFMR_LAYER)
    rules += _plain([
        (_T2U_ENC + ".layer_norm.", "t2u_model.encoder.layer_norm."),
        (_T2U_DEC + ".embed_tokens_text.", "t2u_model.decoder_frontend.embed_char."),
        (_T2U_DEC + ".embed_tokens_unit.", "t2u_model.decoder_frontend.embed."),
        (_T2U_DEC + ".embed_tokens.", "t2u_model.decoder_frontend.embed."),
        (_T2U_DEC + ".var_adaptor.duration_predictor.", "t2u_model.decoder_frontend.variance_adaptor.duration_predictor."),
        (_T2U_DEC + ".dec_pos_emb_alpha", "t2u_model.decoder_frontend.pos_emb_alpha"),
        (_T2U_DEC + ".char_upsampler.pos_emb_alpha", "t2u_model.decoder_frontend.pos_emb_alpha_char"),
    ])
    rules += _stack(_T2U_DEC + ".", "t2u_model.decoder.", _NAR_DECODER_LAYER)
    rules += _plain([
        (_T2U_DEC + ".layer_norm.", "t2u_model.decoder.layer_norm."),
        (_T2U_DEC + ".output_projection.", "t2u_model.final_proj."),
    ])
    return rules


def rename_key(key: str, rules: Sequence[Tuple[re.Pattern, str]]) -> str:
    for pat, repl in rules:
        new = pat.sub(repl, key)
        if new != key:
            return new
    return key


def char_index_mapping(spm_tokens: Sequence[str]) -> List[int]:
    """loader.py:158-176: row i of the converted char embedding is row ``mapping[i]`` of the fairseq
    table, whose entries after the 4 control symbols are in SORTED order of the SentencePiece pieces."""
    spm_order = list(spm_tokens)[4:]
    dict_pos = {ch: idx for idx, ch in zip(range(4, len(spm_tokens)), sorted(spm_order))}
    return [0, 1, 2, 3] + [dict_pos[ch] for ch in spm_order]


def convert_unity_checkpoint(checkpoint: Mapping[str, Any], char_spm_tokens: Optional[Sequence[str]] = None,
                             use_text_encoder: bool = True, expressive: bool = False) -> Dict[str, torch.Tensor]:
    """fairseq-keyed UnitY2 checkpoint (``{"model": state_dict}`` or a bare state dict) -> fairseq2-keyed
    state dict.  A checkpoint that is already fairseq2-keyed passes through (loader.py:32-34).
    ``expressive``: the config has a prosody encoder (the expressive key map, unity_v2_key_rules)."""
    sd_in = checkpoint["model"] if "model" in checkpoint else checkpoint
    if FAIRSEQ2_MARKER in sd_in:
        return dict(sd_in)
    rules = unity_v2_key_rules(expressive)
    _ENC, _DEC, _T2U_ENC, _T2U_DEC = _EXPRESSIVE_PREFIXES if expressive else _PLAIN_PREFIXES
    # fairseq2's convert_fairseq_checkpoint drops these before renaming
    generic_drop = {"encoder.version", "decoder.version", "encoder.embed_positions._float_tensor",
                    "decoder.embed_positions._float_tensor"}
    sd: Dict[str, torch.Tensor] = {rename_key(k, rules): v for k, v in sd_in.items() if k not in generic_drop}
    # loader.py:62-117 (names are matched after renaming, as in the reference)
    drop = {
        f"{_DEC}.version", f"{_DEC}.embed_positions._float_tensor",
        f"{_ENC}.w2v_encoder.w2v_model.mask_emb",
        f"{_T2U_DEC}.char_upsampler.embed_positions._float_tensor",
        f"{_T2U_DEC}.char_upsampler.embed_tokens_char.weight",
        "decoder_target_letter_decoder.proj.weight", "decoder_target_letter_decoder.proj.bias",
    }
    if use_text_encoder:
        drop |= {"text_encoder.version", "text_encoder.embed_positions._float_tensor"}
    for k in list(sd):
        if k in drop or k.startswith(f"{_T2U_DEC}.alignment_encoder."):
            del sd[k]
    embeds = sd["final_proj.weight"]
    if embeds.size(0) == NLLB100_FAIRSEQ_VOCAB:  # fairseq's dummy token in the NLLB-100 table
        embeds = embeds[:-1]
        sd["final_proj.weight"] = embeds
    sd["text_decoder_frontend.embed.weight"] = embeds
    if use_text_encoder:
        sd["text_encoder_frontend.embed.weight"] = embeds
    with torch.inference_mode():
        # (BOS, PAD, EOS, UNK) -> (PAD, UNK, BOS, EOS)
        embeds[[0, 1, 2, 3]] = embeds[[1, 3, 0, 2]]
    char_embeds = sd.get("t2u_model.decoder_frontend.embed_char.weight")
    if char_embeds is not None:
        if char_spm_tokens is None:
            raise ValueError("the checkpoint carries a char embedding: pass the char tokenizer's pieces (char_spm_tokens)")
        mapping = char_index_mapping(char_spm_tokens)
        with torch.inference_mode():
            char_embeds[torch.arange(len(mapping))] = char_embeds[mapping]
    if "t2u_model.final_proj.weight" in sd and "t2u_model.decoder_frontend.embed.weight" in sd:
        sd["t2u_model.decoder_frontend.embed.weight"] = sd["t2u_model.final_proj.weight"]
    return sd


def convert_vocoder_checkpoint(checkpoint: Mapping[str, Any]) -> Dict[str, torch.Tensor]:
    """models/vocoder/loader.py:20-36.  The published fairseq vocoder checkpoint is ``{"generator": {<unprefixed keys>}}``:
    every key becomes ``code_generator.<key>``.  A checkpoint that already carries ``model`` with
    ``code_generator.resblocks.0.convs1.0.weight_g`` (the reference's own test for "converted") passes through.  Returns
    the state dict (the reference returns the checkpoint whose ``model`` entry is that dict)."""
    if "model" in checkpoint and "code_generator.resblocks.0.convs1.0.weight_g" in checkpoint["model"]:
        return dict(checkpoint["model"])
    if "generator" not in checkpoint:
        # not a layout the reference's converter accepts (it would raise KeyError): a bare, already prefixed state dict is
        # accepted as a convenience, anything else is an error rather than a silently wrong weight table
        if any(k.startswith("code_generator.") for k in checkpoint):
            return dict(checkpoint)
        raise KeyError("vocoder checkpoint holds neither 'generator' (fairseq layout) nor a converted 'model' state dict")
    return {f"code_generator.{k}": v for k, v in checkpoint["generator"].items()}


ALIGNER_MARKER = "alignment_encoder.t_conv.1.weight"


def convert_unity2_aligner_checkpoint(checkpoint: Mapping[str, Any], char_spm_tokens: Optional[Sequence[str]] = None) -> Dict[str, torch.Tensor]:
    """models/aligner/loader.py:22-57.  The published layout is ``{"text_emb_state": {"weight"}, "unit_emb_state": {"weight"},
    "aligner_state": {<encoder keys>}}``: the embeddings move to ``alignment_frontend.embed_{text,unit}.weight``, the encoder
    keys get the ``alignment_encoder.`` prefix and the rows of the char embedding are re-ordered from the fairseq dictionary's
    sorted order to the SentencePiece model's (:func:`char_index_mapping`).  A checkpoint whose ``model`` entry already holds
    ``alignment_encoder.t_conv.1.weight`` passes through.  Returns the state dict (the reference returns the checkpoint whose
    ``model`` entry is that dict)."""
    if "model" in checkpoint and ALIGNER_MARKER in checkpoint["model"]:
        return dict(checkpoint["model"])
    sd: Dict[str, torch.Tensor] = {f"alignment_encoder.{k}": v for k, v in checkpoint["aligner_state"].items()}
    for side in ("text", "unit"):
        state = checkpoint[f"{side}_emb_state"]
        if set(state) != {"weight"}:
            raise KeyError(f"{side}_emb_state holds {sorted(state)}; only 'weight' is known")
        sd[f"alignment_frontend.embed_{side}.weight"] = state["weight"]
    if char_spm_tokens is None:
        raise ValueError("the aligner checkpoint carries a char embedding: pass the char tokenizer's pieces (char_spm_tokens)")
    mapping = char_index_mapping(char_spm_tokens)
    char_embeds = sd["alignment_frontend.embed_text.weight"]
    with torch.inference_mode():
        char_embeds[torch.arange(len(mapping))] = char_embeds[mapping]
    return sd


def load_converted_checkpoint(path: str, kind: str, char_spm_tokens: Optional[Sequence[str]] = None,
                              expressive: bool = False) -> Dict[str, torch.Tensor]:
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if kind == "vocoder":
        return convert_vocoder_checkpoint(ckpt)
    if kind == "aligner":
        return convert_unity2_aligner_checkpoint(ckpt, char_spm_tokens=char_spm_tokens)
    return convert_unity_checkpoint(ckpt, char_spm_tokens=char_spm_tokens, expressive=expressive)


def convert_wav2vec2_checkpoint(checkpoint: Mapping[str, Any]) -> Dict[str, torch.Tensor]:
    """fairseq wav2vec 2.0 names -> fairseq2's, the shared entries of models/conformer_shaw/loader.py:44-71 plus
    ``final_layer_norm`` -> ``ffn_layer_norm``; quantiser, mask and projection-head tensors are dropped.  A dict that is
    already fairseq2-keyed (``encoder_frontend.*``) passes through."""
    sd = checkpoint.get("model", checkpoint)
    if any(k.startswith("encoder_frontend.") for k in sd):
        return {k: v for k, v in sd.items() if k.startswith(("encoder_frontend.", "encoder."))}
    rules = [
        (re.compile(r"^encoder\.layers\.([0-9]+)\.self_attn\.out_proj\."), r"encoder.layers.\1.self_attn.output_proj."),
        (re.compile(r"^encoder\.layers\.([0-9]+)\.fc1\."), r"encoder.layers.\1.ffn.inner_proj."),
        (re.compile(r"^encoder\.layers\.([0-9]+)\.fc2\."), r"encoder.layers.\1.ffn.output_proj."),
        (re.compile(r"^encoder\.layers\.([0-9]+)\.final_layer_norm\."), r"encoder.layers.\1.ffn_layer_norm."),
        (re.compile(r"^encoder\.pos_conv\.0\."), r"encoder_frontend.pos_encoder.conv."),
        (re.compile(r"^feature_extractor\.conv_layers\.([0-9]+)\.0\."), r"encoder_frontend.feature_extractor.layers.\1.conv."),
        (re.compile(r"^feature_extractor\.conv_layers\.([0-9]+)\.2\.1\."), r"encoder_frontend.feature_extractor.layers.\1.layer_norm."),
        (re.compile(r"^layer_norm\."), r"encoder_frontend.post_extract_layer_norm."),
        (re.compile(r"^post_extract_proj\."), r"encoder_frontend.model_dim_proj."),
    ]
    dropped = ("quantizer.", "project_q.", "final_proj.", "mask_emb", "encoder.layer_norm.", "mlm_proj.")
    out: Dict[str, torch.Tensor] = {}
    for k, v in sd.items():
        if k.startswith(dropped):
            continue
        for pat, rep in rules:
            k2, n = pat.subn(rep, k)
            if n:
                k = k2
                break
        out[k] = v
    return out
