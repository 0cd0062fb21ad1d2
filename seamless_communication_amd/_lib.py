"""ctypes binding of libseamless_hip.so (C ABI in include/seamless_hip.h).

The product path has no CPU fallback: if the shared library is missing or a
call fails, a :class:`SeamlessHipError` is raised.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Optional

import os

# SC_LIB_VARIANT=<name> loads libseamless_hip.<name>.so (an A/B build of `python -m seamless_communication_amd.build --variant
# name --flags "..."`; kernel development only - the product and the driver's runs use the plain name)
_VARIANT = os.environ.get("SC_LIB_VARIANT", "")
LIB_PATH = Path(__file__).resolve().parent / (f"libseamless_hip.{_VARIANT}.so" if _VARIANT else "libseamless_hip.so")

SC_ABI_VERSION = 10
SC_MAX_UPSAMPLES = 8
SC_MAX_RESBLOCK_KERNELS = 4
SC_MAX_RESBLOCK_DILATIONS = 4
SC_F16, SC_F32, SC_I32 = 0, 1, 2


class SeamlessHipError(RuntimeError):
    pass


class sc_tensor_desc(C.Structure):
    _fields_ = [
        ("name", C.c_char_p),
        ("dtype", C.c_int32),
        ("ndim", C.c_int32),
        ("shape", C.c_int64 * 4),
        ("data", C.c_void_p),
        ("on_device", C.c_int32),
    ]


_i = C.c_int32


class sc_config(C.Structure):
    _fields_ = [
        ("abi_version", _i), ("model_dim", _i), ("num_heads", _i),
        ("num_fbank_channels", _i), ("fbank_stride", _i),
        ("enc_layers", _i), ("enc_ffn_dim", _i), ("depthwise_conv_kernel_size", _i),
        ("shaw_max_left", _i), ("shaw_max_right", _i),
        ("adaptor_kernel_size", _i), ("adaptor_stride", _i), ("adaptor_ffn_dim", _i), ("adaptor_proj_dim", _i),
        ("dec_layers", _i), ("dec_ffn_dim", _i), ("text_vocab_size", _i), ("text_max_seq_len", _i),
        ("pad_idx", _i), ("unk_idx", _i), ("bos_idx", _i), ("eos_idx", _i),
        ("t2u_enc_layers", _i), ("t2u_dec_layers", _i), ("t2u_ffn_dim", _i), ("t2u_conv_kernel", _i),
        ("t2u_conv_inner_dim", _i),
        ("unit_vocab_size", _i), ("unit_pad_idx", _i), ("unit_eos_idx", _i), ("unit_max_seq_len", _i),
        ("char_vocab_size", _i), ("char_max_seq_len", _i), ("var_pred_hidden_dim", _i), ("var_pred_kernel_size", _i),
        ("voc_num_upsamples", _i),
        ("voc_upsample_rates", _i * SC_MAX_UPSAMPLES),
        ("voc_upsample_kernel_sizes", _i * SC_MAX_UPSAMPLES),
        ("voc_upsample_initial_channel", _i),
        ("voc_num_resblock_kernels", _i),
        ("voc_resblock_kernel_sizes", _i * SC_MAX_RESBLOCK_KERNELS),
        ("voc_num_resblock_dilations", _i),
        ("voc_resblock_dilation_sizes", (_i * SC_MAX_RESBLOCK_DILATIONS) * SC_MAX_RESBLOCK_KERNELS),
        ("voc_num_embeddings", _i), ("voc_embedding_dim", _i), ("voc_lang_embedding_dim", _i), ("voc_num_langs", _i),
        ("voc_spkr_embedding_dim", _i), ("voc_num_spkrs", _i),
        ("has_t2u", _i), ("has_vocoder", _i),
        ("text_enc_layers", _i), ("text_enc_ffn_dim", _i),
        ("mma_layers", _i), ("mma_ffn_dim", _i), ("mma_energy_layers", _i), ("mma_pre_decision_ratio", _i),
        ("mma_temperature", C.c_float),
        ("enc_variant", _i),
        ("voc_dur_pred_hidden_dim", _i), ("voc_dur_pred_kernel_size", _i),
        ("t2u_variant", _i),
    ]


SC_FFN_RELU, SC_FFN_GELU = 0, 1


class sc_load_ext_opts(C.Structure):
    _fields_ = [("abi_version", _i), ("ffn_activation", _i), ("t2u_ffn_activation", _i), ("film_cond_dim", _i)]


def make_load_ext(cfg) -> sc_load_ext_opts:
    """The sc_load_ext extension of a config: zeroed (= sc_load) for every model but the expressive one."""
    acts = {"relu": SC_FFN_RELU, "gelu": SC_FFN_GELU}
    e = sc_load_ext_opts()
    fa, ta, fd = getattr(cfg, "ffn_activation", "relu"), getattr(cfg, "t2u_ffn_activation", "relu"), int(getattr(cfg, "film_cond_dim", 0))
    if fa not in acts or ta not in acts:
        raise ValueError(f"unknown FFN activation ({fa!r}, {ta!r}); supported: relu, gelu")
    if fa != "relu" or ta != "relu" or fd:
        e.abi_version = SC_ABI_VERSION
        e.ffn_activation, e.t2u_ffn_activation, e.film_cond_dim = acts[fa], acts[ta], fd
    return e


class sc_gen_opts(C.Structure):
    _fields_ = [
        ("beam_size", _i), ("soft_max_seq_len_a", C.c_float), ("soft_max_seq_len_b", _i),
        ("hard_max_seq_len", _i), ("min_seq_len", _i), ("unk_penalty", C.c_float), ("use_graph", _i),
        ("len_penalty", C.c_float), ("normalize_scores", _i), ("no_repeat_ngram_size", _i), ("source_len", _i),
    ]


class sc_sample_opts(C.Structure):
    _fields_ = [("abi_version", _i), ("num_gens", _i), ("top_k", _i), ("top_p", C.c_float), ("temperature", C.c_float), ("seed", C.c_uint64)]


class sc_engine_opts(C.Structure):
    _fields_ = [
        ("slots", _i), ("rows", _i), ("max_len", _i), ("s_enc", _i), ("min_seq_len", _i), ("unk_penalty", C.c_float),
        ("poll", _i), ("low_water", _i), ("max_wait_ms", _i), ("use_graph", _i),
    ]


class sc_engine_stats(C.Structure):
    _fields_ = [
        ("steps", C.c_int64), ("row_steps", C.c_int64), ("useful_row_steps", C.c_int64), ("rows_admitted", C.c_int64),
        ("rows_retired", C.c_int64), ("requests", C.c_int64), ("max_live", C.c_int64), ("busy_us", C.c_double), ("wait_us", C.c_double),
        ("self_kv_bytes", C.c_int64), ("cross_kv_bytes", C.c_int64), ("hidden_bytes", C.c_int64),
    ]


class sc_mma_pool_opts(C.Structure):
    _fields_ = [("abi_version", _i), ("sessions", _i), ("max_len", _i), ("s_enc_cap", _i)]


class sc_mma_pool_stats(C.Structure):
    _fields_ = [("self_kv_bytes", C.c_int64), ("cross_kv_bytes", C.c_int64), ("work_bytes", C.c_int64), ("begins", C.c_int64),
                ("steps", C.c_int64), ("row_steps", C.c_int64)]


class sc_unit_extractor_config(C.Structure):
    _fields_ = [
        ("abi_version", _i), ("model_dim", _i), ("heads", _i), ("ffn_dim", _i), ("layers", _i), ("feature_dim", _i), ("fe_layers", _i),
        ("fe_kernel", _i * 8), ("fe_stride", _i * 8), ("pos_conv_kernel", _i), ("pos_conv_groups", _i), ("num_centroids", _i),
    ]


class sc_pretssel_config(C.Structure):
    _fields_ = [
        ("abi_version", _i), ("model_dim", _i), ("num_heads", _i), ("enc_layers", _i), ("dec_layers", _i), ("conv_inner_dim", _i), ("conv_kernel", _i),
        ("film_cond_dim", _i), ("lang_embed_dim", _i), ("num_langs", _i), ("pred_hidden_dim", _i), ("pred_kernel", _i), ("vocab_size", _i),
        ("pad_idx", _i), ("max_seq_len", _i), ("mel_dim", _i), ("post_layers", _i), ("post_dim", _i), ("post_kernel", _i), ("upsample_delta", C.c_float),
    ]


class sc_pretssel_wave_config(C.Structure):
    _fields_ = [
        ("abi_version", _i), ("mel_dim", _i), ("post_layers", _i), ("upsample_initial_channel", _i), ("num_upsamples", _i),
        ("upsample_rates", _i * 8), ("upsample_kernel_sizes", _i * 8), ("resblock_kernel_sizes", _i * 3), ("resblock_dilation_sizes", (_i * 3) * 3),
        ("n_filters", _i), ("ratios", _i * 4), ("dimension", _i),
    ]


class sc_prosody_encoder_config(C.Structure):
    _fields_ = [
        ("abi_version", _i), ("input_dim", _i), ("embed_dim", _i), ("res2net_scale", _i), ("se_channels", _i), ("attention_channels", _i),
        ("global_context", _i), ("n_blocks", _i), ("channels", _i * 8), ("kernel_sizes", _i * 8), ("dilations", _i * 8),
    ]


class sc_resample_opts(C.Structure):
    _fields_ = [("abi_version", _i), ("lowpass_filter_width", _i), ("rolloff", C.c_float), ("method", _i), ("beta", C.c_float)]


class sc_tsm_opts(C.Structure):
    _fields_ = [("abi_version", _i), ("frame", _i), ("radius", _i)]


class sc_vad_opts(C.Structure):
    _fields_ = [("abi_version", _i), ("hangover", _i), ("floor_quantile", C.c_float), ("peak_quantile", C.c_float),
                ("noise_ceiling_db", C.c_float), ("min_margin_db", C.c_float), ("range_fraction", C.c_float), ("slope_db", C.c_float)]


class sc_vad_stream_opts(C.Structure):
    _fields_ = sc_vad_opts._fields_ + [("history_windows", _i)]


class sc_mbr_opts(C.Structure):
    _fields_ = [("abi_version", _i), ("max_order", _i), ("beta", C.c_float), ("reserved", _i)]


class sc_aligner_config(C.Structure):
    _fields_ = [
        ("abi_version", _i), ("model_dim", _i), ("feat_dim", _i), ("text_layers", _i), ("feat_layers", _i),
        ("temperature", C.c_float), ("reduction_factor", _i), ("char_vocab_size", _i), ("unit_vocab_size", _i),
    ]


_P = C.c_void_p
_PI = C.POINTER(C.c_int32)

# name -> (restype, argtypes); every symbol include/seamless_hip.h declares
SIGNATURES = {
    "sc_last_error": (C.c_char_p, []),
    "sc_abi_version": (C.c_int, []),
    "sc_load": (_P, [C.POINTER(sc_tensor_desc), C.c_size_t, C.POINTER(sc_config), C.c_int]),
    "sc_load_ext": (_P, [C.POINTER(sc_tensor_desc), C.c_size_t, C.POINTER(sc_config), C.POINTER(sc_load_ext_opts), C.c_int]),
    "sc_fork": (_P, [_P]),
    "sc_free": (None, [_P]),
    "sc_synchronize": (C.c_int, [_P]),
    "sc_wait_stream": (C.c_int, [_P, _P]),
    "sc_decoder_step_family": (C.c_int, [_P, C.c_int, C.c_int]),
    "sc_set_nar_tables": (C.c_int, [_P, _i, _P, _P, _P, _P, _P]),
    "sc_fbank": (C.c_int, [_P, _P, _i, C.c_int64, _P, _i, _P, _i, _P]),
    "sc_fbank_rate": (C.c_int, [_P, _P, _i, C.c_int64, _P, _i, _i, _P, _i, _P]),
    "sc_fbank_frames": (_i, [C.c_int64, _i]),
    "sc_encoder_out_len": (_i, [_P, _i]),
    "sc_encode_speech": (C.c_int, [_P, _P, _i, _i, _P, _P, _P]),
    "sc_encode_speech_ragged": (C.c_int, [_P, _P, _i, _i, _P, _P, _i, _P]),
    "sc_encode_text": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    "sc_mma_begin": (C.c_int, [_P, _P, C.c_int32, C.c_int32]),
    "sc_mma_step": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    "sc_mma_pool_create": (_P, [_P, C.POINTER(sc_mma_pool_opts)]),
    "sc_mma_pool_free": (None, [_P]),
    "sc_mma_pool_begin": (C.c_int, [_P, _P, _i, _P, _P]),
    "sc_mma_pool_step": (C.c_int, [_P, _P, _i, _P, _i, _P, _P, _i, _P, _P, _P, _P]),
    "sc_mma_pool_get_stats": (C.c_int, [_P, C.POINTER(sc_mma_pool_stats), _i]),
    "sc_text_max_len": (_i, [_P, C.POINTER(sc_gen_opts), _i]),
    "sc_generate_text": (C.c_int, [_P, _P, _i, _i, _P, C.POINTER(sc_gen_opts), _P, _i, _P, _P, _P, _P]),
    "sc_generate_text_banned": (C.c_int, [_P, _P, _i, _i, _P, C.POINTER(sc_gen_opts), _P, _i, _P, _P, _P, _P, _P, _P, _i]),
    "sc_generate_text_boosted": (C.c_int, [_P, _P, _i, _i, _P, C.POINTER(sc_gen_opts), _P, _i, _P, _P, _P, _P, _P, _P, _i, _P, _P, _i,
                                           C.c_float]),
    "sc_generate_text_sampled": (C.c_int, [_P, _P, _i, _i, _P, C.POINTER(sc_gen_opts), C.POINTER(sc_sample_opts), _P, _P, _i, _P, _P, _P, _P, _P,
                                           _P, _P, _i]),
    "sc_generate_text_capture": (C.c_int, [_P, _P, _i, _i, _P, C.POINTER(sc_gen_opts), _P, _i, _P, _P, _P, _P, _P, _P]),
    "sc_decode_text": (C.c_int, [_P, _P, _i, _i, _P, _P, _i, _P]),
    "sc_score_text": (C.c_int, [_P, _P, _i, _i, _P, _P, _P, _i, _P, _P, _P, _P]),
    "sc_score_text_capture": (C.c_int, [_P, _P, _i, _i, _P, _P, _P, _i, _P, _P, _P, _P, _P]),
    "sc_op_xattn_rows": (C.c_int, [_P, C.c_int64, _P, C.c_int64, _i, _i, _i, _i, _P, _P, _P]),
    "sc_op_xattn_rows_tile": (C.c_int32, [_i]),
    "sc_identify_language": (C.c_int, [_P, _P, _i, _i, _P, _P, _i, _P, _i, _P, _P]),
    "sc_generate_text_rows": (C.c_int, [_P, _P, _i, _i, _P, _P, _P, _i, _P, _P, _P, _P]),
    "sc_generate_text_prompts": (C.c_int, [_P, _P, _i, _i, _P, C.POINTER(sc_gen_opts), _P, _i, _P, _P, _P, _P, _P, _P, _P, _i, _P, _P, _i,
                                           C.c_float]),
    "sc_generate_text_nbest": (C.c_int, [_P, _P, _i, _i, _P, C.POINTER(sc_gen_opts), _P, _i, _P, _i, _P, _P, _P, _P, _P, _P, _P, _i, _P, _P,
                                         _i, C.c_float]),
    "sc_engine_create": (_P, [_P, C.POINTER(sc_engine_opts)]),
    "sc_engine_free": (None, [_P]),
    "sc_engine_attach": (C.c_int, [_P, _P]),
    "sc_engine_expect": (C.c_int, [_P, _i]),
    "sc_engine_get_stats": (C.c_int, [_P, C.POINTER(sc_engine_stats), _i]),
    "sc_t2u_nar": (C.c_int, [_P, _P, _i, _i, _P, _P, C.c_float, _P, _PI, _PI]),
    "sc_t2u_nar_cond": (C.c_int, [_P, _P, _i, _i, _P, _P, C.c_float, _P, _P, _PI, _PI]),
    "sc_t2u_nar_fit": (C.c_int, [_P, _P, _i, _i, _P, _P, _P, _P, _P, _P, _P, _PI, _PI, _P, _P]),
    "sc_op_t2u_last_launches": (C.c_int32, [_P]),
    "sc_op_t2u_encoder": (C.c_int, [_P, _P, _i, _i, _P, _P, _P]),
    "sc_get_units": (C.c_int, [_P, _P]),
    "sc_get_durations": (C.c_int, [_P, _P, _P, _P]),
    "sc_vocoder_hop": (_i, [_P]),
    "sc_vocode": (C.c_int, [_P, _P, _i, _i, _P, _P, _P]),
    "sc_vocode_ragged": (C.c_int, [_P, _P, _i, _i, _P, _P, _P, _P]),
    "sc_vocoder_durations": (C.c_int, [_P, _P, _i, _i, _P]),
    "sc_t2u_ar": (C.c_int, [_P, _P, _i, _i, _P, C.POINTER(sc_gen_opts), _P, _i, _P, _i, _P, _P]),
    "sc_t2u_ar_max_len": (_i, [_P, C.POINTER(sc_gen_opts), _i]),
    "sc_last_padding": (C.c_int, [_P, _P, _P, _P]),
    "sc_s2st": (C.c_int, [_P, _P, _i, _i, _P, C.POINTER(sc_gen_opts), _P, _i, C.c_float, _P, _P, _P, _i, _P, _P, _i, _P, _P, _P]),
    "sc_prof_enable": (C.c_int, [C.c_int]),
    "sc_prof_reset": (C.c_int, []),
    "sc_prof_report": (C.c_int64, [C.c_char_p, C.c_int64]),
    "sc_text_to_char_seqs": (C.c_int32, [C.c_int32, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32,
                                         _P, _P, C.c_int32, _P]),
    "sc_ngram_blocked_tokens": (C.c_int32, [_PI, C.c_int32, C.c_int32, _PI, C.c_int32]),
    "sc_banned_blocked_tokens": (C.c_int32, [_PI, C.c_int32, _PI, _PI, C.c_int32, _PI, C.c_int32]),
    "sc_boost_deltas": (C.c_int32, [_PI, C.c_int32, _PI, _PI, C.c_int32, _PI, _PI, C.c_int32, _PI]),
    "sc_aligner_load": (_P, [C.POINTER(sc_tensor_desc), C.c_size_t, C.POINTER(sc_aligner_config), C.c_int]),
    "sc_aligner_free": (None, [_P]),
    "sc_align": (C.c_int, [_P, _P, _i, _i, _P, _P, _i, _P, _P, _P]),
    "sc_op_align_lprob": (C.c_int, [_P, _P, _i, _i, _i, _i, _P, _P, C.c_float, _P]),
    "sc_op_mas": (C.c_int, [_P, _i, _i, _i, _P, _P, _P]),
    "sc_unit_extractor_load": (_P, [C.POINTER(sc_tensor_desc), C.c_size_t, C.POINTER(sc_unit_extractor_config), C.c_int]),
    "sc_unit_extractor_free": (None, [_P]),
    "sc_unit_extractor_num_frames": (C.c_int32, [C.POINTER(sc_unit_extractor_config), C.c_int64]),
    "sc_extract_units": (C.c_int, [_P, _P, _i, C.c_int64, _P, _i, _P, _i, _P, _P]),
    "sc_op_attention_hd": (C.c_int, [_P, _P, _P, _P, _i, _i, _i, _i, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P, _i]),
    "sc_op_w2v2_frontend": (C.c_int, [_P, C.c_int64, _P, _i, _P, _P, _P, _P, _i, _i, _i, _P, _i, _P]),
    "sc_op_w2v2_pos_conv": (C.c_int, [_P, _P, _P, _P, _i, _i, _i, _i, _i, _P]),
    "sc_op_kmeans": (C.c_int, [_P, _P, _i, _i, _i, _P]),
    "sc_prosody_encoder_load": (_P, [C.POINTER(sc_tensor_desc), C.c_size_t, C.POINTER(sc_prosody_encoder_config), C.c_int]),
    "sc_prosody_encoder_free": (None, [_P]),
    "sc_prosody_encode": (C.c_int, [_P, _P, _i, _i, _P, _P, _P, _P]),
    "sc_op_ecapa_chain": (C.c_int, [_P, _P, _P, _P, _P, _P, _i, _i, _i, _i, _i]),
    "sc_op_ecapa_chain_tile": (C.c_int32, [_i, _i, _i]),
    "sc_op_ecapa_relu_ln": (C.c_int, [_P, _P, _i, _P, _P, _P, _i, _i, _i]),
    "sc_op_ecapa_se_gate": (C.c_int, [_P, _i, _i, _P, _i, _i, _P, _P, _P, _P, _P]),
    "sc_op_ecapa_pool": (C.c_int, [_P, _P, _i, _i, _i, _P, _P, _P]),
    "sc_op_ecapa_tail": (C.c_int, [_P, _i, _i, _P, _P, _P, _P, _i, _P]),
    "sc_op_prosody_last_launches": (C.c_int32, [_P]),
    "sc_pretssel_load": (_P, [C.POINTER(sc_tensor_desc), C.c_size_t, C.POINTER(sc_pretssel_config), C.c_int]),
    "sc_pretssel_free": (None, [_P]),
    "sc_pretssel_mel": (C.c_int, [_P, _P, _i, _i, _P, _P, _i, _P, _P, _i, _P]),
    "sc_op_attention128": (C.c_int, [_P, _P, _P, _P, _i, _i, _i, _i, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P, _P, _P, _P, C.c_int64]),
    "sc_op_pretssel_film": (C.c_int, [_P, _i, _P, _i, _P, _P, _P, _P, _i, _i, _P]),
    "sc_op_pretssel_film_ln": (C.c_int, [_P, _P, _P, _P, _i, _i, _P, _P, _P, _P, _i, _i, _i]),
    "sc_op_pretssel_var_tail": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _i]),
    "sc_op_pretssel_upsample": (C.c_int, [_P, _P, _P, _i, _i, C.c_float, _P, C.c_float, _P, _P, _P, _P]),
    "sc_op_pretssel_ups_cutoff": (C.c_float, []),
    "sc_op_pretssel_postnet": (C.c_int, [_P, _P, _i, _P, _P, _i]),
    "sc_op_pretssel_postnet_tile": (C.c_int32, [_i, _i]),
    "sc_op_pretssel_last_launches": (C.c_int32, [_P]),
    "sc_pretssel_wave_load": (_P, [C.POINTER(sc_tensor_desc), C.c_size_t, C.POINTER(sc_pretssel_wave_config), C.c_int]),
    "sc_pretssel_wave_free": (None, [_P]),
    "sc_pretssel_wave": (C.c_int, [_P, _P, _i, _i, _P, _P, _i, _P, _i]),
    "sc_op_pretssel_wave_probe": (C.c_int, [_P, _P, _P, _P, _P]),
    "sc_op_pretssel_wave_lens": (C.c_int, [_P, _i, _P, _P]),
    "sc_op_pretssel_wave_last_launches": (C.c_int32, [_P]),
    "sc_op_pretssel_wave_stage_ms": (C.c_int, [_P, _P]),
    "sc_op_lstm2": (C.c_int, [_P, _P, _i, _i, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sc_op_seanet_resblock_tile": (C.c_int32, []),
    "sc_op_seanet_resblock": (C.c_int, [_P, _P, _i, _i, _P, _P, _P, _P, _P]),
    "sc_op_sconv": (C.c_int, [_P, _P, _i, _i, _i, _i, _i, _i, _i, _P, _P, _P, _P, _P]),
    "sc_op_seanet_tail": (C.c_int, [_P, _P, _P, _i, _i, _i, _P, _P, _P, _P, C.c_int64]),
    "sc_resample_len": (C.c_int64, [C.c_int64, _i, _i]),
    "sc_resample": (C.c_int, [_P, _i, C.c_int64, _P, _i, _i, C.POINTER(sc_resample_opts), _P, C.c_int64, _P]),
    "sc_mix_timeline": (C.c_int, [_P, _i, C.c_int64, _P, _P, _P, _i, _P, C.c_float, _i, _P, C.c_int64]),
    "sc_time_stretch": (C.c_int, [_P, _i, C.c_int64, _P, C.POINTER(sc_tsm_opts), _P, C.c_int64, _P]),
    "sc_vad_windows": (C.c_int64, [C.c_int64, _i]),
    "sc_vad_probs": (C.c_int, [_P, _i, C.c_int64, _P, _i, C.POINTER(sc_vad_opts), _P, C.c_int64, _P, _P]),
    "sc_vad_stream_create": (C.c_int, [_i, _i, C.POINTER(sc_vad_stream_opts), C.POINTER(_P)]),
    "sc_vad_stream_destroy": (None, [_P]),
    "sc_vad_stream_reset": (C.c_int, [_P, _P, _i]),
    "sc_vad_stream_push": (C.c_int, [_P, _P, _i, _P, C.c_int64, _P, _P, C.c_int64, _P, _P]),
    "sc_mbr_select": (C.c_int, [_P, _i, _i, _i, _P, _P, _P, C.POINTER(sc_mbr_opts), _P, _P, _P, _P]),
    "sc_ngram_match": (C.c_int, [_P, _P, _i, _P, C.c_int64, _i, _P]),
    "sc_edit_distance": (C.c_int, [_P, _P, _i, _P, C.c_int64, _P]),
    "sc_op_resample_bank": (C.c_int, [_i, _i, C.POINTER(sc_resample_opts), _PI, _PI, _P, _P, C.c_int64]),
    "sc_op_resample_plan": (C.c_int, [_i, _i, C.POINTER(sc_resample_opts), _P]),
    "sc_op_fit_durations": (C.c_int, [_P, _i, _i, _P, _P, _P, _P, _i, _P, _P, _P, _P]),
    "sc_op_tsm_centres": (C.c_int, [_P, _i, C.c_int64, _P, _P, C.POINTER(sc_tsm_opts), _P, C.c_int64]),
    "sc_op_knob": (C.c_int, [C.c_char_p, C.c_int]),
    "sc_op_force_general_gemm": (C.c_int, [C.c_int]),
    "sc_op_voc_pack_plan": (C.c_int32, [_PI, C.c_int32, C.c_int64, _PI, C.c_int32]),
    "sc_op_voc_tile_first": (C.c_int32, [_PI, C.c_int32, C.c_int32, C.c_int32, _PI]),
    "sc_op_last_vocoder_packed_groups": (C.c_int32, [_P]),
    "sc_op_single_plane": (C.c_int, [C.c_int]),
    "sc_op_layernorm": (C.c_int, [_P, _P, _P, _P, _i, _i, _i]),
    "sc_op_linear": (C.c_int, [_P, _P, _P, _P, _P, _i, _i, _i, _i, C.c_float, _i, _i]),
    "sc_op_skinny_linear": (C.c_int, [_P, _P, _P, _P, _P, _i, _i, _i, _i, C.c_float]),
    "sc_op_skinny_res_ln": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _i, _i, _i, _i]),
    "sc_op_skinny_argmax": (C.c_int, [_P, _P, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.c_float, _P, _P]),
    "sc_op_dstep_res_ln": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _i, _i, _i, _i]),
    "sc_op_dstep_linear_planes": (C.c_int, [_P, _P, _P, _P, _i, _i, _i, _i]),
    "sc_op_dstep_argmax": (C.c_int, [_P, _P, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.c_float, _i, _P, _P]),
    "sc_op_resblock_pair_ps": (C.c_int, [_P, _P, _P, _P, _P, _P, _i, _i, _i, _i, _i]),
    "sc_op_glu_dwconv_ln": (C.c_int, [_P, _P, _P, _P, _i, _P, _P, _i, _i, _i, _i, _P, _i]),
    "sc_op_glu_dwconv_ln_packed": (C.c_int, [_P, _P, _P, _P, _i, _P, _P, _i, _P, _P, _i, _i, _i]),
    "sc_op_layernorm2": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _i]),
    "sc_op_dstep3_gemv": (C.c_int, [_i, _P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _i, _i, _i, _i]),
    "sc_op_dstep3_argmax": (C.c_int, [_P, _P, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.c_float, _P, _P]),
    "sc_op_chain_bench": (C.c_int, [_i, _i, _i, _i, _P]),
    "sc_op_dstep_attention": (C.c_int, [_P, _i, _P, _P, _P, _i, _i, _P, _i, _i, _i, _P]),
    "sc_op_conv1d": (C.c_int, [_P, _P, _P, _P, _P, _i, _i, _i, _i, _i, _i, _i, _i, _P, _i, _i]),
    "sc_op_pack_conv_weight": (C.c_int, [_P, _P, _i, _i, _i]),
    "sc_op_conv_transpose1d": (C.c_int, [_P, _P, _P, _P, _P, _i, _i, _i, _i, _i, _i, _i, _i]),
    "sc_op_linear_presplit": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _i, _i, _i, _i, C.c_float]),
    "sc_op_linear_presplit_glu": (C.c_int, [_P, _P, _P, _P, _i, _i, _i, _i]),
    "sc_op_linear_presplit_argmax": (C.c_int, [_P, _P, _P, _P, _i, _i, _i]),
    "sc_op_linear_presplit_score": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _i]),
    "sc_op_linear_presplit_score_grouped": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _i, _i]),
    "sc_op_score_candidates": (C.c_int, [_P, _P, _P, _P, _i, _P, _P, _i, _i, _i]),
    "sc_op_score_record_cols": (_i, [_i]),
    "sc_op_score_group_rows": (_i, [_i]),
    "sc_op_conv1d_presplit": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _i, _i, _i, _i, _i, _i, _i, _P, _i]),
    "sc_op_mrf_fused": (C.c_int, [_P, _P, _P, _P, _P, _P, _i, _i, _i, _P, _P, C.c_float]),
    "sc_op_resblock_pair": (C.c_int, [_P, _P, _P, _P, _P, _P, _i, _i, _i, _i, _i, C.c_float, _P, _P]),
    "sc_op_attention": (C.c_int, [_P, _P, _P, _P, _i, _i, _i, _i, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P, _i,
                                  _P, _i, _i]),
    "sc_op_attention_ex": (C.c_int, [_P, _P, _P, _P, _i, _i, _i, _i, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P, _i,
                                     _P, _i, _i, _P, _P, C.c_int64, _P, _P, _P, _P, C.c_int64]),
    "sc_op_glu_dwconv": (C.c_int, [_P, _P, _P, _i, _i, _i, _i, _P]),
    "sc_op_argmax": (C.c_int, [_P, _i, _i, _P, _P]),
    "sc_op_beam_candidates": (C.c_int, [_P, C.c_int64, _i, _i, _i, _P, _i, _i, _i, _i, _i, _i, C.c_float, _i, _P, _P, _P, _i, _i, _i,
                                        _P, _P, _i]),
    "sc_op_beam_candidates_banned": (C.c_int, [_P, C.c_int64, _i, _i, _i, _P, _i, _i, _i, _i, _i, _i, C.c_float, _i, _P, _P, _P, _i, _i,
                                               _i, _P, _P, _i, _P, _P, _i]),
    "sc_op_beam_candidates_boost": (C.c_int, [_P, C.c_int64, _i, _i, _i, _P, _i, _i, _i, _i, _i, _i, C.c_float, _i, _P, _P, _P, _i, _i,
                                              _i, _P, _P, _i, _P, _P, _i, _P, _P, _i, C.c_float]),
    "sc_op_sample_rows": (C.c_int, [_P, C.c_int64, _i, _i, _P, _P, _P, C.c_float, _i, C.c_float, C.c_uint64, _i, _i, _i, _i, _i, C.c_float,
                                    _P, _i, _i, _i, _P, _P, _i, _P, _P, _P, _P]),
    "sc_op_beam_select": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _P, _P, _i, _i, _i, _i, _i, _i, _i, _i,
                                    _i, C.c_float]),
    "sc_op_beam_compact": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _i, _i, _i, _i]),
    "sc_op_beam_select_hist": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _P, _P, _i, _i, _i, _i, _i, _i, _i,
                                         _i, _i, C.c_float, _P, _P, _P]),
    "sc_op_beam_compact_hist": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _i, _i, _i, _i, _i, _i, _P]),
    "sc_op_beam_nbest": (C.c_int, [_P, _P, _P, _P, _P, _i, _i, _i, _i, _i, _P, _P, _P, _P, _P]),
    "sc_op_gather_cache": (C.c_int, [_P, _P, _P, _i, _i, _i, _i, _i, C.c_int64]),
    "sc_op_row_token_lprob": (C.c_int, [_P, C.c_int64, _i, _i, _i, _i, _P]),
    "sc_op_dstep_attention_ex": (C.c_int, [_P, _i, _P, _P, _P, _i, _i, _i, _P, _i, _i, _i, _P, _P, _P, _P, _i, _P, _P]),
    "sc_op_engine_step_close": (C.c_int, [_P, _P, _i, _i, _i, _i, _i, _i, _i, C.c_float, _P, _P, _i, _i, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sc_op_engine_admit": (C.c_int, [_P, _i, _i, _i, _i, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sc_op_engine_set_slots": (C.c_int, [_P, _i, _i, _i, _P, _P, _P, _P]),
    "sc_op_engine_retire": (C.c_int, [_P, _P, _P, _i, _i, _i, _i, _P, _P, _P, _P, _P]),
    "sc_op_dstep3_embed_ex": (C.c_int, [_P, _P, C.c_float, _P, _i, _P, _P, _i, _i, _i, _i, _i, _P]),
    "sc_op_dstep3_reduce_capture_ex": (C.c_int, [_P, _i, _P, _P, _P, _P, _P, _P, C.c_int64, _i, _i, _P, _P, _i, _i, _i]),
    "sc_op_step_update": (C.c_int, [_P, _P, _i, _P, _P, _P, _P, _i, _i, _i, _i, _P]),
    "sc_op_row_swap": (C.c_int, [_P, _P, _P, _i, _i, _P, _P, _i, _i, _i, _i, _i, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sc_op_layernorm_ex": (C.c_int, [_P, C.c_int64, _P, _P, _P, C.c_int64, _P, _P, C.c_int64, _i, _i, _i, _P, _i]),
    "sc_op_embed_tokens": (C.c_int, [_P, _i, _P, _i, C.c_float, _P, _P, _i, _P, C.c_int64]),
    "sc_op_gather_rows": (C.c_int, [_P, C.c_int64, _P, _P, C.c_int64, _i, _P, C.c_int64, _i, _i]),
    "sc_op_char_embed_add": (C.c_int, [_P, C.c_int64, _P, _P, _P, _i, C.c_float, C.c_float, _i, _i]),
    "sc_op_pos_add": (C.c_int, [_P, C.c_int64, _P, _i, _P, C.c_float, _i, _i]),
    "sc_op_durations": (C.c_int, [_P, C.c_int64, _P, _P, _i, _i, _i, _P, C.c_float, _i, _P]),
    "sc_op_vocoder_embed": (C.c_int, [_P, _i, _i, _P, _i, _P, _i, _P, _P, _i, _P, _P, _P, _i]),
    "sc_op_item_row_pos": (C.c_int, [_P, _i, _i, _i, _P]),
    "sc_op_scatter_items": (C.c_int, [_P, _P, _P, _i, _i, _i, C.c_int64, _P]),
    "sc_op_glu_dwconv_ex": (C.c_int, [_P, _P, _P, _i, _i, _i, _i, _P, _i, _P, _P, _P, _P]),
    "sc_op_relpos_table": (C.c_int, [_i, _i, _P]),
}

_lib: Optional[C.CDLL] = None


def load_library() -> C.CDLL:
    """dlopen the in-tree library and bind every declared entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise SeamlessHipError(
            f"{LIB_PATH} is missing: build it with `python -m seamless_communication_amd.build` "
            "(there is no CPU fallback for the HIP path)"
        )
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.sc_abi_version() != SC_ABI_VERSION:
        raise SeamlessHipError(f"ABI mismatch: library {lib.sc_abi_version()} vs binding {SC_ABI_VERSION}")
    _lib = lib
    return lib


def banned_csr(banned_seqs):
    """Token sequences -> (tokens int32, offsets int32 [n + 1]): the CSR form sc_generate_text_banned and
    sc_banned_blocked_tokens take.  An empty sequence is a ``ValueError`` (the C side would refuse it too)."""
    import numpy as np

    seqs = [[int(t) for t in (s.tolist() if hasattr(s, "tolist") else s)] for s in banned_seqs]
    if any(len(s) == 0 for s in seqs):
        raise ValueError("a banned sequence must hold at least one token")
    off = np.zeros(len(seqs) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.int64)
    tok = np.asarray([t for s in seqs for t in s], dtype=np.int32)
    return tok, off


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load_library().sc_last_error()
        raise SeamlessHipError(f"{what} failed with status {status}: {msg.decode() if msg else '?'}")


def make_config(cfg, has_t2u: bool = True, has_vocoder: bool = True, has_text_encoder: bool = False,
                has_monotonic_decoder: bool = False, has_vocoder_dur_predictor: bool = False) -> sc_config:
    c = sc_config()
    c.abi_version = SC_ABI_VERSION
    for f in (
        "model_dim num_heads num_fbank_channels fbank_stride enc_layers enc_ffn_dim depthwise_conv_kernel_size "
        "shaw_max_left shaw_max_right adaptor_kernel_size adaptor_stride adaptor_ffn_dim adaptor_proj_dim dec_layers "
        "dec_ffn_dim text_vocab_size text_max_seq_len pad_idx unk_idx bos_idx eos_idx t2u_enc_layers t2u_dec_layers "
        "t2u_ffn_dim t2u_conv_kernel t2u_conv_inner_dim unit_vocab_size unit_pad_idx unit_eos_idx unit_max_seq_len "
        "char_vocab_size char_max_seq_len var_pred_hidden_dim var_pred_kernel_size"
    ).split():
        setattr(c, f, int(getattr(cfg, f)))
    v = cfg.vocoder
    if len(v.upsample_rates) > SC_MAX_UPSAMPLES or len(v.resblock_kernel_sizes) > SC_MAX_RESBLOCK_KERNELS:
        raise ValueError("vocoder config exceeds the ABI's fixed array sizes")
    c.voc_num_upsamples = len(v.upsample_rates)
    for i, (r, k) in enumerate(zip(v.upsample_rates, v.upsample_kernel_sizes)):
        c.voc_upsample_rates[i] = r
        c.voc_upsample_kernel_sizes[i] = k
    c.voc_upsample_initial_channel = v.upsample_initial_channel
    c.voc_num_resblock_kernels = len(v.resblock_kernel_sizes)
    nd = len(v.resblock_dilation_sizes[0])
    if nd > SC_MAX_RESBLOCK_DILATIONS or any(len(d) != nd for d in v.resblock_dilation_sizes):
        raise ValueError("unsupported resblock dilation layout")
    c.voc_num_resblock_dilations = nd
    for j, (rk, dils) in enumerate(zip(v.resblock_kernel_sizes, v.resblock_dilation_sizes)):
        c.voc_resblock_kernel_sizes[j] = rk
        for d, dv in enumerate(dils):
            c.voc_resblock_dilation_sizes[j][d] = dv
    c.voc_num_embeddings = v.num_embeddings
    c.voc_embedding_dim = v.embedding_dim
    c.voc_lang_embedding_dim = v.lang_embedding_dim
    c.voc_num_langs = v.num_langs
    c.voc_spkr_embedding_dim = v.spkr_embedding_dim
    c.voc_num_spkrs = v.num_spkrs
    c.has_t2u = int(has_t2u)
    c.has_vocoder = int(has_vocoder)
    c.text_enc_layers = int(cfg.text_enc_layers) if has_text_encoder else 0
    c.text_enc_ffn_dim = int(cfg.text_enc_ffn_dim)
    c.mma_layers = int(cfg.mma_layers) if has_monotonic_decoder else 0
    c.mma_ffn_dim = int(cfg.mma_ffn_dim)
    c.mma_energy_layers = int(cfg.mma_energy_layers)
    c.mma_pre_decision_ratio = int(cfg.mma_pre_decision_ratio)
    c.mma_temperature = float(cfg.mma_temperature)
    c.enc_variant = int(getattr(cfg, "enc_variant", 0))
    c.voc_dur_pred_hidden_dim = int(v.dur_pred_hidden_dim) if has_vocoder_dur_predictor else 0
    c.voc_dur_pred_kernel_size = int(v.dur_pred_kernel_size)
    c.t2u_variant = int(getattr(cfg, "t2u_variant", 0))
    return c
