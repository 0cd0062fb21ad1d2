"""Architecture configuration of the S2ST hot path.

Field values of :func:`seamless_m4t_v2_large` restate the reference configs
(citations are relative to /root/reference/src/seamless_communication):

* ``base_v2`` UnitY arch                 models/unity/builder.py:165-192
* conformer_shaw 600m speech encoder     models/conformer_shaw/builder.py:54-68
* ``base_nar`` T2U arch                  models/unity/t2u_builder.py:186-232
* vocoder ``base`` arch                  models/vocoder/builder.py:42-64

The S2ST path is speech in -> text -> units -> waveform; the NLLB text encoder
(``text_enc_*``) serves the text-input tasks (T2TT / T2ST) of the same API.
"""
from __future__ import annotations

from dataclasses import dataclass, field, asdict
from typing import Any, Dict, List, Optional, Tuple


@dataclass
class VocoderConfig:
    """Code-HiFi-GAN generator (models/vocoder/builder.py:44-63)."""

    upsample_rates: List[int] = field(default_factory=lambda: [5, 4, 4, 2, 2])
    upsample_kernel_sizes: List[int] = field(default_factory=lambda: [11, 8, 8, 4, 4])
    upsample_initial_channel: int = 512
    resblock_kernel_sizes: List[int] = field(default_factory=lambda: [3, 7, 11])
    resblock_dilation_sizes: List[List[int]] = field(
        default_factory=lambda: [[1, 3, 5], [1, 3, 5], [1, 3, 5]]
    )
    num_embeddings: int = 10000
    embedding_dim: int = 1280
    lang_embedding_dim: int = 256
    num_langs: int = 36
    spkr_embedding_dim: int = 256
    num_spkrs: int = 200
    # duration predictor on the unit embeddings (builder.py:53-58; used with dur_prediction=True, the v1 AR-T2U path)
    dur_pred_hidden_dim: int = 1280
    dur_pred_kernel_size: int = 3

    @property
    def model_in_dim(self) -> int:
        return self.embedding_dim + self.lang_embedding_dim + self.spkr_embedding_dim

    @property
    def hop(self) -> int:
        h = 1
        for r in self.upsample_rates:
            h *= r
        return h


@dataclass
class S2STConfig:
    """Everything the HIP runtime needs to lay the model out in HBM."""

    name: str = "seamlessM4T_v2_large"
    model_dim: int = 1024
    num_heads: int = 16  # head_dim must be 64 (kernels are specialised for it)

    # speech encoder: W2v-BERT 2.0 Conformer with Shaw rel-pos attention (enc_variant 0, the v2 model) or the v1 w2v-BERT
    # (enc_variant 1: Transformer-XL relative positions + BatchNorm conv module; models/unity/builder.py:109-162)
    enc_variant: int = 0
    num_fbank_channels: int = 80
    fbank_stride: int = 2
    enc_layers: int = 24
    enc_ffn_dim: int = 4096
    depthwise_conv_kernel_size: int = 31
    shaw_max_left: int = 64
    shaw_max_right: int = 8
    adaptor_kernel_size: int = 8
    adaptor_stride: int = 8
    adaptor_ffn_dim: int = 4096  # = w2v2 ffn_inner_dim (builder.py:508)
    adaptor_proj_dim: int = 4096  # model_dim * 4 (adaptor_block.py:79-87)

    # NLLB dense_1b text encoder (text-input tasks; builder.py:169-173 use_text_encoder=True)
    text_enc_layers: int = 24
    text_enc_ffn_dim: int = 8192

    # streaming monotonic text decoder `dense_1b` (models/monotonic_decoder/builder.py:81-99); a separate checkpoint
    mma_layers: int = 24
    mma_ffn_dim: int = 8192
    mma_energy_bias_value: float = -0.5
    mma_temperature: float = 0.2
    mma_energy_layers: int = 4
    mma_pre_decision_ratio: int = 2

    # NLLB dense_1b text decoder
    dec_layers: int = 24
    dec_ffn_dim: int = 8192
    text_vocab_size: int = 256102
    text_max_seq_len: int = 4096
    pad_idx: int = 0
    unk_idx: int = 1
    bos_idx: int = 2
    eos_idx: int = 3

    # UnitY2 NAR T2U (t2u_variant 0) or the v1 autoregressive UnitYT2UModel (t2u_variant 1: unit embedding frontend +
    # pre-LN decoder, beam search; models/unity/t2u_builder.py:140-183)
    t2u_variant: int = 0
    t2u_enc_layers: int = 6
    t2u_dec_layers: int = 6
    t2u_ffn_dim: int = 8192
    t2u_conv_kernel: int = 7
    t2u_conv_inner_dim: int = 1024
    unit_vocab_size: int = 10082
    unit_pad_idx: int = 1
    unit_eos_idx: int = 2
    unit_max_seq_len: int = 4096
    char_vocab_size: int = 10943
    char_max_seq_len: int = 4096
    var_pred_hidden_dim: int = 256
    var_pred_kernel_size: int = 3

    vocoder: VocoderConfig = field(default_factory=VocoderConfig)

    # SeamlessExpressive (unity arch `expressivity_v2`, T2U arch `expressivity_nar`; builder.py:195-224, t2u_builder.py:235-281).
    # ffn_activation: inner activation of the adaptor layer's FFN and the NLLB FFNs (use_gelu; "relu" or "gelu" = torch.nn.GELU(),
    # the erf form); t2u_ffn_activation: the same of the T2U encoder FFNs; film_cond_dim > 0: FiLM in the duration predictor and
    # every FFT decoder layer plus `t2u_model.prosody_proj`, all conditioned on the output of `prosody_encoder` (the model's own
    # ECAPA-TDNN, tensors `prosody_encoder_model.*`).  The defaults describe every other model.
    ffn_activation: str = "relu"
    t2u_ffn_activation: str = "relu"
    film_cond_dim: int = 0
    prosody_encoder: Optional["EcapaTDNNConfig"] = None

    @property
    def head_dim(self) -> int:
        return self.model_dim // self.num_heads

    @property
    def shaw_num_pos(self) -> int:
        return self.shaw_max_left + 1 + self.shaw_max_right

    def to_dict(self) -> dict:
        return asdict(self)


def seamless_m4t_v2_large() -> S2STConfig:
    return S2STConfig()


@dataclass
class AlignerConfig:
    """UnitY2 forced aligner (models/aligner/builder.py:64-87, the only architecture: ``nar_t2u_aligner``)."""

    name: str = "nar_t2u_aligner"
    model_dim: int = 1024
    feat_dim: int = 1024
    num_text_layers: int = 2
    num_feat_layers: int = 3
    temperature: float = 1.0
    reduction_factor: int = 1
    unit_vocab_size: int = 10082
    unit_pad_idx: int = 1
    char_vocab_size: int = 10943


@dataclass
class Wav2Vec2UnitConfig:
    """wav2vec 2.0 encoder of the UnitExtractor (models/unit_extractor/wav2vec2_layer_output.py:23-53, ``xlsr2_1b_v2``):
    pre-norm Transformer, convolutional position encoder, LayerNorm after every extractor convolution, no feature LayerNorm."""

    name: str = "xlsr2_1b_v2"
    model_dim: int = 1280
    num_heads: int = 16
    ffn_dim: int = 5120
    num_layers: int = 48
    feature_dim: int = 512
    layer_descs: Tuple[Tuple[int, int, int], ...] = ((512, 10, 5),) + ((512, 3, 2),) * 4 + ((512, 2, 2),) * 2
    pos_conv_kernel: int = 128
    pos_conv_groups: int = 16

    def num_frames(self, num_samples: int) -> int:
        """floor((L - k) / s) + 1 per extractor layer; 0 when the input is too short for one frame."""
        n = int(num_samples)
        for _, k, s in self.layer_descs:
            if n < k:
                return 0
            n = (n - k) // s + 1
        return n

    def min_samples(self) -> int:
        n = 1
        for _, k, s in reversed(self.layer_descs):
            n = (n - 1) * s + k
        return n


def xlsr2_1b_v2(num_layers: int = 48) -> Wav2Vec2UnitConfig:
    return Wav2Vec2UnitConfig(num_layers=num_layers)


def tiny_w2v2_config(head_dim: int = 80) -> Wav2Vec2UnitConfig:
    """A small encoder of the same structure for parity tests: 2 heads of 80 (the XLS-R head size) or 64, conv width 32."""
    return Wav2Vec2UnitConfig(name=f"tiny_w2v2_{head_dim}", model_dim=2 * head_dim, num_heads=2, ffn_dim=320 if head_dim == 80 else 256, num_layers=3,
                              feature_dim=32, layer_descs=((32, 10, 5),) + ((32, 3, 2),) * 4 + ((32, 2, 2),) * 2)


@dataclass
class EcapaTDNNConfig:
    """ECAPA-TDNN prosody encoder of SeamlessExpressive (models/pretssel/ecapa_tdnn_builder.py, arch ``base``): one TDNN block,
    ``len(channels) - 2`` SE-Res2Net blocks, multi-layer feature aggregation, attentive statistics pooling, a projection."""

    name: str = "base"
    channels: Tuple[int, ...] = (512, 512, 512, 512, 1536)
    kernel_sizes: Tuple[int, ...] = (5, 3, 3, 3, 1)
    dilations: Tuple[int, ...] = (1, 2, 3, 4, 1)
    attention_channels: int = 128
    res2net_scale: int = 8
    se_channels: int = 128
    global_context: bool = True
    groups: Tuple[int, ...] = (1, 1, 1, 1, 1)
    embed_dim: int = 512
    input_dim: int = 80


def ecapa_tdnn_config(arch: str = "base") -> EcapaTDNNConfig:
    """``base``: the reference's only architecture.  ``small``: the same structure at a quarter of the width (Res2Net chunks of
    32 channels) for parity tests."""
    if arch == "base":
        return EcapaTDNNConfig()
    if arch == "small":
        return EcapaTDNNConfig(name="small", channels=(128, 128, 128, 128, 384), attention_channels=32, res2net_scale=4, se_channels=32,
                               embed_dim=64)
    raise ValueError(f"unknown ECAPA-TDNN arch '{arch}' (supported: base, small)")


@dataclass
class PretsselWaveConfig:
    """Waveform generator of the PRETSSEL vocoder (models/generator/builder.py): the mel HiFi-GAN, and the SEANet-style encoder,
    two 2-layer LSTMs and decoder over its output.  The defaults are arch ``24khz``."""

    upsample_rates: List[int] = field(default_factory=lambda: [5, 4, 4, 3])
    upsample_kernel_sizes: List[int] = field(default_factory=lambda: [10, 8, 8, 6])
    upsample_initial_channel: int = 512
    resblock_kernel_sizes: List[int] = field(default_factory=lambda: [3, 7, 11])
    resblock_dilation_sizes: List[List[int]] = field(default_factory=lambda: [[1, 3, 5], [1, 3, 5], [1, 3, 5]])
    n_filters: int = 32
    ratios: List[int] = field(default_factory=lambda: [8, 5, 4, 2])
    dimension: int = 128
    kernel_size: int = 7
    residual_kernel_size: int = 3

    @property
    def hop(self) -> int:
        h = 1
        for r in self.upsample_rates:
            h *= r
        return h

    def layer_index(self, post_layers: int) -> Dict[str, Any]:
        """Where the pieces sit in ``PretsselVocoder.layers``: the 32 stream layers go in four chunks of 8 around conv_pre, the
        upsampling convolutions, the HiFi-GAN ResBlocks and conv_post."""
        p, u = post_layers, len(self.upsample_rates)
        chunk = [p, p + 9, p + 17 + u, p + 25 + 4 * u]
        return {"stream": [chunk[i // 8] + i % 8 for i in range(32)], "conv_pre": p + 8, "ups": [p + 17 + i for i in range(u)],
                "resblocks": [p + 25 + u + i for i in range(3 * u)], "conv_post": p + 33 + 4 * u}

    def lengths(self, frames: int) -> Tuple[int, int, int]:
        """(samples, LSTM steps, decoder samples) of an item of ``frames`` mel frames: every strided level rounds up, the decoder
        runs on the rounded-up length."""
        n = frames * self.hop
        steps = n
        for r in reversed(self.ratios):
            steps = -(-steps // r)
        dec = steps
        for r in self.ratios:
            dec *= r
        return n, steps, dec


@dataclass
class PretsselConfig:
    """Acoustic model of the PRETSSEL vocoder (models/generator/builder.py, archs ``16khz`` / ``24khz``: identical up to the mel
    spectrogram): unit embedding, FiLM-conditioned FFT encoder, variance adaptor with Gaussian upsampling, FFT decoder,
    projection to the mel bins and the Conv-BatchNorm-Tanh post-net."""

    name: str = "24khz"
    model_dim: int = 256
    num_heads: int = 2
    encoder_layers: int = 4
    decoder_layers: int = 4
    conv_inner_dim: int = 1024
    conv_kernel: int = 9
    film_cond_dim: int = 576
    lang_embed_dim: int = 64
    num_langs: int = 6
    pred_hidden_dim: int = 512
    pred_kernel: int = 5
    vocab_size: int = 10004
    pad_idx: int = 1
    eos_idx: int = 2
    max_seq_len: int = 10000
    mel_dim: int = 80
    post_layers: int = 5
    post_dim: int = 512
    post_kernel: int = 5
    upsample_delta: float = 0.1
    prosody_encoder: EcapaTDNNConfig = field(default_factory=EcapaTDNNConfig)
    waveform: PretsselWaveConfig = field(default_factory=PretsselWaveConfig)


def pretssel_config(arch: str = "24khz") -> PretsselConfig:
    """``16khz`` / ``24khz``: the reference's architectures (they differ in the waveform generator only; ``16khz`` ships without
    languages in its builder, the card supplies them).  ``small``: 1 + 1 layers at the same width and head size for parity tests."""
    if arch == "24khz":
        return PretsselConfig(name=arch)
    if arch == "16khz":
        return PretsselConfig(name=arch, waveform=PretsselWaveConfig(upsample_rates=[5, 4, 4, 2], upsample_kernel_sizes=[10, 8, 8, 4]))
    if arch == "small":
        # waveform half: one wide (128) and two narrow (64, 32) HiFi-GAN stages through the rates 5 and 3, a 128-wide LSTM
        return PretsselConfig(name="small", encoder_layers=1, decoder_layers=1, conv_inner_dim=256, pred_hidden_dim=128, post_dim=128, num_langs=2,
                              film_cond_dim=64 + 64, prosody_encoder=ecapa_tdnn_config("small"),
                              waveform=PretsselWaveConfig(upsample_rates=[5, 3, 2], upsample_kernel_sizes=[10, 6, 4], upsample_initial_channel=256, n_filters=8,
                                                          dimension=32))
    raise ValueError(f"unknown PRETSSEL arch '{arch}' (supported: 16khz, 24khz, small)")


def nar_t2u_aligner() -> AlignerConfig:
    return AlignerConfig()


def tiny_aligner_config(reduction_factor: int = 1) -> AlignerConfig:
    """A small aligner of the same structure for parity tests: the vocabularies of tiny_config()."""
    return AlignerConfig(name="tiny_aligner", model_dim=64, feat_dim=64, reduction_factor=reduction_factor, unit_vocab_size=340,
                         char_vocab_size=96)


def seamless_m4t_large() -> S2STConfig:
    """seamlessM4T_large (v1), unity arch `base` (models/unity/builder.py:109-134): w2v-BERT 600m with relative positions,
    NLLB dense_1b, vocabulary 256102.  The speech encoder, text encoder / decoder run on this path; the v1 autoregressive T2U
    (beam search over units) and the vocoder's duration predictor complete the v1 chain."""
    return S2STConfig(name="seamlessM4T_large", enc_variant=1, text_max_seq_len=1024, t2u_variant=1, unit_max_seq_len=2048)


def seamless_m4t_medium() -> S2STConfig:
    """seamlessM4T_medium (v1), unity arch `medium` (models/unity/builder.py:137-162): w2v-BERT 300m (12 layers), NLLB
    dense_600m (12 + 12 layers, FFN 4096), NLLB-200 vocabulary 256206.  BASELINE configs[0] (T2TT plumbing) names it."""
    return S2STConfig(name="seamlessM4T_medium", enc_variant=1, enc_layers=12, text_enc_layers=12, text_enc_ffn_dim=4096,
                      dec_layers=12, dec_ffn_dim=4096, text_vocab_size=256206, text_max_seq_len=1024, t2u_variant=1,
                      t2u_enc_layers=4, t2u_dec_layers=4, unit_max_seq_len=2048)


def seamless_expressivity() -> S2STConfig:
    """seamless_expressivity, unity arch `expressivity_v2` (models/unity/builder.py:195-224) over the T2U arch `expressivity_nar`
    (t2u_builder.py:235-281): GELU feed-forward networks, no NLLB text encoder, 4 + 4 T2U layers over 10005 units and 10904
    characters, sequences up to 10000, FiLM conditioning on the 512-wide output of its own ECAPA-TDNN (arch `base`)."""
    return S2STConfig(name="seamless_expressivity", text_enc_layers=0, mma_layers=0, text_max_seq_len=10000, t2u_enc_layers=4, t2u_dec_layers=4,
                      unit_vocab_size=10005, unit_max_seq_len=10000, char_vocab_size=10904, char_max_seq_len=10000,
                      ffn_activation="gelu", t2u_ffn_activation="gelu", film_cond_dim=512, prosody_encoder=ecapa_tdnn_config("base"))


def tiny_expressive_config() -> S2STConfig:
    """tiny_config() with what the expressive model changes (parity tests): GELU, FiLM on a 64-wide conditioning vector from the
    `small` ECAPA-TDNN, no text encoder, no monotonic decoder."""
    c = tiny_config()
    c.name = "tiny_expressive"
    c.text_enc_layers = 0
    c.mma_layers = 0
    c.ffn_activation = "gelu"
    c.t2u_ffn_activation = "gelu"
    c.film_cond_dim = 64
    c.prosody_encoder = ecapa_tdnn_config("small")
    return c


def tiny_v1_config() -> S2STConfig:
    """tiny_config() with the v1 speech encoder (parity tests of row f5)."""
    c = tiny_config()
    c.name = "tiny_v1"
    c.enc_variant = 1
    c.t2u_variant = 1
    return c


def tiny_config() -> S2STConfig:
    """A structurally identical, small model for parity tests and golden
    fixtures (the oracle finishes it in well under a second on CPU)."""
    return S2STConfig(
        name="tiny_v2",
        model_dim=128,
        num_heads=2,
        enc_layers=2,
        enc_ffn_dim=256,
        depthwise_conv_kernel_size=31,
        adaptor_ffn_dim=256,
        adaptor_proj_dim=512,
        text_enc_layers=2,
        text_enc_ffn_dim=256,
        mma_layers=2,
        mma_ffn_dim=256,
        mma_energy_layers=2,
        dec_layers=2,
        dec_ffn_dim=256,
        text_vocab_size=1200,
        text_max_seq_len=256,
        t2u_enc_layers=2,
        t2u_dec_layers=2,
        t2u_ffn_dim=256,
        t2u_conv_kernel=7,
        t2u_conv_inner_dim=128,
        unit_vocab_size=340,
        unit_max_seq_len=1024,
        char_vocab_size=96,
        char_max_seq_len=1024,
        var_pred_hidden_dim=64,
        var_pred_kernel_size=3,
        vocoder=VocoderConfig(
            upsample_rates=[5, 4, 4, 2, 2],
            upsample_kernel_sizes=[11, 8, 8, 4, 4],
            upsample_initial_channel=128,
            num_embeddings=300,
            embedding_dim=48,
            lang_embedding_dim=8,
            num_langs=36,
            spkr_embedding_dim=8,
            num_spkrs=200,
            dur_pred_hidden_dim=64,
        ),
    )
