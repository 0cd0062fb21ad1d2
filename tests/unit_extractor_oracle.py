"""Float64 restatement of the UnitExtractor's arithmetic (wav2vec 2.0 pre-norm encoder with per-layer extractor LayerNorm,
convolutional position encoder, k-means arg-min) in plain torch, parameterised by a fairseq2-keyed state dict.  ``dtype``
float32 gives the fp32-CPU evaluation the GPU tests scale their bars by."""
import torch
import torch.nn.functional as F


def _p(sd, k, dtype):
    return sd[k].to(dtype)


def normalise(wave, dtype=torch.float64):
    """unit_extractor.py:91-94: pad to an even length with 1.0, then layer_norm over the whole utterance."""
    w = wave.to(dtype).reshape(-1)
    if w.numel() % 2:
        w = torch.cat([w, torch.ones(1, dtype=dtype)])
    return F.layer_norm(w, w.shape)


def pos_weight(sd, dtype=torch.float64):
    pre = "encoder_frontend.pos_encoder.conv."
    if pre + "weight" in sd:
        return sd[pre + "weight"].to(dtype)
    v, g = sd[pre + "weight_v"].to(torch.float64), sd[pre + "weight_g"].to(torch.float64).reshape(1, 1, -1)
    return (g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()).to(dtype)


def pos_conv(x, w, b, groups):
    """x [T, C] -> x + GELU(conv(x)) with padding k // 2 and the last step dropped (k even)."""
    k = w.shape[-1]
    y = F.conv1d(x.t().unsqueeze(0), w, b, padding=k // 2, groups=groups)[0, :, : x.shape[0]].t()
    return x + F.gelu(y)


def attention(q, k, v, heads, kv_len=None):
    """q [Sq, M], k / v [Skv, M] -> [Sq, M]; keys behind kv_len are masked; scale head_dim ** -0.5."""
    Sq, M = q.shape
    hd = M // heads
    kv_len = k.shape[0] if kv_len is None else kv_len
    qh = q.reshape(Sq, heads, hd).transpose(0, 1)
    kh = k[:kv_len].reshape(kv_len, heads, hd).transpose(0, 1)
    vh = v[:kv_len].reshape(kv_len, heads, hd).transpose(0, 1)
    p = torch.softmax(qh @ kh.transpose(1, 2) * hd ** -0.5, dim=-1)
    return (p @ vh).transpose(0, 1).reshape(Sq, M)


def forward(cfg, sd, wave, out_layer_idx, dtype=torch.float64, stages=None):
    """One item: the raw output of layer out_layer_idx, [frames, model_dim].  ``stages`` (a dict) receives the intermediates."""
    n_frames = cfg.num_frames(int(wave.numel()))
    x = normalise(wave, dtype).reshape(1, 1, -1)
    if stages is not None:
        stages["wave"] = x.reshape(-1)
    for i, (_, k, s) in enumerate(cfg.layer_descs):
        p = f"encoder_frontend.feature_extractor.layers.{i}."
        x = F.conv1d(x, _p(sd, p + "conv.weight", dtype), _p(sd, p + "conv.bias", dtype), stride=s)
        x = F.layer_norm(x.transpose(1, 2), (x.shape[1],), _p(sd, p + "layer_norm.weight", dtype), _p(sd, p + "layer_norm.bias", dtype)).transpose(1, 2)
        x = F.gelu(x)
        if stages is not None:
            stages[f"fe{i}"] = x[0].t()
    x = x[0].t()[:n_frames]  # the frame the pad sample may add is masked
    x = F.layer_norm(x, (x.shape[1],), _p(sd, "encoder_frontend.post_extract_layer_norm.weight", dtype),
                     _p(sd, "encoder_frontend.post_extract_layer_norm.bias", dtype))
    x = F.linear(x, _p(sd, "encoder_frontend.model_dim_proj.weight", dtype), _p(sd, "encoder_frontend.model_dim_proj.bias", dtype))
    if stages is not None:
        stages["proj"] = x
    x = pos_conv(x, pos_weight(sd, dtype), _p(sd, "encoder_frontend.pos_encoder.conv.bias", dtype), cfg.pos_conv_groups)
    if stages is not None:
        stages["pos"] = x
    M = cfg.model_dim
    for i in range(out_layer_idx + 1):
        p = f"encoder.layers.{i}."
        h = F.layer_norm(x, (M,), _p(sd, p + "self_attn_layer_norm.weight", dtype), _p(sd, p + "self_attn_layer_norm.bias", dtype))
        q, k, v = (F.linear(h, _p(sd, p + f"self_attn.{n}_proj.weight", dtype), _p(sd, p + f"self_attn.{n}_proj.bias", dtype)) for n in "qkv")
        a = attention(q, k, v, cfg.num_heads)
        x = x + F.linear(a, _p(sd, p + "self_attn.output_proj.weight", dtype), _p(sd, p + "self_attn.output_proj.bias", dtype))
        h = F.layer_norm(x, (M,), _p(sd, p + "ffn_layer_norm.weight", dtype), _p(sd, p + "ffn_layer_norm.bias", dtype))
        h = F.gelu(F.linear(h, _p(sd, p + "ffn.inner_proj.weight", dtype), _p(sd, p + "ffn.inner_proj.bias", dtype)))
        x = x + F.linear(h, _p(sd, p + "ffn.output_proj.weight", dtype), _p(sd, p + "ffn.output_proj.bias", dtype))
        if stages is not None:
            stages[f"layer{i}"] = x
    return x


def kmeans_dist(x, centroids):
    """kmeans.py:24-30 with centroids [C, K]."""
    return x.pow(2).sum(1, keepdim=True) - 2 * torch.matmul(x, centroids) + (centroids ** 2).sum(0, keepdim=True)


def kmeans(x, centroids):
    return kmeans_dist(x, centroids).argmin(dim=-1)
