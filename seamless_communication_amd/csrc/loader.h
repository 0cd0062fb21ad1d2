// The weight loader of every load entry (definitions in model_load.hip): the caller's tensors by name (m.raw, uploaded by
// upload_tensors into memory the handle owns), handed out in the precision the kernels read or repacked for them.
//
// Retention: f16 / f32 hand an upload out as it is when its precision matches and remember that they did; everything else they
// return is a copy the handle owns.  A load that is done with its uploads calls release_unused(), which frees the uploads that
// were never handed out - a pointer that left the loader is never freed.  A load that fails half-way needs no clean-up of its
// own: uploads and copies alike sit in m.owned, which ~Model frees.
#pragma once
#include <initializer_list>
#include <string>
#include <unordered_set>

#include "model.h"

namespace sc {

struct Loader {
    using Shape = std::initializer_list<int64_t>;
    Model& m;
    const char* who;  // the calling entry ("sc_aligner_load"): every message starts with it
    std::unordered_set<const void*> handed_out;
    // uploads the caller's tensors (upload_tensors)
    Loader(Model& mm, const char* entry, const sc_tensor_desc* t, size_t n);

    void* dalloc(size_t bytes);  // device memory the handle owns
    bool has(const std::string& k) const { return m.raw.count(k) != 0; }
    const Model::Raw& get(const std::string& k) const;
    const Model::Raw& get(const std::string& k, Shape shape) const;
    // keep = false: the pointer only feeds a repacking launch of the loader itself, so the upload behind it may be released
    const __half* f16(const std::string& k, Shape shape, bool keep = true);
    const float* f32(const std::string& k, Shape shape, bool keep = true);
    // the same values copied or converted into memory the caller allocated (fused and stacked weights)
    void f16_into(const std::string& k, Shape shape, __half* dst);
    void f32_into(const std::string& k, Shape shape, float* dst);
    float scalar(const std::string& k);
    LNorm ln(const std::string& p, int dim);
    Linear lin(const std::string& p, int out, int in, bool bias = true);
    Linear lin_pw(const std::string& p, int out, int in);  // pointwise Conv1d stored as (out, in, 1)
    // several (out_each, in) projections as one [sum out_i][in] weight
    Linear fuse(const std::vector<std::string>& ps, int out_each, int in);
    // Conv1d weight `name` [cout][cin][k] -> tap-major rows [cout][kpad] at dst; input channels cin .. cin_pad-1 are zeros
    void pack_conv(const std::string& name, int cout, int cin, int k, int cin_pad, int kpad, __half* dst);
    // cin_pad > cin: a convolution over cin_pad input channels whose last ones meet zero weights
    Conv conv(const std::string& p, int cout, int cin, int k, bool bias = true, int cin_pad = 0);
    Conv conv_wn(const std::string& p, int cout, int cin, int k);                  // weight-normed Conv1d
    ConvT convT_wn(const std::string& p, int cin, int cout, int k, int stride);  // weight-normed ConvTranspose1d
    // second copy of a decoder-step weight in MFMA fragment order (k_dstep.hip)
    const __half* packed(const __half* w, int64_t ldw, int out, int in);
    void pack_decoder_layer(DecoderLayer& l);
    // synchronises the stream, frees every upload that was never handed out and forgets the names
    void release_unused();
};

// the caller's tensors into memory the handle owns, by name (m.raw); tied tensors share storage
void upload_tensors(Model& m, const char* who, const sc_tensor_desc* t, size_t n);
struct HifiganNames {
    std::string pre, post;
    std::vector<std::string> ups, res;
};
// The HiFi-GAN stack of a handle whose tensors carry other names (the PRETSSEL waveform generator: layers.N): geometry from
// m.cfg's voc_* fields, conv_pre over `in_dim` input channels.  res holds num_upsamples * num_resblock_kernels names.
void load_hifigan_stack(Loader& L, const HifiganNames& nm, int in_dim);

}  // namespace sc
