// UnitY2 forced aligner: a handle of its own (separate checkpoint, vocabularies, stream and scratch pool) and its C entries.
//
// Reference call sites (src/seamless_communication/models/aligner/...):
//   builder.py:64-87     the nar_t2u_aligner_base architecture
//   model.py:25-71       UnitY2AlignmentFrontend (two embedding tables)
//   model.py:79-190      UnitY2AlignmentEncoder: conv stacks, distance, masked log-softmax
//   model.py:212-277     _monotonic_alignment_search / viterbi_decode
//   loader.py:22-57      names of the converted checkpoint
#include <algorithm>
#include <cmath>
#include <string>

#include "handle.h"
#include "loader.h"

using namespace sc;

// The stage helpers (conv1d) take a Model for its stream, scratch pool and list of owned allocations; the aligner embeds one and
// uses nothing else of it (its other members stay empty; ~Model copes with that).
struct sc_aligner {
    Model m;
    sc_aligner_config cfg{};
    const __half* embed_text = nullptr;  // [char_vocab][model_dim]
    const __half* embed_unit = nullptr;  // [unit_vocab][feat_dim]
    std::vector<Conv> t_conv, f_conv;    // k = 3 (+ ReLU) ..., the last one k = 1
};

namespace {

void load_aligner(sc_aligner& a, const sc_tensor_desc* t, size_t n) {
    const sc_aligner_config& c = a.cfg;
    SC_CHECK(c.model_dim > 0 && c.model_dim % 32 == 0 && c.feat_dim > 0 && c.feat_dim % 32 == 0,
             "sc_aligner_load: model_dim=%d / feat_dim=%d must be positive multiples of 32", c.model_dim, c.feat_dim);
    SC_CHECK(c.text_layers >= 1 && c.feat_layers >= 1 && c.text_layers <= 16 && c.feat_layers <= 16, "sc_aligner_load: bad layer counts");
    SC_CHECK(c.reduction_factor >= 1 && c.char_vocab_size > 0 && c.unit_vocab_size > 0, "sc_aligner_load: bad configuration");
    Loader L(a.m, "sc_aligner_load", t, n);
    a.embed_text = L.f16("alignment_frontend.embed_text.weight", {c.char_vocab_size, c.model_dim});
    a.embed_unit = L.f16("alignment_frontend.embed_unit.weight", {c.unit_vocab_size, c.feat_dim});
    // the Conv1d modules sit at positions 1, 4, 7, ... of the nn.Sequential (Permute12, then Conv1d / ReLU / Dropout per layer)
    for (int i = 0; i < c.text_layers; ++i)
        a.t_conv.push_back(L.conv("alignment_encoder.t_conv." + std::to_string(1 + 3 * i), c.model_dim, c.model_dim, i < c.text_layers - 1 ? 3 : 1));
    for (int i = 0; i < c.feat_layers; ++i)
        a.f_conv.push_back(L.conv("alignment_encoder.f_conv." + std::to_string(1 + 3 * i), c.model_dim, i == 0 ? c.feat_dim : c.model_dim,
                                  i < c.feat_layers - 1 ? 3 : 1));
    L.release_unused();
}

void check_lens(const char* who, const int32_t* lens, int n, int cap, const char* what, int* longest) {
    *longest = 0;
    for (int b = 0; b < n; ++b) {
        SC_CHECK(lens[b] >= 1 && lens[b] <= cap, "%s: %s[%d]=%d outside 1..%d", who, what, b, lens[b], cap);
        *longest = std::max(*longest, lens[b]);
    }
}

// One stack of model.py:99-144 on [n][S][cin] rows: every convolution sees zeros behind an item's own length (what the item
// sees as a batch of one), ReLU after all but the last, the last one with `last_stride`.  Returns the buffer of the result.
Buf<float> conv_stack(Model& m, const std::vector<Conv>& convs, Buf<float> x, int n, int S, const int* d_lens, int last_stride) {
    for (size_t i = 0; i < convs.size(); ++i) {
        const bool last = i + 1 == convs.size();
        const int stride = last ? last_stride : 1;
        const int t_out = (S - 1) / stride + 1;
        Buf<float> y(m.pp(), (size_t)n * t_out * convs[i].cout);
        conv1d(m, x, convs[i], nullptr, y, n, S, stride, convs[i].k / 2, 1, d_lens, IN_NONE, last ? ACT_NONE : ACT_RELU);
        x = std::move(y);
    }
    return x;
}

void run_align(sc_aligner& a, const int32_t* h_text_ids, int n, int St, const int32_t* h_text_lens, const int32_t* h_unit_ids, int Su,
               const int32_t* h_unit_lens, int32_t* h_durations, float* d_lprob) {
    Model& m = a.m;
    const sc_aligner_config& c = a.cfg;
    SC_CHECK(n > 0 && St > 0 && Su > 0, "sc_align: empty batch (n=%d s_text=%d s_unit=%d)", n, St, Su);
    int max_t = 0, max_u = 0;
    check_lens("sc_align", h_text_lens, n, St, "text_lens", &max_t);
    check_lens("sc_align", h_unit_lens, n, Su, "unit_lens", &max_u);
    const int rf = c.reduction_factor, Sf = (Su - 1) / rf + 1, max_f = (max_u - 1) / rf + 1;
    SC_CHECK(max_t <= mas_max_text(), "sc_align: %d characters exceed the limit of %d per item", max_t, mas_max_text());
    SC_CHECK(max_f <= mas_max_feat(), "sc_align: %d frames exceed the limit of %d per item", max_f, mas_max_feat());
    SC_CHECK((int64_t)n * St * c.model_dim < (1ll << 31) && (int64_t)n * Su * std::max(c.model_dim, c.feat_dim) < (1ll << 31),
             "sc_align: batch too large (n=%d s_text=%d s_unit=%d)", n, St, Su);
    for (int64_t i = 0; i < (int64_t)n * St; ++i)
        SC_CHECK(h_text_ids[i] >= 0 && h_text_ids[i] < c.char_vocab_size, "sc_align: character id %d outside the vocabulary of %d", h_text_ids[i],
                 c.char_vocab_size);
    for (int64_t i = 0; i < (int64_t)n * Su; ++i)
        SC_CHECK(h_unit_ids[i] >= 0 && h_unit_ids[i] < c.unit_vocab_size, "sc_align: unit id %d outside the vocabulary of %d", h_unit_ids[i],
                 c.unit_vocab_size);
    prof::set_tag("align");
    std::vector<int32_t> flens(n);
    for (int b = 0; b < n; ++b) flens[b] = (h_unit_lens[b] - 1) / rf + 1;  // ceil(len / reduction_factor), model.py:167-168
    Buf<int> d_tid(m.pp(), (size_t)n * St), d_uid(m.pp(), (size_t)n * Su), d_tlens(m.pp(), n), d_ulens(m.pp(), n), d_flens(m.pp(), n);
    SC_HIP(hipMemcpyAsync(d_tid.get(), h_text_ids, (size_t)n * St * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipMemcpyAsync(d_uid.get(), h_unit_ids, (size_t)n * Su * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipMemcpyAsync(d_tlens.get(), h_text_lens, (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipMemcpyAsync(d_ulens.get(), h_unit_lens, (size_t)n * 4, hipMemcpyHostToDevice, m.stream));
    SC_HIP(hipMemcpyAsync(d_flens.get(), flens.data(), (size_t)n * 4, hipMemcpyHostToDevice, m.stream));

    Buf<float> te(m.pp(), (size_t)n * St * c.model_dim), fe(m.pp(), (size_t)n * Su * c.feat_dim);
    launch_align_embed(d_tid, n * St, a.embed_text, c.model_dim, te, m.stream);
    launch_align_embed(d_uid, n * Su, a.embed_unit, c.feat_dim, fe, m.stream);
    Buf<float> ts = conv_stack(m, a.t_conv, std::move(te), n, St, d_tlens, 1);
    Buf<float> fs = conv_stack(m, a.f_conv, std::move(fe), n, Su, d_ulens, rf);

    Buf<float> own;
    if (!d_lprob) {
        own = Buf<float>(m.pp(), (size_t)n * Sf * St);
        d_lprob = own.get();
    }
    launch_align_lprob(ts, fs, n, St, Sf, c.model_dim, d_tlens, d_flens, c.temperature, d_lprob, m.stream);
    Buf<unsigned long long> bits(m.pp(), (size_t)n * mas_bits_words(max_t, Sf));
    Buf<int> d_dur(m.pp(), (size_t)n * St);
    launch_mas(d_lprob, n, St, Sf, d_tlens, d_flens, max_t, max_f, bits, d_dur, m.stream);
    SC_HIP(hipMemcpyAsync(h_durations, d_dur.get(), (size_t)n * St * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipStreamSynchronize(m.stream));  // the host arrays are the caller's; outputs complete on return
}

}  // namespace

extern "C" {

sc_aligner* sc_aligner_load(const sc_tensor_desc* tensors, size_t n_tensors, const sc_aligner_config* cfg, int device) {
    return open_handle<sc_aligner>("sc_aligner_load", tensors, n_tensors, cfg, device, load_aligner);
}

void sc_aligner_free(sc_aligner* a) { free_handle(a); }

int sc_align(sc_aligner* a, const int32_t* h_text_ids, int32_t n, int32_t s_text, const int32_t* h_text_lens, const int32_t* h_unit_ids,
             int32_t s_unit, const int32_t* h_unit_lens, int32_t* h_durations, float* d_lprob_or_null) {
    SC_API_BEGIN
    SC_CHECK(a && h_text_ids && h_text_lens && h_unit_ids && h_unit_lens && h_durations, "sc_align: null argument");
    SC_HIP(hipSetDevice(a->m.device));
    run_align(*a, h_text_ids, n, s_text, h_text_lens, h_unit_ids, s_unit, h_unit_lens, h_durations, d_lprob_or_null);
    SC_API_END
}

int sc_op_align_lprob(const float* d_text, const float* d_feat, int32_t n, int32_t s_text, int32_t s_feat, int32_t C,
                      const int32_t* h_text_lens, const int32_t* h_feat_lens, float temperature, float* d_lprob) {
    SC_API_BEGIN
    SC_CHECK(d_text && d_feat && h_text_lens && h_feat_lens && d_lprob, "sc_op_align_lprob: null argument");
    SC_CHECK(n > 0 && s_text > 0 && s_feat > 0, "sc_op_align_lprob: empty batch");
    int mt = 0, mf = 0;
    check_lens("sc_op_align_lprob", h_text_lens, n, s_text, "text_lens", &mt);
    check_lens("sc_op_align_lprob", h_feat_lens, n, s_feat, "feat_lens", &mf);
    OpScratch sc_;
    const int* d_t = sc_.put(std::vector<int>(h_text_lens, h_text_lens + n));
    const int* d_f = sc_.put(std::vector<int>(h_feat_lens, h_feat_lens + n));
    launch_align_lprob(d_text, d_feat, n, s_text, s_feat, C, d_t, d_f, temperature, d_lprob, nullptr);
    SC_HIP(hipStreamSynchronize(nullptr));
    SC_API_END
}

int sc_op_mas(const float* d_lprob, int32_t n, int32_t s_text, int32_t s_feat, const int32_t* h_text_lens, const int32_t* h_feat_lens,
              int32_t* h_durations) {
    SC_API_BEGIN
    SC_CHECK(d_lprob && h_text_lens && h_feat_lens && h_durations, "sc_op_mas: null argument");
    SC_CHECK(n > 0 && s_text > 0 && s_feat > 0 && (int64_t)s_text * s_feat < (1ll << 31), "sc_op_mas: bad geometry");
    int mt = 0, mf = 0;
    check_lens("sc_op_mas", h_text_lens, n, s_text, "text_lens", &mt);
    check_lens("sc_op_mas", h_feat_lens, n, s_feat, "feat_lens", &mf);
    SC_CHECK(mt <= mas_max_text(), "sc_op_mas: %d text positions exceed the limit of %d per item", mt, mas_max_text());
    SC_CHECK(mf <= mas_max_feat(), "sc_op_mas: %d frames exceed the limit of %d per item", mf, mas_max_feat());
    OpScratch sc_;
    const int* d_t = sc_.put(std::vector<int>(h_text_lens, h_text_lens + n));
    const int* d_f = sc_.put(std::vector<int>(h_feat_lens, h_feat_lens + n));
    unsigned long long* bits = sc_.get<unsigned long long>((size_t)n * mas_bits_words(mt, s_feat));
    int* dur = sc_.get<int>((size_t)n * s_text);
    launch_mas(d_lprob, n, s_text, s_feat, d_t, d_f, mt, mf, bits, dur, nullptr);
    SC_HIP(hipMemcpy(h_durations, dur, (size_t)n * s_text * 4, hipMemcpyDeviceToHost));
    SC_API_END
}

}  // extern "C"
