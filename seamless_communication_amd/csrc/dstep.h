// Decoder-step context, scratch and graph replay shared by every loop that drives the step chain (model_dstep.hip:
// decoder_step and its three kernel families): greedy generation, beam search and the
// streaming monotonic decoder (model_decoder.hip), sampled generation (model_sample.hip) and the decode engine (engine.hip).
#pragma once
#include <mutex>

#include "model.h"

namespace sc {

struct PoolStep {  // what a step of the streaming session pool adds to the slot-mode chain (StepCtx::pool)
    bool capture = false;       // the call's last step: keep the p_choose hook's inputs
    float* hq = nullptr;        // [layers][slots][M]
    const int* feat_row = nullptr;  // [slots] row of `features` slot b's decoder output goes to
    float* features = nullptr;  // the caller's packed [sum n_tokens][M]
};

struct StepCtx {
    int nb = 0, cap = 0, s_enc = 0;
    int* d_pos = nullptr;
    int* d_tok = nullptr;
    int* d_hist = nullptr;
    int* d_finished = nullptr;
    int* d_out_len = nullptr;
    int* d_enc_lens = nullptr;
    // greedy generation with per-row prompts (sc_generate_text_prompts): [nb] prompt lengths, read by the step's closing
    // launch; it lives in the session's own int block (a replayed step graph holds this pointer) and is written per call
    int* d_prompt_len = nullptr;
    float* d_lprob = nullptr;
    float* d_score = nullptr;
    float *x = nullptr, *h = nullptr, *wide = nullptr, *att = nullptr, *hN = nullptr, *logits = nullptr;
    std::vector<float*> kcache, vcache;  // per layer [nb][cap][M]
    std::vector<float*> cross_kv;        // per layer [nb*s_enc][2M]
    float* dec_hidden = nullptr;         // [nb][cap-1][M] or null
    float* partial = nullptr;            // split-K partial sums [splits][nb][<=3M]
    float4* am_part = nullptr;           // fused arg-max records [tiles][nb]
    int am_tiles = 0;
    float* am_eos_logit = nullptr;       // [nb]
    int min_seq_len = 1, force_eos_step = -1;
    float unk_penalty = 0.f;
    // which decoder stack runs (null = the UnitY text decoder) and the monotonic p_choose hook
    const DecStack* stack = nullptr;
    bool pchoose = false;           // compute p_choose[layer][head] of this step's (single) row
    const float* d_kenergy = nullptr;  // [layers][M]: k_energy_proj of the last pooled encoder position
    float* d_pchoose = nullptr;        // [layers][heads]
    float* qe0 = nullptr;              // [layers][M] scratch x2 for the query energy MLPs
    float* qe1 = nullptr;
    float* d_hq = nullptr;             // [layers][M]: every layer's normed cross-attention input of the p_choose step
    // second-generation step (k_dstep.hip): activations between the launches as split fp16 planes [K/8][rb][8]
    int rb = 0;  // row slots of the planes (32 or 64); 0 = first-generation step
    int am_ntl = 4;  // 32-feature tiles per workgroup of the fused vocabulary projection
    __half *hH = nullptr, *hL = nullptr;      // LayerNorm output       [M/8][rb][8]
    __half *attH = nullptr, *attL = nullptr;  // attention output       [M/8][rb][8]
    __half *wideH = nullptr, *wideL = nullptr;  // FFN inner activation [ffn/8][rb][8]
    Buf<__half> planes;                       // backing store of the six planes
    // third-generation step (k_dstep3.hip): fp32 residual stream in k-group-major order, complete q / k / v rows
    bool gen3 = false;
    float* xg = nullptr;    // [M/8][rb][8]
    float* qkvr = nullptr;  // [nb][M]: the cross-attention query rows
    int rg_small = 16, rg_ffn = 32;  // rows per row group of the N = M products / FFN-in (tuning knobs, SC_D3_*)
    int ffn_in_mode = 1;   // 0: partials + reduce/LN launch + packed product; 1 / 2: LayerNorm inside the product (2 tiles / 1 tile)
    int ffn_out_mode = 1;  // 0: gemvp, 8 K ranges; 1: gemv3 2 tiles x 512-wide K slices; 2: gemv3 1 tile x 1024-wide
    int cross_row_div = 1;  // beam search: live row r reads the encoder K / V of cache row r / cross_row_div (one per utterance)
    const int* anc = nullptr;  // beam search on the packed step kernels: K/V ancestor table [nb][cap] (DAttnArgs::anc)
    // beam search, row-group chain: live rows packed to the front, *d_rows of them; slot u holds utterance kv_item[u]
    const int* d_rows = nullptr;
    int* d_rows_greedy = nullptr;  // greedy generation: the same counter, written by the live-row compaction (run_generate_text)
    const int* kv_item = nullptr;
    float* qkv3 = nullptr;  // [nb][3M] complete q | k | v rows: the wide step (> 64 live rows) projects them on gemv3
    // decode engine (engine.hip): slot s of the step works on ROW STATE slot_rp[s].x at position slot_rp[s].y.  d_tok / d_hist /
    // d_finished / d_out_len / d_enc_lens / d_score, the encoder K / V and dec_hidden are then indexed by row
    // state, every row has its own position (pos_row), length limit and prompt length, and the closing launch of the step
    // (engine_finalize_kernel) advances the positions itself.  null: slot = row, one scalar position (*d_pos).
    int2* slot_rp = nullptr;
    int* slot_lane = nullptr;  // self K / V cache row of slot s (the caches are [slots][cap][M]: see DAttnArgs::slot_lane)
    int* pos_row = nullptr;
    int* limit_row = nullptr;
    int* prefix_row = nullptr;
    // streaming session pool (mma_pool.hip): a slot-mode step without generation rules.  The step is never projected; its
    // closing launch (launch_pool_close) takes engine_finalize_kernel's place, and a step with `capture` keeps every layer's
    // normed cross-attention input of the live slots for the row-batched p_choose hook.  null: not a pool step.
    const PoolStep* pool = nullptr;
};

// the pool's closing launch: slot b < *d_rows copies its decoder output hN[b] into row feat_row[b] of the caller's packed
// feature matrix and advances pos_row of its row state (nothing else: no EOS rule, no score)
void launch_pool_close(const float* hN, const int2* slot_rp, const int* d_rows, int* pos_row, const int* feat_row, float* features,
                       int slots, int M, hipStream_t s);
// out[b] = LayerNorm(x[b]) of the k-group-major residual stream as fp32 rows [slots][M], live slots only (ln3_kernel's arithmetic)
void launch_pool_capture_ln(const float* xg, int XRB, const float* gamma, const float* beta, float* out, int slots, int M,
                            const int* d_rows, hipStream_t s);

// ---- the step chain (model_dstep.hip) ---------------------------------------------------------------------------------
DecStack unity_stack(const Model& m);
DecStack t2u_ar_stack(const Model& m);
DecStack mma_stack(const Model& m);
bool step2_eligible(const Model& m, const DecStack& W, int nb);
bool step3_eligible(const Model& m, const DecStack& W, int nb);
bool step3_wide_eligible(const Model& m, const DecStack& W, int nb);
int choose_family(const Model& m, const DecStack& W, int rows, int caller);
// the greedy step projects with the arg-max in the product's epilogue (no logits in HBM) at this many rows and model width
inline bool fused_argmax_rows(int rows, int M) { return rows <= 64 && M % 64 == 0; }
// the step rules of a fused vocabulary projection of this context and decoder stack
ArgmaxEpi step_argmax_epi(const StepCtx& c, const DecStack& W);
// One decoder step for all batch rows: feeds d_tok at position *d_pos (engine: every slot at its row's position)
void decoder_step(Model& m, StepCtx& c, bool project);
// the six planes of a context of c.nb rows (sets c.rb, owns them in c.planes) / the same layout over an existing allocation
void alloc_step2(Model& m, StepCtx& c, int ffn_dim);
void alloc_step2_views(Model& m, StepCtx& c, int ffn_dim, __half* base);
// monotonic decoder: EnergyProjection, (Linear, ReLU) x n on `rows` rows (returns the buffer holding the result), and one
// level of it for every layer in one launch (energy_level_kernel: Wt / Bt are one level's pointer tables)
float* energy_mlp(Model& m, const std::vector<Linear>& layers, const float* in, int64_t ld_in, float* a, float* b, int rows);
void launch_energy_level(Model& m, const __half* const* Wt, const float* const* Bt, int layers, const float* in, int64_t in_ls, float* out);

// Row-group tuning of the third-generation chain (StepCtx::rg_small / rg_ffn / ffn_in_mode / ffn_out_mode).  Which caller
// honours which knob is kept as found:
//   greedy generation and beam search read SC_D3_* (from_knobs);
//   sampled generation: not honoured; kept as found (defaults);
//   the decode engine: not honoured; kept as found - it has its own SC_ENGINE_RG_SMALL, above 64 slots (engine.hip).
struct StepTuning {
    int rg_small = 16, rg_ffn = 32, ffn_in_mode = 1, ffn_out_mode = 1;
    // N = M products: 16-row groups are tuned for <= 64 rows; above 128 live rows 32-row groups halve the workgroups that
    // re-read a weight tile - same bits whatever the grouping (tests/test_dstep3_gpu.py)
    static StepTuning defaults(int rows) {
        StepTuning t;
        t.rg_small = rows > 128 ? 32 : 16;
        return t;
    }
    // the knobs, clamped to what the launches accept (an out-of-range value would otherwise only surface as a failed check
    // inside a captured step)
    static StepTuning from_knobs(int rows);
};

// The buffers a step needs whatever loop drives it.  What differs per caller - the int / float state blocks, logits, the
// arg-max records, dec_hidden, the self and cross K / V - stays with the caller.
struct StepScratch {
    Buf<float> x, h, wide, att, hN, partial, xg, qkvr, qkv3;
};
// The packed chains' share, for c.nb = `rows` rows on kernel family `family` (choose_family): hN, partial, the six planes
// (family >= 2), xg / qkvr and c.gen3 (family >= 3), qkv3 (the wide step's complete q | k | v rows: > 64 rows, never
// the decode engine, whose slots keep the packed product), and the tuning fields.  The decode engine calls this alone.
void init_chain_scratch(Model& m, StepScratch& s, StepCtx& c, const DecStack& W, int rows, int family, const StepTuning& t);
// ... plus the general step's fp32 rows x / h / att / wide.  wide_always = false (the greedy session, kept across calls):
// a 4-element placeholder when a packed chain runs, which never reads it.
void init_step_scratch(Model& m, StepScratch& s, StepCtx& c, const DecStack& W, int rows, int family, const StepTuning& t,
                       bool wide_always = true);

// graph captures and instantiations are serialised process-wide (another handle's host thread may allocate while one records)
std::mutex& capture_mutex();

// One captured step chain: THE capture site of the library.  ensure() records once (thread-local capture under
// capture_mutex(); an exception out of `record` ends the capture, drops the dead graph and goes on up); launch() replays.
// Kept apart so that a caller's profiler scope can cover the replay alone.
class StepGraph {
   public:
    StepGraph() = default;
    StepGraph(const StepGraph&) = delete;
    StepGraph& operator=(const StepGraph&) = delete;
    StepGraph(StepGraph&& o) noexcept : graph_(o.graph_), exec_(o.exec_) { o.graph_ = nullptr, o.exec_ = nullptr; }
    StepGraph& operator=(StepGraph&& o) noexcept {
        if (this != &o) {
            reset();
            graph_ = o.graph_, exec_ = o.exec_;
            o.graph_ = nullptr, o.exec_ = nullptr;
        }
        return *this;
    }
    ~StepGraph() { reset(); }
    bool ready() const { return exec_ != nullptr; }
    template <class F>
    void ensure(hipStream_t stream, F&& record) {
        if (ready()) return;
        std::lock_guard<std::mutex> lock(capture_mutex());
        reset();  // a graph whose instantiation failed last time
        SC_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        try {
            record();
        } catch (...) {
            hipGraph_t dead = nullptr;
            (void)hipStreamEndCapture(stream, &dead);
            if (dead) (void)hipGraphDestroy(dead);
            throw;
        }
        SC_HIP(hipStreamEndCapture(stream, &graph_));
        SC_HIP(hipGraphInstantiate(&exec_, graph_, nullptr, nullptr, 0));
    }
    void launch(hipStream_t stream) { SC_HIP(hipGraphLaunch(exec_, stream)); }

   private:
    void reset() {
        if (exec_) (void)hipGraphExecDestroy(exec_);
        if (graph_) (void)hipGraphDestroy(graph_);
        graph_ = nullptr, exec_ = nullptr;
    }
    hipGraph_t graph_ = nullptr;
    hipGraphExec_t exec_ = nullptr;
};

// ---- shared by beam search (model_decoder.hip) and sampled generation (model_sample.hip) ------------------------------
// the limits of a generation call, before any device work; `who` prefixes every message
void check_generation_limits(const char* who, const sc_gen_opts& o, int prefix_len, int max_len, int decoder_max_seq_len, int n, int s_enc,
                             const int32_t* h_enc_lens);
// the caller's banned sequences on the device (validated on the host first; an empty list makes no device work)
struct BannedDevice {
    BannedList list;
    Buf<int> store;
};
BannedDevice upload_banned(Model& m, const BannedHost& banned, int V);
// the host checks of a phrase list and its boost (boost_list.h; no device work): the sorted list, or the reason as an error
BoostSorted check_boost_host(const BoostHost& boost, int V, int pad_idx, int eos_idx);
// the caller's boost phrases on the device, sorted (checked on the host first; an empty list or boost == 0 makes no device work)
struct BoostDevice {
    BoostList list;
    Buf<int> store;
};
BoostDevice upload_boost(Model& m, const BoostHost& boost, int V, int pad_idx, int eos_idx);
// the general step reads one encoder K / V per row: the encoder output [n][s_enc][M] repeated `per_item` times per item
Buf<float> fan_out_encoder(Model& m, const float* d_enc, int n, int per_item, int s_enc);
// vocabulary logits of the live rows into c.logits (row stride ldl): the streaming kernel on the packed embedding when v3
// (it stops at *c.d_rows where the caller set that), the tiled product on c.hN otherwise
void project_logits(Model& m, StepCtx& c, const DecStack& W, bool v3, int64_t ldl);
// What both loops set up before their first step: q.n * per_item hypothesis rows on one step chain.  The kernel family and,
// for the general step, the encoder output fanned out to the rows; the step context's scalars and its integer slices
// (8 + 5 * rows: position block, d_tok, d_finished, d_out_len, d_enc_lens and one spare [rows] slice); the step scratch under
// `tuning`; the logits with their row stride; the encoder K / V of every layer, projected once per utterance where the packed
// step kernels run (c.cross_row_div).  The self-attention caches stay with the caller.
struct HypRows {
    StepCtx c;
    bool packed_step = false;  // family != 1: the rows of an utterance share its encoder K / V
    bool proj_v3 = false;      // project_logits' v3
    int64_t ldl = 0;           // logits row stride
    int* d_spare = nullptr;    // the fifth [rows] slice (beam search: the source row of every beam; sampling: unused)
    Buf<int> ints;
    Buf<float> enc_rep, logits;
    StepScratch scratch;
    std::vector<Buf<float>> cross;
};
void setup_hyp_rows(Model& m, HypRows& h, const DecStack& W, const GenRequest& q, int per_item, int max_len, const StepTuning& tuning);
// decoder outputs of the chosen hypothesis per utterance (row u * ids_stride of h_ids / h_lens): the reference's
// teacher-forced pass over text_seqs[:, :-1] (generator.py:281-299) into d_dec_hidden [n][max_len - 1][M]
void hidden_of_best(Model& m, const float* d_enc, int n, int s_enc, const int32_t* h_enc_lens, const int32_t* h_ids, const int32_t* h_lens,
                    int ids_stride, int max_len, int pad_idx, float* d_dec_hidden);

}  // namespace sc
