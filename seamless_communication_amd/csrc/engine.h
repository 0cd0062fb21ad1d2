// Decode engine (engine.hip): one greedy decoder-step chain per GPU shared by all passes in flight.
#pragma once
#include <memory>

#include "../../include/seamless_hip.h"

namespace sc {

struct Model;
struct GenRequest;

class Engine {
   public:
    Engine(const Model& parent, const sc_engine_opts& opts);  // starts the engine thread
    ~Engine();                                                // stops it; outstanding requests fail
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;
    const sc_engine_opts& opts() const;
    // can a greedy sc_generate_text call of this shape go through the engine?  prefix_len: the call's LONGEST prompt.  The admit
    // record carries at most ENGINE_MAX_PREFIX (12) prompt tokens per row, so a call holding a longer prompt - one row of a
    // ragged sc_generate_text_prompts call is enough - does not fit and runs on the handle's own chain as a whole.
    bool fits(int n, int s_enc, int max_len, int prefix_len, const sc_gen_opts& o) const;
    // is there anything to share the chain with - rows of other requests inside, or rows announced (this handle's included)?  A lone
    // call on an idle engine is faster on the handle's own chain (kernels sized for its rows, not for the engine's slots)
    bool has_company() const;
    // n > 0: handle m announces n rows it will submit; n < 0: up to -n announced rows of m arrived or will not come
    void expect(Model& m, int n);
    void stats(sc_engine_stats* out, bool reset);
    // greedy generation of q.n rows through the shared chain; blocks until every row has finished.  The request as
    // run_generate_text takes it (h_prefix_lens: per-row prompt lengths, each within the admit record's capacity; the row state
    // keeps its own length).
    void generate(Model& m, const GenRequest& q, int max_len);

   private:
    struct Impl;
    std::unique_ptr<Impl> p_;
};

}  // namespace sc
