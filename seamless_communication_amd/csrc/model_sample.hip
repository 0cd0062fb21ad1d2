// Sampled text generation (sc_generate_text_sampled): num_gens stochastic hypotheses per utterance, drawn with temperature and
// top-k / top-p inside the step loop (fairseq2 0.2 SamplingSeq2SeqGenerator + TopKSampler / TopPSampler, restated).
// A sibling of run_generate_beam (model_decoder.hip) on the same step chain and the same shared pieces (dstep.h): row
// u * num_gens + g is hypothesis g of utterance u, the encoder K / V are projected once per utterance, and rows never change
// places - no ancestor table, no cache re-ordering, a finished row rides along (its draws are skipped).  Per step: decoder step,
// vocabulary projection, ONE sampling launch (k_sample.hip: log-softmax under the temperature, step processors, step rules,
// kept set, draw, and the bookkeeping of the row: sequence, next token, cumulative score, finished flag).  The host polls the
// count of unfinished rows every fourth step.
#include <algorithm>
#include <cmath>

#include "dstep.h"
#include "engine.h"

namespace sc {

void run_generate_sampled(Model& m, const GenRequest& q, const sc_sample_opts& so, const uint64_t* h_streams, float* h_step_lprob) {
    const DecStack W = unity_stack(m);
    const sc_gen_opts& o = q.opts;
    const int n = q.n, s_enc = q.s_enc, prefix_len = q.prefix_len;
    const int32_t *h_prefix = q.h_prefix, *h_enc_lens = q.h_enc_lens;
    const int M = m.cfg.model_dim, V = W.vocab, B = so.num_gens, L = (int)W.layers->size();
    // ---- limits, before any device work ---------------------------------------------------------------------------------
    SC_CHECK(n > 0 && s_enc > 0, "sc_generate_text_sampled: empty batch");
    SC_CHECK(B >= 1 && B <= 64, "sc_generate_text_sampled: num_gens %d (1..64)", B);
    SC_CHECK((int64_t)n * B <= 512, "sc_generate_text_sampled: %d x %d rows (at most 512: the widest step chain)", n, B);
    SC_CHECK(so.temperature > 0.f && std::isfinite(so.temperature), "sc_generate_text_sampled: temperature %g (positive and finite)",
             (double)so.temperature);
    SC_CHECK(so.top_k >= 0, "sc_generate_text_sampled: top_k %d", so.top_k);
    SC_CHECK(so.top_p > 0.f && so.top_p <= 1.f, "sc_generate_text_sampled: top_p %g (0 < top_p <= 1)", (double)so.top_p);
    SC_CHECK(o.no_repeat_ngram_size >= 0, "sc_generate_text_sampled: no_repeat_ngram_size=%d", o.no_repeat_ngram_size);
    const int nb = n * B;
    const int max_len = text_max_len(m, o, s_enc);
    check_generation_limits("sc_generate_text_sampled", o, prefix_len, max_len, W.max_seq_len, n, s_enc, h_enc_lens);
    const BannedDevice banned_dev = upload_banned(m, q.banned, V);  // validated here, before any other device work
    const BannedList& bl = banned_dev.list;
    prof::set_tag("dec");
    if (m.engine) m.engine->expect(m, -n);  // never on the decode engine, like the banned-sequence calls

    // ---- the step context: hypotheses of an utterance share its encoder K / V; rows never change places ------------------
    HypRows hyp;
    setup_hyp_rows(m, hyp, W, q, B, max_len, StepTuning::defaults(nb));
    StepCtx& c = hyp.c;
    const int64_t ldl = hyp.ldl;
    const int64_t layer_stride = (int64_t)nb * max_len * M;
    Buf<float> kv(m.pp(), (size_t)2 * L * layer_stride);
    for (int li = 0; li < L; ++li) {
        c.kcache.push_back(kv.get() + (int64_t)(2 * li) * layer_stride);
        c.vcache.push_back(kv.get() + (int64_t)(2 * li + 1) * layer_stride);
    }
    auto project_rows = [&]() { project_logits(m, c, W, hyp.proj_v3, ldl); };  // c.d_rows stays null: every row, always

    // ---- per-row state, device resident ----------------------------------------------------------------------------------------
    std::vector<int32_t> seqs((size_t)nb * max_len, W.pad_idx), init(8 + 4 * nb, 0), tok(nb), gens(nb);
    std::vector<unsigned long long> streams(nb);
    for (int r = 0; r < nb; ++r) {
        for (int t = 0; t < prefix_len; ++t) seqs[(size_t)r * max_len + t] = h_prefix[t];
        init[8 + r] = h_prefix[0];
        init[8 + 3 * nb + r] = h_enc_lens[r / B];
        gens[r] = r % B;
        streams[r] = h_streams ? h_streams[r / B] : (unsigned long long)(r / B);
    }
    Buf<int> d_seqs(m.pp(), (size_t)nb * max_len), d_state(m.pp(), (size_t)3 * nb + 1);
    Buf<float> d_cum(m.pp(), (size_t)nb), d_slp(m.pp(), (size_t)nb * max_len), d_pref(m.pp(), (size_t)n);
    Buf<unsigned long long> d_streams(m.pp(), (size_t)nb);
    int* d_gen = d_state.get();
    int* d_fin = d_state.get() + nb;
    int* d_len = d_state.get() + 2 * nb;
    int* d_remaining = d_state.get() + 3 * nb;
    {
        std::vector<int32_t> st((size_t)3 * nb + 1, 0);
        std::copy(gens.begin(), gens.end(), st.begin());
        st[3 * nb] = nb;
        SC_HIP(hipMemcpyAsync(hyp.ints.get(), init.data(), init.size() * 4, hipMemcpyHostToDevice, m.stream));
        SC_HIP(hipMemcpyAsync(d_state.get(), st.data(), st.size() * 4, hipMemcpyHostToDevice, m.stream));
        SC_HIP(hipMemcpyAsync(d_seqs.get(), seqs.data(), seqs.size() * 4, hipMemcpyHostToDevice, m.stream));
        SC_HIP(hipMemcpyAsync(d_streams.get(), streams.data(), streams.size() * 8, hipMemcpyHostToDevice, m.stream));
        SC_HIP(hipMemsetAsync(d_slp.get(), 0, (size_t)nb * max_len * 4, m.stream));
        SC_HIP(hipMemsetAsync(d_pref.get(), 0, (size_t)n * 4, m.stream));
        SC_HIP(hipStreamSynchronize(m.stream));  // `st` is a host temporary
    }

    // ---- prompt echo: feed prefix[:-1]; cum = sum_j lprob(prefix[j] | prefix[<j]) under the temperature, the same for every
    // hypothesis of an utterance --------------------------------------------------------------------------------------------------
    for (int t = 0; t + 1 < prefix_len; ++t) {
        decoder_step(m, c, /*project=*/false);
        project_rows();
        launch_sample_prompt_lprob(c.logits, ldl, n, V, B, h_prefix[t + 1], so.temperature, d_pref, m.stream);
        for (int r = 0; r < nb; ++r) tok[r] = h_prefix[t + 1];
        SC_HIP(hipMemcpyAsync(c.d_tok, tok.data(), (size_t)nb * 4, hipMemcpyHostToDevice, m.stream));
        SC_HIP(hipStreamSynchronize(m.stream));
    }
    {
        std::vector<float> pref(n), cum(nb);
        SC_HIP(hipMemcpyAsync(pref.data(), d_pref.get(), (size_t)n * 4, hipMemcpyDeviceToHost, m.stream));
        SC_HIP(hipStreamSynchronize(m.stream));
        for (int r = 0; r < nb; ++r) cum[r] = pref[r / B];
        SC_HIP(hipMemcpyAsync(d_cum.get(), cum.data(), (size_t)nb * 4, hipMemcpyHostToDevice, m.stream));
        SC_HIP(hipStreamSynchronize(m.stream));
    }

    // ---- generation: device work only; the host polls `remaining` every fourth step --------------------------------------------
    StepGraph graph;
    const bool step_graph = o.use_graph != 0 && c.rb > 0;
    const int start = prefix_len - 1, G = o.no_repeat_ngram_size;
    int remaining = nb;
    for (int step = start; step <= max_len - 2 && remaining > 0; ++step) {
        if (step_graph) {
            graph.ensure(m.stream, [&] { decoder_step(m, c, /*project=*/false); });
            graph.launch(m.stream);
        } else {
            decoder_step(m, c, /*project=*/false);  // feeds d_tok at position `step`, advances *d_pos
        }
        project_rows();
        SampleArgs a;
        a.logits = c.logits, a.ld = ldl, a.rows = nb, a.V = V;
        a.stream = d_streams.get(), a.gen = d_gen, a.pos = step + 1;
        a.temperature = so.temperature, a.top_k = so.top_k, a.top_p = so.top_p, a.seed = so.seed;
        a.no_eos = step < o.min_seq_len, a.force_eos = step == max_len - 2;
        a.pad_idx = W.pad_idx, a.eos_idx = W.eos_idx, a.unk_idx = W.unk_idx, a.unk_penalty = o.unk_penalty;
        if ((G > 0 || bl.n > 0) && !a.force_eos) {  // step processors: not on the forced-EOS step
            a.seqs_in = d_seqs.get(), a.S = step + 1, a.G = G, a.banned = bl;
        }
        a.seq_ld = max_len;
        a.seqs = d_seqs.get(), a.next_tok = c.d_tok, a.cum = d_cum.get(), a.step_lprob = d_slp.get();
        a.finished = d_fin, a.out_len = d_len, a.remaining = d_remaining;
        launch_sample_rows(a, m.stream);
        if (((step - start) & 3) == 3 || step == max_len - 2) {
            SC_HIP(hipMemcpyAsync(&remaining, d_remaining, 4, hipMemcpyDeviceToHost, m.stream));
            SC_HIP(hipStreamSynchronize(m.stream));
        }
    }

    // ---- results: hypotheses of an utterance sorted by score (NaN first, then the higher score, ties keep the gen order) ----
    std::vector<int32_t> lens(nb);
    std::vector<float> cum(nb), slp((size_t)nb * max_len);
    SC_HIP(hipMemcpyAsync(seqs.data(), d_seqs.get(), seqs.size() * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipMemcpyAsync(lens.data(), d_len, (size_t)nb * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipMemcpyAsync(cum.data(), d_cum.get(), (size_t)nb * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipMemcpyAsync(slp.data(), d_slp.get(), slp.size() * 4, hipMemcpyDeviceToHost, m.stream));
    SC_HIP(hipStreamSynchronize(m.stream));
    std::vector<float> score(nb);
    for (int r = 0; r < nb; ++r) {
        SC_CHECK(lens[r] > prefix_len && lens[r] <= max_len, "sc_generate_text_sampled: row %d did not finish (length %d)", r, lens[r]);
        // beam_select_kernel's expression: the EOS is appended at step = len - 2
        score[r] = o.normalize_scores ? cum[r] / powf((float)(lens[r] - 1), o.len_penalty) : cum[r];
    }
    for (int u = 0; u < n; ++u) {
        std::vector<int> ord(B);
        for (int g = 0; g < B; ++g) ord[g] = u * B + g;
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
            const float s = score[a], t = score[b];
            return std::isnan(t) ? false : (std::isnan(s) || s > t);
        });
        for (int g = 0; g < B; ++g) {
            const int r = ord[g], dst = u * B + g, len = lens[r];
            for (int t = 0; t < max_len; ++t) {
                q.h_out_ids[(size_t)dst * max_len + t] = t < len ? seqs[(size_t)r * max_len + t] : W.pad_idx;
                if (h_step_lprob) h_step_lprob[(size_t)dst * max_len + t] = t < len ? slp[(size_t)r * max_len + t] : 0.f;
            }
            q.h_out_lens[dst] = len;
            if (q.h_scores) q.h_scores[dst] = score[r];
        }
    }
    // ---- decoder outputs of the best hypothesis per utterance: the teacher-forced pass, as behind a beam search ----------------
    // (slot 0 of every utterance after sorting)
    if (q.d_dec_hidden) hidden_of_best(m, q.d_enc, n, s_enc, h_enc_lens, q.h_out_ids, q.h_out_lens, B, max_len, W.pad_idx, q.d_dec_hidden);
}

}  // namespace sc
