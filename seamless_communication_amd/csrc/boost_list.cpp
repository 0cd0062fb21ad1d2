// Phrase boosting, the host side (boost_list.h): validation, the sort, the prefix-free check and the host restatement.
#include "boost_list.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include <numeric>

namespace sc {

namespace {
std::string fmt(const char* f, long long a = 0, long long b = 0) {
    char buf[160];
    std::snprintf(buf, sizeof buf, f, a, b);
    return buf;
}
}  // namespace

std::string boost_value_check(float boost) {
    if (!std::isfinite(boost) || std::fabs(boost) > BOOST_MAX_ABS) return fmt("boost phrases: boost must be finite with |boost| <= %lld", (long long)BOOST_MAX_ABS);
    return "";
}

std::string boost_list_build(const int32_t* tokens, const int32_t* offsets, int n, int V, int pad_idx, int eos_idx, BoostSorted& out) {
    out = BoostSorted{};
    if (n < 0 || n > BOOST_MAX_PHRASES) return fmt("boost phrases: %lld phrases (at most %lld)", n, BOOST_MAX_PHRASES);
    out.offsets.assign(1, 0);
    if (n == 0) return "";
    if (!tokens || !offsets) return "boost phrases: null list";
    if (offsets[0] != 0) return fmt("boost phrases: offsets[0] = %lld", offsets[0]);
    for (int q = 0; q < n; ++q) {
        const int64_t L = (int64_t)offsets[q + 1] - offsets[q];
        if (L < 1 || L > BOOST_MAX_LEN) return fmt("boost phrases: phrase %lld has %lld tokens", q, L) + fmt(" (1..%lld)", BOOST_MAX_LEN);
    }
    const int total = offsets[n];
    if (total > BOOST_MAX_TOKENS) return fmt("boost phrases: %lld tokens in all (at most %lld)", total, BOOST_MAX_TOKENS);
    for (int i = 0; i < total; ++i) {
        const int t = tokens[i];
        if (t < 0 || (V >= 0 && t >= V)) return fmt("boost phrases: token %lld outside the vocabulary of %lld", t, V);
        if (pad_idx >= 0 && t == pad_idx) return fmt("boost phrases: token %lld is the pad token", t);
        if (eos_idx >= 0 && t == eos_idx) return fmt("boost phrases: token %lld is the end-of-sentence token", t);
    }
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    auto less = [&](int a, int b) {
        return std::lexicographical_compare(tokens + offsets[a], tokens + offsets[a + 1], tokens + offsets[b], tokens + offsets[b + 1]);
    };
    std::stable_sort(order.begin(), order.end(), less);
    // every phrase that starts with phrase a follows a directly in the sorted order: adjacent pairs suffice
    for (int i = 0; i + 1 < n; ++i) {
        const int a = order[i], b = order[i + 1];
        const int la = offsets[a + 1] - offsets[a], lb = offsets[b + 1] - offsets[b];
        if (la <= lb && std::equal(tokens + offsets[a], tokens + offsets[a + 1], tokens + offsets[b]))
            return fmt("boost phrases: not prefix-free (phrase %lld is a prefix of phrase %lld)", a, b);
    }
    out.n = n;
    out.tokens.reserve(total);
    for (int i = 0; i < n; ++i) {
        const int q = order[i];
        out.tokens.insert(out.tokens.end(), tokens + offsets[q], tokens + offsets[q + 1]);
        out.offsets.push_back((int32_t)out.tokens.size());
        out.max_len = std::max(out.max_len, offsets[q + 1] - offsets[q]);
    }
    return "";
}

int boost_depth(const int32_t* seq, int S, const BoostSorted& b, int* out_dp) {
    int d = 0, leaf = 0;
    for (int q = 0; q < b.n; ++q) {
        const int32_t* w = b.tokens.data() + b.offsets[q];
        const int L = b.offsets[q + 1] - b.offsets[q];
        for (int P = std::min(L, S); P > d; --P)
            if (std::equal(w, w + P, seq + S - P)) {
                d = P;
                leaf = P == L;
                break;
            }
    }
    if (out_dp) *out_dp = leaf ? 0 : d;
    return d;
}

void boost_deltas(const int32_t* seq, int S, const BoostSorted& b, std::vector<int32_t>& out_tokens, std::vector<int32_t>& out_depth, int* out_dp) {
    boost_depth(seq, S, b, out_dp);
    std::map<int32_t, int32_t> best;  // token -> d(y + t)
    for (int q = 0; q < b.n; ++q) {
        const int32_t* w = b.tokens.data() + b.offsets[q];
        const int L = b.offsets[q + 1] - b.offsets[q];
        for (int P = 0; P < L && P <= S; ++P)  // the row's last P tokens, then w[P]
            if (std::equal(w, w + P, seq + S - P)) {
                int32_t& v = best[w[P]];
                v = std::max(v, P + 1);
            }
    }
    out_tokens.clear();
    out_depth.clear();
    for (const auto& kv : best) {
        out_tokens.push_back(kv.first);
        out_depth.push_back(kv.second);
    }
}

}  // namespace sc
