// Host check of the phrase-boost list code (csrc/boost_list.cpp): validation of every limit, the sort, the prefix-free check
// and the host restatement of the rule on the edge lists (a 64-token phrase, a phrase longer than the sequence, the whole
// sequence as a phrase prefix, a single-token phrase, an empty sequence, the largest list the limits allow), against a
// brute-force loop.  No HIP.  Stand-alone: build with the host sanitizers and run, from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/host/boost_host.cpp seamless_communication_amd/csrc/boost_list.cpp -o build/boost_host && build/boost_host
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../seamless_communication_amd/csrc/boost_list.h"

using Phrases = std::vector<std::vector<int32_t>>;

static void csr(const Phrases& p, std::vector<int32_t>& tok, std::vector<int32_t>& off) {
    tok.clear();
    off.assign(1, 0);
    for (const auto& q : p) {
        tok.insert(tok.end(), q.begin(), q.end());
        off.push_back((int32_t)tok.size());
    }
}

static std::string build(const Phrases& p, sc::BoostSorted& out, int V = -1, int pad = -1, int eos = -1) {
    std::vector<int32_t> tok, off;
    csr(p, tok, off);
    return sc::boost_list_build(tok.data(), off.data(), (int)p.size(), V, pad, eos, out);
}

// the rule as a loop over every phrase and every prefix length
static void brute(const std::vector<int32_t>& y, const Phrases& p, std::map<int32_t, int32_t>& next, int& dp) {
    int d = 0;
    bool leaf = false;
    next.clear();
    for (const auto& q : p)
        for (size_t n = 0; n <= q.size() && n <= y.size(); ++n) {
            if (!std::equal(q.begin(), q.begin() + n, y.end() - n)) continue;
            if ((int)n > d) d = (int)n, leaf = n == q.size();
            if (n < q.size()) next[q[n]] = std::max(next[q[n]], (int32_t)n + 1);
        }
    dp = leaf ? 0 : d;
}

static int g_bad = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("boost_host: line %d: %s\n", __LINE__, #cond);     \
            ++g_bad;                                                  \
        }                                                             \
    } while (0)

static void check_rule(const Phrases& p, const std::vector<int32_t>& y) {
    sc::BoostSorted s;
    EXPECT(build(p, s).empty());
    std::vector<int32_t> toks, depth;
    int dp = -1, want_dp = -1;
    sc::boost_deltas(y.data(), (int)y.size(), s, toks, depth, &dp);
    std::map<int32_t, int32_t> want;
    brute(y, p, want, want_dp);
    EXPECT(dp == want_dp);
    EXPECT(toks.size() == want.size() && std::is_sorted(toks.begin(), toks.end()));
    for (size_t i = 0; i < toks.size() && i < want.size(); ++i) EXPECT(want.count(toks[i]) && want[toks[i]] == depth[i]);
    int dp2 = -1;
    const int d = sc::boost_depth(y.data(), (int)y.size(), s, &dp2);
    EXPECT(dp2 == want_dp && d >= dp2 && (dp2 == 0 || dp2 == d));
}

int main() {
    sc::BoostSorted s;
    // ---- the limits, each with its reason ------------------------------------------------------------------------------
    EXPECT(build({}, s).empty() && s.n == 0 && s.offsets.size() == 1);
    EXPECT(build(Phrases(4097, {1}), s).find("4097 phrases") != std::string::npos);
    EXPECT(build({std::vector<int32_t>(65, 7)}, s).find("65 tokens") != std::string::npos);
    {
        std::vector<int32_t> tok{1}, off{0, 0};  // an empty phrase
        EXPECT(sc::boost_list_build(tok.data(), off.data(), 1, -1, -1, -1, s).find("0 tokens") != std::string::npos);
        std::vector<int32_t> off2{1, 2};
        EXPECT(sc::boost_list_build(tok.data(), off2.data(), 1, -1, -1, -1, s).find("offsets[0]") != std::string::npos);
        EXPECT(sc::boost_list_build(nullptr, nullptr, 1, -1, -1, -1, s).find("null") != std::string::npos);
    }
    {
        Phrases many;  // 1025 distinct phrases of 64 tokens: 65600 tokens
        for (int i = 0; i < 1025; ++i) {
            std::vector<int32_t> q(64, 4);
            q[0] = 10 + i;
            many.push_back(q);
        }
        EXPECT(build(many, s).find("65600 tokens in all") != std::string::npos);
        many.pop_back();  // 65536 tokens: the largest list
        EXPECT(build(many, s).empty() && s.n == 1024 && s.max_len == 64 && s.tokens.size() == 65536);
    }
    EXPECT(build({{5, 40}}, s, 40).find("outside the vocabulary") != std::string::npos);
    EXPECT(build({{5, -1}}, s, 40).find("outside the vocabulary") != std::string::npos);
    EXPECT(build({{5, -1}}, s).find("outside the vocabulary") != std::string::npos);
    EXPECT(build({{5, 0}}, s, 40, 0, 3).find("pad") != std::string::npos);
    EXPECT(build({{5, 3}}, s, 40, 0, 3).find("end-of-sentence") != std::string::npos);
    EXPECT(build({{5, 6}, {7}, {5, 6, 8}}, s).find("prefix-free") != std::string::npos);
    EXPECT(build({{5, 6}, {7}, {5, 6}}, s).find("prefix-free") != std::string::npos);
    EXPECT(build({{5, 6}, {5}}, s).find("prefix-free") != std::string::npos);
    EXPECT(build({{5, 6}, {6, 5}, {5, 7}, {6}}, s).find("prefix-free") != std::string::npos);
    EXPECT(sc::boost_value_check(100.f).empty() && sc::boost_value_check(-100.f).empty() && sc::boost_value_check(0.f).empty());
    EXPECT(!sc::boost_value_check(100.5f).empty() && !sc::boost_value_check(std::nanf("")).empty());
    EXPECT(!sc::boost_value_check(std::numeric_limits<float>::infinity()).empty());
    // ---- the sort ------------------------------------------------------------------------------------------------------
    EXPECT(build({{9, 1}, {2}, {9, 0, 5}, {3, 3}}, s).empty());
    EXPECT((s.tokens == std::vector<int32_t>{2, 3, 3, 9, 0, 5, 9, 1}) && (s.offsets == std::vector<int32_t>{0, 1, 3, 6, 8}) && s.max_len == 3);
    // ---- the restatement on the edge lists -----------------------------------------------------------------------------
    const std::vector<int32_t> y{2, 5, 6, 5, 6, 7};
    std::vector<int32_t> long64(64, 8);
    std::copy(y.begin(), y.end(), long64.begin());            // the whole sequence is the head of a 64-token phrase
    Phrases edge{long64, {9}, {6, 7, 5, 5, 5, 5, 5, 5}, {5, 6, 7}, {6, 5, 6, 9}};
    check_rule(edge, y);
    check_rule(edge, {});                                      // no token yet: the roots only
    check_rule(edge, {9});                                     // a single-token phrase just completed
    check_rule(edge, {6});
    check_rule({std::vector<int32_t>(64, 8)}, std::vector<int32_t>(64, 8));  // a 64-token phrase completed
    check_rule({std::vector<int32_t>(64, 8)}, std::vector<int32_t>(70, 8));
    check_rule({std::vector<int32_t>(64, 8)}, std::vector<int32_t>(63, 8));
    check_rule({{5, 6, 7}, {6, 8}}, {5, 6});                   // the slide: 8 moves from one phrase's prefix onto another's
    check_rule({{5, 6, 7}, {6, 7}}, {5, 6});                   // one token offered at two depths
    // ---- random lists over a small alphabet ----------------------------------------------------------------------------
    std::mt19937 rng(7);
    for (int it = 0; it < 300; ++it) {
        Phrases p;
        for (int tries = 0; tries < 12; ++tries) {
            std::vector<int32_t> q(1 + rng() % 5);
            for (auto& t : q) t = 4 + (int32_t)(rng() % 6);
            bool ok = true;
            for (const auto& o : p) {
                const size_t m = std::min(o.size(), q.size());
                ok = ok && !std::equal(o.begin(), o.begin() + m, q.begin());
            }
            if (ok) p.push_back(q);
        }
        std::vector<int32_t> seq(rng() % 10);
        for (auto& t : seq) t = 4 + (int32_t)(rng() % 6);
        check_rule(p, seq);
    }
    printf(g_bad ? "boost_host: FAILED (%d)\n" : "boost_host: ok\n", g_bad);
    return g_bad ? 1 : 0;
}
