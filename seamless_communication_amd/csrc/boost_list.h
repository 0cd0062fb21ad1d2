// Phrase boosting (PhraseBoostProcessor), the host side: limits of a phrase list, its sorted form for the device, and the host
// restatement of the rule.  Plain C++ without HIP: the library calls it (api.hip, model_decoder.hip) and the stand-alone program
// tests/host/boost_host.cpp runs it under the host sanitizers.
//
// The rule (this project's own).  y: a row's S tokens so far, prompt included.
//   d(y)     length of the longest suffix of y that is a prefix of some phrase (a whole phrase counts), 0 if none;
//   dp(y)    d(y) if that suffix is a proper prefix of a phrase (bonus handed out, not yet earned), 0 if it is a whole phrase;
//   k(y, t)  d(y + t) - dp(y), in -63 .. 64; the logit of t becomes fmaf(boost, (float)k, x[t]).
// The list is prefix-free (no phrase is a prefix of another, duplicates included): whole phrases are the leaves of the trie.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace sc {

constexpr int BOOST_MAX_PHRASES = 4096, BOOST_MAX_LEN = 64, BOOST_MAX_TOKENS = 65536;
constexpr float BOOST_MAX_ABS = 100.f;

// a validated list, phrases in lexicographic order (CSR)
struct BoostSorted {
    std::vector<int32_t> tokens;
    std::vector<int32_t> offsets;  // [n + 1]
    int n = 0;
    int max_len = 0;
};

// Checks the limits (at most BOOST_MAX_PHRASES phrases of 1..BOOST_MAX_LEN tokens, BOOST_MAX_TOKENS in all, every token in
// [0, V) and neither pad_idx nor eos_idx, prefix-free) and sorts the phrases.  V < 0: no vocabulary to check against; pad_idx /
// eos_idx < 0: none.  Returns an empty string, or the reason of the refusal (out is then unspecified).
std::string boost_list_build(const int32_t* tokens, const int32_t* offsets, int n, int V, int pad_idx, int eos_idx, BoostSorted& out);
// the boost value: finite, |boost| <= BOOST_MAX_ABS.  Returns an empty string or the reason.
std::string boost_value_check(float boost);

// d(y); *out_dp = dp(y)
int boost_depth(const int32_t* seq, int S, const BoostSorted& b, int* out_dp);
// the tokens t with d(y + t) > 0 in ascending order with d(y + t); *out_dp = dp(y)
void boost_deltas(const int32_t* seq, int S, const BoostSorted& b, std::vector<int32_t>& out_tokens, std::vector<int32_t>& out_depth, int* out_dp);

}  // namespace sc
