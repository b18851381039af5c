// lr_lm_dev.h — the packed word language model: the blob's layout and the device lookups, shared by lr_ctc_beam.hip
// (which also holds the packer, lr_ctc_beam_lm_pack) and lr_attn_beam.hip (the attention and joint searches' fusion,
// DESIGN.md §21).  Internal: every includer gets its own copy (anonymous namespace).
#pragma once
#include "lr_common.h"

namespace {

// ---------------------------------------------------------------------------------------
// the language-model blob: its layout is owned here (lm_pack writes it, the loop reads it)
// ---------------------------------------------------------------------------------------
// Little-endian, every section 16-byte aligned, offsets in bytes from the blob's start:
//   LmHeader           kLmHeaderBytes
//   uni[V]             float2 (ln p, ln backoff) of unigram w (word id w = its row in the ARPA \1-grams: section)
//   ngram[ngram_slots] LmNgram, ngram_slots a power of two at load <= 1/2.  Entry ids: 0 is the empty context, 1+w
//                      unigram w, V+1+slot the n-gram in that slot.  The n-gram (w1..wk), k >= 2, has key
//                      (entry id of w1..w(k-1)) << 24 | wk; its (k-1)-gram prefix is always listed.
//   trie[trie_slots]   LmTrie, trie_slots a power of two at load <= 1/2; key (node << 8) | class, root node 0;
//                      child is the node reached, word the vocabulary word id it spells (-1: only a prefix).
// Empty slots of both tables hold key kLmEmpty.  Values are natural logs (ln 10 * the ARPA's log10), fp32.
constexpr uint32_t kLmMagic = 0x4d4c524cu;   // "LRLM"
constexpr uint32_t kLmVersion = 1;
constexpr int kLmMaxOrder = 6;
constexpr int kLmMaxCtx = kLmMaxOrder - 1;
constexpr int64_t kLmMaxVocab = (int64_t)1 << 24;
constexpr uint64_t kLmEmpty = ~0ull;
constexpr float kLmOov = -1000.f;
constexpr size_t kLmHeaderBytes = 128;
constexpr int kRoleTransparent = 0, kRoleWord = 1, kRoleSpace = 2;

struct LmHeader {
  uint32_t magic, version;
  int32_t order, vocab, bos, pad_;   // bos: word id of <s>, -1 if the ARPA has none
  int64_t ngram_slots, trie_slots;
  int64_t uni_off, ngram_off, trie_off, bytes;
};
static_assert(sizeof(LmHeader) <= kLmHeaderBytes, "LmHeader");
struct LmNgram {
  uint64_t key;
  float lp, lbow;
};
struct LmTrie {
  uint64_t key;
  int32_t child, word;
};
static_assert(sizeof(LmNgram) == 16 && sizeof(LmTrie) == 16, "16-byte slots");

__host__ __device__ inline uint64_t lm_mix(uint64_t x) {   // splitmix64's finaliser
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}
__host__ __device__ inline uint64_t lm_ngram_key(int64_t entry, int word) {
  return ((uint64_t)entry << 24) | (uint64_t)(uint32_t)word;
}
__host__ __device__ inline uint64_t lm_trie_key(int node, int cls) {
  return ((uint64_t)(uint32_t)node << 8) | (uint64_t)(uint32_t)cls;
}

// The device view, read from the header once per workgroup.
struct LmView {
  const float2* uni;
  const LmNgram* ngram;
  const LmTrie* trie;
  uint64_t nmask, tmask;
  int vocab, m;   // m = order - 1 context words
};

__device__ __forceinline__ LmView lm_view(const uint8_t* blob) {
  const LmHeader* h = reinterpret_cast<const LmHeader*>(blob);
  LmView v;
  v.uni = reinterpret_cast<const float2*>(blob + h->uni_off);
  v.ngram = reinterpret_cast<const LmNgram*>(blob + h->ngram_off);
  v.trie = reinterpret_cast<const LmTrie*>(blob + h->trie_off);
  v.nmask = (uint64_t)h->ngram_slots - 1;
  v.tmask = (uint64_t)h->trie_slots - 1;
  v.vocab = h->vocab;
  v.m = h->order - 1;
  return v;
}

// entry id of the n-gram (entry's words, word), or -1 if it is not listed
__device__ __forceinline__ int64_t lm_ngram_find(const LmView& L, int64_t entry, int word, float* lp, float* lbow) {
  const uint64_t key = lm_ngram_key(entry, word);
  for (uint64_t s = lm_mix(key) & L.nmask;; s = (s + 1) & L.nmask) {
    const LmNgram g = L.ngram[s];
    if (g.key == key) { *lp = g.lp; *lbow = g.lbow; return (int64_t)L.vocab + 1 + (int64_t)s; }
    if (g.key == kLmEmpty) return -1;
  }
}

// child of a trie node by class: .x = child node (-1 if the word leaves the vocabulary), .y = the word it spells
__device__ __forceinline__ int2 lm_trie_find(const LmView& L, int node, int cls) {
  const uint64_t key = lm_trie_key(node, cls);
  for (uint64_t s = lm_mix(key) & L.tmask;; s = (s + 1) & L.tmask) {
    const LmTrie e = L.trie[s];
    if (e.key == key) return make_int2(e.child, e.word);
    if (e.key == kLmEmpty) return make_int2(-1, -1);
  }
}

// lm(w | ctx): ctx holds L.m word ids, oldest first (-1 = not a unigram)
__device__ float lm_score(const LmView& L, const int* ctx, int w) {
  if (w < 0) return kLmOov;
  int c[kLmMaxCtx];
  for (int j = 0; j < L.m; ++j) {
    c[j] = ctx[j];
    if (c[j] < 0) return kLmOov;
  }
  float acc = 0.f;
  for (int j = 0; j < L.m; ++j) {   // context c[j..m-1], longest first
    int64_t e = 1 + c[j];
    float lp, lbow = L.uni[c[j]].y;
    for (int q = j + 1; q < L.m && e >= 0; ++q) e = lm_ngram_find(L, e, c[q], &lp, &lbow);
    if (e < 0) continue;   // the context is not listed: neither is (context, w), and its backoff is 0
    float wbow;
    if (lm_ngram_find(L, e, w, &lp, &wbow) >= 0) return acc + lp;
    acc += lbow;
  }
  return acc + L.uni[w].x;
}

}  // namespace
