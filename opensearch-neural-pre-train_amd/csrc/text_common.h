// Device code shared by the text kernels (wordpiece.hip, unigram.hip, tfidf.hip, cooc.hip), each piece stated once:
//   TEXT_HASH_BASE, text_hash_powers   the polynomial hash of a vocabulary key (include/snx.h "WordPiece tokenizer":
//                                      h = h * BASE + c + 1 over its code points) and the table BASE^L that takes the hash
//                                      of a piece out of two prefix hashes, filled by thread 0
//   text_hash_mix                      the finalizer that turns (hash ^ what tells keys of one hash apart) into a slot
//   text_probe                         the bounded linear probe of the open-addressed vocabulary table (slots, ent_ptr):
//                                      the entry of L code points that `same(entry, first code point's place)` accepts
//   text_bitonic_asc<THREADS>          ascending sort of 64-bit keys by the whole workgroup
// Every kernel of unigram.hip, tfidf.hip and cooc.hip compiles to the code of its written-out form
// (profiles/text_front_refactor.txt).  wordpiece.hip takes the base and the finalizer from here and keeps its own probe
// loop (wp_lookup) and power fill: with text_probe or with text_hash_powers wp_pieces_kernel compiles to other code, and
// a changed kernel has to be timed against its parent before it may replace it.  A change to text_probe's loop or to the
// fill has to be made there as well.
// Local on purpose, not here: the three white-space predicates (tx_space is str.isspace, ug_space Rust's White_Space, the
// WordPiece class table: different sets), the long-row forms' walk over workspace slots (the slots differ), and
// block_sum, which these files take from sparse_common.h.
#pragma once
#include "common.h"

namespace {

constexpr uint32_t TEXT_HASH_BASE = 0x9E3779B1u;

// pw[L] = TEXT_HASH_BASE^L for L in [0, max_entry]; the caller's barrier publishes it
__device__ __forceinline__ void text_hash_powers(uint32_t* pw, int max_entry) {
  if (threadIdx.x == 0) {
    uint32_t p = 1u;
    for (int L = 0; L <= max_entry; ++L) { pw[L] = p; p *= TEXT_HASH_BASE; }
  }
}

__device__ __forceinline__ uint32_t text_hash_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

// the entry e of L code points with same(e, ent_ptr[e]), looked for from the slot of the mixed hash x; -1 when the
// vocabulary has none
template <typename Same>
__device__ __forceinline__ int32_t text_probe(const int32_t* slots, const int32_t* ent_ptr, int32_t n_slots,
                                              int32_t n_entries, uint32_t x, int L, Same same) {
  const uint32_t m = (uint32_t)n_slots - 1u;
  uint32_t s = x & m;
  for (int32_t probe = 0; probe < n_slots; ++probe) {        // bounded: a full table has no free slot to stop at
    const int32_t e = slots[s];
    if (e < 0 || e >= n_entries) return -1;
    const int32_t b = ent_ptr[e];
    if (ent_ptr[e + 1] - b == L && same(e, b)) return e;
    s = (s + 1u) & m;
  }
  return -1;
}

// ascending bitonic sort of a[0..P), P a power of two, by the whole workgroup; a is LDS or the workgroup's workspace slot
template <int THREADS>
__device__ __forceinline__ void text_bitonic_asc(unsigned long long* a, int64_t P) {
  for (int64_t size = 2; size <= P; size <<= 1)
    for (int64_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (int64_t t = threadIdx.x; t < (P >> 1); t += THREADS) {
        const int64_t lo = 2 * t - (t & (stride - 1));
        const int64_t hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const unsigned long long x = a[lo], y = a[hi];
        if ((x > y) == asc) { a[lo] = y; a[hi] = x; }
      }
      __syncthreads();
    }
}

}  // namespace
