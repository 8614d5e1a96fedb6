// Device code shared by the sparse-retrieval kernels (retrieval.hip, seismic.hip, two_phase.hip, hybrid.hip, qrels.hip).
// Every kernel of those files is pinned to one contract (include/snx.h): s(q, d) is the fmaf chain over the shared terms
// in ascending term id starting from +0, and results are ordered score descending, then doc ascending, bit for bit.
// The pieces that state that contract live here once:
//   rank_key / rank_bits / rank_id   the 64-bit key (score bits << 32 | ~id): descending keys = the ABI's order
//   row_dot, row_dot_search,         s(a, b) by a linear merge (one lane), by binary search from the last hit (one
//   row_dot_lanes                    lane), and by binary search with the lanes over the query terms, lane 0 folding
//   SelectSmem, radix_select,        top k of a key sequence under (key desc, index asc), taken in index order
//   ordered_take
//   bitonic_desc, block_sum          descending sort of 64-bit keys and an integer sum by the whole workgroup
//   ChunkSmem, accumulate_chunk,     the chunk stage of the exact searches (sr_chunk_kernel, sb_chunk_kernel): the scores
//   count_ahead, select_chunk        of a chunk of docs in LDS by the ABI's chain, a thread's share of the count of docs
//                                    ranked ahead of a target, and the chunk's top k as rank keys in doc order
//   RankLists, merge_lists,          the merge stage (sr_merge_kernel, sb_merge_kernel; dn_merge_kernel of dense.hip):
//   write_ranks                      the top hi over a query's candidate lists, sorted, ranks lo .. hi-1 written.
//                                    iv_merge_kernel (ivf.hip) selects by another rule and shares the list view and tail
// These kernels compile to other code than their written-out forms did, so each was timed against its parent before the
// copies went: profiles/sparse_chunk_merge_refactor.txt.  qr_count_kernel (qrels.hip) failed that timing with the chunk
// helpers (first_relevant at 1,000,000 docs x 2,000 queries: medians 1.4 % and 0.7 % over the parent's best, margin
// 1.0 %) and keeps its written-out copy of the accumulation, the count and its wave-array sum; a change to
// accumulate_chunk or count_ahead has to be made there as well.
// The dense searches (dense.hip, ivf.hip) rank by the same 64-bit key and select with the same functions; what only they
// share -- the fp32 MFMA tile, its order key, the candidate lists' compaction -- is in dense_common.h, which includes this
// file.  The host's split planner of the tiled searches (split_plan: dense.hip, infogain.hip) sits below, next to
// pow2_at_least.
// Local on purpose, not here: hybrid.hip's HY_BITONIC and float64 helpers (other comparators); the 8-bit radix selects of
// sz_prune_kernel and tp_prune_kernel (their bodies differ); tp_prune_kernel's wave-array sum (block_sum's LDS-word form
// compiles it to more code, profiles/retrieval_refactor_isa.txt); the ascending sorts (text_common.h's, infogain's pairs).
// A helper that depends on the workgroup size takes it as a template parameter (the files use 512, 256 and 64 threads);
// the select, chunk and merge helpers are for SR_THREADS.
#pragma once
#include "common.h"
#include "runtime.h"   // align256

namespace {

// chunked exact search (retrieval.hip) and everything that repeats its accumulation (qrels.hip)
constexpr int SR_THREADS = 512;
constexpr int SR_WAVES = SR_THREADS / 64;
constexpr int SR_TG = SR_THREADS / 2;          // query terms whose chunk bounds are searched at once
constexpr int SR_KMAX = 1024;
constexpr int SR_CHUNK_DEFAULT = 16384;        // 64 KiB of scores: two workgroups per CU
constexpr int SR_CHUNK_MAX = 32768;            // 128 KiB of scores + ~14 KiB static LDS (160 KiB per workgroup)

inline int sr_chunk(int32_t chunk_docs) { return chunk_docs > 0 ? chunk_docs : SR_CHUNK_DEFAULT; }
inline int sr_nch(int32_t nd, int chunk) { return nd > 0 ? (int)((nd + (long)chunk - 1) / chunk) : 1; }

template <typename T>                          // int in hybrid.hip, long elsewhere: the loop width shows in the code
__host__ __device__ inline T pow2_at_least(T n) {
  T p = 1;
  while (p < n) p <<= 1;
  return p;
}

// The tiled searches that split the row range over workgroups (dense.hip, infogain.hip): a workgroup owns `tile` queries
// and one split of split_tiles tiles of the n rows.  chunk > 0 sets the split length in rows; otherwise as many splits as
// bring the launch to wg_target workgroups, at most splits_max (the lists per query that the merge has to read).
struct SplitPlan {
  int qtiles, split_tiles, nsplit;
  long tiles;
};

inline SplitPlan split_plan(int32_t nq, int32_t n, int32_t chunk, int tile, int wg_target, int splits_max) {
  SplitPlan p;
  p.qtiles = (int)((nq + (long)tile - 1) / tile);
  p.tiles = (n + (long)tile - 1) / tile;
  if (chunk > 0) {
    p.split_tiles = (int)((chunk + (long)tile - 1) / tile);
  } else {
    long want = (wg_target + (long)p.qtiles - 1) / (p.qtiles > 0 ? p.qtiles : 1);
    if (want > splits_max) want = splits_max;
    if (want > p.tiles) want = p.tiles;
    if (want < 1) want = 1;
    p.split_tiles = (int)((p.tiles + want - 1) / want);
  }
  if (p.split_tiles < 1) p.split_tiles = 1;
  const long ns = (p.tiles + p.split_tiles - 1) / p.split_tiles;
  p.nsplit = (int)(ns < 1 ? 1 : (ns > 0x7FFFFFFFL ? 0x7FFFFFFFL : ns));
  return p;
}

__device__ __forceinline__ uint32_t fbits(float x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ float bitsf(uint32_t x) { return __builtin_bit_cast(float, x); }

// (bits << 32 | ~id): larger bits first, ties lowest id first, when sorted descending; 0 = no entry
__device__ __forceinline__ unsigned long long rank_key(uint32_t bits, uint32_t id) {
  return ((unsigned long long)bits << 32) | (0xFFFFFFFFull - id);
}
__device__ __forceinline__ uint32_t rank_bits(unsigned long long key) { return (uint32_t)(key >> 32); }
__device__ __forceinline__ int32_t rank_id(unsigned long long key) {
  return (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
}

template <typename T>
__device__ __forceinline__ int64_t lower_bound(const T* __restrict__ a, int64_t lo, int64_t hi, T x) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------------ s(a, b)
// s(a, b) of the ABI: fmaf over the shared terms in ascending term id, from +0 (rows strictly ascending)
__device__ __forceinline__ float row_dot(const int32_t* at, const float* aw, int64_t a0, int64_t a1,
                                         const int32_t* bt, const float* bw, int64_t b0, int64_t b1) {
  float acc = 0.f;
  while (a0 < a1 && b0 < b1) {
    const int32_t x = at[a0], y = bt[b0];
    if (x == y) {
      acc = fmaf(aw[a0], bw[b0], acc);
      ++a0;
      ++b0;
    } else if (x < y) {
      ++a0;
    } else {
      ++b0;
    }
  }
  return acc;
}

// the same value with every term of the (short) row a looked up in row b by binary search behind the previous hit
__device__ __forceinline__ float row_dot_search(const int32_t* __restrict__ at, const float* __restrict__ aw, int64_t a0,
                                                int64_t a1, const int32_t* __restrict__ bt,
                                                const float* __restrict__ bw, int64_t b0, int64_t b1) {
  float acc = 0.f;
  for (int64_t j = a0; j < a1 && b0 < b1; ++j) {             // ascending term id: the ABI's accumulation order
    const int32_t term = at[j];
    const int64_t p = lower_bound(bt, b0, b1, term);
    if (p < b1 && bt[p] == term) acc = fmaf(aw[j], bw[p], acc);
    b0 = p;
  }
  return acc;
}

// the same value by a workgroup of THREADS lanes: the lanes find THREADS terms of row a in row b at once, lane 0 applies
// fmaf in ascending term id.  The result is valid on lane 0.
template <int THREADS>
__device__ __forceinline__ float row_dot_lanes(const int32_t* __restrict__ at, const float* __restrict__ aw, int64_t a0,
                                               int64_t a1, const int32_t* __restrict__ bt,
                                               const float* __restrict__ bw, int64_t b0, int64_t b1) {
  __shared__ float qv[THREADS], dv[THREADS];
  __shared__ int hit[THREADS];
  const int lane = threadIdx.x;
  float acc = 0.f;
  for (int64_t g = a0; g < a1; g += THREADS) {
    const int64_t j = g + lane;
    hit[lane] = 0;
    if (j < a1) {
      const int32_t term = at[j];
      const int64_t p = lower_bound(bt, b0, b1, term);
      if (p < b1 && bt[p] == term) { hit[lane] = 1; qv[lane] = aw[j]; dv[lane] = bw[p]; }
    }
    __syncthreads();
    if (lane == 0) {
      const int m = (int)min((int64_t)THREADS, a1 - g);
      for (int i = 0; i < m; ++i)
        if (hit[i]) acc = fmaf(qv[i], dv[i], acc);
    }
    __syncthreads();
  }
  return acc;
}

// ------------------------------------------------------------------------------------------------ workgroup helpers
// sum of v over the workgroup, returned to every thread; `slot` is an LDS word no one else touches meanwhile
__device__ __forceinline__ int block_sum(int v, int& slot) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (tid == 0) slot = 0;
  __syncthreads();
  if ((tid & 63) == 0 && v) atomicAdd(&slot, v);
  __syncthreads();
  const int r = slot;
  __syncthreads();
  return r;
}

// descending bitonic sort of a[0..P), P a power of two, by the whole workgroup.  a is LDS, or (prune and summary kernels)
// LDS or the workgroup's own workspace slot; Index is the type the caller counts entries in.
template <int THREADS, typename Index>
__device__ __forceinline__ void bitonic_desc(unsigned long long* a, Index P) {
  for (Index size = 2; size <= P; size <<= 1)
    for (Index stride = size >> 1; stride > 0; stride >>= 1) {
      for (Index t = threadIdx.x; t < (P >> 1); t += THREADS) {
        const Index lo = 2 * t - (t & (stride - 1));
        const Index hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long x = a[lo], y = a[hi];
        if ((x < y) == desc) { a[lo] = y; a[hi] = x; }
      }
      __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ selection
struct SelectSmem {
  uint32_t hist[2048];
  int wcnt[2][SR_WAVES];
  int sh[4];                      // 0: count, 1: bin, 2: remaining
  int run[2];                     // ordered take: eq seen, taken so far
};

// Radix select over key(i), i in [0, n), key 0 = no candidate.  -> thr, need_eq, nsel (block-uniform): the top k are
// every key > thr and the first need_eq (lowest i) keys == thr; when at most k keys are non-zero, thr = 0 and all are.
template <typename KeyF>
__device__ void radix_select(KeyF key, long n, int k, SelectSmem& S, uint32_t& thr, int& need_eq, int& nsel) {
  const int tid = threadIdx.x;
  int local = 0;
  for (long i = tid; i < n; i += SR_THREADS) local += key(i) != 0u;
  const int npos = block_sum(local, S.sh[0]);
  if (npos <= k) { thr = 0u; need_eq = 0; nsel = npos; return; }
  uint32_t prefix = 0u, known = 0u;
  int remaining = k;
  const int shifts[3] = {21, 10, 0}, widths[3] = {11, 11, 10};
  for (int p = 0; p < 3; ++p) {
    const int shift = shifts[p];
    const uint32_t bm = (1u << widths[p]) - 1u;
    for (int i = tid; i < 2048; i += SR_THREADS) S.hist[i] = 0u;
    __syncthreads();
    for (long i = tid; i < n; i += SR_THREADS) {
      const uint32_t kk = key(i);
      if (kk != 0u && (kk & known) == prefix) atomicAdd(&S.hist[(kk >> shift) & bm], 1u);
    }
    __syncthreads();
    if (tid == 0) {                                          // walk the bins from the top
      int rem = remaining, b = (int)bm;
      for (; b > 0; --b) {
        const int c = (int)S.hist[b];
        if (c >= rem) break;
        rem -= c;
      }
      S.sh[1] = b;
      S.sh[2] = rem;
    }
    __syncthreads();
    prefix |= (uint32_t)S.sh[1] << shift;
    known |= bm << shift;
    remaining = S.sh[2];
    __syncthreads();
  }
  thr = prefix;
  need_eq = remaining;
  nsel = k;
}

// The selection of radix_select in index order: emit(i, pos) with pos = 0, 1, ... following i.
template <typename KeyF, typename EmitF>
__device__ void ordered_take(KeyF key, long n, uint32_t thr, int need_eq, SelectSmem& S, EmitF emit) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  if (tid == 0) { S.run[0] = 0; S.run[1] = 0; }
  __syncthreads();
  for (long base = 0; base < n; base += SR_THREADS) {
    const long i = base + tid;
    const uint32_t kk = i < n ? key(i) : 0u;
    const bool gt = kk > thr;
    const bool eq = thr != 0u && kk == thr;
    const unsigned long long mg = __ballot(gt), me = __ballot(eq);
    if (lane == 0) { S.wcnt[0][wave] = __popcll(mg); S.wcnt[1][wave] = __popcll(me); }
    __syncthreads();
    int E = S.run[0], T = S.run[1];
    for (int w = 0; w < wave; ++w) {
      T += S.wcnt[0][w] + min(max(need_eq - E, 0), S.wcnt[1][w]);
      E += S.wcnt[1][w];
    }
    const int eq_below = __popcll(me & below);
    const bool take = gt || (eq && E + eq_below < need_eq);
    if (take) emit(i, T + __popcll(mg & below) + min(max(need_eq - E, 0), eq_below));
    __syncthreads();
    if (tid == 0) {
      int e = S.run[0], t = S.run[1];
      for (int w = 0; w < SR_WAVES; ++w) {
        t += S.wcnt[0][w] + min(max(need_eq - e, 0), S.wcnt[1][w]);
        e += S.wcnt[1][w];
      }
      S.run[0] = e;
      S.run[1] = t;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ chunk stage
struct ChunkSmem {
  int64_t seg0[SR_TG], seg1[SR_TG];  // a term's postings inside the chunk: [seg0, seg1)
  float segw[SR_TG];                 // its query weight
};

// sc[d - c0] = s(q, d) for the n docs from c0 on, q the query row [qa, qb): the chunk's scores start at +0 and take
// fmaf(q_w, d_w, .) term by term in ascending term id, the ABI's chain, with a barrier between terms (a doc appears at
// most once per posting list, so no float atomics).  The chunk bounds of SR_TG terms are searched at once, the lower one
// by the first half of the workgroup and the upper one by the second.  Ends on a barrier.
__device__ __forceinline__ void accumulate_chunk(const int32_t* __restrict__ q_term, const float* __restrict__ q_w,
                                                 int64_t qa, int64_t qb, const int64_t* __restrict__ term_ptr,
                                                 const int32_t* __restrict__ post_doc, const float* __restrict__ post_w,
                                                 int32_t V, int c0, int n, float* sc, ChunkSmem& C) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += SR_THREADS) sc[i] = 0.f;
  for (int64_t g = qa; g < qb; g += SR_TG) {
    const int ng = (int)min((int64_t)SR_TG, qb - g);
    const int j = tid < SR_TG ? tid : tid - SR_TG;
    if (j < ng) {
      const int32_t term = q_term[g + j];
      int64_t lo = 0, hi = 0;
      if ((unsigned)term < (unsigned)V) { lo = term_ptr[term]; hi = term_ptr[term + 1]; }
      if (tid < SR_TG) {
        C.seg0[j] = lower_bound(post_doc, lo, hi, c0);
        C.segw[j] = q_w[g + j];
      } else {
        C.seg1[j] = lower_bound(post_doc, lo, hi, c0 + n);
      }
    }
    __syncthreads();                                         // (also orders the zero fill before the first term)
    for (int jj = 0; jj < ng; ++jj) {                        // ascending term id: the ABI's accumulation order
      const int64_t e = C.seg1[jj];
      const float w = C.segw[jj];
      for (int64_t i = C.seg0[jj] + tid; i < e; i += SR_THREADS) {
        const int d = post_doc[i] - c0;
        if ((unsigned)d < (unsigned)n) sc[d] = fmaf(w, post_w[i], sc[d]);
      }
      __syncthreads();
    }
  }
  __syncthreads();
}

// this thread's share of #{s_d > ts} + #{d < tt : s_d == ts} over the chunk: the docs ranked ahead of doc tt with score ts
__device__ __forceinline__ int count_ahead(const float* sc, int c0, int n, float ts, int tt) {
  int local = 0;
  for (int i = threadIdx.x; i < n; i += SR_THREADS) {
    const float s = sc[i];
    local += (s > ts) || (s == ts && c0 + i < tt);
  }
  return local;
}

// the chunk's top k under key(i), i in [0, n), as rank keys of doc c0 + i in doc order into out[0 ..), their number into
// *count
template <typename KeyF>
__device__ __forceinline__ void select_chunk(KeyF key, int c0, int n, int k, SelectSmem& S, unsigned long long* out,
                                             int32_t* count) {
  uint32_t thr;
  int need_eq, nsel;
  radix_select(key, n, k, S, thr, need_eq, nsel);
  ordered_take(key, n, thr, need_eq, S, [&](long i, int pos) { out[pos] = rank_key(key(i), (uint32_t)(c0 + (int)i)); });
  if (threadIdx.x == 0) *count = nsel;
}

// ------------------------------------------------------------------------------------------------ merge stage
// A query's candidate lists as the merge kernels read them: `cap` apart, each holding cnt[list] <= hi rank keys, under the
// flat index f = list * hi + i; past a list's count reads as 0, "no entry".  Called as a function it gives the score key.
struct RankLists {
  const unsigned long long* cand;
  const int32_t* cnt;
  int cap, hi;
  __device__ __forceinline__ unsigned long long at(long f) const {
    const int s = (int)(f / hi), i = (int)(f - (long)s * hi);
    return i < cnt[s] ? cand[(size_t)s * (size_t)cap + i] : 0ull;
  }
  __device__ __forceinline__ uint32_t operator()(long f) const { return rank_bits(at(f)); }
};

// the output tail of a merge kernel: ranks lo .. hi-1 of the nsel selected entries of sbuf, sorted descending, into query
// q's rows, the score decoded from its key by Score (bitsf: sparse scores are their bits; dense_unkey: the dense order
// key); unused slots 0 / -1; found, when asked for = the slots used
template <float (*Score)(uint32_t)>
__device__ __forceinline__ void write_ranks(const unsigned long long* sbuf, int nsel, int q, int lo, int hi,
                                            int32_t* __restrict__ out_doc, float* __restrict__ out_score,
                                            int32_t* __restrict__ out_found) {
  const int tid = threadIdx.x, w = hi - lo;
  int32_t* od = out_doc + (long)q * w;
  float* os = out_score + (long)q * w;
  for (int j = tid; j < w; j += SR_THREADS) {
    const int r = lo + j;
    if (r < nsel) {
      const unsigned long long e = sbuf[r];
      os[j] = Score(rank_bits(e));
      od[j] = rank_id(e);
    } else {
      os[j] = 0.f;
      od[j] = -1;
    }
  }
  if (out_found && tid == 0) out_found[q] = max(0, nsel - lo);
}

// The top hi of query q over its nlist lists, which follow each other in doc order and are in doc order inside (equal
// keys are met lowest doc first, which is what ordered_take's tie rule needs), sorted, ranks lo .. hi-1 written.
template <float (*Score)(uint32_t)>
__device__ __forceinline__ void merge_lists(const RankLists& lists, int nlist, SelectSmem& S, int q, int lo, int hi,
                                            int32_t* __restrict__ out_doc, float* __restrict__ out_score,
                                            int32_t* __restrict__ out_found) {
  __shared__ unsigned long long sbuf[SR_KMAX];               // rank keys: descending = the ABI's order
  const int tid = threadIdx.x;
  const long n = (long)nlist * hi;
  uint32_t thr;
  int need_eq, nsel;
  radix_select(lists, n, hi, S, thr, need_eq, nsel);
  const int P = pow2_at_least(nsel);
  for (int i = tid; i < P; i += SR_THREADS) sbuf[i] = 0ull;
  __syncthreads();
  ordered_take(lists, n, thr, need_eq, S, [&](long f, int pos) { sbuf[pos] = lists.at(f); });
  bitonic_desc<SR_THREADS, int>(sbuf, P);
  write_ranks<Score>(sbuf, nsel, q, lo, hi, out_doc, out_score, out_found);
}

}  // namespace
