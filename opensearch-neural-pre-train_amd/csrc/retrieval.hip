// Exact sparse retrieval for the mid-training evaluator (src/train/eval): the work the reference hands to an
// OpenSearch cluster (ref:benchmark/searchers.py:155-188, NeuralSparseSearcher) and scores with
// ref:benchmark/metrics.py:52-99.
//
// Index build (doc CSR -> term-major inverted index, every posting list in doc-id order), deterministic by construction:
//   docs are cut into nblk contiguous blocks; ix_count counts each (block, term) pair into C[nblk][V] (integer atomics:
//   the totals do not depend on arrival order); ix_colscan turns every column of C into an exclusive prefix over the
//   blocks and leaves the term totals in term_ptr; ix_scan makes term_ptr exclusive; ix_scatter walks the docs of a
//   block IN ORDER (one barrier per doc; a doc holds each term at most once, so no two lanes share a cursor within a
//   doc) and places doc d of term t at term_ptr[t] + C[b][t]++.  The result is the stable counting sort of the doc CSR
//   by term: byte-identical from run to run, no per-term sort needed.
//
// Search (term-at-a-time, exact): one workgroup per (query, chunk of `chunk` docs).  The chunk's fp32 scores live in LDS;
// for each query term, in ascending id order, the posting segment inside the chunk is found by binary search and
// s[d] = fmaf(q_w, d_w, s[d]) is applied to it, with a barrier between terms (a doc appears at most once per posting
// list, so no float atomics).  Every score is therefore fmaf over the shared terms in ascending term id starting from
// +0, the ABI's definition, whatever the chunking.  Then a radix select on the score bit patterns (scores >= 0, so the
// bits order like the floats; the trick of topk.hip) picks the chunk's top k under (score desc, doc asc), compacted in
// doc order, and an integer count gives the chunk's share of the target rank.  sr_merge reduces the chunks of a query
// the same way (its candidates are in doc order too) and sorts the <= k winners.  Chunk size changes no bit.
//
// From sparse_common.h: the chunk constants, lower_bound, the radix select and ordered take, block_sum, the pair score
// (row_dot_lanes) and the rank key.  The chunk accumulation (sr_chunk_kernel, sb_chunk_kernel; qr_count_kernel in
// qrels.hip) and the merge front (sr_merge_kernel, sb_merge_kernel) stay written out in their kernels: as functions they
// compile to other code, which would have to be timed against this one first.
#include "sparse_common.h"
#include "snx.h"

namespace {

constexpr int IX_THREADS = 256;
constexpr int IX_MAX_BLOCKS = 1024;
constexpr long IX_TABLE_BUDGET = 1L << 24;     // entries of the [nblk, V] cursor table (int64): <= 128 MiB
constexpr int SCAN_THREADS = 1024;

constexpr int TS_THREADS = 64;

// ------------------------------------------------------------------------------------------------ index build
inline int ix_blocks(int32_t nd, int32_t V) {
  if (nd <= 0) return 0;
  long nb = IX_TABLE_BUDGET / (V > 0 ? V : 1);
  if (nb > IX_MAX_BLOCKS) nb = IX_MAX_BLOCKS;
  if (nb < 1) nb = 1;
  if (nb > nd) nb = nd;
  const long dpb = (nd + nb - 1) / nb;
  return (int)((nd + dpb - 1) / dpb);
}

__global__ __launch_bounds__(IX_THREADS) void ix_count_kernel(const int64_t* __restrict__ doc_ptr,
                                                              const int32_t* __restrict__ doc_term, int32_t nd,
                                                              int32_t V, int64_t nnz, int32_t dpb,
                                                              unsigned long long* __restrict__ C) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d0 = b * dpb, d1 = min(nd, d0 + dpb);
  unsigned long long* row = C + (long)b * V;
  for (int d = d0 + wave; d < d1; d += IX_THREADS / 64) {
    const int64_t p0 = doc_ptr[d], p1 = min(doc_ptr[d + 1], nnz);
    for (int64_t j = p0 + lane; j < p1; j += 64) {
      const int t = doc_term[j];
      if ((unsigned)t < (unsigned)V) atomicAdd(&row[t], 1ull);
    }
  }
}

// per term: C[b][t] <- sum_{b' < b} C[b'][t]; term_ptr[t] <- sum_b C[b][t]
__global__ __launch_bounds__(IX_THREADS) void ix_colscan_kernel(unsigned long long* __restrict__ C, int nblk, int32_t V,
                                                                int64_t* __restrict__ term_ptr) {
  const int t = blockIdx.x * IX_THREADS + threadIdx.x;
  if (t >= V) return;
  unsigned long long acc = 0;
  for (int b = 0; b < nblk; ++b) {
    const unsigned long long c = C[(long)b * V + t];
    C[(long)b * V + t] = acc;
    acc += c;
  }
  term_ptr[t] = (int64_t)acc;
}

// term_ptr[0..V) counts -> exclusive offsets, term_ptr[V] = total (one workgroup; each thread owns a contiguous run)
__global__ __launch_bounds__(SCAN_THREADS) void ix_scan_kernel(int64_t* __restrict__ term_ptr, int32_t V) {
  __shared__ int64_t part[2][SCAN_THREADS];
  const int tid = threadIdx.x;
  const int per = (V + SCAN_THREADS - 1) / SCAN_THREADS;
  const int i0 = min(V, tid * per), i1 = min(V, i0 + per);
  int64_t s = 0;
  for (int i = i0; i < i1; ++i) s += term_ptr[i];
  part[0][tid] = s;
  __syncthreads();
  int cur = 0;
  for (int off = 1; off < SCAN_THREADS; off <<= 1) {        // inclusive Hillis-Steele scan over the thread sums
    const int64_t v = part[cur][tid] + (tid >= off ? part[cur][tid - off] : 0);
    part[cur ^ 1][tid] = v;
    cur ^= 1;
    __syncthreads();
  }
  int64_t run = part[cur][tid] - s;
  for (int i = i0; i < i1; ++i) {
    const int64_t c = term_ptr[i];
    term_ptr[i] = run;
    run += c;
  }
  if (tid == SCAN_THREADS - 1) term_ptr[V] = part[cur][tid];
}

__global__ __launch_bounds__(IX_THREADS) void ix_scatter_kernel(const int64_t* __restrict__ doc_ptr,
                                                                const int32_t* __restrict__ doc_term,
                                                                const float* __restrict__ doc_w, int32_t nd, int32_t V,
                                                                int64_t nnz, int32_t dpb, unsigned long long* C,
                                                                const int64_t* __restrict__ term_ptr,
                                                                int32_t* __restrict__ post_doc,
                                                                float* __restrict__ post_w) {
  const int b = blockIdx.x;
  const int d0 = b * dpb, d1 = min(nd, d0 + dpb);
  unsigned long long* row = C + (long)b * V;
  for (int d = d0; d < d1; ++d) {                            // docs in order: the stable part of the counting sort
    const int64_t p0 = doc_ptr[d], p1 = min(doc_ptr[d + 1], nnz);
    for (int64_t j = p0 + threadIdx.x; j < p1; j += IX_THREADS) {
      const int t = doc_term[j];
      if ((unsigned)t >= (unsigned)V) continue;
      const unsigned long long slot = row[t];
      row[t] = slot + 1;
      const int64_t pos = term_ptr[t] + (int64_t)slot;
      post_doc[pos] = d;
      post_w[pos] = doc_w[j];
    }
    __syncthreads();                                         // the next doc's cursor reads see this doc's increments
  }
}

// ------------------------------------------------------------------------------------------------ search
__device__ __forceinline__ uint32_t score_key(float s) { return s > 0.f ? fbits(s) : 0u; }

// s(q, target[q]) by row_dot_lanes: fmaf in ascending term id, the order of the LDS accumulation, so the value is
// bit-equal to the ranked one.
__global__ __launch_bounds__(TS_THREADS) void sr_target_kernel(const int64_t* __restrict__ q_ptr,
                                                               const int32_t* __restrict__ q_term,
                                                               const float* __restrict__ q_w,
                                                               const int64_t* __restrict__ doc_ptr,
                                                               const int32_t* __restrict__ doc_term,
                                                               const float* __restrict__ doc_w, int32_t nd,
                                                               const int32_t* __restrict__ target,
                                                               float* __restrict__ out_tscore) {
  const int q = blockIdx.x, t = target[q];
  float acc = 0.f;
  if ((unsigned)t < (unsigned)nd)
    acc = row_dot_lanes<TS_THREADS>(q_term, q_w, q_ptr[q], q_ptr[q + 1], doc_term, doc_w, doc_ptr[t], doc_ptr[t + 1]);
  if (threadIdx.x == 0) out_tscore[q] = acc;
}

__global__ __launch_bounds__(SR_THREADS) void sr_chunk_kernel(const int64_t* __restrict__ q_ptr,
                                                              const int32_t* __restrict__ q_term,
                                                              const float* __restrict__ q_w,
                                                              const int64_t* __restrict__ term_ptr,
                                                              const int32_t* __restrict__ post_doc,
                                                              const float* __restrict__ post_w, int32_t nd, int32_t V,
                                                              int32_t chunk, int32_t nch, int32_t k,
                                                              const int32_t* __restrict__ target,
                                                              const float* __restrict__ tscore,
                                                              unsigned long long* __restrict__ cand,
                                                              int32_t* __restrict__ ccount,
                                                              int32_t* __restrict__ rcount) {
  extern __shared__ float sc[];                            // [chunk] scores of this chunk's docs
  __shared__ SelectSmem S;
  __shared__ int64_t seg0[SR_TG], seg1[SR_TG];
  __shared__ float segw[SR_TG];
  const int tid = threadIdx.x;
  const long qc = blockIdx.x;
  const int q = (int)(qc / nch), c = (int)(qc - (long)q * nch);
  const int c0 = c * chunk;
  const int n = max(0, min(chunk, nd - c0));
  for (int i = tid; i < n; i += SR_THREADS) sc[i] = 0.f;
  const int64_t qa = q_ptr[q], qb = q_ptr[q + 1];
  for (int64_t g = qa; g < qb; g += SR_TG) {
    const int ng = (int)min((int64_t)SR_TG, qb - g);
    const int j = tid < SR_TG ? tid : tid - SR_TG;
    if (j < ng) {                                          // both bounds of every term of the group at once
      const int32_t term = q_term[g + j];
      int64_t lo = 0, hi = 0;
      if ((unsigned)term < (unsigned)V) { lo = term_ptr[term]; hi = term_ptr[term + 1]; }
      if (tid < SR_TG) {
        seg0[j] = lower_bound(post_doc, lo, hi, c0);
        segw[j] = q_w[g + j];
      } else {
        seg1[j] = lower_bound(post_doc, lo, hi, c0 + n);
      }
    }
    __syncthreads();                                       // (also orders the zero fill before the first term)
    for (int jj = 0; jj < ng; ++jj) {                      // ascending term id: the ABI's accumulation order
      const int64_t e = seg1[jj];
      const float w = segw[jj];
      for (int64_t i = seg0[jj] + tid; i < e; i += SR_THREADS) {
        const int d = post_doc[i] - c0;
        if ((unsigned)d < (unsigned)n) sc[d] = fmaf(w, post_w[i], sc[d]);
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (target) {                                            // 1 + #{s_d > s_t} + #{d < t: s_d == s_t}, summed by sr_merge
    const float ts = tscore[q];
    const int tt = target[q];
    int local = 0;
    if (ts > 0.f)
      for (int i = tid; i < n; i += SR_THREADS) {
        const float s = sc[i];
        local += (s > ts) || (s == ts && c0 + i < tt);
      }
    const int r = block_sum(local, S.sh[0]);
    if (tid == 0) rcount[qc] = r;
  }
  auto key = [&](long i) -> uint32_t { return score_key(sc[i]); };
  uint32_t thr;
  int need_eq, nsel;
  radix_select(key, n, k, S, thr, need_eq, nsel);
  unsigned long long* out = cand + qc * k;
  ordered_take(key, n, thr, need_eq, S, [&](long i, int pos) {
    out[pos] = ((unsigned long long)score_key(sc[i]) << 32) | (uint32_t)(c0 + (int)i);
  });
  if (tid == 0) ccount[qc] = nsel;
}

__global__ __launch_bounds__(SR_THREADS) void sr_merge_kernel(const unsigned long long* __restrict__ cand,
                                                              const int32_t* __restrict__ ccount,
                                                              const int32_t* __restrict__ rcount, int32_t nd,
                                                              int32_t nch, int32_t k,
                                                              const int32_t* __restrict__ target,
                                                              const float* __restrict__ tscore,
                                                              int32_t* __restrict__ out_doc,
                                                              float* __restrict__ out_score,
                                                              int32_t* __restrict__ out_rank) {
  __shared__ SelectSmem S;
  __shared__ unsigned long long sbuf[SR_KMAX];              // (score bits << 32 | ~doc): descending = the ABI's order
  const int tid = threadIdx.x, q = blockIdx.x;
  const long base = (long)q * nch;
  if (target) {
    int local = 0;
    for (int c = tid; c < nch; c += SR_THREADS) local += rcount[base + c];
    const int r = block_sum(local, S.sh[0]);
    const int tt = target[q];
    if (tid == 0) out_rank[q] = ((unsigned)tt < (unsigned)nd && tscore[q] > 0.f) ? 1 + r : 0;
  }
  const unsigned long long* qcand = cand + base * k;
  const int32_t* qcnt = ccount + base;
  auto key = [&](long f) -> uint32_t {                      // flat index c * k + i: doc order among the valid entries
    const int c = (int)(f / k), i = (int)(f - (long)c * k);
    return i < qcnt[c] ? (uint32_t)(qcand[f] >> 32) : 0u;
  };
  const long n = (long)nch * k;
  uint32_t thr;
  int need_eq, nsel;
  radix_select(key, n, k, S, thr, need_eq, nsel);
  const int P = pow2_at_least(nsel);
  for (int i = tid; i < P; i += SR_THREADS) sbuf[i] = 0ull;
  __syncthreads();
  ordered_take(key, n, thr, need_eq, S, [&](long f, int pos) {
    const unsigned long long e = qcand[f];
    sbuf[pos] = rank_key((uint32_t)(e >> 32), (uint32_t)e);
  });
  for (int size = 2; size <= P; size <<= 1)                 // bitonic sort, descending; written out (see sparse_common.h, bitonic_desc)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (P >> 1); t += SR_THREADS) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long a = sbuf[lo], b = sbuf[hi];
        if ((a < b) == desc) { sbuf[lo] = b; sbuf[hi] = a; }
      }
      __syncthreads();
    }
  int32_t* od = out_doc + (long)q * k;
  float* os = out_score + (long)q * k;
  for (int i = tid; i < k; i += SR_THREADS) {
    if (i < nsel) {
      const unsigned long long e = sbuf[i];
      os[i] = bitsf(rank_bits(e));
      od[i] = rank_id(e);
    } else {
      os[i] = 0.f;
      od[i] = -1;
    }
  }
}

// s(q, d) of a list of (query, doc) pairs: sr_target_kernel with one pair per workgroup instead of one target per query.
// A pair whose query or doc index is out of range scores 0.
__global__ __launch_bounds__(TS_THREADS) void sr_pair_kernel(const int64_t* __restrict__ q_ptr,
                                                             const int32_t* __restrict__ q_term,
                                                             const float* __restrict__ q_w, int32_t nq,
                                                             const int64_t* __restrict__ doc_ptr,
                                                             const int32_t* __restrict__ doc_term,
                                                             const float* __restrict__ doc_w, int32_t nd,
                                                             const int32_t* __restrict__ pair_q,
                                                             const int32_t* __restrict__ pair_d,
                                                             float* __restrict__ out) {
  const long p = blockIdx.x;
  const int q = pair_q[p], t = pair_d[p];
  float acc = 0.f;
  if ((unsigned)q < (unsigned)nq && (unsigned)t < (unsigned)nd)
    acc = row_dot_lanes<TS_THREADS>(q_term, q_w, q_ptr[q], q_ptr[q + 1], doc_term, doc_w, doc_ptr[t], doc_ptr[t + 1]);
  if (threadIdx.x == 0) out[p] = acc;
}

// Band search, chunk stage: the LDS accumulation of sr_chunk_kernel, then the query's excluded docs inside the chunk (a
// binary search of the ascending exclusion row for the chunk's doc range) are zeroed, and a score that is not below the
// query's ceiling gets key 0.  Key 0 is "no candidate" to radix_select, so the chunk keeps its top `hi` ADMISSIBLE docs.
__global__ __launch_bounds__(SR_THREADS) void sb_chunk_kernel(const int64_t* __restrict__ q_ptr,
                                                              const int32_t* __restrict__ q_term,
                                                              const float* __restrict__ q_w,
                                                              const int64_t* __restrict__ term_ptr,
                                                              const int32_t* __restrict__ post_doc,
                                                              const float* __restrict__ post_w, int32_t nd, int32_t V,
                                                              int32_t chunk, int32_t nch, int32_t hi,
                                                              const int64_t* __restrict__ ex_ptr,
                                                              const int32_t* __restrict__ ex_doc,
                                                              const float* __restrict__ ceiling,
                                                              unsigned long long* __restrict__ cand,
                                                              int32_t* __restrict__ ccount) {
  extern __shared__ float sc[];
  __shared__ SelectSmem S;
  __shared__ int64_t seg0[SR_TG], seg1[SR_TG];
  __shared__ float segw[SR_TG];
  const int tid = threadIdx.x;
  const long qc = blockIdx.x;
  const int q = (int)(qc / nch), c = (int)(qc - (long)q * nch);
  const int c0 = c * chunk;
  const int n = max(0, min(chunk, nd - c0));
  for (int i = tid; i < n; i += SR_THREADS) sc[i] = 0.f;
  const int64_t qa = q_ptr[q], qb = q_ptr[q + 1];
  for (int64_t g = qa; g < qb; g += SR_TG) {
    const int ng = (int)min((int64_t)SR_TG, qb - g);
    const int j = tid < SR_TG ? tid : tid - SR_TG;
    if (j < ng) {
      const int32_t term = q_term[g + j];
      int64_t lo = 0, hi2 = 0;
      if ((unsigned)term < (unsigned)V) { lo = term_ptr[term]; hi2 = term_ptr[term + 1]; }
      if (tid < SR_TG) {
        seg0[j] = lower_bound(post_doc, lo, hi2, c0);
        segw[j] = q_w[g + j];
      } else {
        seg1[j] = lower_bound(post_doc, lo, hi2, c0 + n);
      }
    }
    __syncthreads();
    for (int jj = 0; jj < ng; ++jj) {                      // ascending term id: the ABI's accumulation order
      const int64_t e = seg1[jj];
      const float w = segw[jj];
      for (int64_t i = seg0[jj] + tid; i < e; i += SR_THREADS) {
        const int d = post_doc[i] - c0;
        if ((unsigned)d < (unsigned)n) sc[d] = fmaf(w, post_w[i], sc[d]);
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (ex_ptr) {                                            // the row's docs in [c0, c0 + n): one binary search per bound
    if (tid < 2) {
      const int64_t a = ex_ptr[q], b = ex_ptr[q + 1];
      seg0[tid] = lower_bound(ex_doc, a, b, tid == 0 ? c0 : c0 + n);
    }
    __syncthreads();
    const int64_t e0 = seg0[0], e1 = seg0[1];
    for (int64_t i = e0 + tid; i < e1; i += SR_THREADS) {
      const int d = ex_doc[i] - c0;
      if ((unsigned)d < (unsigned)n) sc[d] = 0.f;
    }
    __syncthreads();
  }
  const float ceil_q = ceiling ? ceiling[q] : __builtin_huge_valf();
  auto key = [&](long i) -> uint32_t {
    const float s = sc[i];
    return s < ceil_q ? score_key(s) : 0u;                 // a NaN ceiling admits nothing
  };
  uint32_t thr;
  int need_eq, nsel;
  radix_select(key, n, hi, S, thr, need_eq, nsel);
  unsigned long long* out = cand + qc * hi;
  ordered_take(key, n, thr, need_eq, S, [&](long i, int pos) {
    out[pos] = ((unsigned long long)score_key(sc[i]) << 32) | (uint32_t)(c0 + (int)i);
  });
  if (tid == 0) ccount[qc] = nsel;
}

// Band search, merge stage: sr_merge_kernel's selection of the top `hi` over the chunks' candidates, then ranks
// lo .. hi-1 are written.
__global__ __launch_bounds__(SR_THREADS) void sb_merge_kernel(const unsigned long long* __restrict__ cand,
                                                              const int32_t* __restrict__ ccount, int32_t nch,
                                                              int32_t lo, int32_t hi, int32_t* __restrict__ out_doc,
                                                              float* __restrict__ out_score,
                                                              int32_t* __restrict__ out_found) {
  __shared__ SelectSmem S;
  __shared__ unsigned long long sbuf[SR_KMAX];
  const int tid = threadIdx.x, q = blockIdx.x;
  const long base = (long)q * nch;
  const unsigned long long* qcand = cand + base * hi;
  const int32_t* qcnt = ccount + base;
  auto key = [&](long f) -> uint32_t {
    const int c = (int)(f / hi), i = (int)(f - (long)c * hi);
    return i < qcnt[c] ? (uint32_t)(qcand[f] >> 32) : 0u;
  };
  const long n = (long)nch * hi;
  uint32_t thr;
  int need_eq, nsel;
  radix_select(key, n, hi, S, thr, need_eq, nsel);
  const int P = pow2_at_least(nsel);
  for (int i = tid; i < P; i += SR_THREADS) sbuf[i] = 0ull;
  __syncthreads();
  ordered_take(key, n, thr, need_eq, S, [&](long f, int pos) {
    const unsigned long long e = qcand[f];
    sbuf[pos] = rank_key((uint32_t)(e >> 32), (uint32_t)e);
  });
  for (int size = 2; size <= P; size <<= 1)                 // the sort of sr_merge_kernel
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < (P >> 1); t += SR_THREADS) {
        const int a0 = 2 * t - (t & (stride - 1));
        const int a1 = a0 + stride;
        const bool desc = (a0 & size) == 0;
        const unsigned long long a = sbuf[a0], b = sbuf[a1];
        if ((a < b) == desc) { sbuf[a0] = b; sbuf[a1] = a; }
      }
      __syncthreads();
    }
  const int w = hi - lo;
  int32_t* od = out_doc + (long)q * w;
  float* os = out_score + (long)q * w;
  for (int j = tid; j < w; j += SR_THREADS) {
    const int r = lo + j;
    if (r < nsel) {
      const unsigned long long e = sbuf[r];
      os[j] = bitsf(rank_bits(e));
      od[j] = rank_id(e);
    } else {
      os[j] = 0.f;
      od[j] = -1;
    }
  }
  if (tid == 0) out_found[q] = max(0, nsel - lo);
}

}  // namespace

extern "C" size_t snx_sparse_index_workspace_bytes(int32_t nd, int32_t V) {
  if (nd < 0 || V <= 0) return 0;
  return (size_t)ix_blocks(nd, V) * (size_t)V * sizeof(unsigned long long);
}

extern "C" int snx_sparse_index_build(const int64_t* doc_ptr, const int32_t* doc_term, const float* doc_w, int32_t nd,
                                      int32_t V, int64_t nnz, int64_t* term_ptr, int32_t* post_doc, float* post_w,
                                      void* workspace, size_t ws_bytes, hipStream_t st) {
  if (!doc_ptr || !term_ptr) return SNX_E_ARG;
  if (nd < 0 || V <= 0 || nnz < 0) return SNX_E_SHAPE;
  if (nnz > 0 && (!doc_term || !doc_w || !post_doc || !post_w)) return SNX_E_ARG;
  const int nblk = ix_blocks(nd, V);
  const size_t need = (size_t)nblk * (size_t)V * sizeof(unsigned long long);
  if (need && (!workspace || ws_bytes < need)) return SNX_E_ARG;
  if (nblk == 0 || nnz == 0) {                              // no postings: all-zero offsets
    if (hipMemsetAsync(term_ptr, 0, (size_t)(V + 1) * sizeof(int64_t), st) != hipSuccess) return SNX_E_ARG;
    return SNX_OK;
  }
  const int dpb = (int)((nd + (long)nblk - 1) / nblk);
  unsigned long long* C = (unsigned long long*)workspace;
  const hipError_t e = hipMemsetAsync(C, 0, need, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(ix_count_kernel, dim3(nblk), dim3(IX_THREADS), 0, st, doc_ptr, doc_term, nd, V, nnz, dpb, C);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(ix_colscan_kernel, dim3(cdiv(V, IX_THREADS)), dim3(IX_THREADS), 0, st, C, nblk, V, term_ptr);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(ix_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, term_ptr, V);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(ix_scatter_kernel, dim3(nblk), dim3(IX_THREADS), 0, st, doc_ptr, doc_term, doc_w, nd, V, nnz, dpb,
                     C, (const int64_t*)term_ptr, post_doc, post_w);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" size_t snx_sparse_search_workspace_bytes(int32_t nq, int32_t nd, int32_t k, int32_t chunk_docs) {
  if (nq <= 0 || nd < 0 || k <= 0 || chunk_docs < 0) return 0;
  const size_t blocks = (size_t)nq * (size_t)sr_nch(nd, sr_chunk(chunk_docs));
  return align256(blocks * (size_t)k * 8) + 2 * align256(blocks * 4);
}

extern "C" int snx_sparse_search(const int64_t* q_ptr, const int32_t* q_term, const float* q_w, int32_t nq,
                                 const int64_t* term_ptr, const int32_t* post_doc, const float* post_w,
                                 const int64_t* doc_ptr, const int32_t* doc_term, const float* doc_w, int32_t nd,
                                 int32_t V, const int32_t* target, int32_t k, int32_t chunk_docs, int32_t* out_doc,
                                 float* out_score, int32_t* out_rank, float* out_tscore, void* workspace,
                                 size_t ws_bytes, hipStream_t st) {
  if (!q_ptr || !term_ptr || !doc_ptr || !out_doc || !out_score) return SNX_E_ARG;
  if (target && (!out_rank || !out_tscore)) return SNX_E_ARG;
  if (nq < 0 || nd < 0 || V <= 0 || k < 1 || k > SR_KMAX || chunk_docs < 0 || chunk_docs > SR_CHUNK_MAX)
    return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  const int chunk = sr_chunk(chunk_docs);
  const int nch = sr_nch(nd, chunk);
  const long blocks = (long)nq * nch;
  if (blocks > (1L << 31) / SR_THREADS) return SNX_E_SHAPE;       // one launch of the chunk grid
  const size_t need = snx_sparse_search_workspace_bytes(nq, nd, k, chunk_docs);
  if (!workspace || ws_bytes < need) return SNX_E_ARG;
  char* w = (char*)workspace;
  unsigned long long* cand = (unsigned long long*)w;
  int32_t* ccount = (int32_t*)(w + align256((size_t)blocks * k * 8));
  int32_t* rcount = (int32_t*)((char*)ccount + align256((size_t)blocks * 4));
  if (target) {
    hipLaunchKernelGGL(sr_target_kernel, dim3(nq), dim3(TS_THREADS), 0, st, q_ptr, q_term, q_w, doc_ptr, doc_term,
                       doc_w, nd, target, out_tscore);
    SNX_CHECK_LAUNCH();
  }
  const size_t lds = (size_t)chunk * sizeof(float);
  if (lds > 48 * 1024) {
    static LdsOptIn optin;
    if (const int rc = optin.ensure((const void*)sr_chunk_kernel, SR_CHUNK_MAX * (int)sizeof(float))) return rc;
  }
  hipLaunchKernelGGL(sr_chunk_kernel, dim3((unsigned)blocks), dim3(SR_THREADS), lds, st, q_ptr, q_term, q_w, term_ptr,
                     post_doc, post_w, nd, V, chunk, nch, k, target, (const float*)out_tscore, cand, ccount, rcount);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(sr_merge_kernel, dim3(nq), dim3(SR_THREADS), 0, st, (const unsigned long long*)cand,
                     (const int32_t*)ccount, (const int32_t*)rcount, nd, nch, k, target, (const float*)out_tscore,
                     out_doc, out_score, out_rank);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}


extern "C" int snx_sparse_pair_scores(const int64_t* q_ptr, const int32_t* q_term, const float* q_w, int32_t nq,
                                      const int64_t* doc_ptr, const int32_t* doc_term, const float* doc_w, int32_t nd,
                                      const int32_t* pair_q, const int32_t* pair_d, int64_t npairs, float* out,
                                      hipStream_t st) {
  if (!q_ptr || !doc_ptr) return SNX_E_ARG;
  if (nq < 0 || nd < 0 || npairs < 0 || npairs > 0x7FFFFFFFL) return SNX_E_SHAPE;
  if (npairs == 0) return SNX_OK;
  if (!pair_q || !pair_d || !out) return SNX_E_ARG;
  hipLaunchKernelGGL(sr_pair_kernel, dim3((unsigned)npairs), dim3(TS_THREADS), 0, st, q_ptr, q_term, q_w, nq, doc_ptr,
                     doc_term, doc_w, nd, pair_q, pair_d, out);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" size_t snx_sparse_search_band_workspace_bytes(int32_t nq, int32_t nd, int32_t hi, int32_t chunk_docs) {
  if (nq <= 0 || nd < 0 || hi <= 0 || chunk_docs < 0) return 0;
  const size_t blocks = (size_t)nq * (size_t)sr_nch(nd, sr_chunk(chunk_docs));
  return align256(blocks * (size_t)hi * 8) + align256(blocks * 4);
}

extern "C" int snx_sparse_search_band(const int64_t* q_ptr, const int32_t* q_term, const float* q_w, int32_t nq,
                                      const int64_t* term_ptr, const int32_t* post_doc, const float* post_w,
                                      int32_t nd, int32_t V, const int64_t* ex_ptr, const int32_t* ex_doc,
                                      const float* ceiling, int32_t lo, int32_t hi, int32_t chunk_docs,
                                      int32_t* out_doc, float* out_score, int32_t* out_found, void* workspace,
                                      size_t ws_bytes, hipStream_t st) {
  if (!q_ptr || !term_ptr || !out_doc || !out_score || !out_found) return SNX_E_ARG;
  if (ex_ptr && !ex_doc) return SNX_E_ARG;
  if (nq < 0 || nd < 0 || V <= 0 || lo < 0 || hi <= lo || hi > SR_KMAX || chunk_docs < 0 ||
      chunk_docs > SR_CHUNK_MAX)
    return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  const int chunk = sr_chunk(chunk_docs);
  const int nch = sr_nch(nd, chunk);
  const long blocks = (long)nq * nch;
  if (blocks > (1L << 31) / SR_THREADS) return SNX_E_SHAPE;
  const size_t need = snx_sparse_search_band_workspace_bytes(nq, nd, hi, chunk_docs);
  if (!workspace || ws_bytes < need) return SNX_E_ARG;
  char* w = (char*)workspace;
  unsigned long long* cand = (unsigned long long*)w;
  int32_t* ccount = (int32_t*)(w + align256((size_t)blocks * hi * 8));
  const size_t lds = (size_t)chunk * sizeof(float);
  if (lds > 48 * 1024) {
    static LdsOptIn optin;
    if (const int rc = optin.ensure((const void*)sb_chunk_kernel, SR_CHUNK_MAX * (int)sizeof(float))) return rc;
  }
  hipLaunchKernelGGL(sb_chunk_kernel, dim3((unsigned)blocks), dim3(SR_THREADS), lds, st, q_ptr, q_term, q_w, term_ptr,
                     post_doc, post_w, nd, V, chunk, nch, hi, ex_ptr, ex_doc, ceiling, cand, ccount);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(sb_merge_kernel, dim3(nq), dim3(SR_THREADS), 0, st, (const unsigned long long*)cand,
                     (const int32_t*)ccount, nch, lo, hi, out_doc, out_score, out_found);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
