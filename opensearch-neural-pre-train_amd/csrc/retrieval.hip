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
// From sparse_common.h: the chunk constants, lower_bound, the pair score (row_dot_lanes), block_sum, the chunk stage
// (accumulate_chunk, count_ahead, select_chunk over radix_select / ordered_take; qr_count_kernel of qrels.hip keeps a
// written-out copy of the first two, see there) and the merge stage (RankLists, merge_lists with its sort and output tail).  A kernel here keeps
// what only it does: its target-rank reduction, the band's exclusions and ceiling.  The candidates in the workspace are
// rank keys (score bits << 32 | ~doc), as the merge sorts them.
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
  __shared__ ChunkSmem C;
  const long qc = blockIdx.x;
  const int q = (int)(qc / nch), c = (int)(qc - (long)q * nch);
  const int c0 = c * chunk;
  const int n = max(0, min(chunk, nd - c0));
  accumulate_chunk(q_term, q_w, q_ptr[q], q_ptr[q + 1], term_ptr, post_doc, post_w, V, c0, n, sc, C);
  if (target) {                                            // the chunk's share of the target rank, summed by sr_merge_kernel
    const float ts = tscore[q];
    const int r = block_sum(ts > 0.f ? count_ahead(sc, c0, n, ts, target[q]) : 0, S.sh[0]);
    if (threadIdx.x == 0) rcount[qc] = r;
  }
  select_chunk([&](long i) -> uint32_t { return score_key(sc[i]); }, c0, n, k, S, cand + qc * k, ccount + qc);
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
  const int tid = threadIdx.x, q = blockIdx.x;
  const long base = (long)q * nch;
  if (target) {
    int local = 0;
    for (int c = tid; c < nch; c += SR_THREADS) local += rcount[base + c];
    const int r = block_sum(local, S.sh[0]);
    const int tt = target[q];
    if (tid == 0) out_rank[q] = ((unsigned)tt < (unsigned)nd && tscore[q] > 0.f) ? 1 + r : 0;
  }
  const RankLists lists = {cand + base * k, ccount + base, k, k};    // a chunk's k slots: doc order across and inside
  merge_lists<bitsf>(lists, nch, S, q, 0, k, out_doc, out_score, nullptr);
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
  __shared__ ChunkSmem C;
  const int tid = threadIdx.x;
  const long qc = blockIdx.x;
  const int q = (int)(qc / nch), c = (int)(qc - (long)q * nch);
  const int c0 = c * chunk;
  const int n = max(0, min(chunk, nd - c0));
  accumulate_chunk(q_term, q_w, q_ptr[q], q_ptr[q + 1], term_ptr, post_doc, post_w, V, c0, n, sc, C);
  if (ex_ptr) {                                            // the row's docs in [c0, c0 + n): one binary search per bound
    if (tid < 2) {                                         // (the staging words of the accumulation are free again)
      const int64_t a = ex_ptr[q], b = ex_ptr[q + 1];
      C.seg0[tid] = lower_bound(ex_doc, a, b, tid == 0 ? c0 : c0 + n);
    }
    __syncthreads();
    const int64_t e0 = C.seg0[0], e1 = C.seg0[1];
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
  select_chunk(key, c0, n, hi, S, cand + qc * hi, ccount + qc);
}

// Band search, merge stage: the top `hi` over the chunks' candidates as in sr_merge_kernel, ranks lo .. hi-1 written.
__global__ __launch_bounds__(SR_THREADS) void sb_merge_kernel(const unsigned long long* __restrict__ cand,
                                                              const int32_t* __restrict__ ccount, int32_t nch,
                                                              int32_t lo, int32_t hi, int32_t* __restrict__ out_doc,
                                                              float* __restrict__ out_score,
                                                              int32_t* __restrict__ out_found) {
  __shared__ SelectSmem S;
  const int q = blockIdx.x;
  const long base = (long)q * nch;
  const RankLists lists = {cand + base * hi, ccount + base, hi, hi};
  merge_lists<bitsf>(lists, nch, S, q, lo, hi, out_doc, out_score, out_found);
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
