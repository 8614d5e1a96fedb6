// Relevance judgments (include/snx.h "relevance judgments"): scoring retrieval against qrels, the protocol behind the
// reference's headline numbers (ref:benchmark/hf_runner.py:191-215 takes the first retrieved doc that is in the query's
// relevant SET; ref:benchmark/metrics.py:180-215 resamples the per-query values 1000 times).  The reference walks Python
// lists per query and rebuilds a list per resample; here the judgments are a CSR on the device next to the index.
//
//   qr_best_kernel      one workgroup per query, one thread per relevant doc of its row: s(q, d) by row_dot_search (the
//                       fmaf chain of the exact search, so the value is bit-equal to the ranked one), then a workgroup
//                       maximum of the rank key: highest score, ties lowest doc id.
//   qr_count_kernel     one workgroup per (query, chunk of docs): the LDS score accumulation of retrieval.hip's
//                       sr_chunk_kernel (same constants, sparse_common.h) and its integer count of the docs in front of
//                       the best relevant doc.  No selection pass: one accumulation per query whatever the row length.
//                       Written out here, not accumulate_chunk / count_ahead / block_sum of sparse_common.h: with them
//                       first_relevant measured up to 1.4 % over the parent against a margin of 1.0 %
//                       (profiles/sparse_chunk_merge_refactor.txt).  A change to that accumulation is made here too.
//   qr_rank_kernel      adds the chunks' counts of a query (integers: the chunking changes no bit).
//   qr_ranked_kernel    one wave per ranked list, 64 positions at a time: every lane tests its entry by binary search in
//                       the sorted row, a ballot puts the hits in position order, and the wave walks the set bits: one
//                       running float64 sum, read off at every cutoff, is the left fold of each cutoff.
//   qr_boot_kernel      one workgroup per resample.  Thread j folds segment j of SNX_BOOTSTRAP_SEGMENT indices from +0.0
//                       in ascending order into LDS; thread m then folds the segment sums of column m in ascending
//                       segment order.  The order is a function of n alone.
#include <math.h>

#include "sparse_common.h"
#include "snx.h"

namespace {

constexpr int QB_THREADS = 256;
constexpr int QR_THREADS = 256;
constexpr int QR_WAVES = QR_THREADS / 64;
constexpr int QR_RMAX = 4096;
constexpr int QR_CUTS = 8;
constexpr int BT_THREADS = 256;
constexpr int BT_MMAX = 16;
constexpr int BT_SEG = SNX_BOOTSTRAP_SEGMENT;

// ------------------------------------------------------------------------------------------------ first relevant
__global__ __launch_bounds__(QB_THREADS) void qr_best_kernel(
    const int64_t* __restrict__ q_ptr, const int32_t* __restrict__ q_term, const float* __restrict__ q_w,
    const int64_t* __restrict__ doc_ptr, const int32_t* __restrict__ doc_term, const float* __restrict__ doc_w, int32_t nd,
    const int64_t* __restrict__ rel_ptr, const int32_t* __restrict__ rel_doc, int32_t* __restrict__ out_doc,
    float* __restrict__ out_score, int32_t* __restrict__ out_nrel) {
  __shared__ unsigned long long wbest[QB_THREADS / 64];
  __shared__ int wcnt[QB_THREADS / 64];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int64_t qa = q_ptr[q], qb = q_ptr[q + 1];
  const int64_t ra = rel_ptr[q], rb = rel_ptr[q + 1];
  unsigned long long best = 0ull;                            // 0: no relevant doc with a positive score
  int cnt = 0;
  for (int64_t r = ra + tid; r < rb; r += QB_THREADS) {
    const int d = rel_doc[r];
    if ((unsigned)d >= (unsigned)nd) continue;               // skipped, never read through
    ++cnt;
    const int64_t a = doc_ptr[d], b = doc_ptr[d + 1];
    const float acc = row_dot_search(q_term, q_w, qa, qb, doc_term, doc_w, a, b);
    if (acc > 0.f) {
      const unsigned long long key = rank_key(fbits(acc), (uint32_t)d);
      if (key > best) best = key;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, 64);
    if (other > best) best = other;
    cnt += __shfl_xor(cnt, o, 64);
  }
  if ((tid & 63) == 0) { wbest[tid >> 6] = best; wcnt[tid >> 6] = cnt; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < QB_THREADS / 64; ++w) {
      if (wbest[w] > best) best = wbest[w];
      cnt += wcnt[w];
    }
    out_nrel[q] = cnt;
    if (best != 0ull) {
      out_doc[q] = rank_id(best);
      out_score[q] = bitsf(rank_bits(best));
    } else {
      out_doc[q] = -1;
      out_score[q] = 0.f;
    }
  }
}

__global__ __launch_bounds__(SR_THREADS) void qr_count_kernel(
    const int64_t* __restrict__ q_ptr, const int32_t* __restrict__ q_term, const float* __restrict__ q_w,
    const int64_t* __restrict__ term_ptr, const int32_t* __restrict__ post_doc, const float* __restrict__ post_w, int32_t nd,
    int32_t V, int32_t chunk, int32_t nch, const int32_t* __restrict__ best_doc, const float* __restrict__ best_score,
    int32_t* __restrict__ rcount) {
  extern __shared__ float sc[];                              // [chunk] scores of this chunk's docs
  __shared__ int64_t seg0[SR_TG], seg1[SR_TG];
  __shared__ float segw[SR_TG];
  __shared__ int wsum[SR_WAVES];
  const int tid = threadIdx.x;
  const long qc = blockIdx.x;
  const int q = (int)(qc / nch), c = (int)(qc - (long)q * nch);
  const float ts = best_score[q];
  if (!(ts > 0.f)) {                                         // block-uniform: no relevant doc scores, the rank is 0
    if (tid == 0) rcount[qc] = 0;
    return;
  }
  const int tt = best_doc[q];
  const int c0 = c * chunk;
  const int n = max(0, min(chunk, nd - c0));
  for (int i = tid; i < n; i += SR_THREADS) sc[i] = 0.f;
  const int64_t qa = q_ptr[q], qb = q_ptr[q + 1];
  for (int64_t g = qa; g < qb; g += SR_TG) {
    const int ng = (int)min((int64_t)SR_TG, qb - g);
    const int j = tid < SR_TG ? tid : tid - SR_TG;
    if (j < ng) {                                            // both bounds of every term of the group at once
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
    __syncthreads();                                         // (also orders the zero fill before the first term)
    for (int jj = 0; jj < ng; ++jj) {                        // ascending term id: the ABI's accumulation order
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
  int local = 0;                                             // #{s_d > s*} + #{d < d*: s_d == s*} inside the chunk
  for (int i = tid; i < n; i += SR_THREADS) {
    const float s = sc[i];
    local += (s > ts) || (s == ts && c0 + i < tt);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o, 64);
  if ((tid & 63) == 0) wsum[tid >> 6] = local;
  __syncthreads();
  if (tid == 0) {
    int r = 0;
    for (int w = 0; w < SR_WAVES; ++w) r += wsum[w];
    rcount[qc] = r;
  }
}

__global__ __launch_bounds__(64) void qr_rank_kernel(const int32_t* __restrict__ rcount, int32_t nq, int32_t nch,
                                                     const float* __restrict__ best_score,
                                                     int32_t* __restrict__ out_rank) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= nq) return;
  int r = 0;
  for (int c = 0; c < nch; ++c) r += rcount[(long)q * nch + c];
  out_rank[q] = best_score[q] > 0.f ? 1 + r : 0;
}

// ------------------------------------------------------------------------------------------------ ranked lists
struct Cutoffs {
  int32_t n;
  int32_t at[QR_CUTS];
};

__global__ __launch_bounds__(QR_THREADS) void qr_ranked_kernel(
    const int32_t* __restrict__ docs, int32_t nq, int32_t R, int32_t nd, const int64_t* __restrict__ rel_ptr,
    const int32_t* __restrict__ rel_doc, Cutoffs cuts, const double* __restrict__ disc, int32_t* __restrict__ out_first,
    int32_t* __restrict__ out_hits, double* __restrict__ out_dcg) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * QR_WAVES + (threadIdx.x >> 6);
  if (q >= nq) return;                                       // wave-uniform
  const int32_t* row = docs + (int64_t)q * R;
  const int64_t ra = rel_ptr[q], rb = rel_ptr[q + 1];
  const int last = cuts.at[cuts.n - 1];                      // positions behind the last cutoff only matter to `first`
  int first = 0, hits = 0, next = 0;
  double acc = 0.0;
  bool ended = false;
  for (int base = 0; base < R && !ended; base += 64) {
    const int i = base + lane;
    const int d = i < R ? row[i] : -1;
    bool rel = false;
    if ((unsigned)d < (unsigned)nd) {
      const int64_t p = lower_bound(rel_doc, ra, rb, (int32_t)d);
      rel = p < rb && rel_doc[p] == d;
    }
    const unsigned long long neg = __ballot(d < 0);          // the list ends at its first negative id
    unsigned long long m = __ballot(rel);
    if (neg) {
      m &= (neg & (0ull - neg)) - 1ull;                      // the lanes in front of the first negative one
      ended = true;
    }
    while (m) {                                              // wave-uniform walk of the hits in position order
      const int p = base + __builtin_ctzll(m) + 1;           // 1-based position
      m &= m - 1ull;
      if (first == 0) first = p;
      if (p > last) { ended = true; break; }
      while (next < cuts.n && p > cuts.at[next]) {           // the fold of cutoff `next` is complete
        if (lane == 0) {
          out_hits[(int64_t)q * cuts.n + next] = hits;
          out_dcg[(int64_t)q * cuts.n + next] = acc;
        }
        ++next;
      }
      ++hits;
      acc = acc + disc[p - 1];
    }
    if (first != 0 && base + 64 >= last) ended = true;
  }
  if (lane == 0) {
    for (; next < cuts.n; ++next) {
      out_hits[(int64_t)q * cuts.n + next] = hits;
      out_dcg[(int64_t)q * cuts.n + next] = acc;
    }
    out_first[q] = first;
  }
}

// ------------------------------------------------------------------------------------------------ bootstrap
__global__ __launch_bounds__(BT_THREADS) void qr_boot_kernel(const double* __restrict__ values, int32_t n, int32_t M,
                                                             const int32_t* __restrict__ idx,
                                                             double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double part[BT_THREADS * BT_MMAX];              // 32 KiB: the sums of BT_THREADS segments, [segment][M]
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int32_t* row = idx + b * (int64_t)n;
  const int nseg = (n + BT_SEG - 1) / BT_SEG;
  double total = 0.0;                                        // thread m < M: the fold across segments of column m
  for (int s0 = 0; s0 < nseg; s0 += BT_THREADS) {
    const int s = s0 + tid;
    if (s < nseg) {
      double acc[BT_MMAX];
#pragma unroll
      for (int m = 0; m < BT_MMAX; ++m) acc[m] = 0.0;
      const int i1 = min(n, (s + 1) * BT_SEG);
      for (int i = s * BT_SEG; i < i1; ++i) {
        const int r = row[i];
        if ((unsigned)r >= (unsigned)n) continue;            // precondition of the header; never read through
        const double* v = values + (int64_t)r * M;
#pragma unroll
        for (int m = 0; m < BT_MMAX; ++m)
          if (m < M) acc[m] = acc[m] + v[m];
      }
#pragma unroll
      for (int m = 0; m < BT_MMAX; ++m)
        if (m < M) part[tid * M + m] = acc[m];
    }
    __syncthreads();
    if (tid < M) {
      const int ns = min(BT_THREADS, nseg - s0);
      for (int j = 0; j < ns; ++j) total = total + part[j * M + tid];
    }
    __syncthreads();
  }
  if (tid < M) out[b * M + tid] = total / (double)n;
}

LdsOptIn g_count_lds;

}  // namespace

extern "C" size_t snx_sparse_first_relevant_workspace_bytes(int32_t nq, int32_t nd, int32_t chunk_docs) {
  if (nq <= 0 || nd < 0 || chunk_docs < 0) return 0;
  return align256((size_t)nq * (size_t)sr_nch(nd, sr_chunk(chunk_docs)) * 4);
}

extern "C" int snx_sparse_first_relevant(const int64_t* q_ptr, const int32_t* q_term, const float* q_w, int32_t nq,
                                         const int64_t* term_ptr, const int32_t* post_doc, const float* post_w,
                                         const int64_t* doc_ptr, const int32_t* doc_term, const float* doc_w, int32_t nd,
                                         int32_t V, const int64_t* rel_ptr, const int32_t* rel_doc, int32_t chunk_docs,
                                         int32_t* out_doc, float* out_score, int32_t* out_rank, int32_t* out_nrel,
                                         void* workspace, size_t ws_bytes, hipStream_t st) {
  if (!q_ptr || !term_ptr || !doc_ptr || !rel_ptr || !out_doc || !out_score || !out_rank || !out_nrel) return SNX_E_ARG;
  if (nq < 0 || nd < 0 || V <= 0 || chunk_docs < 0 || chunk_docs > SR_CHUNK_MAX) return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  const int chunk = sr_chunk(chunk_docs);
  const int nch = sr_nch(nd, chunk);
  const long blocks = (long)nq * nch;
  if (blocks > (1L << 31) / SR_THREADS) return SNX_E_SHAPE;       // one launch of the chunk grid
  const size_t need = snx_sparse_first_relevant_workspace_bytes(nq, nd, chunk_docs);
  if (!workspace || ws_bytes < need) return SNX_E_ARG;
  int32_t* rcount = (int32_t*)workspace;
  hipLaunchKernelGGL(qr_best_kernel, dim3(nq), dim3(QB_THREADS), 0, st, q_ptr, q_term, q_w, doc_ptr, doc_term, doc_w, nd,
                     rel_ptr, rel_doc, out_doc, out_score, out_nrel);
  SNX_CHECK_LAUNCH();
  const size_t lds = (size_t)chunk * sizeof(float);
  if (lds > 48 * 1024) {
    if (const int rc = g_count_lds.ensure((const void*)qr_count_kernel, SR_CHUNK_MAX * (int)sizeof(float))) return rc;
  }
  hipLaunchKernelGGL(qr_count_kernel, dim3((unsigned)blocks), dim3(SR_THREADS), lds, st, q_ptr, q_term, q_w, term_ptr,
                     post_doc, post_w, nd, V, chunk, nch, (const int32_t*)out_doc, (const float*)out_score, rcount);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(qr_rank_kernel, dim3(cdiv(nq, 64)), dim3(64), 0, st, (const int32_t*)rcount, nq, nch,
                     (const float*)out_score, out_rank);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_ranked_relevance(const int32_t* docs, int32_t nq, int32_t R, int32_t nd, const int64_t* rel_ptr,
                                    const int32_t* rel_doc, const int32_t* cutoffs /*[host]*/, int32_t ncut,
                                    const double* disc, int32_t* out_first, int32_t* out_hits, double* out_dcg,
                                    hipStream_t st) {
  if (!cutoffs || ncut < 1 || ncut > QR_CUTS) return SNX_E_ARG;
  if (nq < 0 || nd < 0 || R < 1 || R > QR_RMAX) return SNX_E_SHAPE;
  Cutoffs cuts = {};
  cuts.n = ncut;
  for (int j = 0; j < ncut; ++j) {
    cuts.at[j] = cutoffs[j];
    if (cutoffs[j] < 1 || cutoffs[j] > R || (j > 0 && cutoffs[j] <= cutoffs[j - 1])) return SNX_E_ARG;
  }
  if (nq == 0) return SNX_OK;
  if (!docs || !rel_ptr || !disc || !out_first || !out_hits || !out_dcg) return SNX_E_ARG;
  hipLaunchKernelGGL(qr_ranked_kernel, dim3(cdiv(nq, QR_WAVES)), dim3(QR_THREADS), 0, st, docs, nq, R, nd, rel_ptr,
                     rel_doc, cuts, disc, out_first, out_hits, out_dcg);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_bootstrap_means(const double* values, int32_t n, int32_t M, const int32_t* idx, int32_t nboot,
                                   double* out, hipStream_t st) {
  if (n < 1 || M < 1 || M > BT_MMAX || nboot < 0) return SNX_E_SHAPE;
  if (nboot == 0) return SNX_OK;
  if (!values || !idx || !out) return SNX_E_ARG;
  hipLaunchKernelGGL(qr_boot_kernel, dim3(nboot), dim3(BT_THREADS), 0, st, values, n, M, idx, out);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
