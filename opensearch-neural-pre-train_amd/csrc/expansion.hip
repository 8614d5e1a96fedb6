// Term-expansion evaluation (include/snx.h "term-expansion evaluation"): where a query's judged tokens fall in the ranking
// of the model's own vocabulary row, and the graded metrics that follow from those positions -- the reference's
// RankingMetrics (ref:src/evaluation/ranking_metrics.py:435-680), which clones the row, masks the special ids one element
// at a time, runs torch.topk and pulls up to 100 (id, value) pairs to the host with .item().  Nothing here sorts the row:
// the position of a judged token is a count,
//     rank(t) = 1 + #{ranked v: rep[v] > rep[t]} + #{ranked v < t: rep[v] == rep[t]},
// so one streaming read of rep [B, V] against the row's few thresholds gives every metric.
//
//   ex_count_kernel     one workgroup per (row, column slice).  The row's judged tokens become thresholds (weight bits,
//                       id) in LDS, EX_CHUNK at a time; every entry of the slice becomes its weight bits (0 when it is
//                       not ranked) and is compared against each threshold of the chunk (ex_compare).  The compare's lane
//                       mask is counted on the scalar unit and the count is added in the lane that owns the threshold:
//                       no per-thread counter array, no shuffle.  16-byte loads over the aligned body of the slice,
//                       scalar loads for the head in front of it and the tail behind, decided from the slice's address
//                       (rows of a V that is no multiple of 4 start misaligned).  The partial counts of a slice go to the
//                       workspace by integer atomics: they commute, so the number of slices changes no bit.
//   ex_finalize_kernel  one wave per row: counts -> positions (out_rank), then a walk over the row's judged positions in
//                       ascending order (a wave minimum per step) with one running float64 sum read off at every cutoff,
//                       the left fold of include/snx.h.
#include "sparse_common.h"
#include "snx.h"

namespace {

constexpr int EX_THREADS = 256;
constexpr int EX_WAVES = EX_THREADS / 64;
constexpr int EX_CHUNK = 64;                   // thresholds per LDS chunk: one per lane of a wave
constexpr int EX_CUTS = 8;
constexpr int EX_VMAX = 1 << 30;               // the slice arithmetic stays in int32
constexpr int EX_SLICE_MIN = 4096;             // columns per slice at least, when the call chooses the slices
constexpr int EX_WG_TARGET = 1024;             // workgroups the chosen slicing aims at (256 CUs x 4)
constexpr uint32_t EX_NEVER = 0xFFFFFFFFu;   // weight bits of a threshold nothing is in front of (its tb - 1 too)

struct ExCutoffs {
  int32_t n;
  int32_t at[EX_CUTS];
};

// weight bits of a ranked entry, 0 otherwise: NaN, -0.0 and negatives are not > 0
__device__ __forceinline__ uint32_t ex_key(float x, uint8_t ex) { return (x > 0.f && ex == 0) ? fbits(x) : 0u; }

// In front of threshold (tb, tok) lie the entries with bits > tb and, among ids < tok, those with bits == tb: an entry of
// id v is counted when its key > (v < tok ? tb - 1 : tb).  A wave's group of 4 keys per lane covers the 256 ids from vw[g]
// on, so which of the two applies is wave-uniform except in the one group that holds tok.  Lane j owns the count of
// threshold j.
template <int NG>
__device__ __forceinline__ void ex_compare(const uint32_t (&k)[NG][4], const int (&vw)[NG], int lane,
                                           const uint32_t* thr_b, const int32_t* thr_tok, int nt, int& cnt) {
  for (int j = 0; j < nt; ++j) {
    const uint32_t tb = __builtin_amdgcn_readfirstlane(thr_b[j]);
    const int tok = __builtin_amdgcn_readfirstlane(thr_tok[j]);
    const uint32_t tm1 = tb - 1u;
    int c = 0;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int d = tok - vw[g];                             // both in [0, 2^31): no overflow
      if (d <= 0 || d >= 256) {                              // scalar branch
        const uint32_t ts = d <= 0 ? tb : tm1;
#pragma unroll
        for (int e = 0; e < 4; ++e) c += __popcll(__ballot(k[g][e] > ts));
      } else {
        const int v0 = vw[g] + 4 * lane;
#pragma unroll
        for (int e = 0; e < 4; ++e) c += __popcll(__ballot(k[g][e] > (v0 + e < tok ? tm1 : tb)));
      }
    }
    cnt += lane == j ? c : 0;
  }
}

// the same for one key per lane at any id v (the head and the tail of a slice)
__device__ __forceinline__ void ex_compare_one(uint32_t k, int v, int lane, const uint32_t* thr_b, const int32_t* thr_tok,
                                               int nt, int& cnt) {
  for (int j = 0; j < nt; ++j) {
    const uint32_t tb = __builtin_amdgcn_readfirstlane(thr_b[j]);
    const int tok = __builtin_amdgcn_readfirstlane(thr_tok[j]);
    const int c = __popcll(__ballot(k > (v < tok ? tb - 1u : tb)));
    cnt += lane == j ? c : 0;
  }
}

__device__ __forceinline__ void ex_row_bounds(const int64_t* __restrict__ j_ptr, int b, int64_t nj, int64_t& ja,
                                              int64_t& jb) {
  ja = min(max(j_ptr[b], (int64_t)0), nj);                   // a broken ptr reads nothing out of bounds
  jb = min(max(j_ptr[b + 1], ja), nj);
}

__global__ __launch_bounds__(EX_THREADS) void ex_count_kernel(
    const float* __restrict__ rep, int32_t V, const uint8_t* __restrict__ excluded, const int64_t* __restrict__ j_ptr,
    const int32_t* __restrict__ j_tok, int64_t nj, int32_t slices, int32_t slice_cols, int32_t* __restrict__ ws_count,
    int32_t* __restrict__ ws_nranked) {
  __shared__ uint32_t thr_b[EX_CHUNK];
  __shared__ int32_t thr_tok[EX_CHUNK];
  __shared__ int tot[EX_CHUNK];
  __shared__ int nrk;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = (int)(blockIdx.x / (unsigned)slices), s = (int)(blockIdx.x - (unsigned)b * (unsigned)slices);
  const float* row = rep + (int64_t)b * V;
  const int c0 = (int)min((int64_t)s * slice_cols, (int64_t)V);
  const int n = (int)min((int64_t)slice_cols, (int64_t)V - c0);              // block-uniform
  int64_t ja, jb;
  ex_row_bounds(j_ptr, b, nj, ja, jb);
  // head: the entries in front of the first 16-byte boundary; body: whole float4s; tail: what is left
  const uintptr_t addr = (uintptr_t)(row + c0);
  const int head = min(n, (int)(((16u - (unsigned)(addr & 15u)) & 15u) >> 2));
  const int nvec = (n - head) >> 2;
  const int tail0 = head + 4 * nvec;
  const float4* body = (const float4*)(row + c0 + head);
  if (tid == 0) nrk = 0;
  for (int64_t g = ja; g == ja || g < jb; g += EX_CHUNK) {   // a row without judgments still counts its ranked entries
    const int nt = (int)max((int64_t)0, min((int64_t)EX_CHUNK, jb - g));
    __syncthreads();                                         // the previous chunk's flush has read tot
    if (tid < EX_CHUNK) {
      tot[tid] = 0;
      uint32_t tb = EX_NEVER;
      int32_t tk = 0;
      if (tid < nt) {
        const int32_t tok = j_tok[g + tid];
        if ((unsigned)tok < (unsigned)V) {                   // an id outside [0, V) is never read through
          const uint32_t k = ex_key(row[tok], excluded[tok]);
          if (k != 0u) { tb = k; tk = tok; }
        }
      }
      thr_b[tid] = tb;
      thr_tok[tid] = tk;
    }
    __syncthreads();
    const bool count_ranked = g == ja;
    int cnt = 0, nr = 0;
    if (head > 0) {                                          // at most 3 entries
      const uint32_t k = tid < head ? ex_key(row[c0 + tid], excluded[c0 + tid]) : 0u;
      if (count_ranked) nr += __popcll(__ballot(k != 0u));
      ex_compare_one(k, c0 + tid, lane, thr_b, thr_tok, nt, cnt);
    }
    for (int base = 0; base < nvec; base += 2 * EX_THREADS) {   // block-uniform trip count: every lane keeps its counter
      uint32_t k[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
      int vw[2];
      float4 x[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {                          // both loads first
        const int i = base + h * EX_THREADS + tid;
        vw[h] = c0 + head + 4 * (base + h * EX_THREADS + 64 * wave);
        if (i < nvec) x[h] = body[i];
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = base + h * EX_THREADS + tid;
        if (i < nvec) {
          const int v = c0 + head + 4 * i;
          k[h][0] = ex_key(x[h].x, excluded[v]);
          k[h][1] = ex_key(x[h].y, excluded[v + 1]);
          k[h][2] = ex_key(x[h].z, excluded[v + 2]);
          k[h][3] = ex_key(x[h].w, excluded[v + 3]);
        }
      }
      if (count_ranked) {
#pragma unroll
        for (int e = 0; e < 8; ++e) nr += __popcll(__ballot(k[e >> 2][e & 3] != 0u));
      }
      ex_compare<2>(k, vw, lane, thr_b, thr_tok, nt, cnt);
    }
    if (tail0 < n) {                                         // at most 3 entries
      const int v = c0 + tail0 + tid;
      const uint32_t k = tail0 + tid < n ? ex_key(row[v], excluded[v]) : 0u;
      if (count_ranked) nr += __popcll(__ballot(k != 0u));
      ex_compare_one(k, v, lane, thr_b, thr_tok, nt, cnt);
    }
    if (lane < nt && cnt) atomicAdd(&tot[lane], cnt);
    if (count_ranked && lane == 0 && nr) atomicAdd(&nrk, nr);
    __syncthreads();
    if (tid < nt && tot[tid]) atomicAdd(&ws_count[g + tid], tot[tid]);
    if (count_ranked && tid == 0 && nrk) atomicAdd(&ws_nranked[b], nrk);
  }
}

// MODE 0: positions only (snx_expansion_ranks); MODE 1: positions and the metrics
template <int MODE>
__global__ __launch_bounds__(EX_THREADS) void ex_finalize_kernel(
    const float* __restrict__ rep, int32_t B, int32_t V, const uint8_t* __restrict__ excluded,
    const int64_t* __restrict__ j_ptr, const int32_t* __restrict__ j_tok, const uint8_t* __restrict__ j_grade,
    const uint8_t* __restrict__ j_rel, int64_t nj, int32_t max_k, ExCutoffs cuts, const double* __restrict__ gain,
    int32_t G, const int32_t* __restrict__ ws_count, const int32_t* __restrict__ ws_nranked, int32_t* __restrict__ out_rank,
    int32_t* __restrict__ out_nranked, int32_t* __restrict__ out_first, int32_t* __restrict__ out_hits,
    double* __restrict__ out_dcg) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * EX_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;                                        // wave-uniform
  const float* row = rep + (int64_t)b * V;
  int64_t ja, jb;
  ex_row_bounds(j_ptr, b, nj, ja, jb);
  // key of a judged entry in the cut list: position << 8 | grade << 1 | rel; NONE otherwise.  The lane keeps the key
  // of its first entry; a row with more than 64 judgments reads the others back from out_rank (its own stores).
  constexpr unsigned long long NONE = ~0ull;
  unsigned long long mine = NONE;
  for (int64_t i = ja + lane; i < jb; i += 64) {
    const int32_t tok = j_tok[i];
    int pos = 0;
    if ((unsigned)tok < (unsigned)V && ex_key(row[tok], excluded[tok]) != 0u) {
      const int c = ws_count[i];
      pos = c < max_k ? c + 1 : 0;
    }
    out_rank[i] = pos;
    if (MODE == 1 && i == ja + lane && pos > 0)
      mine = ((unsigned long long)pos << 8) | ((unsigned long long)(j_grade[i] & 3) << 1) | (j_rel[i] != 0);
  }
  if (lane == 0) out_nranked[b] = min(max_k, ws_nranked[b]);
  if (MODE == 0) return;
  int first = 0, hits = 0, next = 0, last = 0;
  double acc = 0.0;
  for (;;) {
    unsigned long long best = (mine != NONE && (int)(mine >> 8) > last) ? mine : NONE;
    for (int64_t i = ja + lane + 64; i < jb; i += 64) {
      const int pos = out_rank[i];
      if (pos > last) {
        const unsigned long long k =
            ((unsigned long long)pos << 8) | ((unsigned long long)(j_grade[i] & 3) << 1) | (j_rel[i] != 0);
        if (k < best) best = k;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(best, o, 64);
      if (other < best) best = other;
    }
    if (best == NONE) break;                                  // wave-uniform
    const int p = (int)(best >> 8), grade = (int)(best >> 1) & 3;
    const bool rel = (best & 1ull) != 0ull;
    last = p;
    if (rel && first == 0) first = p;
    while (next < cuts.n && p > cuts.at[next]) {             // the fold of cutoff `next` is complete
      if (lane == 0) {
        out_hits[(int64_t)b * cuts.n + next] = hits;
        out_dcg[(int64_t)b * cuts.n + next] = acc;
      }
      ++next;
    }
    if (next < cuts.n) {
      hits += rel;
      if (grade > 0 && p <= G) acc = acc + gain[(int64_t)(grade - 1) * G + (p - 1)];
    }
  }
  if (lane == 0) {
    for (; next < cuts.n; ++next) {
      out_hits[(int64_t)b * cuts.n + next] = hits;
      out_dcg[(int64_t)b * cuts.n + next] = acc;
    }
    out_first[b] = first;
  }
}

int ex_slices(int32_t B, int32_t V, int32_t slices) {
  int s = slices;
  if (s <= 0) s = (int)min((long)cdiv(EX_WG_TARGET, B), (long)cdiv(V, EX_SLICE_MIN));
  return (int)max(1L, min((long)s, (long)V));
}

int ex_launch(bool metrics, const float* rep, int32_t B, int32_t V, const uint8_t* excluded, const int64_t* j_ptr,
              const int32_t* j_tok, const uint8_t* j_grade, const uint8_t* j_rel, int64_t nj, int32_t max_k,
              const ExCutoffs& cuts, const double* gain, int32_t G, int32_t slices, int32_t* out_rank,
              int32_t* out_nranked, int32_t* out_first, int32_t* out_hits, double* out_dcg, void* workspace,
              size_t ws_bytes, hipStream_t st) {
  const int ns = ex_slices(B, V, slices);
  if ((long)B * ns > (1L << 31) - 1) return SNX_E_SHAPE;          // one launch of the (row, slice) grid
  const size_t need = snx_expansion_workspace_bytes(B, nj);
  if (!workspace || ws_bytes < need) return SNX_E_ARG;
  int32_t* ws_nranked = (int32_t*)workspace;
  int32_t* ws_count = ws_nranked + B;
  if (const hipError_t e = hipMemsetAsync(workspace, 0, ((size_t)B + (size_t)nj) * 4, st)) return (int)e;
  const int slice_cols = (cdiv(V, ns) + 3) & ~3;
  hipLaunchKernelGGL(ex_count_kernel, dim3((unsigned)((long)B * ns)), dim3(EX_THREADS), 0, st, rep, V, excluded, j_ptr,
                     j_tok, nj, ns, slice_cols, ws_count, ws_nranked);
  SNX_CHECK_LAUNCH();
  if (metrics)
    hipLaunchKernelGGL(ex_finalize_kernel<1>, dim3(cdiv(B, EX_WAVES)), dim3(EX_THREADS), 0, st, rep, B, V, excluded, j_ptr,
                       j_tok, j_grade, j_rel, nj, max_k, cuts, gain, G, (const int32_t*)ws_count,
                       (const int32_t*)ws_nranked, out_rank, out_nranked, out_first, out_hits, out_dcg);
  else
    hipLaunchKernelGGL(ex_finalize_kernel<0>, dim3(cdiv(B, EX_WAVES)), dim3(EX_THREADS), 0, st, rep, B, V, excluded, j_ptr,
                       j_tok, j_grade, j_rel, nj, max_k, cuts, gain, G, (const int32_t*)ws_count,
                       (const int32_t*)ws_nranked, out_rank, out_nranked, out_first, out_hits, out_dcg);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

}  // namespace

extern "C" size_t snx_expansion_workspace_bytes(int32_t B, int64_t nj) {
  if (B <= 0 || nj < 0) return 0;
  return align256(((size_t)B + (size_t)nj) * 4);
}

extern "C" int snx_expansion_ranks(const float* rep, int32_t B, int32_t V, const uint8_t* excluded, const int64_t* j_ptr,
                                   const int32_t* j_tok, int64_t nj, int32_t max_k, int32_t slices, int32_t* out_rank,
                                   int32_t* out_nranked, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (B < 0 || V < 1 || V > EX_VMAX || max_k < 1) return SNX_E_SHAPE;
  if (nj < 0 || slices < 0) return SNX_E_ARG;
  if (B == 0) return SNX_OK;
  if (!rep || !excluded || !j_ptr || !out_nranked || (nj > 0 && (!j_tok || !out_rank))) return SNX_E_ARG;
  ExCutoffs cuts = {};
  return ex_launch(false, rep, B, V, excluded, j_ptr, j_tok, nullptr, nullptr, nj, max_k, cuts, nullptr, 0, slices,
                   out_rank, out_nranked, nullptr, nullptr, nullptr, workspace, ws_bytes, st);
}

extern "C" int snx_expansion_metrics(const float* rep, int32_t B, int32_t V, const uint8_t* excluded,
                                     const int64_t* j_ptr, const int32_t* j_tok, const uint8_t* j_grade,
                                     const uint8_t* j_rel, int64_t nj, int32_t max_k, const int32_t* cutoffs /*[host]*/,
                                     int32_t ncut, const double* gain, int32_t G, int32_t slices, int32_t* out_rank,
                                     int32_t* out_nranked, int32_t* out_first, int32_t* out_hits, double* out_dcg,
                                     void* workspace, size_t ws_bytes, hipStream_t st) {
  if (!cutoffs || ncut < 1 || ncut > EX_CUTS) return SNX_E_ARG;
  if (B < 0 || V < 1 || V > EX_VMAX || max_k < 1) return SNX_E_SHAPE;
  ExCutoffs cuts = {};
  cuts.n = ncut;
  for (int j = 0; j < ncut; ++j) {
    cuts.at[j] = cutoffs[j];
    if (cutoffs[j] < 1 || (j > 0 && cutoffs[j] <= cutoffs[j - 1])) return SNX_E_ARG;
  }
  if (nj < 0 || slices < 0 || G < min(max_k, cuts.at[ncut - 1])) return SNX_E_ARG;
  if (B == 0) return SNX_OK;
  if (!rep || !excluded || !j_ptr || !gain || !out_nranked || !out_first || !out_hits || !out_dcg) return SNX_E_ARG;
  if (nj > 0 && (!j_tok || !j_grade || !j_rel || !out_rank)) return SNX_E_ARG;
  return ex_launch(true, rep, B, V, excluded, j_ptr, j_tok, j_grade, j_rel, nj, max_k, cuts, gain, G, slices, out_rank,
                   out_nranked, out_first, out_hits, out_dcg, workspace, ws_bytes, st);
}
