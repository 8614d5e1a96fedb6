// IDF line (include/snx.h "IDF"): document frequencies, the IDF-aware FLOPS penalty and the inference-free query
// (ref:tools/idf-compute/src/main.rs, ref:docs/concepts/04-loss-functions.md §5, ref:scripts/test_idf_math.py:61-246,
// ref:tests/test_korean_neural_sparse.py:94-122).  The logarithms stay on the host (V entries, one libm: snx/idf.py).
//
//   idf_doc_freq_kernel    a workgroup walks documents b, b + grid, ...  Per document a V-bit presence bitmap in LDS: the
//                          lane whose ds_or flips a bit owns that (document, id) pair.  It does not add to df at once: a
//                          stop-word would take one global add PER DOCUMENT on one address (one word saturates at ~88
//                          returning atomics/us, and 64 lanes in 64 rows run ~17x below the streaming atomic rate), so the
//                          pair first goes to a direct-mapped LDS table of IDF_SLOTS (id, count) entries that lives as
//                          long as the workgroup; only a pair whose slot is held by another id goes to global memory
//                          directly.  The table is flushed once at the end: a hot id costs one global add per WORKGROUP.
//                          The touched bitmap words are cleared by re-walking the tokens.  Integer adds: exact, in any
//                          order.
//   idf_flops_cols_kernel  one wave per 64 columns: the column sum over ascending rows in fp32, divided by R (the order and
//                          the division of loss_partial_kernel, loss.hip), t1 = w|a|, t2 = w(a a) in fp32, each product
//                          rounded on its own; the wave's 64 terms are summed in float64 by the xor tree.
//   idf_flops_sum_kernel   one workgroup: thread t folds the partials t, t + 256, ... ascending, then the xor tree and the
//                          four waves as (0 + 1) + (2 + 3).  The order depends on (R, V) alone: two runs give the same bits.
//   idf_flops_bwd_kernel   dx[r, j] += coef_j, a thread per column, rows of a slice in turn.
//   idf_query_kernel       a workgroup owns a column slice of one row: zero fill, barrier, scatter of the ids in its slice.
#include "common.h"
#include "snx.h"

namespace {

constexpr int IDF_THREADS = 256;
constexpr int IDF_SLOTS = 1024;                  // hot-id table entries per workgroup (power of two)
constexpr int IDF_GRID_MAX = 2048;               // doc_freq workgroups: 8 per CU on 256 CUs
constexpr int IDF_VMAX = 1 << 20;                // 128 KiB of bitmap
constexpr int IDF_QSLICE = 8192;                 // query_dense: columns per workgroup

__global__ __launch_bounds__(IDF_THREADS) void idf_doc_freq_kernel(const int64_t* __restrict__ ids,
                                                                   const int64_t* __restrict__ mask, int64_t n,
                                                                   int64_t S, int32_t V, int32_t words,
                                                                   unsigned long long* __restrict__ df,
                                                                   unsigned long long* __restrict__ num_docs) {
  extern __shared__ __attribute__((aligned(16))) uint32_t idf_sm[];
  uint32_t* bm = idf_sm;                                     // [words]
  int32_t* skey = (int32_t*)(idf_sm + words);                // [IDF_SLOTS]
  uint32_t* scnt = (uint32_t*)(skey + IDF_SLOTS);            // [IDF_SLOTS]
  const int tid = threadIdx.x;
  for (int i = tid; i < words; i += IDF_THREADS) bm[i] = 0u;
  for (int i = tid; i < IDF_SLOTS; i += IDF_THREADS) { skey[i] = -1; scnt[i] = 0u; }
  __syncthreads();
  for (int64_t doc = blockIdx.x; doc < n; doc += gridDim.x) {
    const int64_t* rid = ids + doc * S;
    const int64_t* rm = mask + doc * S;
    for (int64_t i = tid; i < S; i += IDF_THREADS) {
      if (rm[i] == 0) continue;
      const int64_t id = rid[i];
      if (id < 0 || id >= (int64_t)V) continue;
      const uint32_t bit = 1u << (id & 31);
      if (atomicOr(&bm[id >> 5], bit) & bit) continue;       // another position of this document came first
      const int s = (int)(id & (IDF_SLOTS - 1));
      const int32_t old = atomicCAS(&skey[s], -1, (int32_t)id);
      if (old == -1 || old == (int32_t)id) atomicAdd(&scnt[s], 1u);
      else atomicAdd(&df[id], 1ull);
    }
    __syncthreads();
    for (int64_t i = tid; i < S; i += IDF_THREADS) {
      if (rm[i] == 0) continue;
      const int64_t id = rid[i];
      if (id >= 0 && id < (int64_t)V) bm[id >> 5] = 0u;
    }
    __syncthreads();
  }
  for (int i = tid; i < IDF_SLOTS; i += IDF_THREADS)
    if (skey[i] >= 0 && scnt[i] != 0u) atomicAdd(&df[skey[i]], (unsigned long long)scnt[i]);
  if (num_docs && blockIdx.x == 0 && tid == 0) atomicAdd(num_docs, (unsigned long long)n);
}

__global__ __launch_bounds__(64) void idf_flops_cols_kernel(const float* __restrict__ x, int32_t R, int32_t V,
                                                            const float* __restrict__ w, float* __restrict__ mean,
                                                            double* __restrict__ part) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  double d1 = 0.0, d2 = 0.0;
  if (j < V) {
    const float* c = x + j;
    float s = 0.f;
    int r = 0;
    for (; r + 7 < R; r += 8) {                              // eight loads in flight, added in row order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = c[(long)(r + u) * V];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; r < R; ++r) s += c[(long)r * V];
    s /= (float)R;
    mean[j] = s;
    const float wj = w[j];
    d1 = (double)mul_rn(wj, fabsf(s));
    d2 = (double)mul_rn(wj, mul_rn(s, s));
  }
  d1 = wave_sum_f64(d1);
  d2 = wave_sum_f64(d2);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = d1; part[2 * blockIdx.x + 1] = d2; }
}

__global__ __launch_bounds__(IDF_THREADS) void idf_flops_sum_kernel(const double* __restrict__ part, int32_t nblk,
                                                                    float beta, float lambda, float* __restrict__ out3,
                                                                    float* __restrict__ loss) {
  __shared__ double red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s1 = 0.0, s2 = 0.0;
  for (int i = tid; i < nblk; i += IDF_THREADS) { s1 += part[2 * i]; s2 += part[2 * i + 1]; }
  s1 = wave_sum_f64(s1);
  s2 = wave_sum_f64(s2);
  if (lane == 0) { red[0][wave] = s1; red[1][wave] = s2; }
  __syncthreads();
  if (tid == 0) {
    const double t1 = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    const double t2 = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const float P = (float)fma((double)beta, t2, t1);
    out3[0] = (float)t1; out3[1] = (float)t2; out3[2] = P;
    if (loss) loss[0] = loss[0] + mul_rn(lambda, P);
  }
}

// coef_j = (w_j * (sign(a_j) + 2 beta * a_j)) * ((g * lambda) / R): six fp32 roundings (2 beta is exact)
__global__ __launch_bounds__(IDF_THREADS) void idf_flops_bwd_kernel(float* __restrict__ dx, int32_t R, int32_t V,
                                                                    int32_t rows_per, const float* __restrict__ mean,
                                                                    const float* __restrict__ w, float beta, float lambda,
                                                                    const float* __restrict__ g) {
  const int j = blockIdx.x * IDF_THREADS + threadIdx.x;
  if (j >= V) return;
  const float a = mean[j];
  const float sg = a > 0.f ? 1.f : (a < 0.f ? -1.f : 0.f);
  const float inner = sg + mul_rn(2.f * beta, a);
  const float scale = mul_rn(g[0], lambda) / (float)R;
  const float coef = mul_rn(mul_rn(w[j], inner), scale);
  if (coef == 0.f) return;                                   // sign(0) = 0: the column keeps its bits
  const int r0 = blockIdx.y * rows_per, r1 = min(R, r0 + rows_per);
  for (int r = r0; r < r1; ++r) {
    float* p = dx + (long)r * V + j;
    *p = *p + coef;
  }
}

__global__ __launch_bounds__(IDF_THREADS) void idf_query_kernel(const int64_t* __restrict__ ids,
                                                                const int64_t* __restrict__ mask,
                                                                const uint8_t* __restrict__ allowed,
                                                                const float* __restrict__ idf, int32_t slices, int64_t S,
                                                                int32_t V, float* __restrict__ q) {
  const int64_t b = blockIdx.x / slices;
  const int c0 = (int)(blockIdx.x % slices) * IDF_QSLICE, c1 = min(V, c0 + IDF_QSLICE);
  float* row = q + b * (int64_t)V;
  for (int c = c0 + threadIdx.x; c < c1; c += IDF_THREADS) row[c] = 0.f;
  __syncthreads();
  const int64_t* rid = ids + b * S;
  const int64_t* rm = mask + b * S;
  for (int64_t i = threadIdx.x; i < S; i += IDF_THREADS) {
    if (rm[i] == 0) continue;
    const int64_t id = rid[i];
    if (id < (int64_t)c0 || id >= (int64_t)c1 || allowed[id] == 0) continue;
    row[id] = idf[id];                                       // duplicates store the same value
  }
}

LdsOptIn g_doc_freq_lds;

inline size_t flops_mean_floats(int32_t V) { return ((size_t)V + 1) & ~(size_t)1; }   // the partials stay 8-byte aligned

}  // namespace

extern "C" int snx_idf_doc_freq(const int64_t* input_ids, const int64_t* attention_mask, int64_t n, int64_t S, int32_t V,
                                int64_t* df, int64_t* num_docs, hipStream_t st) {
  if (n < 0 || S < 1 || V < 1 || V > IDF_VMAX) return SNX_E_SHAPE;
  if (!df) return SNX_E_ARG;
  if (n == 0) return SNX_OK;
  if (!input_ids || !attention_mask) return SNX_E_ARG;
  const int words = cdiv(V, 32);
  const size_t lds = (size_t)words * 4 + (size_t)IDF_SLOTS * 8;
  if (lds > 64 * 1024) {
    const int rc = g_doc_freq_lds.ensure((const void*)idf_doc_freq_kernel, (IDF_VMAX / 32) * 4 + IDF_SLOTS * 8);
    if (rc) return rc;
  }
  const int grid = (int)(n < IDF_GRID_MAX ? n : IDF_GRID_MAX);
  hipLaunchKernelGGL(idf_doc_freq_kernel, dim3(grid), dim3(IDF_THREADS), lds, st, input_ids, attention_mask, n, S, V, words,
                     (unsigned long long*)df, (unsigned long long*)num_docs);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" size_t snx_idf_flops_workspace_bytes(int32_t V) {
  if (V < 1) return 0;
  return flops_mean_floats(V) * sizeof(float) + (size_t)cdiv(V, 64) * 2 * sizeof(double);
}

extern "C" int snx_idf_flops_fwd(const float* x, int32_t R, int32_t V, const float* w, float beta, float lambda,
                                 void* workspace, float* out3, float* loss, hipStream_t st) {
  if (R < 1 || V < 1) return SNX_E_SHAPE;
  if (!x || !w || !workspace || !out3 || ((uintptr_t)workspace & 7)) return SNX_E_ARG;
  float* mean = (float*)workspace;
  double* part = (double*)(mean + flops_mean_floats(V));
  const int nblk = cdiv(V, 64);
  hipLaunchKernelGGL(idf_flops_cols_kernel, dim3(nblk), dim3(64), 0, st, x, R, V, w, mean, part);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(idf_flops_sum_kernel, dim3(1), dim3(IDF_THREADS), 0, st, part, nblk, beta, lambda, out3, loss);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_idf_flops_bwd_accum(float* dx, int32_t R, int32_t V, const void* workspace, const float* w, float beta,
                                       float lambda, const float* gout, hipStream_t st) {
  if (R < 1 || V < 1) return SNX_E_SHAPE;
  if (!dx || !workspace || !w || !gout) return SNX_E_ARG;
  const int gy = R < 16 ? R : 16;
  const int rows_per = cdiv(R, gy);
  hipLaunchKernelGGL(idf_flops_bwd_kernel, dim3(cdiv(V, IDF_THREADS), cdiv(R, rows_per)), dim3(IDF_THREADS), 0, st, dx, R, V,
                     rows_per, (const float*)workspace, w, beta, lambda, gout);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_idf_query_dense(const int64_t* input_ids, const int64_t* attention_mask, const uint8_t* allowed,
                                   const float* idf, int32_t B, int64_t S, int32_t V, float* q, hipStream_t st) {
  if (B < 0 || S < 1 || V < 1) return SNX_E_SHAPE;
  if (B == 0) return SNX_OK;
  if (!input_ids || !attention_mask || !allowed || !idf || !q) return SNX_E_ARG;
  const int slices = cdiv(V, IDF_QSLICE);
  if ((int64_t)B * slices > 0x7FFFFFFFll) return SNX_E_SHAPE;
  hipLaunchKernelGGL(idf_query_kernel, dim3((unsigned)((int64_t)B * slices)), dim3(IDF_THREADS), 0, st, input_ids,
                     attention_mask, allowed, idf, slices, S, V, q);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
