// Exact L2 nearest neighbours (include/snx.h "exact L2 nearest neighbours"): the distance work of the reference's
// information-gain filter (ref:src/information_gain.py:156-195, 340-364: a float64 cdist of every target and every source
// against the whole corpus, then one argsort over the corpus per pair inside a Python loop).
//
// Distance (the ABI): d2(q, c) = float64 acc from +0, for j ascending t = (double)q[j] - (double)c[j], acc = fma(t, t, acc).
// The difference form: a row against an identical row is exactly 0.0, which the estimator tells apart from a tiny distance,
// and a near neighbour keeps its leading digits.  The Gram form that MFMA would need gives neither, so this is v_fma_f64
// work.  Zero padding of a ragged D changes nothing: fma(0, 0, acc) is acc, and acc is never -0.
//
// Search: a workgroup owns 64 queries and one split of the corpus and walks the split in tiles of 64 rows.  fp32 slices of
// 16 columns of both go through LDS, transposed and double-buffered behind a register prefetch; a thread keeps a 4 x 4
// square of float64 accumulators and walks j ascending through the slices: the ABI's chain.  The 64-bit pattern of a
// non-negative double is a monotone key.  Every finished d2 goes through the query's running threshold (the k-th best key
// so far) and, when below it, into the query's candidate list in the workspace (LDS atomic cursor).  When the next tile
// could overflow a list the workgroup sorts it in LDS by (key, id), keeps the best k and lowers the threshold to the k-th
// key: ids ascend along the walk, so a later row that only ties the threshold loses to the k already kept, and
// `key < threshold` is exact.  At the end every list is sorted and cut to k; l2_merge_kernel folds a query's per-split
// lists into one by bitonic merges under the same order.
//
// Gather: one workgroup per pair.  The K neighbour rows are staged through LDS in slices of 32 columns with coalesced
// loads; thread r walks row r serially from LDS (pitch 33: no bank conflict) by the same chain, then the K keys are sorted.
#include "sparse_common.h"
#include "snx.h"

namespace {

constexpr int L2_THREADS = 256;
constexpr int L2_TILE = 64;                    // query rows and corpus rows of a workgroup's tile
constexpr int L2_KT = 16;                      // columns per LDS stage
constexpr int L2_PITCH = 68;                   // LDS row pitch (floats): 16-byte aligned rows for the b128 reads
constexpr int L2_CAP_MAX = 2 * SNX_L2_KMAX;    // candidate list entries for k = 256
constexpr int L2_DMAX = 4096;
constexpr int L2_WG_TARGET = 4096;             // default split count: four rounds of four workgroups per CU ...
constexpr int L2_SPLITS_MAX = 64;              // ... but no more than this many lists per query to merge
constexpr int L2_GT = 32;                      // columns per stage of the gather
constexpr int L2_GPITCH = 33;
constexpr unsigned long long L2_NONE = ~0ull;  // key of an empty slot: above every distance (+inf is 0x7FF0...)
constexpr uint32_t L2_NOID = 0xFFFFFFFFu;

inline SplitPlan l2_plan(int32_t nq, int32_t n, int32_t chunk_rows) {
  return split_plan(nq, n, chunk_rows, L2_TILE, L2_WG_TARGET, L2_SPLITS_MAX);
}
inline int l2_cap(int32_t k) { return (int)pow2_at_least((long)(2 * k > 2 * L2_TILE ? 2 * k : 2 * L2_TILE)); }

inline size_t l2_workspace(int32_t nq, int nsplit, int cap) {
  const size_t lists = (size_t)nq * (size_t)nsplit;
  return align256(lists * (size_t)cap * 8) + align256(lists * (size_t)cap * 4) + align256(lists * 4);
}

__device__ __forceinline__ unsigned long long dbits(double x) { return __builtin_bit_cast(unsigned long long, x); }
__device__ __forceinline__ double bitsd(unsigned long long x) { return __builtin_bit_cast(double, x); }

// ascending bitonic sort of (key, id) pairs in LDS under (key, then id), P a power of two, by the whole workgroup
template <int THREADS>
__device__ __forceinline__ void l2_sort(unsigned long long* key, uint32_t* id, int P) {
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += THREADS) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const unsigned long long kx = key[lo], ky = key[hi];
        const uint32_t ix = id[lo], iy = id[hi];
        const bool gt = kx > ky || (kx == ky && ix > iy);
        const bool lt = kx < ky || (kx == ky && ix < iy);
        if (asc ? gt : lt) { key[lo] = ky; key[hi] = kx; id[lo] = iy; id[hi] = ix; }
      }
      __syncthreads();
    }
}

// the merge half of that sort: a[0..P) ascending then descending (bitonic) -> ascending
template <int THREADS>
__device__ __forceinline__ void l2_merge(unsigned long long* key, uint32_t* id, int P) {
  for (int stride = P >> 1; stride > 0; stride >>= 1) {
    for (int t = threadIdx.x; t < (P >> 1); t += THREADS) {
      const int lo = 2 * t - (t & (stride - 1));
      const int hi = lo + stride;
      const unsigned long long kx = key[lo], ky = key[hi];
      const uint32_t ix = id[lo], iy = id[hi];
      if (kx > ky || (kx == ky && ix > iy)) { key[lo] = ky; key[hi] = kx; id[lo] = iy; id[hi] = ix; }
    }
    __syncthreads();
  }
}

// this thread's share of a 64 x 16 operand tile of a row-major [nrows, D] matrix: row t / 4, 4 columns; rows past the
// matrix and columns past D read as zero
__device__ __forceinline__ void l2_fetch(const float* __restrict__ P, long nrows, long row0, int D, int k0, int vec, int t,
                                         float (&v)[4]) {
  const int kk = k0 + (t & 3) * 4;
  const long row = row0 + (t >> 2);
  if (row < nrows && vec && kk < D) {                        // vec: D % 4 == 0 and 16-byte aligned rows
    const f32x4 x = *(const f32x4*)(P + row * D + kk);
    v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = (row < nrows && kk + u < D) ? P[row * D + kk + u] : 0.f;
  }
}
__device__ __forceinline__ void l2_put(int t, const float (&v)[4], float (*S)[L2_PITCH]) {
  const int kk = (t & 3) * 4, r = t >> 2;
#pragma unroll
  for (int u = 0; u < 4; ++u) S[kk + u][r] = v[u];
}

__global__ __launch_bounds__(L2_THREADS, 4) void l2_search_kernel(
    const float* __restrict__ Q, int32_t nq, const float* __restrict__ E, int32_t n, int32_t D, int32_t vec,
    int32_t qtiles, int32_t split_tiles, int32_t nsplit, int32_t k, int32_t cap, unsigned long long* candk,
    uint32_t* candi, int32_t* __restrict__ ccount) {
  __shared__ __attribute__((aligned(16))) float As[2][L2_KT][L2_PITCH];
  __shared__ __attribute__((aligned(16))) float Bs[2][L2_KT][L2_PITCH];
  __shared__ unsigned long long sk[L2_CAP_MAX];
  __shared__ uint32_t si[L2_CAP_MAX];
  __shared__ unsigned long long thr[L2_TILE];
  __shared__ int cnt[L2_TILE];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int qt = (int)(blockIdx.x % (unsigned)qtiles), split = (int)(blockIdx.x / (unsigned)qtiles);
  const long q0 = (long)qt * L2_TILE;
  const long tiles = (n + (long)L2_TILE - 1) / L2_TILE;
  const long t0 = (long)split * split_tiles;
  const long t1 = min(tiles, t0 + split_tiles);
  if (t < L2_TILE) {
    thr[t] = L2_NONE;
    cnt[t] = 0;
  }
  __syncthreads();
  // the candidate list of query row `row`: ((q0 + row) * nsplit + split) * cap
  const size_t list0 = ((size_t)q0 * (size_t)nsplit + (size_t)split) * (size_t)cap;
  const size_t list_step = (size_t)nsplit * (size_t)cap;
  const int nk = (D + L2_KT - 1) / L2_KT;

  // sort the list of `row`, keep the best k, lower its threshold
  auto compact = [&](int row) {
    const int m0 = min(cnt[row], cap);
    unsigned long long* bk = candk + list0 + (size_t)row * list_step;
    uint32_t* bi = candi + list0 + (size_t)row * list_step;
    for (int i = t; i < cap; i += L2_THREADS) {
      sk[i] = i < m0 ? bk[i] : L2_NONE;
      si[i] = i < m0 ? bi[i] : L2_NOID;
    }
    __syncthreads();
    l2_sort<L2_THREADS>(sk, si, cap);
    const int m = min(m0, k);
    for (int i = t; i < m; i += L2_THREADS) {
      bk[i] = sk[i];
      bi[i] = si[i];
    }
    if (t == 0) {
      cnt[row] = m;
      if (m0 >= k) thr[row] = sk[k - 1];
    }
    __syncthreads();
  };

  for (long tile = t0; tile < t1; ++tile) {
    const long n0 = tile * L2_TILE;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    float va[4], vb[4];
    l2_fetch(Q, nq, q0, D, 0, vec, t, va);
    l2_fetch(E, n, n0, D, 0, vec, t, vb);
    l2_put(t, va, As[0]);
    l2_put(t, vb, Bs[0]);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      l2_fetch(Q, nq, q0, D, (kt + 1) * L2_KT, vec, t, va);      // past D: zeros, no load (the last stage's put is idle)
      l2_fetch(E, n, n0, D, (kt + 1) * L2_KT, vec, t, vb);
#pragma unroll
      for (int s = 0; s < L2_KT; ++s) {                      // j ascending: the ABI's chain
        const f32x4 a = *(const f32x4*)&As[cur][s][ty * 4];
        const f32x4 b = *(const f32x4*)&Bs[cur][s][tx * 4];
        const double a0 = (double)a[0], a1 = (double)a[1], a2 = (double)a[2], a3 = (double)a[3];
        const double b0 = (double)b[0], b1 = (double)b[1], b2 = (double)b[2], b3 = (double)b[3];
        const double av[4] = {a0, a1, a2, a3}, bv[4] = {b0, b1, b2, b3};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double d = av[i] - bv[j];
            acc[i][j] = __builtin_fma(d, d, acc[i][j]);
          }
      }
      l2_put(t, va, As[cur ^ 1]);
      l2_put(t, vb, Bs[cur ^ 1]);
      __syncthreads();
    }
    // acc[i][j] = d2(q0 + 4 ty + i, n0 + 4 tx + j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = ty * 4 + i;
      const bool rok = q0 + row < nq;
      const unsigned long long th = thr[row];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long id = n0 + tx * 4 + j;
        const unsigned long long key = dbits(acc[i][j]);
        if (rok && id < n && key < th) {
          const int pos = atomicAdd(&cnt[row], 1);
          if (pos < cap) {
            candk[list0 + (size_t)row * list_step + pos] = key;
            candi[list0 + (size_t)row * list_step + pos] = (uint32_t)id;
          }
        }
      }
    }
    __syncthreads();
    // a tile adds at most L2_TILE entries to a list: compact every list that the next tile could overflow
    for (int row = 0; row < L2_TILE && q0 + row < nq; ++row)
      if (__builtin_amdgcn_readfirstlane(cnt[row]) > cap - L2_TILE) compact(row);
  }
  for (int row = 0; row < L2_TILE && q0 + row < nq; ++row) compact(row);
  if (t < L2_TILE && q0 + t < nq) ccount[(size_t)(q0 + t) * (size_t)nsplit + (size_t)split] = cnt[t];
}

// the best k over a query's per-split lists (each sorted, at most k long): the running best sits ascending in the lower
// half of the buffer, the next list goes into the upper half reversed, and one bitonic merge orders the whole
__global__ __launch_bounds__(L2_THREADS) void l2_merge_kernel(const unsigned long long* __restrict__ candk,
                                                              const uint32_t* __restrict__ candi,
                                                              const int32_t* __restrict__ ccount, int32_t nsplit,
                                                              int32_t cap, int32_t k, int32_t* __restrict__ out_id,
                                                              double* __restrict__ out_d2) {
  __shared__ unsigned long long mk[L2_CAP_MAX];
  __shared__ uint32_t mi[L2_CAP_MAX];
  const int t = threadIdx.x;
  const long q = blockIdx.x;
  const int kp = pow2_at_least((int)k);
  for (int i = t; i < kp; i += L2_THREADS) {
    mk[i] = L2_NONE;
    mi[i] = L2_NOID;
  }
  for (int s = 0; s < nsplit; ++s) {
    const size_t list = (size_t)q * (size_t)nsplit + (size_t)s;
    const int c = min(ccount[list], k);
    for (int i = t; i < kp; i += L2_THREADS) {
      mk[2 * kp - 1 - i] = i < c ? candk[list * (size_t)cap + i] : L2_NONE;
      mi[2 * kp - 1 - i] = i < c ? candi[list * (size_t)cap + i] : L2_NOID;
    }
    __syncthreads();
    l2_merge<L2_THREADS>(mk, mi, 2 * kp);
  }
  __syncthreads();
  for (int r = t; r < k; r += L2_THREADS) {
    const bool has = mi[r] != L2_NOID;
    out_id[q * k + r] = has ? (int32_t)mi[r] : -1;
    out_d2[q * k + r] = has ? bitsd(mk[r]) : __builtin_huge_val();
  }
}

// d2(T[i], E[nb[i, r]]) for r < K by the serial chain from LDS, sorted ascending; an id outside [0, n) is skipped
__global__ __launch_bounds__(L2_THREADS) void l2_gather_kernel(const float* __restrict__ T, const float* __restrict__ E,
                                                               int32_t n, int32_t D, int32_t vec,
                                                               const int32_t* __restrict__ nb, int32_t K,
                                                               double* __restrict__ out) {
  __shared__ float S[SNX_L2_KMAX][L2_GPITCH];
  __shared__ float Ts[L2_GT];
  __shared__ int32_t ids[SNX_L2_KMAX];
  __shared__ unsigned long long sk[SNX_L2_KMAX];
  __shared__ uint32_t si[SNX_L2_KMAX];
  const int t = threadIdx.x;
  const long pair = blockIdx.x;
  if (t < K) {
    const int32_t id = nb[pair * K + t];
    ids[t] = (uint32_t)id < (uint32_t)n ? id : -1;
  }
  __syncthreads();
  const float* trow = T + pair * D;
  double acc = 0.0;
  for (int k0 = 0; k0 < D; k0 += L2_GT) {
    if (t < L2_GT) Ts[t] = k0 + t < D ? trow[k0 + t] : 0.f;
    for (int idx = t; idx < K * (L2_GT / 4); idx += L2_THREADS) {      // 8 lanes take a row's 128 bytes
      const int r = idx >> 3, c = (idx & 7) * 4;
      const int32_t id = ids[r];
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (id >= 0) {
        const float* e = E + (long)id * D + k0 + c;
        if (vec && k0 + c < D) {
          const f32x4 x = *(const f32x4*)e;
          v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = k0 + c + u < D ? e[u] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) S[r][c + u] = v[u];
    }
    __syncthreads();
    if (t < K) {
#pragma unroll
      for (int j = 0; j < L2_GT; ++j) {                      // j ascending: the ABI's chain
        const double d = (double)Ts[j] - (double)S[t][j];
        acc = __builtin_fma(d, d, acc);
      }
    }
    __syncthreads();
  }
  const int P = pow2_at_least((int)K);
  if (t < P) {
    const bool has = t < K && ids[t] >= 0;
    sk[t] = has ? dbits(acc) : L2_NONE;
    si[t] = has ? (uint32_t)t : L2_NOID;
  }
  __syncthreads();
  l2_sort<L2_THREADS>(sk, si, P);
  if (t < K) out[pair * K + t] = si[t] != L2_NOID ? bitsd(sk[t]) : __builtin_huge_val();
}

inline int l2_vec(const float* A, const float* B, int32_t D) {
  return D % 4 == 0 && ((uintptr_t)A & 15) == 0 && ((uintptr_t)B & 15) == 0;
}

}  // namespace

extern "C" size_t snx_l2_knn_workspace_bytes(int32_t nq, int32_t n, int32_t k, int32_t chunk_rows) {
  if (nq <= 0 || n < 0 || k <= 0 || k > SNX_L2_KMAX || chunk_rows < 0) return 0;
  return l2_workspace(nq, l2_plan(nq, n, chunk_rows).nsplit, l2_cap(k));
}

extern "C" int snx_l2_knn(const float* Q, int32_t nq, const float* E, int32_t n, int32_t D, int32_t k, int32_t chunk_rows,
                          int32_t* out_id, double* out_d2, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (nq < 0 || n < 0 || D < 1 || D > L2_DMAX || k < 1 || k > SNX_L2_KMAX || chunk_rows < 0) return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  if (!Q || (n > 0 && !E) || !out_id || !out_d2) return SNX_E_ARG;
  const SplitPlan p = l2_plan(nq, n, chunk_rows);
  const int cap = l2_cap(k);
  const long blocks = (long)p.qtiles * p.nsplit;
  if (blocks > 0x7FFFFFFFL || (long)nq * p.nsplit > 0x7FFFFFFFL) return SNX_E_SHAPE;
  if (!workspace || ws_bytes < l2_workspace(nq, p.nsplit, cap)) return SNX_E_ARG;
  const size_t lists = (size_t)nq * (size_t)p.nsplit;
  char* w = (char*)workspace;
  unsigned long long* candk = (unsigned long long*)w;
  uint32_t* candi = (uint32_t*)(w + align256(lists * (size_t)cap * 8));
  int32_t* ccount = (int32_t*)((char*)candi + align256(lists * (size_t)cap * 4));
  hipLaunchKernelGGL(l2_search_kernel, dim3((unsigned)blocks), dim3(L2_THREADS), 0, st, Q, nq, E, n, D, l2_vec(Q, E, D),
                     p.qtiles, p.split_tiles, p.nsplit, k, cap, candk, candi, ccount);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(l2_merge_kernel, dim3((unsigned)nq), dim3(L2_THREADS), 0, st, (const unsigned long long*)candk,
                     (const uint32_t*)candi, (const int32_t*)ccount, p.nsplit, cap, k, out_id, out_d2);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_l2_gather_sorted(const float* T, int32_t m, const float* E, int32_t n, int32_t D, const int32_t* nb,
                                    int32_t K, double* out_d2, hipStream_t st) {
  if (m < 0 || n < 0 || D < 1 || D > L2_DMAX || K < 1 || K > SNX_L2_KMAX) return SNX_E_SHAPE;
  if (m == 0) return SNX_OK;
  if (!T || (n > 0 && !E) || !nb || !out_d2) return SNX_E_ARG;
  hipLaunchKernelGGL(l2_gather_kernel, dim3((unsigned)m), dim3(L2_THREADS), 0, st, T, E, n, D, l2_vec(T, E, D), nb, K,
                     out_d2);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
