// BM25 baseline and hybrid rank fusion (include/snx.h "BM25 baseline and rank fusion"): the lexical baseline and the
// fused rows the reference quotes its retrieval numbers against (ref:huggingface/v33/README.md:189-233,
// ref:benchmark/score_fusion.py, ref:benchmark/hybrid_searcher.py:501-522).  The reference asks an OpenSearch cluster
// for BM25 and fuses Python dicts per query; here token ids, index and top-k lists stay on the device.
//
//   hy_term_counts_kernel  one workgroup per row of input_ids: the counted ids (mask != 0, 0 <= id < V, allowed) go to
//                          LDS as int32 keys (others INT_MAX), an ascending bitonic sort, then run-length encoding: the
//                          run starts are numbered by an ordered ballot count, their positions kept as uint16 in LDS,
//                          tf = next start - own start.  No [n, V] intermediate; integer exact.  S <= HY_SMAX = 8192.
//   hy_doc_freq_kernel     df[term] += 1 per CSR entry (rows hold distinct terms): integer vector atomics, exact and
//                          order-independent, accumulating over batches.
//   hy_bm25_kernel         one wave per CSR row, lanes over its entries; float64 with every product, sum and quotient
//                          rounded on its own (v_mul_f64 / v_add_f64 through asm, IEEE division): no fma contraction, so
//                          the fp32 weights equal a numpy float64 evaluation bit for bit.
//   hy_fuse_kernel         one workgroup per query.  The L * R entries are keyed (doc << 32 | list << 16 | position) and
//                          sorted ascending in LDS: equal docs become neighbours, lists in order.  The head of each group
//                          folds the lists' terms in list order in float64 (operand order of the reference) and writes
//                          an order-preserving image of the fused score next to the doc id; a second bitonic sort by
//                          (score desc, doc asc) gives the whole fused order, from which top_k, the union size and the
//                          target's position are read.  No float atomics: byte-identical from run to run.
#include <math.h>

// pow2_at_least comes from sparse_common.h; the bitonic network (other comparators than the rank key's) and the float64
// helpers are this file's own.
#include "sparse_common.h"
#include "snx.h"

namespace {

constexpr int HY_THREADS = 256;
constexpr int HY_WAVES = HY_THREADS / 64;
constexpr int HY_SMAX = 8192;                    // term counts: row length cap (the model's position limit)
constexpr int HY_LMAX = 4;                       // fusion: lists per query
constexpr int HY_RMAX = 1024;                    // fusion: entries per list (the search's k cap)
constexpr int HY_EMAX = HY_LMAX * HY_RMAX;       // fusion: entries per query
constexpr int HY_INVALID = 0x7FFFFFFF;

// a * b and a + b in float64, each rounded once: hipcc contracts `a * b + c` (and the __d*_rn intrinsics, which are
// plain operators to it) into v_fma_f64 where it sees fit; the contracts of this file are stated per operation.
__device__ __forceinline__ double dmul(double a, double b) {
  double r;
  asm("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double dadd(double a, double b) {
  double r;
  asm("v_add_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double ddiv(double a, double b) {
#pragma clang fp contract(off)
  return a / b;                                              // IEEE: the f64 division expansion is correctly rounded
}

// ascending / descending bitonic network step indices over P = 2^m slots by the whole workgroup
#define HY_BITONIC(P, ...)                                                    \
  for (int size = 2; size <= (P); size <<= 1)                                 \
    for (int stride = size >> 1; stride > 0; stride >>= 1) {                  \
      for (int t = threadIdx.x; t < ((P) >> 1); t += HY_THREADS) {            \
        const int lo = 2 * t - (t & (stride - 1));                            \
        const int hi = lo + stride;                                           \
        const bool up = (lo & size) == 0;                                     \
        __VA_ARGS__                                                           \
      }                                                                       \
      __syncthreads();                                                        \
    }

// ------------------------------------------------------------------------------------------------ term counts
struct CountSmem {
  int32_t key[HY_SMAX];
  uint16_t start[HY_SMAX];
  int wsum[HY_WAVES];
};

__global__ __launch_bounds__(HY_THREADS) void hy_term_counts_kernel(
    const int64_t* __restrict__ ids, const int64_t* __restrict__ mask, const uint8_t* __restrict__ allowed, int32_t S,
    int32_t V, int32_t* __restrict__ out_term, int32_t* __restrict__ out_tf, int32_t* __restrict__ out_cnt,
    int32_t* __restrict__ out_len) {
  __shared__ CountSmem M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int64_t row = blockIdx.x;
  const int64_t* rid = ids + row * S;
  const int64_t* rm = mask + row * S;
  const int P = pow2_at_least(S);                            // <= HY_SMAX (checked on the host)
  for (int i = tid; i < P; i += HY_THREADS) {
    int32_t k = HY_INVALID;
    if (i < S && rm[i] != 0) {
      const int64_t id = rid[i];
      if (id >= 0 && id < (int64_t)V && allowed[id] != 0) k = (int32_t)id;
    }
    M.key[i] = k;
  }
  __syncthreads();
  HY_BITONIC(P, {
    const int32_t x = M.key[lo], y = M.key[hi];
    if ((x > y) == up) { M.key[lo] = y; M.key[hi] = x; }
  })
  // run starts, numbered in order; nu = runs so far, nv = counted positions so far (both uniform)
  int nu = 0, nv = 0;
  for (int c0 = 0; c0 < P; c0 += HY_THREADS) {
    const int i = c0 + tid;
    const int32_t k = i < P ? M.key[i] : HY_INVALID;
    const bool valid = k != HY_INVALID;
    const bool head = valid && (i == 0 || M.key[i - 1] != k);
    const unsigned long long mh = __ballot(head), mv = __ballot(valid);
    __syncthreads();                                         // the previous step's readers of wsum are done
    if (lane == 0) M.wsum[wave] = __popcll(mh) | (__popcll(mv) << 16);
    __syncthreads();
    int pos = nu + __popcll(mh & below);
    for (int x = 0; x < HY_WAVES; ++x) {
      if (x < wave) pos += M.wsum[x] & 0xFFFF;
      nu += M.wsum[x] & 0xFFFF;
      nv += M.wsum[x] >> 16;
    }
    if (head) M.start[pos] = (uint16_t)i;
  }
  __syncthreads();
  int32_t* ot = out_term + row * S;
  int32_t* of = out_tf + row * S;
  for (int j = tid; j < S; j += HY_THREADS) {
    int32_t t = -1, f = 0;
    if (j < nu) {
      const int a = M.start[j];
      t = M.key[a];
      f = (j + 1 < nu ? (int)M.start[j + 1] : nv) - a;
    }
    ot[j] = t;
    of[j] = f;
  }
  if (tid == 0) {
    out_cnt[row] = nu;
    out_len[row] = nv;
  }
}

// ------------------------------------------------------------------------------------------------ document frequencies
__global__ __launch_bounds__(HY_THREADS) void hy_doc_freq_kernel(const int32_t* __restrict__ term, int64_t nnz, int32_t V,
                                                                 int32_t* __restrict__ df) {
  for (int64_t i = (int64_t)blockIdx.x * HY_THREADS + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * HY_THREADS) {
    const int32_t t = term[i];
    if ((uint32_t)t < (uint32_t)V) atomicAdd(&df[t], 1);
  }
}

// ------------------------------------------------------------------------------------------------ BM25 weights
__global__ __launch_bounds__(HY_THREADS) void hy_bm25_kernel(const int64_t* __restrict__ ptr,
                                                             const int32_t* __restrict__ term,
                                                             const int32_t* __restrict__ tf,
                                                             const int32_t* __restrict__ dl,
                                                             const double* __restrict__ idf, int32_t n, int64_t nnz,
                                                             int32_t V, double avgdl, double k1, double b,
                                                             float* __restrict__ w) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * HY_WAVES + (threadIdx.x >> 6);
  const double one_minus_b = dadd(1.0, -b);
  for (int64_t r = wave0; r < n; r += (int64_t)gridDim.x * HY_WAVES) {
    const int64_t a = min(max(ptr[r], (int64_t)0), nnz);
    const int64_t e = min(max(ptr[r + 1], a), nnz);          // never past the arrays, whatever ptr holds
    const double norm = dmul(k1, dadd(one_minus_b, dmul(b, ddiv((double)dl[r], avgdl))));
    for (int64_t i = a + lane; i < e; i += 64) {
      const int32_t t = term[i];
      const double f = (double)tf[i];
      const double x = (uint32_t)t < (uint32_t)V ? idf[t] : 0.0;
      w[i] = (float)dmul(x, ddiv(f, dadd(f, norm)));
    }
  }
}

// ------------------------------------------------------------------------------------------------ rank fusion
struct FuseParams {
  int32_t method;
  double k;
  double alpha;
  double w[HY_LMAX];
};

struct FuseSmem {
  int len[HY_LMAX];
  double mn[HY_LMAX][HY_WAVES], mx[HY_LMAX][HY_WAVES];
  int wsum[HY_WAVES];
  int found;
};

// order-preserving image of a finite double: larger double <-> larger key, all keys > 0; -0.0 counts as +0.0
__device__ __forceinline__ unsigned long long order_key(double s) {
  if (s == 0.0) s = 0.0;
  const unsigned long long u = __builtin_bit_cast(unsigned long long, s);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_score(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __builtin_bit_cast(double, u);
}

__global__ __launch_bounds__(HY_THREADS) void hy_fuse_kernel(const int32_t* __restrict__ docs,
                                                             const float* __restrict__ scores, int32_t L, int32_t nq,
                                                             int32_t R, FuseParams prm,
                                                             const int32_t* __restrict__ target, int32_t top_k,
                                                             int32_t* __restrict__ out_doc,
                                                             double* __restrict__ out_score,
                                                             int32_t* __restrict__ out_total,
                                                             int32_t* __restrict__ out_rank) {
  extern __shared__ __align__(16) unsigned char hy_dyn[];
  __shared__ FuseSmem M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
  const int E = L * R;
  const int P = pow2_at_least(E);                            // <= HY_EMAX
  unsigned long long* A = (unsigned long long*)hy_dyn;       // [P] merge keys, then the doc of every union slot
  unsigned long long* B = A + P;                             // [P] order keys of the fused scores
  if (tid < HY_LMAX) M.len[tid] = R;
  if (tid == 0) M.found = 0;
  __syncthreads();
  // list lengths: the leading entries up to the first negative doc id
  for (int e = tid; e < E; e += HY_THREADS) {
    const int l = e / R, p = e - l * R;
    if (docs[((int64_t)l * nq + q) * R + p] < 0) atomicMin(&M.len[l], p);
  }
  __syncthreads();
  int max_rank = 100;
  for (int l = 0; l < L; ++l) max_rank = max(max_rank, M.len[l] + 1);
  // linear: per list the minimum and maximum of its own scores (fp32 widened; min / max are exact in any order)
  double lo_s[HY_LMAX], hi_s[HY_LMAX];
  if (prm.method == SNX_FUSE_LINEAR) {
    for (int l = 0; l < L; ++l) {
      double mn = INFINITY, mx = -INFINITY;
      const float* s = scores + ((int64_t)l * nq + q) * R;
      for (int p = tid; p < M.len[l]; p += HY_THREADS) {
        const double v = (double)s[p];
        mn = fmin(mn, v);
        mx = fmax(mx, v);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, o, 64));
        mx = fmax(mx, __shfl_xor(mx, o, 64));
      }
      if (lane == 0) { M.mn[l][wave] = mn; M.mx[l][wave] = mx; }
    }
    __syncthreads();
    for (int l = 0; l < L; ++l) {
      lo_s[l] = M.mn[l][0];
      hi_s[l] = M.mx[l][0];
      for (int x = 1; x < HY_WAVES; ++x) {
        lo_s[l] = fmin(lo_s[l], M.mn[l][x]);
        hi_s[l] = fmax(hi_s[l], M.mx[l][x]);
      }
    }
  }
  // merge keys: equal docs become neighbours, lists in order, positions in order; unused slots sort last
  for (int e = tid; e < P; e += HY_THREADS) {
    unsigned long long key = ~0ull;
    if (e < E) {
      const int l = e / R, p = e - l * R;
      if (p < M.len[l])
        key = ((unsigned long long)(uint32_t)docs[((int64_t)l * nq + q) * R + p] << 32) | ((uint32_t)l << 16) | (uint32_t)p;
    }
    A[e] = key;
  }
  __syncthreads();
  HY_BITONIC(P, {
    const unsigned long long x = A[lo], y = A[hi];
    if ((x > y) == up) { A[lo] = y; A[hi] = x; }
  })
  // fused score of every group head (a group: the entries of one doc)
  int nu = 0;                                                // union size (uniform)
  for (int c0 = 0; c0 < P; c0 += HY_THREADS) {
    const int i = c0 + tid;
    const unsigned long long key = i < P ? A[i] : ~0ull;
    const uint32_t d = (uint32_t)(key >> 32);
    const bool head = key != ~0ull && (i == 0 || (uint32_t)(A[i - 1] >> 32) != d);
    unsigned long long ok = 0ull;                            // non-heads sort behind every score
    if (head) {
      int pos[HY_LMAX] = {-1, -1, -1, -1};
      for (int j = i; j < P; ++j) {                          // <= L entries when docs are distinct within a list
        const unsigned long long kj = A[j];
        if (kj == ~0ull || (uint32_t)(kj >> 32) != d) break;
        const int l = (int)((kj >> 16) & 0xFFFFu), p = (int)(kj & 0xFFFFu);
#pragma unroll
        for (int x = 0; x < HY_LMAX; ++x)                    // a doc repeated in a list: its first position
          if (x == l && pos[x] < 0) pos[x] = p;
      }
      double acc = 0.0;
      if (prm.method == SNX_FUSE_LINEAR) {
        double nrm[2];
#pragma unroll
        for (int l = 0; l < 2; ++l) {
          if (pos[l] < 0) {
            nrm[l] = 0.0;
          } else if (hi_s[l] == lo_s[l]) {
            nrm[l] = 1.0;
          } else {
            const double s = (double)scores[((int64_t)l * nq + q) * R + pos[l]];
            nrm[l] = ddiv(dadd(s, -lo_s[l]), dadd(hi_s[l], -lo_s[l]));
          }
        }
        acc = dadd(dmul(prm.alpha, nrm[0]), dmul(dadd(1.0, -prm.alpha), nrm[1]));
      } else {
#pragma unroll
        for (int l = 0; l < HY_LMAX; ++l) {
          if (l < L) {
            const double rank = (double)(pos[l] < 0 ? max_rank : pos[l] + 1);
            const double num = prm.method == SNX_FUSE_WEIGHTED_RRF ? prm.w[l] : 1.0;
            const double term = ddiv(num, dadd(prm.k, rank));
            acc = l == 0 ? term : dadd(acc, term);
          }
        }
      }
      ok = order_key(acc);
    }
    const unsigned long long mh = __ballot(head);
    __syncthreads();                                         // the previous step's readers of wsum are done
    if (lane == 0) M.wsum[wave] = __popcll(mh);
    __syncthreads();
    for (int x = 0; x < HY_WAVES; ++x) nu += M.wsum[x];
    if (i < P) B[i] = ok;
  }
  __syncthreads();
  // the whole fused order: score descending, ties lowest doc id first (A keeps the doc in its upper half)
  HY_BITONIC(P, {
    const unsigned long long x = B[lo], y = B[hi];
    const unsigned long long ax = A[lo], ay = A[hi];
    const bool before = x > y || (x == y && (ax >> 32) <= (ay >> 32));   // lo's entry ranks first
    if (before != up) { B[lo] = y; B[hi] = x; A[lo] = ay; A[hi] = ax; }
  })
  const int tt = target ? target[q] : -1;
  int32_t* od = out_doc + (int64_t)q * top_k;
  double* os = out_score + (int64_t)q * top_k;
  for (int i = tid; i < nu; i += HY_THREADS) {
    const int d = (int)(uint32_t)(A[i] >> 32);
    if (i < top_k) {
      od[i] = d;
      os[i] = key_score(B[i]);
    }
    if (d == tt) M.found = i + 1;
  }
  for (int i = nu + tid; i < top_k; i += HY_THREADS) {
    od[i] = -1;
    os[i] = 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    out_total[q] = nu;
    if (target) out_rank[q] = M.found;
  }
}

LdsOptIn g_fuse_lds;

}  // namespace

extern "C" int32_t snx_term_counts_max_len(void) { return HY_SMAX; }

extern "C" int snx_term_counts(const int64_t* input_ids, const int64_t* attention_mask, const uint8_t* allowed, int32_t n,
                               int32_t S, int32_t V, int32_t* out_term, int32_t* out_tf, int32_t* out_cnt,
                               int32_t* out_len, hipStream_t st) {
  if (n < 0 || S < 1 || S > HY_SMAX || V < 1) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!input_ids || !attention_mask || !allowed || !out_term || !out_tf || !out_cnt || !out_len) return SNX_E_ARG;
  hipLaunchKernelGGL(hy_term_counts_kernel, dim3(n), dim3(HY_THREADS), 0, st, input_ids, attention_mask, allowed, S, V,
                     out_term, out_tf, out_cnt, out_len);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_bm25_doc_freq(const int32_t* term, int64_t nnz, int32_t V, int32_t* df, hipStream_t st) {
  if (nnz < 0 || V < 1) return SNX_E_SHAPE;
  if (nnz == 0) return SNX_OK;
  if (!term || !df) return SNX_E_ARG;
  const int64_t blocks = (nnz + HY_THREADS - 1) / HY_THREADS;
  hipLaunchKernelGGL(hy_doc_freq_kernel, dim3((int)(blocks < 4096 ? blocks : 4096)), dim3(HY_THREADS), 0, st, term, nnz,
                     V, df);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_bm25_weights(const int64_t* ptr, const int32_t* term, const int32_t* tf, const int32_t* dl,
                                const double* idf, int32_t n, int64_t nnz, int32_t V, double avgdl, double k1, double b,
                                float* w, hipStream_t st) {
  if (!(k1 >= 0.0) || !(b >= 0.0 && b <= 1.0) || !isfinite(k1) || !(avgdl >= 0.0) || !isfinite(avgdl)) return SNX_E_ARG;
  if (n < 0 || nnz < 0 || V < 1) return SNX_E_SHAPE;
  if (n == 0 || nnz == 0) return SNX_OK;
  if (!ptr || !term || !tf || !dl || !idf || !w) return SNX_E_ARG;
  if (!(avgdl > 0.0)) return SNX_E_ARG;                       // entries exist: some doc has a length
  const int64_t blocks = ((int64_t)n + HY_WAVES - 1) / HY_WAVES;
  hipLaunchKernelGGL(hy_bm25_kernel, dim3((int)(blocks < 8192 ? blocks : 8192)), dim3(HY_THREADS), 0, st, ptr, term, tf,
                     dl, idf, n, nnz, V, avgdl, k1, b, w);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_fuse_ranked(const int32_t* docs, const float* scores, int32_t L, int32_t nq, int32_t R, int32_t method,
                               const double* params /*[host]*/, const int32_t* target, int32_t top_k, int32_t* out_doc,
                               double* out_score, int32_t* out_total, int32_t* out_rank, hipStream_t st) {
  if (L < 1 || L > HY_LMAX) return SNX_E_ARG;
  if (method != SNX_FUSE_RRF && method != SNX_FUSE_WEIGHTED_RRF && method != SNX_FUSE_LINEAR) return SNX_E_ARG;
  if (method == SNX_FUSE_LINEAR && L != 2) return SNX_E_ARG;
  if (!params) return SNX_E_ARG;
  FuseParams prm = {};
  prm.method = method;
  if (method == SNX_FUSE_LINEAR) {
    prm.alpha = params[0];
    if (!(prm.alpha >= 0.0 && prm.alpha <= 1.0)) return SNX_E_ARG;
  } else {
    prm.k = params[0];
    if (!(prm.k >= 0.0) || !isfinite(prm.k)) return SNX_E_ARG;
    for (int l = 0; l < L; ++l) {
      prm.w[l] = method == SNX_FUSE_WEIGHTED_RRF ? params[1 + l] : 1.0;
      if (!isfinite(prm.w[l])) return SNX_E_ARG;
    }
  }
  if (nq < 0 || R < 1 || R > HY_RMAX || top_k < 1 || top_k > HY_EMAX) return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  if (!docs || !out_doc || !out_score || !out_total) return SNX_E_ARG;
  if (method == SNX_FUSE_LINEAR && !scores) return SNX_E_ARG;
  if (target && !out_rank) return SNX_E_ARG;
  const int rc = g_fuse_lds.ensure((const void*)hy_fuse_kernel, HY_EMAX * 16);
  if (rc != SNX_OK) return rc;
  const size_t lds = (size_t)pow2_at_least(L * R) * 16;
  hipLaunchKernelGGL(hy_fuse_kernel, dim3(nq), dim3(HY_THREADS), lds, st, docs, scores, L, nq, R, prm, target, top_k,
                     out_doc, out_score, out_total, out_rank);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
