// Two-phase dense retrieval (include/snx.h "two-phase dense retrieval"): the exact search's answer with most of the work
// on the bf16 MFMA.  dense.hip computes every score on v_mfma_f32_32x32x2_f32; here a first pass scores bf16 copies of
// the operands on v_mfma_f32_32x32x16_bf16 and proposes k1 candidates per query, a second pass scores the candidates by
// the ABI's chain on the fp32 operands, and a per-query certificate, from norms computed once, proves that the first
// pass hid no better doc (DESIGN.md "Two-phase dense retrieval" has the derivation).
//
// dn2_prepare_kernel   fp32 rows -> a bf16 copy (round to nearest even) padded with zeros to Dp = D rounded up to 32,
//                      and per row the float64 left folds of x^2, xhat^2 and (x - xhat)^2; one thread per row
// dn2_scan_kernel      dn_search_kernel's structure (128 queries by one split of the docs, tiles of 128 docs, four waves
//                      of 2 x 2 accumulators, register prefetch, double-buffered LDS, dn_admit / dn_compact and the
//                      per-split lists of dense_common.h) with the fp32 tile replaced by a bf16 one; no exclusions, no
//                      ceiling, no target.  The K loop is the same for every tile, so a(q, d) is a pure function of the
//                      two bf16 rows and no split or slicing changes a bit.
// dn2_merge_kernel     merge_lists over the splits -> cand_doc / cand_approx [nq, k1]
// dn2_rescore_kernel   one workgroup per query: the chain of dn_pair_kernel for every candidate, admissibility as in
//                      snx_dense_search_band, a bitonic sort by rank key, ranks lo .. hi-1, and the certificate
//
// LDS image of an operand stage: [128 rows][32 bf16] at a pitch of 40 bf16 (80 bytes).  A lane reads its fragment of one
// k-step, 8 consecutive bf16 of row (lane & 31), as one ds_read_b128; that instruction is served in groups of 16 lanes
// over 16 slots of 16 bytes, and row * 80 / 16 = 5 row (mod 16) puts 16 rows that differ mod 16 on 16 different slots.
#include "dense_common.h"
#include "snx.h"

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int D2_KT = 32;                      // bf16 K per LDS stage: two MFMA steps of 16
constexpr int D2_PITCH = 40;                   // LDS row pitch in bf16
constexpr int D2_WG_TARGET = 512;              // split planning as dense.hip's
constexpr int D2_SPLITS_MAX = 64;
constexpr int D2_PREP_THREADS = 256;

__host__ __device__ inline int d2_dp(int32_t D) { return (D + 31) & ~31; }

inline SplitPlan d2_plan(int32_t nq, int32_t nd, int32_t chunk_docs) {
  return split_plan(nq, nd, chunk_docs, DN_TILE, D2_WG_TARGET, D2_SPLITS_MAX);
}

inline size_t d2_workspace(int32_t nq, int nsplit, int cap) {
  const size_t lists = (size_t)nq * (size_t)nsplit;
  return align256(lists * (size_t)cap * 8) + align256(lists * 4);
}

// bf16 bits of a finite fp32 value, round to nearest even (a value past the bf16 range becomes an infinity)
__device__ __forceinline__ uint32_t d2_bf16_rne(float x) {
  const uint32_t u = fbits(x);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// One thread per row.  A float64 holds x^2, xhat^2 and (x - xhat)^2 exactly (24-bit and 16-bit significands), so each
// sum rounds once per addition, in ascending j: a left fold, whatever the launch.  The zero padding adds +0.
__global__ __launch_bounds__(D2_PREP_THREADS) void dn2_prepare_kernel(const float* __restrict__ X, int32_t n, int32_t D,
                                                                      int32_t Dp, uint16_t* __restrict__ Xb,
                                                                      double* __restrict__ norm2,
                                                                      double* __restrict__ hat2,
                                                                      double* __restrict__ res2) {
  const long r = (long)blockIdx.x * D2_PREP_THREADS + threadIdx.x;
  if (r >= n) return;
  const float* x = X + r * D;
  u32x4* o = (u32x4*)(Xb + r * Dp);
  double a = 0.0, b = 0.0, c = 0.0;
  for (int j0 = 0; j0 < Dp; j0 += 8) {
    uint32_t w[4];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = j0 + u;
      const float v = j < D ? x[j] : 0.f;
      const uint32_t hb = d2_bf16_rne(v);
      const double dv = (double)v, dh = (double)bitsf(hb << 16);
      const double e = dv - dh;
      a += dv * dv;
      b += dh * dh;
      c += e * e;
      if (u & 1) w[u >> 1] |= hb << 16; else w[u >> 1] = hb;
    }
    o[j0 >> 3] = (u32x4){w[0], w[1], w[2], w[3]};
  }
  norm2[r] = a;
  hat2[r] = b;
  res2[r] = c;
}

// this thread's share of a 128 x 32 bf16 operand stage of a row-major [*, Dp] matrix: tile rows r and r + 64, 8 k each
template <typename RowF>
__device__ __forceinline__ void d2_fetch(const uint16_t* __restrict__ P, RowF row_of, int Dp, int k0, int t,
                                         u32x4 (&v)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long row = row_of((t >> 2) + 64 * i);
    v[i] = row >= 0 ? *(const u32x4*)(P + row * Dp + k0 + (t & 3) * 8) : (u32x4){0u, 0u, 0u, 0u};
  }
}
__device__ __forceinline__ void d2_put(int t, const u32x4 (&v)[2], uint16_t (*S)[D2_PITCH]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) *(u32x4*)&S[(t >> 2) + 64 * i][(t & 3) * 8] = v[i];
}

// The approximate scores of one 128 x 128 tile: dn_tile_scores' layout (acc[i][j][r] = a(A tile row 64 wm + 32 i +
// (r & 3) + 8 (r >> 2) + 4 h, B tile row 64 wn + 32 j + c)) on the bf16 MFMA.  Lane 32 h + c holds k = 8 h .. 8 h + 7 of
// row c in a k-step of 16; the steps follow each other in ascending k.  Ends on a barrier.
template <typename RowA, typename RowB>
__device__ __forceinline__ void d2_tile_scores(const uint16_t* __restrict__ A, RowA row_a,
                                               const uint16_t* __restrict__ B, RowB row_b, int Dp,
                                               f32x16 (&acc)[2][2]) {
  __shared__ __attribute__((aligned(16))) uint16_t As[2][DN_TILE][D2_PITCH];
  __shared__ __attribute__((aligned(16))) uint16_t Bs[2][DN_TILE][D2_PITCH];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const int nk = Dp / D2_KT;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  u32x4 va[2], vb[2];
  d2_fetch(A, row_a, Dp, 0, t, va);
  d2_fetch(B, row_b, Dp, 0, t, vb);
  d2_put(t, va, As[0]);
  d2_put(t, vb, Bs[0]);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      d2_fetch(A, row_a, Dp, (kt + 1) * D2_KT, t, va);
      d2_fetch(B, row_b, Dp, (kt + 1) * D2_KT, t, vb);
    }
#pragma unroll
    for (int s = 0; s < D2_KT / 16; ++s) {                   // k ascending, the same order for every tile
      const int ko = 16 * s + 8 * h;
      const bf16x8 a0 = *(const bf16x8*)&As[cur][wm * 64 + c][ko], a1 = *(const bf16x8*)&As[cur][wm * 64 + 32 + c][ko];
      const bf16x8 b0 = *(const bf16x8*)&Bs[cur][wn * 64 + c][ko], b1 = *(const bf16x8*)&Bs[cur][wn * 64 + 32 + c][ko];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (kt + 1 < nk) {
      d2_put(t, va, As[cur ^ 1]);
      d2_put(t, vb, Bs[cur ^ 1]);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(DN_THREADS, 2) void dn2_scan_kernel(const uint16_t* __restrict__ Qb, int32_t nq,
                                                                 const uint16_t* __restrict__ Eb, int32_t nd, int32_t Dp,
                                                                 int32_t qtiles, int32_t split_tiles, int32_t nsplit,
                                                                 int32_t k, int32_t cap, unsigned long long* cand,
                                                                 int32_t* __restrict__ ccount) {
  __shared__ uint32_t thr[DN_TILE];
  __shared__ int cnt[DN_TILE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const int qt = (int)(blockIdx.x % (unsigned)qtiles), split = (int)(blockIdx.x / (unsigned)qtiles);
  const long q0 = (long)qt * DN_TILE;
  const long tiles = (nd + (long)DN_TILE - 1) / DN_TILE;
  const long t0 = (long)split * split_tiles;
  const long t1 = min(tiles, t0 + split_tiles);
  if (t < DN_TILE) {
    thr[t] = 0u;
    cnt[t] = 0;
  }
  __syncthreads();
  const size_t list0 = ((size_t)q0 * (size_t)nsplit + (size_t)split) * (size_t)cap;
  const size_t list_step = (size_t)nsplit * (size_t)cap;
  auto list = [&](int row) { return cand + list0 + (size_t)row * list_step; };
  auto compact = [&](int row) { dn_compact(list(row), cnt[row], thr[row], k, cap); };
  auto qrow = [&](int r) -> long { return q0 + r < nq ? q0 + r : -1; };
  const int64_t none = 0;

  for (long tile = t0; tile < t1; ++tile) {
    const long n0 = tile * DN_TILE;
    auto drow = [&](int r) -> long { return n0 + r < nd ? n0 + r : -1; };
    f32x16 acc[2][2];
    d2_tile_scores(Qb, qrow, Eb, drow, Dp, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const bool rok = q0 + row < nq;
        const uint32_t th = thr[row];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const long doc = n0 + wn * 64 + j * 32 + c;
          const float s = acc[i][j][r] + 0.0f;
          dn_admit(rok && doc < nd, s, (int32_t)doc, th, false, 0.f, false, nullptr, none, none, cnt[row], list(row),
                   cap);
        }
      }
    __syncthreads();
    // a tile adds at most DN_TILE entries to a list: compact every list that the next tile could overflow
    for (int row = 0; row < DN_TILE && q0 + row < nq; ++row)
      if (__builtin_amdgcn_readfirstlane(cnt[row]) > cap - DN_TILE) compact(row);
  }
  for (int row = 0; row < DN_TILE && q0 + row < nq; ++row) compact(row);
  if (t < DN_TILE && q0 + t < nq) ccount[(size_t)(q0 + t) * (size_t)nsplit + (size_t)split] = cnt[t];
}

// the k1 best of a query over its per-split lists, approximate score descending, ties lowest doc first
__global__ __launch_bounds__(SR_THREADS) void dn2_merge_kernel(const unsigned long long* __restrict__ cand,
                                                               const int32_t* __restrict__ ccount, int32_t nsplit,
                                                               int32_t cap, int32_t k1, int32_t* __restrict__ cand_doc,
                                                               float* __restrict__ cand_approx) {
  __shared__ SelectSmem S;
  const int q = blockIdx.x;
  const long base = (long)q * nsplit;
  const RankLists lists = {cand + (size_t)base * (size_t)cap, ccount + base, cap, k1};
  merge_lists<dense_unkey>(lists, nsplit, S, q, 0, k1, cand_doc, cand_approx, nullptr);
}

__device__ __forceinline__ bool d2_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// Phase 2 of query blockIdx.x.  dN, dNh, dR: the maxima over the docs of sqrt(norm2), sqrt(hat2), sqrt(res2).
__global__ __launch_bounds__(SR_THREADS) void dn2_rescore_kernel(
    const float* __restrict__ Q, const float* __restrict__ E, int32_t nd, int32_t D, int32_t vec,
    const int32_t* __restrict__ cand_doc, const float* __restrict__ cand_approx, int32_t k1,
    const double* __restrict__ q_norm2, const double* __restrict__ q_hat2, const double* __restrict__ q_res2, double dN,
    double dNh, double dR, const int64_t* __restrict__ ex_ptr, const int32_t* __restrict__ ex_doc,
    const float* __restrict__ ceiling, int32_t lo, int32_t hi, int32_t* __restrict__ out_doc,
    float* __restrict__ out_score, int32_t* __restrict__ out_found, uint8_t* __restrict__ certified) {
  __shared__ unsigned long long sbuf[SR_KMAX];
  __shared__ __attribute__((aligned(16))) float qs[DN_DMAX];
  __shared__ int nadm, bad;
  const int tid = threadIdx.x, q = blockIdx.x;
  const float* qrow = Q + (long)q * D;
  for (int j = tid; j < D; j += SR_THREADS) qs[j] = qrow[j];
  if (tid == 0) {
    nadm = 0;
    bad = 0;
  }
  __syncthreads();
  const bool has_c = ceiling != nullptr, has_x = ex_ptr != nullptr;
  const float cl = has_c ? ceiling[q] : 0.f;
  const int64_t ex0 = has_x ? ex_ptr[q] : 0, ex1 = has_x ? ex_ptr[q + 1] : 0;
  const int P = pow2_at_least((int)k1);
  for (int i = tid; i < P; i += SR_THREADS) {
    unsigned long long key = 0ull;
    const int32_t d = i < k1 ? cand_doc[(long)q * k1 + i] : -1;
    if ((unsigned)d < (unsigned)nd) {
      const float* e = E + (long)d * D;
      float acc = 0.f;
      if (vec) {
        for (int j = 0; j < D; j += 4) {
          const f32x4 x = *(const f32x4*)(qs + j), y = *(const f32x4*)(e + j);
          acc = fmaf(x[0], y[0], acc);
          acc = fmaf(x[1], y[1], acc);
          acc = fmaf(x[2], y[2], acc);
          acc = fmaf(x[3], y[3], acc);
        }
      } else {
        for (int j = 0; j < D; ++j) acc = fmaf(qs[j], e[j], acc);
      }
      const float s = acc + 0.0f;
      const float a = cand_approx[(long)q * k1 + i];
      if (!(fabsf(s) <= 3.402823466e38f) || !(fabsf(a) <= 3.402823466e38f)) bad = 1;
      bool ok = !has_c || s < cl;                             // a NaN ceiling admits nothing
      if (ok && has_x) {
        const int64_t p = lower_bound(ex_doc, ex0, ex1, d);
        ok = !(p < ex1 && ex_doc[p] == d);
      }
      if (ok) {
        key = rank_key(dense_key(s), (uint32_t)d);
        atomicAdd(&nadm, 1);
      }
    }
    sbuf[i] = key;
  }
  __syncthreads();
  bitonic_desc<SR_THREADS, int>(sbuf, P);
  const int nsel = nadm;
  write_ranks<dense_unkey>(sbuf, min(nsel, hi), q, lo, hi, out_doc, out_score, out_found);
  if (tid == 0) {
    const double n2 = q_norm2[q], h2 = q_hat2[q], r2 = q_res2[q];
    const double nq_ = sqrt(n2), nh = sqrt(h2), rq = sqrt(r2);
    // the bound takes every product and partial sum of either pass to stay in the fp32 range: sum |q_j d_j| <= n_q N
    bool cert = !bad && d2_finite(n2) && d2_finite(h2) && d2_finite(r2) && d2_finite(dN) && d2_finite(dNh) &&
                d2_finite(dR) && nq_ * dN <= 0x1p127 && nh * dNh <= 0x1p127;
    if (cert && nd > k1) {
      // every doc the scan dropped has a(d) <= t, hence s(d) <= t + eps: DESIGN.md "Two-phase dense retrieval"
      const double m23 = (double)(2 * d2_dp(D)) * 0x1p-23, m24 = (double)D * 0x1p-24;
      const double g23 = m23 / (1.0 - m23), g24 = m24 / (1.0 - m24);
      double eps = nq_ * dR + rq * dNh + g23 * nh * dNh + g24 * nq_ * dN;
      eps = eps * (1.0 + 0x1p-20) + (double)D * 0x1p-100 * (1.0 + nh + dNh);
      const double t = (double)cand_approx[(long)q * k1 + k1 - 1];
      cert = nsel >= hi && (double)dense_unkey(rank_bits(sbuf[hi - 1])) > t + eps;   // false for a NaN on either side
    }
    certified[q] = cert ? 1 : 0;
  }
}

}  // namespace

extern "C" int snx_dense2_prepare(const float* X, int32_t n, int32_t D, uint16_t* Xb, double* norm2, double* hat2,
                                  double* res2, hipStream_t st) {
  if (n < 0 || D < 1 || D > DN_DMAX) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!X || !Xb || !norm2 || !hat2 || !res2 || ((uintptr_t)Xb & 15) != 0) return SNX_E_ARG;
  hipLaunchKernelGGL(dn2_prepare_kernel, dim3(cdiv(n, D2_PREP_THREADS)), dim3(D2_PREP_THREADS), 0, st, X, n, D, d2_dp(D),
                     Xb, norm2, hat2, res2);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" size_t snx_dense2_workspace_bytes(int32_t nq, int32_t nd, int32_t k1, int32_t chunk_docs) {
  if (nq <= 0 || nd < 0 || k1 <= 0 || k1 > SR_KMAX || chunk_docs < 0 || (chunk_docs > 0 && chunk_docs < DN_TILE))
    return 0;
  return d2_workspace(nq, d2_plan(nq, nd, chunk_docs).nsplit, dn_cap(k1));
}

extern "C" int snx_dense2_scan(const uint16_t* Qb, int32_t nq, const uint16_t* Eb, int32_t nd, int32_t D, int32_t k1,
                               int32_t chunk_docs, int32_t* cand_doc, float* cand_approx, void* workspace,
                               size_t ws_bytes, hipStream_t st) {
  if (nq < 0 || nd < 0 || D < 1 || D > DN_DMAX || k1 < 1 || k1 > SR_KMAX || chunk_docs < 0 ||
      (chunk_docs > 0 && chunk_docs < DN_TILE))
    return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  if (!Qb || (nd > 0 && !Eb) || !cand_doc || !cand_approx) return SNX_E_ARG;
  if (((uintptr_t)Qb & 15) != 0 || ((uintptr_t)Eb & 15) != 0) return SNX_E_ARG;
  const SplitPlan p = d2_plan(nq, nd, chunk_docs);
  const int cap = dn_cap(k1);
  const long blocks = (long)p.qtiles * p.nsplit;
  if (blocks > 0x7FFFFFFFL || (long)nq * p.nsplit > 0x7FFFFFFFL) return SNX_E_SHAPE;
  const size_t need = d2_workspace(nq, p.nsplit, cap);
  if (!workspace || ws_bytes < need) return SNX_E_ARG;
  const size_t lists = (size_t)nq * (size_t)p.nsplit;
  unsigned long long* cand = (unsigned long long*)workspace;
  int32_t* ccount = (int32_t*)((char*)workspace + align256(lists * (size_t)cap * 8));
  hipLaunchKernelGGL(dn2_scan_kernel, dim3((unsigned)blocks), dim3(DN_THREADS), 0, st, Qb, nq, Eb, nd, d2_dp(D),
                     p.qtiles, p.split_tiles, p.nsplit, k1, cap, cand, ccount);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(dn2_merge_kernel, dim3(nq), dim3(SR_THREADS), 0, st, (const unsigned long long*)cand,
                     (const int32_t*)ccount, p.nsplit, cap, k1, cand_doc, cand_approx);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_dense2_rescore(const float* Q, int32_t nq, const float* E, int32_t nd, int32_t D,
                                  const int32_t* cand_doc, const float* cand_approx, int32_t k1, const double* q_norm2,
                                  const double* q_hat2, const double* q_res2, double doc_norm, double doc_hat,
                                  double doc_res, const int64_t* ex_ptr, const int32_t* ex_doc, const float* ceiling,
                                  int32_t lo, int32_t hi, int32_t* out_doc, float* out_score, int32_t* out_found,
                                  uint8_t* certified, hipStream_t st) {
  if (nq < 0 || nd < 0 || D < 1 || D > DN_DMAX || k1 < 1 || k1 > SR_KMAX || lo < 0 || hi <= lo || hi > k1)
    return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  if (!Q || (nd > 0 && !E) || !cand_doc || !cand_approx || !q_norm2 || !q_hat2 || !q_res2 || !out_doc || !out_score ||
      !out_found || !certified || (ex_ptr && !ex_doc))
    return SNX_E_ARG;
  const int vec = D % 4 == 0 && ((uintptr_t)Q & 15) == 0 && ((uintptr_t)E & 15) == 0;
  hipLaunchKernelGGL(dn2_rescore_kernel, dim3(nq), dim3(SR_THREADS), 0, st, Q, E, nd, D, vec, cand_doc, cand_approx, k1,
                     q_norm2, q_hat2, q_res2, doc_norm, doc_hat, doc_res, ex_ptr, ex_doc, ceiling, lo, hi, out_doc,
                     out_score, out_found, certified);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
