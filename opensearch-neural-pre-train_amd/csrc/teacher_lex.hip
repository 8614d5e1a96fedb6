// The lexical (sparse) output of the dense teacher: BGE-M3's sparse_linear head, the per-sequence lexical weights and the
// lexical matching score (include/snx.h "lexical teacher scores").  Three kernels, none of them a GEMM:
//   teacher_tw_kernel   tw[t] = max(0, <h[t], w_s> + b_s).  One wave per token row on the RowVec toolkit of rows.h, 16 B per
//                       lane, one streaming read of the fp32 residual stream.  An output width of 1 fits no matrix
//                       instruction: the row is a dot product, a lane's fma chain and one wave_sum.
//   tl_unique_kernel    lw[s][v] = max of tw over the occurrences of id v in sequence s.  One workgroup per sequence stages
//                       64-bit keys (id << 32 | weight bits) in LDS, sorts them ascending (text_bitonic_asc) and keeps the
//                       last key of every run of one id: weights are >= 0, so their bit patterns order as unsigned integers
//                       and that key holds the maximum.  The survivors (id not unused, weight > 0) are compacted by a
//                       ballot and a per-wave count into the sequence's own slots of a [T] output, ascending id: no scan
//                       over sequences, no second pass, nothing of vocabulary size.
//   tl_pair_kernel      lex(a, b) over a compact CSR.  One wave per pair, four pairs per workgroup; the lanes stride over the
//                       shorter term list and binary-search the longer one, which sits in L2.  A lane adds its products in
//                       ascending order of its own items, then one wave_sum: the order is a function of the two lists alone.
// The file is new with its kernels and is built without packed fp32 VALU forms (snx/asmcheck.py FILE_FLAGS).
#include "common.h"
#include "rows.h"
#include "sparse_common.h"   // pow2_at_least, fbits, bitsf, lower_bound
#include "text_common.h"
#include "teacher_lex.h"
#include "snx.h"

namespace {

constexpr int TL_THREADS = 256;
constexpr int TL_WAVES = TL_THREADS / 64;
constexpr int TL_TAIL = 32;                         // bytes behind the keys: the per-wave counts and the running count
constexpr int TL_PAIRS_PER_BLOCK = TL_THREADS / 64; // one wave per pair
constexpr unsigned long long TL_NONE = ~0ull;       // padding of the sort: behind every key

template <int NV>
__global__ __launch_bounds__(256) void teacher_tw_kernel(const float* __restrict__ h, const float* __restrict__ w, float b,
                                                         float* __restrict__ tw, int T, int H) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (t >= T) return;
  RowVec<NV> x, ws;
  x.load_f32(h + (long)t * H, lane);
  ws.load_f32(w, lane);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) s = fmaf(x.v[i][e], ws.v[i][e], s);
  s = wave_sum(s) + b;
  if (lane == 0) tw[t] = s > 0.f ? s : 0.f;         // relu; a -0.0f or a NaN becomes +0.0f
}

struct TlUnused {
  int32_t n;
  int32_t id[LEX_MAX_UNUSED];
};

__global__ __launch_bounds__(TL_THREADS) void tl_unique_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tw,
                                                               const int32_t* __restrict__ cu, TlUnused unused,
                                                               int32_t* __restrict__ lex_id, float* __restrict__ lex_w,
                                                               int32_t* __restrict__ lex_cnt, int T, int cap) {
  extern __shared__ unsigned long long keys[];      // cap keys, then TL_TAIL bytes
  int* const wcnt = (int*)(keys + cap);             // [TL_WAVES]
  int* const run = wcnt + TL_WAVES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x;
  const int a0 = cu[s];
  int n = cu[s + 1] - a0;
  if (a0 < 0 || n < 0 || (long)a0 + n > T) {        // block-uniform: a cu_seqlens the contract rules out writes nothing
    if (tid == 0) lex_cnt[s] = 0;
    return;
  }
  const int slots = n;
  if (n > cap) n = 0;                               // block-uniform: max_seqlen was understated, an empty term list
  const int P = pow2_at_least(n);
  for (int e = tid; e < P; e += TL_THREADS) {
    unsigned long long k = TL_NONE;
    if (e < n) {
      const float v = tw[a0 + e];
      k = (unsigned long long)(uint32_t)ids[a0 + e] << 32 | (v > 0.f ? fbits(v) : 0u);
    }
    keys[e] = k;
  }
  if (tid == 0) *run = 0;
  __syncthreads();
  text_bitonic_asc<TL_THREADS>(keys, (int64_t)P);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int base = 0; base < n; base += TL_THREADS) {           // block-uniform bounds
    const int i = base + tid;
    bool keep = false;
    unsigned long long k = 0;
    if (i < n) {
      k = keys[i];
      const uint32_t id = (uint32_t)(k >> 32);
      keep = (i == n - 1 || (uint32_t)(keys[i + 1] >> 32) != id) && (uint32_t)k != 0u;   // its id's maximum, and > 0
#pragma unroll
      for (int u = 0; u < LEX_MAX_UNUSED; ++u) keep = keep && !(u < unused.n && (int32_t)id == unused.id[u]);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    if (keep) {
      int pos = *run + __popcll(m & below);
      for (int w = 0; w < wave; ++w) pos += wcnt[w];
      lex_id[a0 + pos] = (int32_t)(k >> 32);
      lex_w[a0 + pos] = bitsf((uint32_t)k);
    }
    __syncthreads();
    if (tid == 0) {
      int r = *run;
      for (int w = 0; w < TL_WAVES; ++w) r += wcnt[w];
      *run = r;
    }
    __syncthreads();
  }
  const int cnt = *run;
  for (int i = cnt + tid; i < slots; i += TL_THREADS) {        // the rest of the sequence's slots
    lex_id[a0 + i] = -1;
    lex_w[a0 + i] = 0.f;
  }
  if (tid == 0) lex_cnt[s] = cnt;
}

__global__ __launch_bounds__(TL_THREADS) void tl_pair_kernel(const int32_t* __restrict__ ids, const float* __restrict__ w,
                                                             const int64_t* __restrict__ ptr,
                                                             const int32_t* __restrict__ pair_q,
                                                             const int32_t* __restrict__ pair_d, int64_t npairs,
                                                             float* __restrict__ score) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * TL_PAIRS_PER_BLOCK + (threadIdx.x >> 6);
  if (p >= npairs) return;                                     // wave-uniform
  const int q = pair_q[p], d = pair_d[p];
  int64_t s0 = ptr[q], s1 = ptr[q + 1], l0 = ptr[d], l1 = ptr[d + 1];
  if (l1 - l0 < s1 - s0) {                                     // stride over the shorter list; ties: the query's
    int64_t t = s0; s0 = l0; l0 = t;
    t = s1; s1 = l1; l1 = t;
  }
  float acc = 0.f;
  for (int64_t j = s0 + lane; j < s1; j += 64) {               // ascending order of the lane's own items
    const int32_t term = ids[j];
    const int64_t at = lower_bound(ids, l0, l1, term);
    if (at < l1 && ids[at] == term) acc += mul_rn(w[j], w[at]);   // an fp32 product, an fp32 sum: never contracted
  }
  acc = wave_sum(acc);
  if (lane == 0) score[p] = acc;
}

// the device image of a scorer call in the workspace: lex_ptr, pair_q, pair_d
struct TlPlan {
  size_t ptr, pq, pd, total;
  TlPlan(int32_t nseq, int64_t npairs) {
    Arena a;
    ptr = a.take(((size_t)nseq + 1) * 8);
    pq = a.take((size_t)npairs * 4);
    pd = a.take((size_t)npairs * 4);
    total = a.off;
  }
};

inline bool tl_bad_shape(int32_t nseq, int64_t npairs) { return nseq <= 0 || npairs < 0 || npairs > 0x7FFFFFFFL; }

LdsOptIn g_unique_lds;

}  // namespace

extern "C" int snx_teacher_token_weights(const float* h, const float* sparse_w, float sparse_b, float* tw, int32_t T,
                                         int32_t H, hipStream_t st) {
  if (!h || !sparse_w || !tw || T <= 0) return SNX_E_ARG;
  if (bad_h(H)) return SNX_E_SHAPE;
  if ((((uintptr_t)h | (uintptr_t)sparse_w) & 15) != 0 || ((uintptr_t)tw & 3) != 0) return SNX_E_ARG;
  DISPATCH_NV(H, hipLaunchKernelGGL((teacher_tw_kernel<NV>), dim3(cdiv(T, ROWS_PER_BLOCK)), dim3(256), 0, st, h, sparse_w,
                                    sparse_b, tw, T, H));
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_lexical_unique(const int64_t* ids, const float* tw, const int32_t* cu_seqlens, const int32_t* unused_ids,
                                  int32_t n_unused, int32_t* lex_id, float* lex_w, int32_t* lex_cnt, int32_t T,
                                  int32_t nseq, int32_t max_seqlen, hipStream_t st) {
  if (!ids || !tw || !cu_seqlens || !lex_id || !lex_w || !lex_cnt || T <= 0 || nseq <= 0 || nseq > T || max_seqlen <= 0 ||
      n_unused < 0 || (n_unused > 0 && !unused_ids))
    return SNX_E_ARG;
  if (max_seqlen > LEX_MAX_SEQLEN || n_unused > LEX_MAX_UNUSED) return SNX_E_SHAPE;
  TlUnused unused = {};
  unused.n = n_unused;
  for (int i = 0; i < n_unused; ++i) unused.id[i] = unused_ids[i];
  const int cap = pow2_at_least((int)max_seqlen);
  const size_t lds = (size_t)cap * 8 + TL_TAIL;
  RC(g_unique_lds.ensure((const void*)tl_unique_kernel, LEX_MAX_SEQLEN * 8 + TL_TAIL));
  hipLaunchKernelGGL(tl_unique_kernel, dim3(nseq), dim3(TL_THREADS), lds, st, ids, tw, cu_seqlens, unused, lex_id, lex_w,
                     lex_cnt, T, cap);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" size_t snx_lexical_pairs_workspace_bytes(int32_t nseq, int64_t npairs) {
  return tl_bad_shape(nseq, npairs) ? 0 : TlPlan(nseq, npairs).total;
}

extern "C" int snx_lexical_pairs(const int32_t* ids, const float* w, int64_t nterms, const int64_t* lex_ptr, int32_t nseq,
                                 const int32_t* pair_q, const int32_t* pair_d, int64_t npairs, float* score,
                                 void* workspace, size_t ws_bytes, hipStream_t st) {
  if (tl_bad_shape(nseq, npairs) || nterms < 0) return SNX_E_SHAPE;
  if (npairs == 0) return SNX_OK;
  if (!lex_ptr || !pair_q || !pair_d || !score || !workspace || (nterms > 0 && (!ids || !w)) ||
      ((uintptr_t)workspace & 15) != 0)
    return SNX_E_ARG;
  // the three index arrays are host memory (pageable, as for snx_maxsim_pairs): everything a kernel will trust is checked
  // here, before any launch
  if (lex_ptr[0] != 0 || lex_ptr[nseq] > nterms) return SNX_E_ARG;
  for (int s = 0; s < nseq; ++s)
    if (lex_ptr[s + 1] < lex_ptr[s]) return SNX_E_ARG;
  for (int64_t p = 0; p < npairs; ++p)
    if ((uint32_t)pair_q[p] >= (uint32_t)nseq || (uint32_t)pair_d[p] >= (uint32_t)nseq) return SNX_E_ARG;
  const TlPlan plan(nseq, npairs);
  if (ws_bytes < plan.total) return SNX_E_ARG;
  char* ws = (char*)workspace;
  const struct { size_t off; const void* src; size_t bytes; } up[3] = {
      {plan.ptr, lex_ptr, ((size_t)nseq + 1) * 8}, {plan.pq, pair_q, (size_t)npairs * 4}, {plan.pd, pair_d, (size_t)npairs * 4}};
  for (const auto& u : up) {
    const hipError_t e = hipMemcpyAsync(ws + u.off, u.src, u.bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(tl_pair_kernel, dim3(cdiv(npairs, TL_PAIRS_PER_BLOCK)), dim3(TL_THREADS), 0, st, ids, w,
                     (const int64_t*)(ws + plan.ptr), (const int32_t*)(ws + plan.pq), (const int32_t*)(ws + plan.pd), npairs,
                     score);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
