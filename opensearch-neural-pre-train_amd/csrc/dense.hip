// Exact dense retrieval (include/snx.h "exact dense retrieval"): teacher scores, dense hard-negative search and the dense
// rows of the hybrid benchmark, over fp32 embeddings that arrive as arrays.  The reference forms
// torch.mm(q_batch[4096, D], doc_embs.T) -- a [4096, n_docs] fp32 matrix -- and then torch.topk
// (ref:scripts/mine_multi_negatives.py:141-222); here the scores never leave the registers they are born in.
//
// Score (the ABI): acc = fmaf(Q[q,j], E[d,j], acc) for j ascending from +0, then acc + 0.0f.  v_mfma_f32_32x32x2_f32 is bit
// for bit that chain (f32_path.hip, tests/test_gpu_f32.py), zero padding of a ragged D changes nothing (fmaf(0, 0, acc) is
// acc up to the sign of a zero, which the final + 0.0f settles), so dn_search_kernel (MFMA) and dn_pair_kernel (a serial
// loop) return the same bits.
//
// Search: a workgroup owns 128 queries and one split of the doc range.  It walks the split in tiles of 128 docs with the
// 128x128x16 fp32 MFMA loop of f32_path.hip (four waves of 2 x 2 accumulators, register prefetch, double-buffered LDS).
// Every score of a tile goes from the accumulator through the query's running threshold key; a wave whose 64 scores of
// one accumulator register all fail leaves on the ballot.  A survivor is appended (LDS atomic cursor) to the query's
// candidate list in the workspace, `cap` entries of (order key << 32 | ~doc).  When a list could overflow in the next
// tile the workgroup sorts it (bitonic, LDS), keeps the best k and raises the threshold to the k-th key: docs ascend
// along the walk, so a later doc that only ties the threshold loses to the k already kept, and `key > threshold` is
// exact.  At the end every list is sorted and cut to k; dn_merge_kernel selects over the splits as sr_merge_kernel does
// over chunks (radix_select / ordered_take of sparse_common.h: equal keys are met in doc order).  The target rank is an
// integer count over the same scores.  The band search is the same kernel: a survivor is dropped when the query's
// exclusion row holds it (binary search) and a score not below the ceiling never survives.
//
// Order key: the usual monotone map of fp32 bits to uint32 (negatives: all bits flipped; others: sign bit set), since
// every doc is a candidate whatever its sign; it is never 0 for a number, so 0 stays radix_select's "no entry".
#include "sparse_common.h"
#include "snx.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int DN_THREADS = 256;
constexpr int DN_TILE = 128;                   // query rows and doc rows of a workgroup's tile
constexpr int DN_KT = 16;                      // K per LDS stage
constexpr int DN_PITCH = 132;                  // LDS row pitch (floats), as the 128-wide tiles of f32_path.hip
constexpr int DN_CAP_MAX = 2048;               // candidate list entries for k = 1024
constexpr int DN_DMAX = 4096;
constexpr int DN_WG_TARGET = 512;              // default split count: enough workgroups for two per CU ...
constexpr int DN_SPLITS_MAX = 64;              // ... but no more than this many lists per query to merge
constexpr int DN_PAIR_THREADS = 256;

struct DnPlan {
  int qtiles, split_tiles, nsplit, cap;
  long tiles;
};

inline DnPlan dn_plan(int32_t nq, int32_t nd, int32_t k, int32_t chunk_docs) {
  DnPlan p;
  p.qtiles = (int)((nq + (long)DN_TILE - 1) / DN_TILE);
  p.tiles = (nd + (long)DN_TILE - 1) / DN_TILE;
  if (chunk_docs > 0) {
    p.split_tiles = (int)((chunk_docs + (long)DN_TILE - 1) / DN_TILE);
  } else {
    long want = (DN_WG_TARGET + (long)p.qtiles - 1) / (p.qtiles > 0 ? p.qtiles : 1);
    if (want > DN_SPLITS_MAX) want = DN_SPLITS_MAX;
    if (want > p.tiles) want = p.tiles;
    if (want < 1) want = 1;
    p.split_tiles = (int)((p.tiles + want - 1) / want);
  }
  if (p.split_tiles < 1) p.split_tiles = 1;
  const long ns = (p.tiles + p.split_tiles - 1) / p.split_tiles;
  p.nsplit = (int)(ns < 1 ? 1 : (ns > 0x7FFFFFFFL ? 0x7FFFFFFFL : ns));
  p.cap = (int)pow2_at_least((long)(2 * k > 512 ? 2 * k : 512));
  return p;
}

inline size_t dn_workspace(int32_t nq, const DnPlan& p) {
  const size_t lists = (size_t)nq * (size_t)p.nsplit;
  return align256(lists * (size_t)p.cap * 8) + 2 * align256(lists * 4);
}

// monotone map fp32 -> uint32 (larger float, larger key) and back
__device__ __forceinline__ uint32_t dense_key(float s) {
  const uint32_t b = fbits(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dense_unkey(uint32_t key) {
  return bitsf((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// this thread's share of a 128 x 16 operand tile of a row-major [nrows, D] matrix: rows r and r + 64, 4 k each; rows past
// the matrix and k past D read as zero
__device__ __forceinline__ void dn_fetch(const float* __restrict__ P, long nrows, long row0, int D, int k0, int vec,
                                         int t, float (&v)[8]) {
  const int kk = k0 + (t & 3) * 4;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long row = row0 + (t >> 2) + 64 * i;
    if (row < nrows && vec && kk < D) {                      // vec: D % 4 == 0 and 16-byte aligned rows
      const f32x4 x = *(const f32x4*)(P + row * D + kk);
      v[4 * i] = x[0]; v[4 * i + 1] = x[1]; v[4 * i + 2] = x[2]; v[4 * i + 3] = x[3];
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[4 * i + u] = (row < nrows && kk + u < D) ? P[row * D + kk + u] : 0.f;
    }
  }
}
__device__ __forceinline__ void dn_put(int t, const float (&v)[8], float (*S)[DN_PITCH]) {
  const int kk = (t & 3) * 4;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (t >> 2) + 64 * i;
#pragma unroll
    for (int u = 0; u < 4; ++u) S[kk + u][r] = v[4 * i + u];
  }
}

__global__ __launch_bounds__(DN_THREADS, 2) void dn_search_kernel(
    const float* __restrict__ Q, int32_t nq, const float* __restrict__ E, int32_t nd, int32_t D, int32_t vec,
    int32_t qtiles, int32_t split_tiles, int32_t nsplit, int32_t k, int32_t cap, const int32_t* __restrict__ target,
    const float* __restrict__ tscore, const int64_t* __restrict__ ex_ptr, const int32_t* __restrict__ ex_doc,
    const float* __restrict__ ceiling, unsigned long long* cand, int32_t* __restrict__ ccount,
    int32_t* __restrict__ rcount) {
  __shared__ __attribute__((aligned(16))) float As[2][DN_KT][DN_PITCH];
  __shared__ __attribute__((aligned(16))) float Bs[2][DN_KT][DN_PITCH];
  __shared__ unsigned long long sbuf[DN_CAP_MAX];
  __shared__ int64_t exa[DN_TILE], exb[DN_TILE];
  __shared__ uint32_t thr[DN_TILE];
  __shared__ int cnt[DN_TILE], rcnt[DN_TILE], tt[DN_TILE];
  __shared__ float ts[DN_TILE], ceilv[DN_TILE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const int qt = (int)(blockIdx.x % (unsigned)qtiles), split = (int)(blockIdx.x / (unsigned)qtiles);
  const long q0 = (long)qt * DN_TILE;
  const long tiles = (nd + (long)DN_TILE - 1) / DN_TILE;
  const long t0 = (long)split * split_tiles;
  const long t1 = min(tiles, t0 + split_tiles);
  const bool has_t = target != nullptr, has_c = ceiling != nullptr, has_x = ex_ptr != nullptr;
  if (t < DN_TILE) {
    const long q = q0 + t;
    const bool ok = q < nq;
    thr[t] = 0u;
    cnt[t] = 0;
    rcnt[t] = 0;
    ts[t] = has_t && ok ? tscore[q] : 0.f;
    tt[t] = has_t && ok ? target[q] : 0;
    ceilv[t] = has_c && ok ? ceiling[q] : 0.f;
    exa[t] = has_x && ok ? ex_ptr[q] : 0;
    exb[t] = has_x && ok ? ex_ptr[q + 1] : 0;
  }
  __syncthreads();
  // the candidate list of query row `row`: cand + ((q0 + row) * nsplit + split) * cap
  const size_t list0 = ((size_t)q0 * (size_t)nsplit + (size_t)split) * (size_t)cap;
  const size_t list_step = (size_t)nsplit * (size_t)cap;
  const int nk = (D + DN_KT - 1) / DN_KT;

  // sort the list of `row`, keep the best k, raise its threshold
  auto compact = [&](int row) {
    const int n = cnt[row];
    unsigned long long* b = cand + list0 + (size_t)row * list_step;
    for (int i = t; i < cap; i += DN_THREADS) sbuf[i] = i < n ? b[i] : 0ull;
    __syncthreads();
    bitonic_desc<DN_THREADS, int>(sbuf, cap);
    const int m = min(n, k);
    for (int i = t; i < m; i += DN_THREADS) b[i] = sbuf[i];
    if (t == 0) {
      cnt[row] = m;
      if (n >= k) thr[row] = rank_bits(sbuf[k - 1]);
    }
    __syncthreads();
  };

  for (long tile = t0; tile < t1; ++tile) {
    const long n0 = tile * DN_TILE;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float va[8], vb[8];
    dn_fetch(Q, nq, q0, D, 0, vec, t, va);
    dn_fetch(E, nd, n0, D, 0, vec, t, vb);
    dn_put(t, va, As[0]);
    dn_put(t, vb, Bs[0]);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) {
        dn_fetch(Q, nq, q0, D, (kt + 1) * DN_KT, vec, t, va);
        dn_fetch(E, nd, n0, D, (kt + 1) * DN_KT, vec, t, vb);
      }
#pragma unroll
      for (int s = 0; s < DN_KT / 2; ++s) {                  // k ascending: the ABI's chain
        const float a0 = As[cur][2 * s + h][wm * 64 + c], a1 = As[cur][2 * s + h][wm * 64 + 32 + c];
        const float b0 = Bs[cur][2 * s + h][wn * 64 + c], b1 = Bs[cur][2 * s + h][wn * 64 + 32 + c];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
      if (kt + 1 < nk) {
        dn_put(t, va, As[cur ^ 1]);
        dn_put(t, vb, Bs[cur ^ 1]);
      }
      __syncthreads();
    }
    // acc[i][j][r] = s(q0 + 64 wm + 32 i + (r & 3) + 8 (r >> 2) + 4 h, n0 + 64 wn + 32 j + c)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const bool rok = q0 + row < nq;
        const uint32_t th = thr[row];
        const float cl = ceilv[row], tsv = ts[row];
        const int ttv = tt[row];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const long doc = n0 + wn * 64 + j * 32 + c;
          const bool ok = rok && doc < nd;
          const float s = acc[i][j][r] + 0.0f;
          const uint32_t key = dense_key(s);
          if (has_t) {                                       // 1 + #{s_d > s_t} + #{d < t: s_d == s_t}: this tile's share
            const bool ahead = ok && (s > tsv || (s == tsv && doc < ttv));
            const unsigned long long m = __ballot(ahead);
            if (m != 0ull && c == 0) {
              const int mine = __popc((uint32_t)(h ? m >> 32 : m));
              if (mine) atomicAdd(&rcnt[row], mine);
            }
          }
          const bool pass = ok && key > th && (!has_c || s < cl);      // a NaN ceiling admits nothing
          if (__ballot(pass) != 0ull && pass) {
            bool excluded = false;
            if (has_x) {
              const int64_t e1 = exb[row];
              const int64_t p = lower_bound(ex_doc, exa[row], e1, (int32_t)doc);
              excluded = p < e1 && ex_doc[p] == (int32_t)doc;
            }
            if (!excluded) {
              const int pos = atomicAdd(&cnt[row], 1);
              if (pos < cap) cand[list0 + (size_t)row * list_step + pos] = rank_key(key, (uint32_t)doc);
            }
          }
        }
      }
    __syncthreads();
    // a tile adds at most DN_TILE entries to a list: compact every list that the next tile could overflow
    for (int row = 0; row < DN_TILE && q0 + row < nq; ++row)
      if (__builtin_amdgcn_readfirstlane(cnt[row]) > cap - DN_TILE) compact(row);
  }
  for (int row = 0; row < DN_TILE && q0 + row < nq; ++row) compact(row);
  if (t < DN_TILE && q0 + t < nq) {
    const size_t slot = (size_t)(q0 + t) * (size_t)nsplit + (size_t)split;
    ccount[slot] = cnt[t];
    rcount[slot] = rcnt[t];
  }
}

// the top `hi` over a query's per-split lists (each sorted, at most hi long), ranks lo .. hi-1 written: sr_merge_kernel
// with lists in place of chunks.  Equal keys are met in doc order (splits ascend, and a list is in search order).
__global__ __launch_bounds__(SR_THREADS) void dn_merge_kernel(const unsigned long long* __restrict__ cand,
                                                              const int32_t* __restrict__ ccount,
                                                              const int32_t* __restrict__ rcount, int32_t nd,
                                                              int32_t nsplit, int32_t cap, int32_t lo, int32_t hi,
                                                              const int32_t* __restrict__ target,
                                                              int32_t* __restrict__ out_doc,
                                                              float* __restrict__ out_score,
                                                              int32_t* __restrict__ out_rank,
                                                              float* __restrict__ out_tscore,
                                                              int32_t* __restrict__ out_found) {
  __shared__ SelectSmem S;
  __shared__ unsigned long long sbuf[SR_KMAX];
  const int tid = threadIdx.x, q = blockIdx.x;
  const long base = (long)q * nsplit;
  if (target) {
    int local = 0;
    for (int s = tid; s < nsplit; s += SR_THREADS) local += rcount[base + s];
    const int r = block_sum(local, S.sh[0]);
    if (tid == 0) {
      const bool valid = (unsigned)target[q] < (unsigned)nd;
      out_rank[q] = valid ? 1 + r : 0;
      if (!valid) out_tscore[q] = 0.f;
    }
  }
  const unsigned long long* qcand = cand + (size_t)base * (size_t)cap;
  const int32_t* qcnt = ccount + base;
  auto at = [&](long f) -> unsigned long long {              // flat index split * hi + i
    const int s = (int)(f / hi), i = (int)(f - (long)s * hi);
    return i < qcnt[s] ? qcand[(size_t)s * (size_t)cap + i] : 0ull;
  };
  auto key = [&](long f) -> uint32_t { return rank_bits(at(f)); };
  const long n = (long)nsplit * hi;
  uint32_t thr;
  int need_eq, nsel;
  radix_select(key, n, hi, S, thr, need_eq, nsel);
  const int P = pow2_at_least(nsel);
  for (int i = tid; i < P; i += SR_THREADS) sbuf[i] = 0ull;
  __syncthreads();
  ordered_take(key, n, thr, need_eq, S, [&](long f, int pos) { sbuf[pos] = at(f); });
  bitonic_desc<SR_THREADS, int>(sbuf, P);
  const int w = hi - lo;
  int32_t* od = out_doc + (long)q * w;
  float* os = out_score + (long)q * w;
  for (int j = tid; j < w; j += SR_THREADS) {
    const int r = lo + j;
    if (r < nsel) {
      const unsigned long long e = sbuf[r];
      os[j] = dense_unkey(rank_bits(e));
      od[j] = rank_id(e);
    } else {
      os[j] = 0.f;
      od[j] = -1;
    }
  }
  if (out_found && tid == 0) out_found[q] = max(0, nsel - lo);
}

// s(q, d) of a list of pairs by the serial chain, one pair per thread; pair_q NULL: pair i belongs to query i
__global__ __launch_bounds__(DN_PAIR_THREADS) void dn_pair_kernel(const float* __restrict__ Q, int32_t nq,
                                                                  const float* __restrict__ E, int32_t nd, int32_t D,
                                                                  int32_t vec, const int32_t* __restrict__ pair_q,
                                                                  const int32_t* __restrict__ pair_d, int64_t n,
                                                                  float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * DN_PAIR_THREADS + threadIdx.x;
  if (p >= n) return;
  const int q = pair_q ? pair_q[p] : (int)p, d = pair_d[p];
  float acc = 0.f;
  if ((unsigned)q < (unsigned)nq && (unsigned)d < (unsigned)nd) {
    const float* a = Q + (long)q * D;
    const float* b = E + (long)d * D;
    if (vec) {
      for (int j = 0; j < D; j += 4) {
        const f32x4 x = *(const f32x4*)(a + j), y = *(const f32x4*)(b + j);
        acc = fmaf(x[0], y[0], acc);
        acc = fmaf(x[1], y[1], acc);
        acc = fmaf(x[2], y[2], acc);
        acc = fmaf(x[3], y[3], acc);
      }
    } else {
      for (int j = 0; j < D; ++j) acc = fmaf(a[j], b[j], acc);
    }
  }
  out[p] = acc + 0.0f;
}

inline int dn_vec(const float* Q, const float* E, int32_t D) {
  return D % 4 == 0 && ((uintptr_t)Q & 15) == 0 && ((uintptr_t)E & 15) == 0;
}

// both searches: lists per (query, split), then the merge
int dn_search(const float* Q, int32_t nq, const float* E, int32_t nd, int32_t D, const int32_t* target,
              const int64_t* ex_ptr, const int32_t* ex_doc, const float* ceiling, int32_t lo, int32_t hi,
              int32_t chunk_docs, int32_t* out_doc, float* out_score, int32_t* out_rank, float* out_tscore,
              int32_t* out_found, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (nq < 0 || nd < 0 || D < 1 || D > DN_DMAX || lo < 0 || hi <= lo || hi > SR_KMAX || chunk_docs < 0 ||
      (chunk_docs > 0 && chunk_docs < DN_TILE))
    return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  if (!Q || (nd > 0 && !E)) return SNX_E_ARG;
  const DnPlan p = dn_plan(nq, nd, hi, chunk_docs);
  const long blocks = (long)p.qtiles * p.nsplit;
  if (blocks > 0x7FFFFFFFL || (long)nq * p.nsplit > 0x7FFFFFFFL) return SNX_E_SHAPE;
  const size_t need = dn_workspace(nq, p);
  if (!workspace || ws_bytes < need) return SNX_E_ARG;
  const size_t lists = (size_t)nq * (size_t)p.nsplit;
  char* w = (char*)workspace;
  unsigned long long* cand = (unsigned long long*)w;
  int32_t* ccount = (int32_t*)(w + align256(lists * (size_t)p.cap * 8));
  int32_t* rcount = (int32_t*)((char*)ccount + align256(lists * 4));
  const int vec = dn_vec(Q, E, D);
  if (target) {
    hipLaunchKernelGGL(dn_pair_kernel, dim3(cdiv(nq, DN_PAIR_THREADS)), dim3(DN_PAIR_THREADS), 0, st, Q, nq, E, nd, D,
                       vec, (const int32_t*)nullptr, target, (int64_t)nq, out_tscore);
    SNX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(dn_search_kernel, dim3((unsigned)blocks), dim3(DN_THREADS), 0, st, Q, nq, E, nd, D, vec, p.qtiles,
                     p.split_tiles, p.nsplit, hi, p.cap, target, (const float*)out_tscore, ex_ptr, ex_doc, ceiling, cand,
                     ccount, rcount);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(dn_merge_kernel, dim3(nq), dim3(SR_THREADS), 0, st, (const unsigned long long*)cand,
                     (const int32_t*)ccount, (const int32_t*)rcount, nd, p.nsplit, p.cap, lo, hi, target, out_doc,
                     out_score, out_rank, out_tscore, out_found);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

inline size_t dn_workspace_bytes(int32_t nq, int32_t nd, int32_t k, int32_t chunk_docs) {
  if (nq <= 0 || nd < 0 || k <= 0 || k > SR_KMAX || chunk_docs < 0 || (chunk_docs > 0 && chunk_docs < DN_TILE)) return 0;
  return dn_workspace(nq, dn_plan(nq, nd, k, chunk_docs));
}

}  // namespace

extern "C" size_t snx_dense_search_workspace_bytes(int32_t nq, int32_t nd, int32_t k, int32_t chunk_docs) {
  return dn_workspace_bytes(nq, nd, k, chunk_docs);
}

extern "C" int snx_dense_search(const float* Q, int32_t nq, const float* E, int32_t nd, int32_t D, const int32_t* target,
                                int32_t k, int32_t chunk_docs, int32_t* out_doc, float* out_score, int32_t* out_rank,
                                float* out_tscore, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (!out_doc || !out_score) return SNX_E_ARG;
  if (target && (!out_rank || !out_tscore)) return SNX_E_ARG;
  if (k < 1) return SNX_E_SHAPE;
  return dn_search(Q, nq, E, nd, D, target, nullptr, nullptr, nullptr, 0, k, chunk_docs, out_doc, out_score, out_rank,
                   out_tscore, nullptr, workspace, ws_bytes, st);
}

extern "C" size_t snx_dense_search_band_workspace_bytes(int32_t nq, int32_t nd, int32_t hi, int32_t chunk_docs) {
  return dn_workspace_bytes(nq, nd, hi, chunk_docs);
}

extern "C" int snx_dense_search_band(const float* Q, int32_t nq, const float* E, int32_t nd, int32_t D,
                                     const int64_t* ex_ptr, const int32_t* ex_doc, const float* ceiling, int32_t lo,
                                     int32_t hi, int32_t chunk_docs, int32_t* out_doc, float* out_score,
                                     int32_t* out_found, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (!out_doc || !out_score || !out_found) return SNX_E_ARG;
  if (ex_ptr && !ex_doc) return SNX_E_ARG;
  return dn_search(Q, nq, E, nd, D, nullptr, ex_ptr, ex_doc, ceiling, lo, hi, chunk_docs, out_doc, out_score, nullptr,
                   nullptr, out_found, workspace, ws_bytes, st);
}

extern "C" int snx_dense_pair_scores(const float* Q, int32_t nq, const float* E, int32_t nd, int32_t D,
                                     const int32_t* pair_q, const int32_t* pair_d, int64_t npairs, float* out,
                                     hipStream_t st) {
  if (nq < 0 || nd < 0 || D < 1 || D > DN_DMAX || npairs < 0 || npairs > 0x7FFFFFFFL * (int64_t)DN_PAIR_THREADS)
    return SNX_E_SHAPE;
  if (npairs == 0) return SNX_OK;
  if (!pair_q || !pair_d || !out || (nq > 0 && !Q) || (nd > 0 && !E)) return SNX_E_ARG;
  hipLaunchKernelGGL(dn_pair_kernel, dim3((unsigned)((npairs + DN_PAIR_THREADS - 1) / DN_PAIR_THREADS)),
                     dim3(DN_PAIR_THREADS), 0, st, Q, nq, E, nd, D, dn_vec(Q, E, D), pair_q, pair_d, npairs, out);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
