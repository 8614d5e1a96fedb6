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
// That loop, the order key, the admission of a score and the list compaction live in dense_common.h, which ivf.hip's
// scan shares.  Every score of a tile goes from the accumulator through the query's
// running threshold key; a wave whose 64 scores of one accumulator register all fail leaves on the ballot.  A survivor
// is appended (LDS atomic cursor) to the query's candidate list in the workspace, `cap` entries of (order key << 32 |
// ~doc).  When a list could overflow in the next tile the workgroup sorts it (bitonic, LDS), keeps the best k and raises
// the threshold to the k-th key (exact: docs ascend along the walk).  At the end every list is sorted and cut to k;
// dn_merge_kernel selects over the splits as sr_merge_kernel does over chunks (merge_lists of sparse_common.h: equal
// keys are met in doc order).  The target rank is an integer count over the same scores.  The band
// search is the same kernel: a survivor is dropped when the query's exclusion row holds it (binary search) and a score
// not below the ceiling never survives.
#include "dense_common.h"
#include "snx.h"

namespace {

constexpr int DN_WG_TARGET = 512;              // default split count: enough workgroups for two per CU ...
constexpr int DN_SPLITS_MAX = 64;              // ... but no more than this many lists per query to merge
constexpr int DN_PAIR_THREADS = 256;

inline SplitPlan dn_plan(int32_t nq, int32_t nd, int32_t chunk_docs) {
  return split_plan(nq, nd, chunk_docs, DN_TILE, DN_WG_TARGET, DN_SPLITS_MAX);
}

inline size_t dn_workspace(int32_t nq, int nsplit, int cap) {
  const size_t lists = (size_t)nq * (size_t)nsplit;
  return align256(lists * (size_t)cap * 8) + 2 * align256(lists * 4);
}

__global__ __launch_bounds__(DN_THREADS, 2) void dn_search_kernel(
    const float* __restrict__ Q, int32_t nq, const float* __restrict__ E, int32_t nd, int32_t D, int32_t vec,
    int32_t qtiles, int32_t split_tiles, int32_t nsplit, int32_t k, int32_t cap, const int32_t* __restrict__ target,
    const float* __restrict__ tscore, const int64_t* __restrict__ ex_ptr, const int32_t* __restrict__ ex_doc,
    const float* __restrict__ ceiling, unsigned long long* cand, int32_t* __restrict__ ccount,
    int32_t* __restrict__ rcount) {
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
  auto list = [&](int row) { return cand + list0 + (size_t)row * list_step; };
  auto compact = [&](int row) { dn_compact(list(row), cnt[row], thr[row], k, cap); };
  auto qrow = [&](int r) -> long { return q0 + r < nq ? q0 + r : -1; };

  for (long tile = t0; tile < t1; ++tile) {
    const long n0 = tile * DN_TILE;
    auto drow = [&](int r) -> long { return n0 + r < nd ? n0 + r : -1; };
    f32x16 acc[2][2];
    dn_tile_scores(Q, qrow, vec, E, drow, vec, D, acc);
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
          if (has_t) {                                       // 1 + #{s_d > s_t} + #{d < t: s_d == s_t}: this tile's share
            const bool ahead = ok && (s > tsv || (s == tsv && doc < ttv));
            const unsigned long long m = __ballot(ahead);
            if (m != 0ull && c == 0) {
              const int mine = __popc((uint32_t)(h ? m >> 32 : m));
              if (mine) atomicAdd(&rcnt[row], mine);
            }
          }
          dn_admit(ok, s, (int32_t)doc, th, has_c, cl, has_x, ex_doc, exa[row], exb[row], cnt[row], list(row), cap);
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

// the top `hi` over a query's per-split lists (each sorted, at most hi long), ranks lo .. hi-1 written: merge_lists, as
// sr_merge_kernel runs it over chunks.  Equal keys are met in doc order (splits ascend; a sorted list has its ties
// lowest doc first).
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
  const RankLists lists = {cand + (size_t)base * (size_t)cap, ccount + base, cap, hi};
  merge_lists<dense_unkey>(lists, nsplit, S, q, lo, hi, out_doc, out_score, out_found);
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
  const SplitPlan p = dn_plan(nq, nd, chunk_docs);
  const int cap = dn_cap(hi);
  const long blocks = (long)p.qtiles * p.nsplit;
  if (blocks > 0x7FFFFFFFL || (long)nq * p.nsplit > 0x7FFFFFFFL) return SNX_E_SHAPE;
  const size_t need = dn_workspace(nq, p.nsplit, cap);
  if (!workspace || ws_bytes < need) return SNX_E_ARG;
  const size_t lists = (size_t)nq * (size_t)p.nsplit;
  char* w = (char*)workspace;
  unsigned long long* cand = (unsigned long long*)w;
  int32_t* ccount = (int32_t*)(w + align256(lists * (size_t)cap * 8));
  int32_t* rcount = (int32_t*)((char*)ccount + align256(lists * 4));
  const int vec = dn_vec(Q, E, D);
  if (target) {
    hipLaunchKernelGGL(dn_pair_kernel, dim3(cdiv(nq, DN_PAIR_THREADS)), dim3(DN_PAIR_THREADS), 0, st, Q, nq, E, nd, D,
                       vec, (const int32_t*)nullptr, target, (int64_t)nq, out_tscore);
    SNX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(dn_search_kernel, dim3((unsigned)blocks), dim3(DN_THREADS), 0, st, Q, nq, E, nd, D, vec, p.qtiles,
                     p.split_tiles, p.nsplit, hi, cap, target, (const float*)out_tscore, ex_ptr, ex_doc, ceiling, cand,
                     ccount, rcount);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(dn_merge_kernel, dim3(nq), dim3(SR_THREADS), 0, st, (const unsigned long long*)cand,
                     (const int32_t*)ccount, (const int32_t*)rcount, nd, p.nsplit, cap, lo, hi, target, out_doc,
                     out_score, out_rank, out_tscore, out_found);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

inline size_t dn_workspace_bytes(int32_t nq, int32_t nd, int32_t k, int32_t chunk_docs) {
  if (nq <= 0 || nd < 0 || k <= 0 || k > SR_KMAX || chunk_docs < 0 || (chunk_docs > 0 && chunk_docs < DN_TILE)) return 0;
  return dn_workspace(nq, dn_plan(nq, nd, chunk_docs).nsplit, dn_cap(k));
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
