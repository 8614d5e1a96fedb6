// Graph dense retrieval (include/snx.h "graph dense retrieval"): a deterministic fixed-degree graph of the CAGRA family
// over dense fp32 embeddings and a best-first beam over it, in the role of the HNSW field behind the reference's
// SemanticSearcher (ref:benchmark/index_manager.py:98-110, ref:benchmark/searchers.py:97-127).  Scores are dense.hip's:
// the fp32 fmaf chain over ascending dimensions from +0, then + 0.0f, here as a serial loop per lane (dn_pair_kernel's),
// so a graph hit carries the bits DenseIndex returns for the same (query, doc).
//
// Optimise (N -> F -> R -> G), integers only.  gr_forward_kernel: one workgroup per node u.  Its row of N goes into an LDS
// hash (id -> column); the rows N[v_i] are streamed once, coalesced, and every entry x = N[v_i][c] that is u's neighbour
// v_j with i < j and c < j is one detour of j (LDS integer add: a count, the order does not show).  Column j then ranks
// itself among (detour, j) by counting and writes F[u][rank].  gr_reverse_kernel: edge (u, p, v = F[u][p]) has the key
// g = p * nd + u, and R[v] is the `degree` smallest keys of v's in-edges in ascending order.  Every edge walks v's row
// with atomicMin, leaving the smaller value in the slot and carrying the larger one on: slot s ends as the minimum of
// everything that passed slot s - 1 except what stayed there, i.e. the (s + 1)-th smallest key, whatever order the edges
// arrive in.  gr_interleave_kernel: one thread per node interleaves F and R and drops repeats.
//
// Walk: one workgroup per query.  The pool P (<= ef keys), the query row, a visited table and the batch of one iteration
// live in LDS.  A pool key is (order key << 32 | (2^31 - 1 - doc) << 1 | unexpanded): descending keys are the ABI's order,
// and the flag rides in a bit that cannot change it (a doc is in P once).  An iteration marks the first `width`
// unexpanded keys (ballots of wave 0), reads their G rows, filters, scores one candidate per lane, appends the new keys
// behind the pool and sorts pool + batch with bitonic_desc.  Filter: the visited table is direct-mapped, stores full doc
// ids and may forget, so it never reports an unscored doc as scored; a doc met twice in a batch is settled by an exact
// LDS hash of the batch (whichever copy wins scores the same bits); and a scored candidate whose key is already in P
// (binary search by key: same doc, same bits) is dropped, so P never holds a doc twice.  A forgotten doc that is NOT in P
// was cut from a full P, whose worst key only rises: scoring it again sorts it behind the cut again.  The seeds go through
// the same batch path.  The final pool goes to the workspace as plain rank keys; gr_output_kernel applies the band's
// exclusion rows and ceiling to it (the walk never sees them) and writes the ranks with write_ranks.
#include "dense_common.h"
#include "snx.h"

namespace {

constexpr int GR_THREADS = SR_THREADS;         // write_ranks strides by SR_THREADS
constexpr int GR_KNN_MAX = 128;
constexpr int GR_DEGREE_MAX = 64;
constexpr int GR_EF_MAX = SR_KMAX;
constexpr int GR_WIDTH_MAX = 8;
constexpr int GR_FWD_THREADS = 256;
constexpr int GR_HASH = 256;                   // slots of the forward kernel's id -> column table (K <= 128)
constexpr int GR_BATCH_MAX = 1024;             // ids of one batch: the seeds (<= ef) or width * degree <= 512
constexpr int GR_BUF = 2048;                   // pool + batch, a power of two
constexpr int GR_SEEN = 4096;                  // slots of the visited table
constexpr int GR_UNIQ = 2048;                  // slots of the batch's exact table (>= 2 * GR_BATCH_MAX)
constexpr unsigned long long GR_EMPTY = ~0ull;

__device__ __forceinline__ uint32_t gr_hash(uint32_t x) { return (x * 2654435761u) >> 7; }

// ------------------------------------------------------------------------------------------------ optimise
__global__ __launch_bounds__(GR_FWD_THREADS) void gr_forward_kernel(const int32_t* __restrict__ N, int32_t nd, int32_t knn,
                                                                    int32_t degree, int32_t* __restrict__ F,
                                                                    unsigned long long* __restrict__ R) {
  __shared__ int32_t nu[GR_KNN_MAX], det[GR_KNN_MAX], hkey[GR_HASH], hval[GR_HASH];
  __shared__ int s_k;
  const int t = threadIdx.x;
  const long u = blockIdx.x;
  if (t < knn) {
    const int32_t x = N[u * knn + t];
    nu[t] = (uint32_t)x < (uint32_t)nd && x != u ? x : -1;
    det[t] = 0;
  }
  for (int i = t; i < GR_HASH; i += GR_FWD_THREADS) hkey[i] = -1;
  for (int i = t; i < degree; i += GR_FWD_THREADS) R[u * degree + i] = GR_EMPTY;
  __syncthreads();
  if (t == 0) {                                              // K: the valid entries lead the row
    int k = 0;
    while (k < knn && nu[k] >= 0) ++k;
    s_k = k;
  }
  __syncthreads();
  const int K = s_k;
  if (t < K) {
    const int32_t x = nu[t];
    uint32_t h = gr_hash((uint32_t)x) & (GR_HASH - 1);
    for (int probe = 0; probe < GR_HASH; ++probe) {
      const int32_t old = atomicCAS(&hkey[h], -1, x);
      if (old == -1 || old == x) { hval[h] = t; break; }
      h = (h + 1) & (GR_HASH - 1);
    }
  }
  __syncthreads();
  for (int f = t; f < K * knn; f += GR_FWD_THREADS) {
    const int i = f / knn, c = f - i * knn;
    const int32_t x = N[(long)nu[i] * knn + c];
    if (x < 0) continue;
    uint32_t h = gr_hash((uint32_t)x) & (GR_HASH - 1);
    for (int probe = 0; probe < GR_HASH; ++probe) {
      const int32_t key = hkey[h];
      if (key == -1) break;
      if (key == x) {
        const int j = hval[h];
        if (i < j && c < j) atomicAdd(&det[j], 1);
        break;
      }
      h = (h + 1) & (GR_HASH - 1);
    }
  }
  __syncthreads();
  if (t < K) {
    const int mine = det[t];
    int pos = 0;
    for (int j = 0; j < K; ++j) pos += det[j] < mine || (det[j] == mine && j < t);
    if (pos < degree) F[u * degree + pos] = nu[t];
  }
  for (int i = K + t; i < degree; i += GR_FWD_THREADS) F[u * degree + i] = -1;
}

__global__ __launch_bounds__(GR_FWD_THREADS) void gr_reverse_kernel(const int32_t* __restrict__ F, int32_t nd,
                                                                    int32_t degree, unsigned long long* R) {
  const long e = (long)blockIdx.x * GR_FWD_THREADS + threadIdx.x;
  if (e >= (long)nd * degree) return;
  const long u = e / degree;
  const int p = (int)(e - u * degree);
  const int32_t v = F[e];
  if ((uint32_t)v >= (uint32_t)nd) return;
  unsigned long long g = (unsigned long long)p * (unsigned long long)nd + (unsigned long long)u;
  unsigned long long* row = R + (long)v * degree;
  // the last slot only falls: a key that is not below it now cannot be among the kept ones
  if (g >= __hip_atomic_load(&row[degree - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  for (int s = 0; s < degree; ++s) {
    const unsigned long long old = atomicMin(&row[s], g);
    if (old == GR_EMPTY) break;
    if (old > g) g = old;                                    // the slot took g: carry what it held
  }
}

__global__ __launch_bounds__(GR_FWD_THREADS) void gr_interleave_kernel(const int32_t* __restrict__ F,
                                                                       const unsigned long long* __restrict__ R,
                                                                       int32_t nd, int32_t degree, int32_t* G) {
  const long v = (long)blockIdx.x * GR_FWD_THREADS + threadIdx.x;
  if (v >= nd) return;
  int32_t* row = G + v * degree;
  int n = 0;
  auto take = [&](int32_t x) {
    if (n >= degree) return;
    for (int i = 0; i < n; ++i)
      if (row[i] == x) return;
    row[n++] = x;
  };
  for (int t = 0; t < degree && n < degree; ++t) {
    const int32_t f = F[v * degree + t];
    if (f >= 0) take(f);
    const unsigned long long r = R[v * degree + t];
    if (r != GR_EMPTY) take((int32_t)(r % (unsigned long long)nd));
  }
  for (; n < degree; ++n) row[n] = -1;
}

struct GrOptLayout {
  size_t r, f, total;
};

inline GrOptLayout gr_opt_layout(int32_t nd, int32_t degree) {
  GrOptLayout l;
  const size_t cells = (size_t)nd * (size_t)degree;
  l.r = 0;
  l.f = align256(cells * 8);
  l.total = l.f + align256(cells * 4);
  return l;
}

inline bool gr_opt_shape_ok(int32_t nd, int32_t knn, int32_t degree) {
  return nd >= 0 && degree >= 1 && degree <= GR_DEGREE_MAX && knn >= degree && knn <= GR_KNN_MAX;
}

// ------------------------------------------------------------------------------------------------ walk
__device__ __forceinline__ unsigned long long gr_key(uint32_t bits, int32_t doc, uint32_t unexpanded) {
  return ((unsigned long long)bits << 32) | (unsigned long long)(((0x7FFFFFFFu - (uint32_t)doc) << 1) | unexpanded);
}
__device__ __forceinline__ int32_t gr_doc(unsigned long long key) {
  return (int32_t)(0x7FFFFFFFu - ((uint32_t)(key & 0xFFFFFFFFull) >> 1));
}

struct GrSmem {
  float q[DN_DMAX];
  unsigned long long buf[GR_BUF];
  int32_t seen[GR_SEEN], uniq[GR_UNIQ], cand[GR_BATCH_MAX], parent[GR_WIDTH_MAX];
  int npool, nnew, nparent;
};

// The batch cand[0 .. nraw): drop what is no doc, what the visited table holds and the later copies of a doc; score the
// rest, one per lane; drop a key that P holds; sort pool + batch and keep the best ef.  Ends on a barrier.
__device__ __forceinline__ void gr_batch(GrSmem& S, int nraw, const float* __restrict__ E, int32_t nd, int32_t D, int vece,
                                         int32_t ef) {
  const int t = threadIdx.x;
  for (int i = t; i < GR_UNIQ; i += GR_THREADS) S.uniq[i] = -1;
  if (t == 0) S.nnew = 0;
  __syncthreads();
  const int npool = S.npool;
  for (int i = t; i < nraw; i += GR_THREADS) {
    const int32_t d = S.cand[i];
    if ((uint32_t)d >= (uint32_t)nd) continue;
    const uint32_t hs = gr_hash((uint32_t)d);
    if (S.seen[hs & (GR_SEEN - 1)] == d) continue;
    bool first = false;
    uint32_t h = (hs >> 3) & (GR_UNIQ - 1);
    for (int probe = 0; probe < GR_UNIQ; ++probe) {
      const int32_t old = atomicCAS(&S.uniq[h], -1, d);
      if (old == -1) { first = true; break; }
      if (old == d) break;
      h = (h + 1) & (GR_UNIQ - 1);
    }
    if (!first) continue;
    S.seen[hs & (GR_SEEN - 1)] = d;
    const float* e = E + (long)d * D;
    float acc = 0.f;
    if (vece) {
      for (int j = 0; j < D; j += 4) {
        const f32x4 y = *(const f32x4*)(e + j);
        acc = fmaf(S.q[j], y[0], acc);
        acc = fmaf(S.q[j + 1], y[1], acc);
        acc = fmaf(S.q[j + 2], y[2], acc);
        acc = fmaf(S.q[j + 3], y[3], acc);
      }
    } else {
      for (int j = 0; j < D; ++j) acc = fmaf(S.q[j], e[j], acc);
    }
    const unsigned long long key = gr_key(dense_key(acc + 0.0f), d, 1u);
    int a = 0, b = npool;                                    // first pool entry that is not above the key, flag aside
    while (a < b) {
      const int mid = (a + b) >> 1;
      if ((S.buf[mid] >> 1) > (key >> 1)) a = mid + 1; else b = mid;
    }
    if (a < npool && (S.buf[a] >> 1) == (key >> 1)) continue;
    S.buf[npool + atomicAdd(&S.nnew, 1)] = key;
  }
  __syncthreads();
  const int total = npool + S.nnew;
  const int P = pow2_at_least(total > 1 ? total : 2);
  for (int i = total + t; i < P; i += GR_THREADS) S.buf[i] = 0ull;
  __syncthreads();
  if (S.nnew > 0) bitonic_desc<GR_THREADS, int>(S.buf, P);
  if (t == 0) S.npool = min(ef, total);
  __syncthreads();
}

__global__ __launch_bounds__(GR_THREADS) void gr_walk_kernel(const float* __restrict__ Q, int32_t D,
                                                             const float* __restrict__ E, int32_t nd, int32_t vece,
                                                             const int32_t* __restrict__ G, int32_t degree,
                                                             const int32_t* __restrict__ seeds, int32_t nseed, int32_t ef,
                                                             int32_t width, int32_t max_iter,
                                                             unsigned long long* __restrict__ pool,
                                                             int32_t* __restrict__ pool_cnt,
                                                             int32_t* __restrict__ out_iters) {
  __shared__ GrSmem S;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long q = blockIdx.x;
  for (int j = t; j < D; j += GR_THREADS) S.q[j] = Q[q * D + j];
  for (int i = t; i < GR_SEEN; i += GR_THREADS) S.seen[i] = -1;
  for (int i = t; i < nseed; i += GR_THREADS) S.cand[i] = seeds[q * nseed + i];
  if (t == 0) S.npool = 0;
  __syncthreads();
  gr_batch(S, nseed, E, nd, D, vece, ef);
  int iters = 0;
  while (max_iter == 0 || iters < max_iter) {
    if (wave == 0) {                                         // the first `width` unexpanded keys, in pool order
      const int npool = S.npool;
      int got = 0;
      for (int base = 0; base < npool && got < width; base += 64) {
        const int i = base + lane;
        const unsigned long long key = i < npool ? S.buf[i] : 0ull;
        const bool un = (key & 1ull) != 0ull;
        const unsigned long long m = __ballot(un);
        const int at = got + __popcll(m & ((1ull << lane) - 1ull));
        if (un && at < width) {
          S.parent[at] = gr_doc(key);
          S.buf[i] = key & ~1ull;
        }
        got += __popcll(m);
      }
      if (lane == 0) S.nparent = min(got, width);
    }
    __syncthreads();
    const int np = S.nparent;
    if (np == 0) break;
    ++iters;
    for (int i = t; i < np * degree; i += GR_THREADS) {
      const int p = i / degree;
      S.cand[i] = G[(long)S.parent[p] * degree + (i - p * degree)];
    }
    __syncthreads();
    gr_batch(S, np * degree, E, nd, D, vece, ef);
  }
  const int npool = S.npool;
  for (int i = t; i < npool; i += GR_THREADS) {
    const unsigned long long key = S.buf[i];
    pool[q * ef + i] = rank_key(rank_bits(key), (uint32_t)gr_doc(key));
  }
  if (t == 0) {
    pool_cnt[q] = npool;
    if (out_iters) out_iters[q] = iters;
  }
}

// ranks lo .. hi-1 of the admissible keys of a query's final pool
__global__ __launch_bounds__(GR_THREADS) void gr_output_kernel(const unsigned long long* __restrict__ pool,
                                                               const int32_t* __restrict__ pool_cnt, int32_t ef,
                                                               const int64_t* __restrict__ ex_ptr,
                                                               const int32_t* __restrict__ ex_doc,
                                                               const float* __restrict__ ceiling, int32_t lo, int32_t hi,
                                                               int32_t* __restrict__ out_doc,
                                                               float* __restrict__ out_score,
                                                               int32_t* __restrict__ out_found) {
  __shared__ unsigned long long sbuf[GR_EF_MAX];
  __shared__ int slot;
  const int t = threadIdx.x, q = blockIdx.x;
  const int n = pool_cnt[q];
  const int P = pow2_at_least(n > 1 ? n : 2);
  const bool has_c = ceiling != nullptr, has_x = ex_ptr != nullptr;
  const float cl = has_c ? ceiling[q] : 0.f;
  const int64_t e0 = has_x ? ex_ptr[q] : 0, e1 = has_x ? ex_ptr[q + 1] : 0;
  int kept = 0;
  for (int i = t; i < P; i += GR_THREADS) {
    unsigned long long key = i < n ? pool[(long)q * ef + i] : 0ull;
    if (key != 0ull) {
      bool ok = !has_c || dense_unkey(rank_bits(key)) < cl;  // a NaN ceiling admits nothing
      if (ok && has_x) {
        const int32_t doc = rank_id(key);
        const int64_t p = lower_bound(ex_doc, e0, e1, doc);
        ok = !(p < e1 && ex_doc[p] == doc);
      }
      if (!ok) key = 0ull;
    }
    kept += key != 0ull;
    sbuf[i] = key;
  }
  const int nsel = block_sum(kept, slot);
  if (nsel < n) bitonic_desc<GR_THREADS, int>(sbuf, P);      // the dropped keys sink behind the kept ones
  write_ranks<dense_unkey>(sbuf, min(nsel, hi), q, lo, hi, out_doc, out_score, out_found);
}

struct GrSearchLayout {
  size_t pool, cnt, total;
};

inline GrSearchLayout gr_search_layout(int32_t nq, int32_t ef) {
  GrSearchLayout l;
  l.pool = 0;
  l.cnt = align256((size_t)nq * (size_t)ef * 8);
  l.total = l.cnt + align256((size_t)nq * 4);
  return l;
}

inline bool gr_search_shape_ok(int32_t nq, int32_t ef, int32_t width, int32_t degree) {
  return nq >= 0 && ef >= 1 && ef <= GR_EF_MAX && width >= 1 && width <= GR_WIDTH_MAX && degree >= 1 &&
         degree <= GR_DEGREE_MAX;
}

}  // namespace

extern "C" size_t snx_graph_optimize_workspace_bytes(int32_t nd, int32_t knn, int32_t degree) {
  if (nd <= 0 || !gr_opt_shape_ok(nd, knn, degree)) return 0;
  return gr_opt_layout(nd, degree).total;
}

extern "C" int snx_graph_optimize(const int32_t* neighbors, int32_t nd, int32_t knn, int32_t degree, int32_t* graph,
                                  int32_t* forward, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (!gr_opt_shape_ok(nd, knn, degree)) return SNX_E_SHAPE;
  if (nd == 0) return SNX_OK;
  if (!neighbors || !graph) return SNX_E_ARG;
  const GrOptLayout l = gr_opt_layout(nd, degree);
  if (!workspace || ws_bytes < l.total) return SNX_E_ARG;
  unsigned long long* R = (unsigned long long*)((char*)workspace + l.r);
  int32_t* F = forward ? forward : (int32_t*)((char*)workspace + l.f);
  const long edges = (long)nd * degree;
  hipLaunchKernelGGL(gr_forward_kernel, dim3((unsigned)nd), dim3(GR_FWD_THREADS), 0, st, neighbors, nd, knn, degree, F, R);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(gr_reverse_kernel, dim3((unsigned)((edges + GR_FWD_THREADS - 1) / GR_FWD_THREADS)),
                     dim3(GR_FWD_THREADS), 0, st, (const int32_t*)F, nd, degree, R);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(gr_interleave_kernel, dim3((unsigned)cdiv(nd, GR_FWD_THREADS)), dim3(GR_FWD_THREADS), 0, st,
                     (const int32_t*)F, (const unsigned long long*)R, nd, degree, graph);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" size_t snx_graph_search_workspace_bytes(int32_t nq, int32_t ef, int32_t width, int32_t degree) {
  if (nq <= 0 || !gr_search_shape_ok(nq, ef, width, degree)) return 0;
  return gr_search_layout(nq, ef).total;
}

extern "C" int snx_graph_search(const float* Q, int32_t nq, int32_t D, const float* E, int32_t nd, const int32_t* graph,
                                int32_t degree, const int32_t* seeds, int32_t nseed, int32_t ef, int32_t width,
                                int32_t max_iter, const int64_t* ex_ptr, const int32_t* ex_doc, const float* ceiling,
                                int32_t lo, int32_t hi, int32_t* out_doc, float* out_score, int32_t* out_found,
                                int32_t* out_iters, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (D < 1 || D > DN_DMAX || nd < 0 || !gr_search_shape_ok(nq, ef, width, degree) || nseed < 0 || nseed > ef ||
      max_iter < 0 || lo < 0 || hi <= lo || hi > ef)
    return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  if (!Q || !out_doc || !out_score || (nd > 0 && (!E || !graph)) || (nseed > 0 && !seeds) || (ex_ptr && !ex_doc))
    return SNX_E_ARG;
  const GrSearchLayout l = gr_search_layout(nq, ef);
  if (!workspace || ws_bytes < l.total) return SNX_E_ARG;
  unsigned long long* pool = (unsigned long long*)((char*)workspace + l.pool);
  int32_t* pool_cnt = (int32_t*)((char*)workspace + l.cnt);
  const int vece = D % 4 == 0 && ((uintptr_t)E & 15) == 0;
  hipLaunchKernelGGL(gr_walk_kernel, dim3((unsigned)nq), dim3(GR_THREADS), 0, st, Q, D, E, nd, vece, graph, degree, seeds,
                     nd > 0 ? nseed : 0, ef, width, max_iter, pool, pool_cnt, out_iters);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(gr_output_kernel, dim3((unsigned)nq), dim3(GR_THREADS), 0, st, (const unsigned long long*)pool,
                     (const int32_t*)pool_cnt, ef, ex_ptr, ex_doc, ceiling, lo, hi, out_doc, out_score, out_found);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
