// IVF-Flat approximate dense retrieval (include/snx.h "IVF-Flat dense retrieval"): the inverted-file index the reference's
// dense miner builds through FAISS (ref:src/preprocessing/miners/bge_m3_miner.py:91-136), its search (ref:166-249) and the
// index's own deterministic spherical k-means.  Scores are dense.hip's: the fp32 fmaf chain over ascending dimensions on
// v_mfma_f32_32x32x2_f32, so an IVF hit carries the bits DenseIndex returns for the same (query, doc).
//
// Build: the list of every doc (dense search, k = 1, over the centroids) arrives as an array; a stable counting sort by
// list -- per-segment integer counts, a column scan, a placement that ranks equal keys inside 256-row chunks -- gives
// list_ptr, list_doc (original ids ascending inside a list) and the rows copied into list order.
//
// Search: the (query, probed list) pairs go through the same counting sort (stable in the query).  iv_tiles_kernel
// counts, per list, query tiles x doc splits and scans that into tile_ptr; iv_scan_kernel is launched with an upper bound
// of workgroups, each finds its list by binary search in tile_ptr and leaves when there is none, so the host never reads
// a count.  A workgroup owns up to 128 gathered query rows of one list and one split of the list's docs and walks the split
// in 128-doc tiles with the 128x128x16 fp32 MFMA loop that dense_common.h holds for this file and dense.hip, together with
// the order key, the admission of a score and the list compaction; the merge's list view and output tail are those of
// every merge kernel (sparse_common.h).  Every score goes through the
// pair's running threshold into the candidate list of its (pair, split), `cap` entries of (order key << 32 | ~original
// doc); a list that the next tile could overflow is sorted and cut to k.  Original ids ascend along a list and so along
// a split: inside one candidate list a later doc that only ties the threshold loses, and `key > threshold` is exact.
// That does NOT hold across lists, so every (pair, split) keeps its own candidate list and its own threshold, and
// iv_merge_kernel selects over a query's nprobe x splits lists by the full 64-bit key: radix_select on the score key,
// then, when the k-th score is tied, a second radix_select on ~doc among the ties (merge_lists' "first need_eq in
// index order" would be wrong here: index order is not doc order across lists).  The band's exclusion rows (binary
// search by original id) and ceiling are applied in the scan kernel, as in dn_search_kernel.
//
// k-means update: one workgroup per centroid, one thread per dimension (coalesced over j), float64, in the fixed order of
// the header: members ascending, serial inside segments of 1024 members, segment sums added in ascending order; no float
// atomics, no dependence on the launch geometry.  fp contraction is off in that kernel: the numpy reference adds and
// multiplies separately.
#include "dense_common.h"
#include "snx.h"

namespace {

constexpr int IV_THREADS = 256;                // the sort, row-copy and k-means kernels; the scan's are DN_THREADS
constexpr int IV_DMAX = DN_DMAX;               // the k-means kernel keeps a row of doubles in LDS
constexpr int IV_NLIST_MAX = 65536;
constexpr int IV_SEGS_MAX = 256;               // segments of the counting sort (one workgroup each)
constexpr int IV_CHUNK = 256;                  // rows ranked at once inside a segment
constexpr int IV_SPLIT_TILES_MIN = 8;          // default doc split: at least 1024 docs ...
constexpr int IV_SPLITS_MAX = 16;              // ... and at most this many splits of the longest list
constexpr int IV_KM_SEG = 1024;                // members per segment of the centroid sum (part of the definition)
constexpr int IV_SCAN_THREADS = 512;

// ------------------------------------------------------------------------------------------------ counting sort
struct IvSort {
  int segs;
  long seg_len;
};

inline IvSort iv_sort_plan(long n) {
  long segs = (n + IV_CHUNK - 1) / IV_CHUNK;
  if (segs > IV_SEGS_MAX) segs = IV_SEGS_MAX;
  if (segs < 1) segs = 1;
  long seg_len = ((n + segs - 1) / segs + IV_CHUNK - 1) / IV_CHUNK * IV_CHUNK;
  if (seg_len < IV_CHUNK) seg_len = IV_CHUNK;
  segs = (n + seg_len - 1) / seg_len;
  if (segs < 1) segs = 1;
  IvSort p;
  p.segs = (int)segs;
  p.seg_len = seg_len;
  return p;
}

inline size_t iv_sort_workspace(long n, int nlist) {
  return align256((size_t)iv_sort_plan(n).segs * (size_t)nlist * 4);
}

// cnt[seg][key] += 1 over the segment's rows (integer atomics: the sums do not depend on the order)
__global__ __launch_bounds__(IV_THREADS) void iv_count_kernel(const int32_t* __restrict__ keys, long n, int nlist,
                                                              long seg_len, int32_t* cnt) {
  const long b = (long)blockIdx.x * seg_len, e = min(n, b + seg_len);
  int32_t* mine = cnt + (size_t)blockIdx.x * (size_t)nlist;
  for (long i = b + threadIdx.x; i < e; i += IV_THREADS) {
    const int c = keys[i];
    if ((unsigned)c < (unsigned)nlist) atomicAdd(&mine[c], 1);
  }
}

// in-place inclusive scan of a[0..n) by one workgroup of IV_SCAN_THREADS: every thread owns one contiguous run
__device__ __forceinline__ void iv_block_scan(int64_t* a, long n, int64_t* part) {
  const int tid = threadIdx.x;
  const long per = (n + IV_SCAN_THREADS - 1) / IV_SCAN_THREADS;
  const long b = min(n, (long)tid * per), e = min(n, b + per);
  int64_t sum = 0;
  for (long i = b; i < e; ++i) sum += a[i];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int i = 0; i < IV_SCAN_THREADS; ++i) {
      const int64_t v = part[i];
      part[i] = run;
      run += v;
    }
  }
  __syncthreads();
  int64_t run = part[tid];
  for (long i = b; i < e; ++i) {
    run += a[i];
    a[i] = run;
  }
  __syncthreads();
}

// cnt[seg][key] -> the rows of earlier segments with that key; ptr[key] = first position of the key (ptr[nlist] = rows)
__global__ __launch_bounds__(IV_SCAN_THREADS) void iv_offsets_kernel(int32_t* cnt, int segs, int nlist, int64_t* ptr) {
  __shared__ int64_t part[IV_SCAN_THREADS];
  for (int c = threadIdx.x; c < nlist; c += IV_SCAN_THREADS) {
    int run = 0;
    for (int s = 0; s < segs; ++s) {
      const size_t at = (size_t)s * (size_t)nlist + c;
      const int v = cnt[at];
      cnt[at] = run;
      run += v;
    }
    ptr[c + 1] = run;
  }
  if (threadIdx.x == 0) ptr[0] = 0;
  __syncthreads();
  iv_block_scan(ptr + 1, nlist, part);
}

// order[ptr[key] + rows of earlier segments + rows of this segment in front] = row: stable.  Inside a chunk of 256 rows a
// thread counts the equal keys in front of it; the last row of a key in the chunk advances the segment's cursor.
__global__ __launch_bounds__(IV_THREADS) void iv_place_kernel(const int32_t* __restrict__ keys, long n, int nlist,
                                                              long seg_len, int32_t* base, const int64_t* __restrict__ ptr,
                                                              int32_t* __restrict__ order) {
  __shared__ int sk[IV_CHUNK];
  const int t = threadIdx.x;
  int32_t* mine = base + (size_t)blockIdx.x * (size_t)nlist;
  const long b = (long)blockIdx.x * seg_len, e = min(n, b + seg_len);
  for (long i0 = b; i0 < e; i0 += IV_CHUNK) {
    const long i = i0 + t;
    int c = -1;
    if (i < e) {
      c = keys[i];
      if ((unsigned)c >= (unsigned)nlist) c = -1;
    }
    sk[t] = c;
    const int start = c >= 0 ? mine[c] : 0;
    __syncthreads();
    if (c >= 0) {
      int before = 0, after = 0;
      for (int u = 0; u < IV_CHUNK; ++u) {
        const bool same = sk[u] == c;
        before += same && u < t;
        after += same && u > t;
      }
      order[ptr[c] + start + before] = (int32_t)i;
      if (!after) mine[c] = start + before + 1;
    }
    __syncthreads();
  }
}

// both sorts: keys [n] in [0, nlist) -> ptr [nlist + 1], order [n] (rows by key, ascending inside a key)
int iv_sort(const int32_t* keys, long n, int nlist, int64_t* ptr, int32_t* order, int32_t* cnt, hipStream_t st) {
  const IvSort p = iv_sort_plan(n);
  if (hipMemsetAsync(cnt, 0, (size_t)p.segs * (size_t)nlist * 4, st) != hipSuccess) return SNX_E_ARG;
  if (n > 0 && hipMemsetAsync(order, 0xFF, (size_t)n * 4, st) != hipSuccess) return SNX_E_ARG;
  if (n > 0) {
    hipLaunchKernelGGL(iv_count_kernel, dim3(p.segs), dim3(IV_THREADS), 0, st, keys, n, nlist, p.seg_len, cnt);
    SNX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(iv_offsets_kernel, dim3(1), dim3(IV_SCAN_THREADS), 0, st, cnt, p.segs, nlist, ptr);
  SNX_CHECK_LAUNCH();
  if (n > 0) {
    hipLaunchKernelGGL(iv_place_kernel, dim3(p.segs), dim3(IV_THREADS), 0, st, keys, n, nlist, p.seg_len, cnt,
                       (const int64_t*)ptr, order);
    SNX_CHECK_LAUNCH();
  }
  return SNX_OK;
}

// out[r] = E[order[r]]: the rows in list order
__global__ __launch_bounds__(IV_THREADS) void iv_rows_kernel(const float* __restrict__ E, const int32_t* __restrict__ order,
                                                             int32_t nd, int32_t D, float* __restrict__ out) {
  const long r = blockIdx.x;
  const int src = order[r];
  const bool ok = (unsigned)src < (unsigned)nd;
  for (int j = threadIdx.x; j < D; j += IV_THREADS) out[r * D + j] = ok ? E[(long)src * D + j] : 0.f;
}

// ------------------------------------------------------------------------------------------------ k-means update
__global__ __launch_bounds__(IV_THREADS) void iv_kmeans_kernel(const float* __restrict__ X, int32_t n, int32_t D,
                                                               const int64_t* __restrict__ ptr,
                                                               const int32_t* __restrict__ member,
                                                               const float* __restrict__ prev, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double mean[IV_DMAX];
  __shared__ double norm;
  const int t = threadIdx.x, c = blockIdx.x;
  const int64_t b = ptr[c], e = ptr[c + 1];
  float* o = out + (long)c * D;
  if (e <= b) {                                              // an empty cluster keeps its centroid
    for (int j = t; j < D; j += IV_THREADS) o[j] = prev[(long)c * D + j];
    return;
  }
  const double count = (double)(e - b);
  for (int j = t; j < D; j += IV_THREADS) {
    double total = 0.0;
    for (int64_t s = b; s < e; s += IV_KM_SEG) {
      const int64_t se = min(e, s + IV_KM_SEG);
      double part = 0.0;
      for (int64_t r = s; r < se; ++r) {
        const int row = member[r];
        if ((unsigned)row < (unsigned)n) part = part + (double)X[(long)row * D + j];
      }
      total = total + part;
    }
    mean[j] = total / count;
  }
  __syncthreads();
  if (t == 0) {
    double ss = 0.0;
    for (int j = 0; j < D; ++j) {
      const double sq = mean[j] * mean[j];
      ss = ss + sq;
    }
    norm = sqrt(ss);
  }
  __syncthreads();
  const double nv = norm;
  for (int j = t; j < D; j += IV_THREADS) o[j] = nv > 0.0 ? (float)(mean[j] / nv) : 0.f;
}

// ------------------------------------------------------------------------------------------------ fine scan
struct IvPlan {
  int split_tiles, smax, cap;
  long pairs, blocks;
};

inline IvPlan iv_plan(int32_t nq, int32_t nlist, int32_t nprobe, int32_t hi, int32_t max_list, int32_t split_docs) {
  IvPlan p;
  const long max_tiles = (max_list + (long)DN_TILE - 1) / DN_TILE;
  long st;
  if (split_docs > 0) {
    st = (split_docs + (long)DN_TILE - 1) / DN_TILE;
  } else {
    st = (max_tiles + IV_SPLITS_MAX - 1) / IV_SPLITS_MAX;
    if (st < IV_SPLIT_TILES_MIN) st = IV_SPLIT_TILES_MIN;
  }
  if (st < 1) st = 1;
  if (st > 0x7FFFFFL) st = 0x7FFFFFL;
  long smax = (max_tiles + st - 1) / st;
  if (smax < 1) smax = 1;
  p.split_tiles = (int)st;
  p.smax = (int)(smax > 0x7FFFFFFFL ? 0x7FFFFFFFL : smax);
  p.cap = dn_cap(hi);
  p.pairs = (long)nq * nprobe;
  // sum over the lists of ceil(pairs of the list / 128) is at most pairs / 128 + lists that hold a pair
  p.blocks = (p.pairs / DN_TILE + (p.pairs < nlist ? p.pairs : (long)nlist)) * smax;
  return p;
}

struct IvLayout {
  size_t cnt, pair_ptr, pair_order, tile_ptr, cand, ccount, total;
};

inline IvLayout iv_layout(const IvPlan& p, int32_t nlist) {
  IvLayout l;
  size_t off = 0;
  l.cnt = off;        off += iv_sort_workspace(p.pairs, nlist);
  l.pair_ptr = off;   off += align256((size_t)(nlist + 1) * 8);
  l.pair_order = off; off += align256((size_t)p.pairs * 4);
  l.tile_ptr = off;   off += align256((size_t)(nlist + 1) * 8);
  const size_t slots = (size_t)p.pairs * (size_t)p.smax;
  l.cand = off;       off += align256(slots * (size_t)p.cap * 8);
  l.ccount = off;     off += align256(slots * 4);
  l.total = off;
  return l;
}

inline bool iv_search_shape_ok(int32_t nq, int32_t nd, int32_t nlist, int32_t nprobe, int32_t hi, int32_t max_list,
                               int32_t split_docs) {
  return nq >= 0 && nd >= 0 && nlist >= 1 && nlist <= IV_NLIST_MAX && nprobe >= 1 && nprobe <= nlist &&
         nprobe <= SR_KMAX && hi >= 1 && hi <= SR_KMAX && max_list >= 0 && max_list <= nd && split_docs >= 0 &&
         (split_docs == 0 || split_docs >= DN_TILE);
}

// tile_ptr[c] = workgroups of the lists in front of c: query tiles x doc splits of every list that holds both
__global__ __launch_bounds__(IV_SCAN_THREADS) void iv_tiles_kernel(const int64_t* __restrict__ list_ptr,
                                                                   const int64_t* __restrict__ pair_ptr, int nlist,
                                                                   int split_tiles, int smax, int64_t* tile_ptr) {
  __shared__ int64_t part[IV_SCAN_THREADS];
  for (int c = threadIdx.x; c < nlist; c += IV_SCAN_THREADS) {
    const int64_t np = pair_ptr[c + 1] - pair_ptr[c], len = list_ptr[c + 1] - list_ptr[c];
    const int64_t qt = (np + DN_TILE - 1) / DN_TILE, dt = (len + DN_TILE - 1) / DN_TILE;
    int64_t ns = (dt + split_tiles - 1) / split_tiles;
    if (ns > smax) ns = smax;                                // max_list below the longest list: no slot past the workspace
    tile_ptr[c + 1] = np > 0 && len > 0 ? qt * ns : 0;
  }
  if (threadIdx.x == 0) tile_ptr[0] = 0;
  __syncthreads();
  iv_block_scan(tile_ptr + 1, nlist, part);
}

__global__ __launch_bounds__(DN_THREADS, 2) void iv_scan_kernel(
    const float* __restrict__ Q, int32_t nq, int32_t D, int32_t vecq, int32_t vece, const float* __restrict__ Es,
    const int64_t* __restrict__ list_ptr, const int32_t* __restrict__ list_doc, int32_t nlist,
    const int64_t* __restrict__ pair_ptr, const int32_t* __restrict__ pair_order, const int64_t* __restrict__ tile_ptr,
    int32_t nprobe, int32_t split_tiles, int32_t smax, int32_t k, int32_t cap, const int64_t* __restrict__ ex_ptr,
    const int32_t* __restrict__ ex_doc, const float* __restrict__ ceiling, unsigned long long* cand,
    int32_t* __restrict__ ccount) {
  __shared__ int64_t exa[DN_TILE], exb[DN_TILE], slot[DN_TILE];
  __shared__ uint32_t thr[DN_TILE];
  __shared__ int cnt[DN_TILE], qrow[DN_TILE];
  __shared__ float ceilv[DN_TILE];
  __shared__ int s_list;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const int64_t wg = blockIdx.x;
  if (t == 0) {                                              // the list of this workgroup: tile_ptr[l] <= wg < tile_ptr[l + 1]
    int l = -1;
    if (wg < tile_ptr[nlist]) {
      int a = 0, b = nlist;
      while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (tile_ptr[mid] <= wg) a = mid; else b = mid;
      }
      l = a;
    }
    s_list = l;
  }
  __syncthreads();
  const int l = s_list;
  if (l < 0) return;                                         // the launch is an upper bound
  const int64_t local = wg - tile_ptr[l];
  const int64_t np = pair_ptr[l + 1] - pair_ptr[l];
  const int64_t qt = (np + DN_TILE - 1) / DN_TILE;
  const int64_t qtile = local % qt;
  const int split = (int)(local / qt);
  const int64_t r0 = pair_ptr[l] + qtile * DN_TILE;
  const int m = (int)min((int64_t)DN_TILE, np - qtile * DN_TILE);
  const int64_t p0 = list_ptr[l] + (int64_t)split * split_tiles * DN_TILE;
  const int64_t p1 = min(list_ptr[l + 1], p0 + (int64_t)split_tiles * DN_TILE);
  const bool has_c = ceiling != nullptr, has_x = ex_ptr != nullptr;
  if (t < DN_TILE) {
    const int pair = t < m ? pair_order[r0 + t] : -1;
    const bool ok = pair >= 0 && pair / nprobe < nq && split < smax;
    const int q = ok ? pair / nprobe : -1;
    qrow[t] = q;
    slot[t] = ok ? (int64_t)pair * smax + split : 0;
    thr[t] = 0u;
    cnt[t] = 0;
    ceilv[t] = has_c && ok ? ceiling[q] : 0.f;
    exa[t] = has_x && ok ? ex_ptr[q] : 0;
    exb[t] = has_x && ok ? ex_ptr[q + 1] : 0;
  }
  __syncthreads();
  auto list = [&](int row) { return cand + (size_t)slot[row] * (size_t)cap; };
  auto compact = [&](int row) { dn_compact(list(row), cnt[row], thr[row], k, cap); };
  auto query = [&](int r) -> long { return qrow[r]; };

  for (int64_t n0 = p0; n0 < p1; n0 += DN_TILE) {
    auto drow = [&](int r) -> long { return n0 + r < p1 ? n0 + r : -1; };   // rows of the list-ordered matrix
    f32x16 acc[2][2];
    dn_tile_scores(Q, query, vecq, Es, drow, vece, D, acc);
    // acc[i][j][r] = s(query of tile row 64 wm + 32 i + (r & 3) + 8 (r >> 2) + 4 h, doc at position n0 + 64 wn + 32 j + c)
    int32_t docj[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t pos = n0 + wn * 64 + j * 32 + c;
      docj[j] = pos < p1 ? list_doc[pos] : -1;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const bool rok = qrow[row] >= 0;
        const uint32_t th = thr[row];
        const float cl = ceilv[row];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int32_t doc = docj[j];
          const bool ok = rok && doc >= 0;
          const float s = acc[i][j][r] + 0.0f;
          dn_admit(ok, s, doc, th, has_c, cl, has_x, ex_doc, exa[row], exb[row], cnt[row], list(row), cap);
        }
      }
    __syncthreads();
    // a tile adds at most DN_TILE entries to a list: compact every list that the next tile could overflow
    for (int row = 0; row < m; ++row)
      if (__builtin_amdgcn_readfirstlane(cnt[row]) > cap - DN_TILE && qrow[row] >= 0) compact(row);
  }
  for (int row = 0; row < m; ++row)
    if (qrow[row] >= 0) compact(row);
  if (t < m && qrow[t] >= 0) ccount[slot[t]] = cnt[t];
}

// ranks lo .. hi-1 over a query's nprobe x smax candidate lists (each sorted, at most hi long) under the full order: score
// key descending, then original doc ascending
__global__ __launch_bounds__(SR_THREADS) void iv_merge_kernel(const unsigned long long* __restrict__ cand,
                                                              const int32_t* __restrict__ ccount, int32_t nslot,
                                                              int32_t cap, int32_t lo, int32_t hi,
                                                              int32_t* __restrict__ out_doc,
                                                              float* __restrict__ out_score,
                                                              int32_t* __restrict__ out_found) {
  __shared__ SelectSmem S;
  __shared__ unsigned long long sbuf[SR_KMAX];
  __shared__ int taken;
  const int tid = threadIdx.x, q = blockIdx.x;
  const long base = (long)q * nslot;
  const RankLists lists ={cand + (size_t)base * (size_t)cap, ccount + base, cap, hi};
  const long n = (long)nslot * hi;
  uint32_t thr, thr2 = 0u;
  int need_eq, nsel;
  radix_select(lists, n, hi, S, thr, need_eq, nsel);
  if (thr != 0u) {                                           // the hi-th score is tied: the need_eq lowest docs of the tie
    auto tie = [&](long f) -> uint32_t {
      const unsigned long long e = lists.at(f);
      return rank_bits(e) == thr ? (uint32_t)(e & 0xFFFFFFFFull) : 0u;
    };
    int ne2, ns2;
    radix_select(tie, n, need_eq, S, thr2, ne2, ns2);
  }
  const int P = pow2_at_least(nsel);
  for (int i = tid; i < P; i += SR_THREADS) sbuf[i] = 0ull;
  if (tid == 0) taken = 0;
  __syncthreads();
  for (long f = tid; f < n; f += SR_THREADS) {
    const unsigned long long e = lists.at(f);
    const uint32_t kb = rank_bits(e);
    if (e != 0ull && (kb > thr || (kb == thr && (uint32_t)(e & 0xFFFFFFFFull) >= thr2))) {
      const int pos = atomicAdd(&taken, 1);                  // any order: the sort below settles it, the keys are unique
      if (pos < P) sbuf[pos] = e;
    }
  }
  __syncthreads();
  bitonic_desc<SR_THREADS, int>(sbuf, P);
  write_ranks<dense_unkey>(sbuf,nsel, q, lo, hi, out_doc, out_score, out_found);
}

}  // namespace

extern "C" size_t snx_ivf_build_workspace_bytes(int32_t nd, int32_t nlist) {
  if (nd < 0 || nlist < 1 || nlist > IV_NLIST_MAX) return 0;
  return iv_sort_workspace(nd, nlist);
}

extern "C" int snx_ivf_build(const int32_t* doc_list, int32_t nd, int32_t nlist, const float* E, int32_t D,
                             int64_t* list_ptr, int32_t* list_doc, float* E_sorted, void* workspace, size_t ws_bytes,
                             hipStream_t st) {
  if (nd < 0 || nlist < 1 || nlist > IV_NLIST_MAX || (E_sorted && (D < 1 || D > IV_DMAX))) return SNX_E_SHAPE;
  if (!list_ptr || (nd > 0 && (!doc_list || !list_doc)) || (E_sorted && nd > 0 && !E)) return SNX_E_ARG;
  if (!workspace || ws_bytes < iv_sort_workspace(nd, nlist)) return SNX_E_ARG;
  const int rc = iv_sort(doc_list, nd, nlist, list_ptr, list_doc, (int32_t*)workspace, st);
  if (rc != SNX_OK) return rc;
  if (E_sorted && nd > 0) {
    hipLaunchKernelGGL(iv_rows_kernel, dim3((unsigned)nd), dim3(IV_THREADS), 0, st, E, (const int32_t*)list_doc, nd, D,
                       E_sorted);
    SNX_CHECK_LAUNCH();
  }
  return SNX_OK;
}

extern "C" int snx_ivf_kmeans_update(const float* X, int32_t n, int32_t D, const int64_t* list_ptr,
                                     const int32_t* list_row, int32_t nlist, const float* C_prev, float* C_out,
                                     hipStream_t st) {
  if (n < 0 || D < 1 || D > IV_DMAX || nlist < 1 || nlist > IV_NLIST_MAX) return SNX_E_SHAPE;
  if (!list_ptr || !C_prev || !C_out || (n > 0 && (!X || !list_row))) return SNX_E_ARG;
  hipLaunchKernelGGL(iv_kmeans_kernel, dim3((unsigned)nlist), dim3(IV_THREADS), 0, st, X, n, D, list_ptr, list_row,
                     C_prev, C_out);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" size_t snx_ivf_search_workspace_bytes(int32_t nq, int32_t nd, int32_t nlist, int32_t nprobe, int32_t hi,
                                                 int32_t max_list, int32_t split_docs) {
  if (nq <= 0 || !iv_search_shape_ok(nq, nd, nlist, nprobe, hi, max_list, split_docs)) return 0;
  const IvPlan p = iv_plan(nq, nlist, nprobe, hi, max_list, split_docs);
  if (p.pairs > 0x7FFFFFFFL) return 0;
  return iv_layout(p, nlist).total;
}

extern "C" int snx_ivf_search(const float* Q, int32_t nq, int32_t D, const float* E_sorted, const int64_t* list_ptr,
                              const int32_t* list_doc, int32_t nd, int32_t nlist, int32_t max_list,
                              const int32_t* probe, int32_t nprobe, const int64_t* ex_ptr, const int32_t* ex_doc,
                              const float* ceiling, int32_t lo, int32_t hi, int32_t split_docs, int32_t* out_doc,
                              float* out_score, int32_t* out_found, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (D < 1 || D > IV_DMAX || lo < 0 || hi <= lo || !iv_search_shape_ok(nq, nd, nlist, nprobe, hi, max_list, split_docs))
    return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  if (!Q || !list_ptr || !probe || !out_doc || !out_score || (nd > 0 && (!E_sorted || !list_doc)) || (ex_ptr && !ex_doc))
    return SNX_E_ARG;
  const IvPlan p = iv_plan(nq, nlist, nprobe, hi, max_list, split_docs);
  if (p.pairs > 0x7FFFFFFFL || p.blocks > 0x7FFFFFFFL || p.pairs * p.smax > 0x7FFFFFFFL) return SNX_E_SHAPE;
  const IvLayout l = iv_layout(p, nlist);
  if (!workspace || ws_bytes < l.total) return SNX_E_ARG;
  char* w = (char*)workspace;
  int32_t* cnt = (int32_t*)(w + l.cnt);
  int64_t* pair_ptr = (int64_t*)(w + l.pair_ptr);
  int32_t* pair_order = (int32_t*)(w + l.pair_order);
  int64_t* tile_ptr = (int64_t*)(w + l.tile_ptr);
  unsigned long long* cand = (unsigned long long*)(w + l.cand);
  int32_t* ccount = (int32_t*)(w + l.ccount);
  const size_t slots = (size_t)p.pairs * (size_t)p.smax;
  if (hipMemsetAsync(ccount, 0, slots * 4, st) != hipSuccess) return SNX_E_ARG;
  const int rc = iv_sort(probe, p.pairs, nlist, pair_ptr, pair_order, cnt, st);
  if (rc != SNX_OK) return rc;
  hipLaunchKernelGGL(iv_tiles_kernel, dim3(1), dim3(IV_SCAN_THREADS), 0, st, list_ptr, (const int64_t*)pair_ptr, nlist,
                     p.split_tiles, p.smax, tile_ptr);
  SNX_CHECK_LAUNCH();
  if (p.blocks > 0 && nd > 0) {
    const int vecq = D % 4 == 0 && ((uintptr_t)Q & 15) == 0, vece = D % 4 == 0 && ((uintptr_t)E_sorted & 15) == 0;
    hipLaunchKernelGGL(iv_scan_kernel, dim3((unsigned)p.blocks), dim3(DN_THREADS), 0, st, Q, nq, D, vecq, vece, E_sorted,
                       list_ptr, list_doc, nlist, (const int64_t*)pair_ptr, (const int32_t*)pair_order,
                       (const int64_t*)tile_ptr, nprobe, p.split_tiles, p.smax, hi, p.cap, ex_ptr, ex_doc, ceiling, cand,
                       ccount);
    SNX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(iv_merge_kernel, dim3(nq), dim3(SR_THREADS), 0, st, (const unsigned long long*)cand,
                     (const int32_t*)ccount, (int32_t)(nprobe * p.smax), p.cap, lo, hi, out_doc, out_score, out_found);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
