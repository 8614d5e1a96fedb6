// Character n-gram TF-IDF (include/snx.h "Character n-gram TF-IDF"): the vectorizer of the reference's first mining step
// (ref:scripts/mine_hard_negatives.py:141-146, scikit-learn's TfidfVectorizer(analyzer="char_wb", ngram_range=(2, 3),
// sublinear_tf=True)), whose scikit-learn / scipy form keeps that step at 50,000 documents.  The rows arrive as code
// points, words joined by one U+0020; what leaves is the CSR a SparseIndex takes.
//
//   tf_count_kernel<false>  one workgroup per row.  Every (position, n) of the padded row is a slot: the thread that owns
//                           it packs the window into the exact 64-bit key, or the sentinel when the window is no n-gram of
//                           one padded word.  The slots are sorted ascending in LDS (bitonic, the sentinels end up behind
//                           the keys); a head is a key that differs from its left neighbour, its count the distance to the
//                           end of its run (binary search), its place among the heads a ballot scan.  Rows of more than
//                           TF_LDS_KEYS slots are left alone.
//   tf_count_kernel<true>   the same code over a slot of the workspace, for the rows the LDS form leaves alone: a fixed
//                           number of workgroups walks the rows, each sorting in its own slot.
//   tf_weight_kernel        one wave per row of (key, count): binary search in the ascending feature keys, the unknown
//                           dropped by a ballot scan, u = tf_table[count] * idf[feature] in float64, the squares summed per
//                           lane in ascending position and folded by a fixed shuffle tree, w = fp32(u / sqrt(sum)).
//                           No logarithm here: tf_table is the host's (libm is not bit-reproducible).
//   tf_compact_kernel       one wave per row: the filled front of a row's slots moves to its place in the CSR.
// No kernel waits for another workgroup; every result is the same bits from run to run.
#include "sparse_common.h"   // block_sum
#include "text_common.h"
#include "snx.h"

namespace {

constexpr int TF_THREADS = 256;
constexpr int TF_WAVES = TF_THREADS / 64;
constexpr int TF_LDS_KEYS = SNX_TFIDF_LDS_KEYS;     // 32 KiB of keys: four workgroups (16 waves) per CU
constexpr int TF_LONG_GROUPS = 64;                  // workgroups (and workspace slots) of the long-row form
constexpr unsigned long long TF_NONE = ~0ull;       // no n-gram in this slot: sorts behind every key
constexpr int32_t TF_SPACE = 0x20;

__host__ __device__ inline int tf_slots_per_pos(int min_n, int max_n) { return max_n - min_n + 1 + (min_n == 1 ? 1 : 0); }

// the key of slot e of a row: position s = e / NS of the padded row p (p[i] = t[i-1], a U+0020 in front of and behind t),
// j = e % NS the n of the window that starts there (the last j of a range from 1: the second copy of a 1-gram U+0020)
__device__ __forceinline__ unsigned long long tf_slot_key(const int32_t* __restrict__ t, int64_t len, int64_t e, int NS,
                                                          int min_n, int max_n) {
  const int64_t s = e / NS;
  const int j = (int)(e % NS);
  const int nn = max_n - min_n + 1;
  const int n = j < nn ? min_n + j : 1;
  auto at = [&](int64_t i) -> int32_t { return i >= 0 && i < len ? t[i] : TF_SPACE; };
  const int32_t c0 = at(s - 1);
  if (n == 1) {
    // a padded word holds its own two U+0020: one between two words counts twice, one beside a single word once
    int mult = 1;
    if (c0 == TF_SPACE) mult = (at(s - 2) != TF_SPACE) + (at(s) != TF_SPACE);
    if (mult < (j < nn ? 1 : 2)) return TF_NONE;
    return (unsigned long long)(uint32_t)(c0 + 1) << 42;
  }
  const int32_t c1 = at(s);
  if (n == 2) {
    if (c0 == TF_SPACE && c1 == TF_SPACE) return TF_NONE;
    return (unsigned long long)(uint32_t)(c0 + 1) << 42 | (unsigned long long)(uint32_t)(c1 + 1) << 21;
  }
  if (c1 == TF_SPACE) return TF_NONE;                         // a window of three never holds a U+0020 inside
  const int32_t c2 = at(s + 1);
  return (unsigned long long)(uint32_t)(c0 + 1) << 42 | (unsigned long long)(uint32_t)(c1 + 1) << 21 |
         (unsigned long long)(uint32_t)(c2 + 1);
}

// one row: slots -> sorted keys in a[0..P) -> distinct keys ascending with their counts at out_key / out_count [off ..)
__device__ __forceinline__ void tf_count_row(const int64_t* __restrict__ ptr, const int32_t* __restrict__ cps, int64_t row,
                                             int min_n, int max_n, unsigned long long* a, int64_t E, int64_t P,
                                             int (&wcnt)[TF_WAVES], int& run, int64_t* __restrict__ out_key,
                                             int32_t* __restrict__ out_count, int32_t* __restrict__ out_cnt) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NS = tf_slots_per_pos(min_n, max_n);
  const int64_t a0 = ptr[row], len = ptr[row + 1] - a0;
  const int64_t off = (a0 + 2 * row) * NS;                   // the row's first slot in the outputs
  for (int64_t e = tid; e < P; e += TF_THREADS) a[e] = e < E ? tf_slot_key(cps + a0, len, e, NS, min_n, max_n) : TF_NONE;
  if (tid == 0) run = 0;
  __syncthreads();
  text_bitonic_asc<TF_THREADS>(a, P);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t base = 0; base < E; base += TF_THREADS) {     // block-uniform bounds
    const int64_t i = base + tid;
    const unsigned long long k = i < E ? a[i] : TF_NONE;
    const bool head = k != TF_NONE && (i == 0 || a[i - 1] != k);
    const unsigned long long m = __ballot(head);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    if (head) {
      int pos = run + __popcll(m & below);
      for (int w = 0; w < wave; ++w) pos += wcnt[w];
      int64_t lo = i + 1, hi = E;                            // the end of the run: the first slot with a larger key
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= k) lo = mid + 1; else hi = mid;
      }
      out_key[off + pos] = (int64_t)k;
      out_count[off + pos] = (int32_t)(lo - i);
    }
    __syncthreads();
    if (tid == 0) {
      int r = run;
      for (int w = 0; w < TF_WAVES; ++w) r += wcnt[w];
      run = r;
    }
    __syncthreads();
  }
  if (tid == 0) out_cnt[row] = run;
  __syncthreads();                                           // the long form goes on to its next row
}

template <bool LONG>
__global__ __launch_bounds__(TF_THREADS) void tf_count_kernel(const int64_t* __restrict__ ptr,
                                                              const int32_t* __restrict__ cps, int32_t n, int32_t min_n,
                                                              int32_t max_n, unsigned long long* __restrict__ ws,
                                                              int64_t ws_keys, int64_t* __restrict__ out_key,
                                                              int32_t* __restrict__ out_count,
                                                              int32_t* __restrict__ out_cnt) {
  __shared__ int wcnt[TF_WAVES];
  __shared__ int run;
  const int NS = tf_slots_per_pos(min_n, max_n);
  if constexpr (!LONG) {
    __shared__ unsigned long long keys[TF_LDS_KEYS];
    const int64_t row = blockIdx.x;
    const int64_t E = (ptr[row + 1] - ptr[row] + 2) * NS;
    if (E > TF_LDS_KEYS) return;                             // block-uniform: the long form's row
    tf_count_row(ptr, cps, row, min_n, max_n, keys, E, pow2_at_least(E), wcnt, run, out_key, out_count, out_cnt);
  } else {
    unsigned long long* a = ws + (int64_t)blockIdx.x * ws_keys;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
      const int64_t E = (ptr[row + 1] - ptr[row] + 2) * NS;
      const int64_t P = pow2_at_least(E);
      if (E <= TF_LDS_KEYS) continue;                        // block-uniform: the LDS form's row
      if (P > ws_keys) {                                     // `longest_row` was understated (precondition): an empty row
        if (threadIdx.x == 0) out_cnt[row] = 0;
        continue;
      }
      tf_count_row(ptr, cps, row, min_n, max_n, a, E, P, wcnt, run, out_key, out_count, out_cnt);
    }
  }
}

__global__ __launch_bounds__(64) void tf_weight_kernel(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ key,
                                                       const int32_t* __restrict__ count,
                                                       const int64_t* __restrict__ feat_key,
                                                       const double* __restrict__ idf, int32_t F,
                                                       const double* __restrict__ tf_table, int32_t tmax,
                                                       int32_t* __restrict__ out_fid, float* __restrict__ out_w,
                                                       int32_t* __restrict__ out_cnt) {
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t r0 = row_ptr[row], r1 = row_ptr[row + 1];
  const unsigned long long below = (1ull << lane) - 1ull;
  int32_t* const cnt_bits = (int32_t*)out_w;                 // a known entry's count waits here for the row's norm
  int known = 0;
  double ss = 0.0;                                           // this lane's squares, ascending position
  for (int64_t base = r0; base < r1; base += 64) {           // wave-uniform bounds
    const int64_t i = base + lane;
    int32_t f = -1, c = 0;
    if (i < r1) {
      const int64_t k = key[i];
      const int64_t p = lower_bound(feat_key, (int64_t)0, (int64_t)F, k);
      if (p < F && feat_key[p] == k) {
        f = (int32_t)p;
        c = min(max(count[i], 1), tmax);                     // a count outside the table (precondition) is clamped
      }
    }
    const unsigned long long m = __ballot(f >= 0);
    if (f >= 0) {
      const int64_t o = r0 + known + __popcll(m & below);
      out_fid[o] = f;
      cnt_bits[o] = c;
      const double u = tf_table[c] * idf[f];
      ss += u * u;
    }
    known += __popcll(m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);   // the same tree on every lane: the same bits
  const double norm = sqrt(ss);
  __threadfence_block();
  __syncthreads();                                           // the counts parked above are read by other lanes
  for (int64_t i = r0 + lane; i < r0 + known; i += 64) {
    const double u = tf_table[cnt_bits[i]] * idf[out_fid[i]];
    out_w[i] = (float)(u / norm);
  }
  if (lane == 0) out_cnt[row] = known;
}

template <typename A, typename B>
__global__ __launch_bounds__(64) void tf_compact_kernel(const int64_t* __restrict__ src_ptr,
                                                        const int64_t* __restrict__ dst_ptr, const A* __restrict__ src_a,
                                                        const B* __restrict__ src_b, A* __restrict__ dst_a,
                                                        B* __restrict__ dst_b) {
  const int64_t row = blockIdx.x;
  const int64_t s = src_ptr[row], d = dst_ptr[row], m = dst_ptr[row + 1] - d;
  for (int64_t i = threadIdx.x; i < m; i += 64) {
    dst_a[d + i] = src_a[s + i];
    dst_b[d + i] = src_b[s + i];
  }
}

bool range_ok(int32_t min_n, int32_t max_n) { return 1 <= min_n && min_n <= max_n && max_n <= 3; }

// keys of a workspace slot of the long-row form, 0 when every row fits the LDS form
int64_t long_slot_keys(int64_t longest_row, int32_t min_n, int32_t max_n) {
  const int64_t E = (longest_row + 2) * tf_slots_per_pos(min_n, max_n);
  return E <= TF_LDS_KEYS ? 0 : pow2_at_least(E);
}

}  // namespace

extern "C" size_t snx_tfidf_counts_workspace_bytes(int64_t longest_row, int32_t min_n, int32_t max_n) {
  if (longest_row < 0 || !range_ok(min_n, max_n)) return 0;
  return (size_t)long_slot_keys(longest_row, min_n, max_n) * sizeof(unsigned long long) * TF_LONG_GROUPS;
}

extern "C" int snx_tfidf_row_counts(const int64_t* ptr, const int32_t* code_points, int32_t n, int64_t longest_row,
                                    int32_t min_n, int32_t max_n, int64_t* out_key, int32_t* out_count, int32_t* out_cnt,
                                    void* workspace, size_t ws_bytes, hipStream_t st) {
  if (n < 0 || longest_row < 0 || !range_ok(min_n, max_n)) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!ptr || !out_key || !out_count || !out_cnt) return SNX_E_ARG;   // code_points may be NULL when every row is empty
  const int64_t slot = long_slot_keys(longest_row, min_n, max_n);
  if (slot && (!workspace || ws_bytes < (size_t)slot * sizeof(unsigned long long) * TF_LONG_GROUPS)) return SNX_E_ARG;
  hipLaunchKernelGGL(tf_count_kernel<false>, dim3((unsigned)n), dim3(TF_THREADS), 0, st, ptr, code_points, n, min_n, max_n,
                     (unsigned long long*)nullptr, (int64_t)0, out_key, out_count, out_cnt);
  SNX_CHECK_LAUNCH();
  if (slot) {
    hipLaunchKernelGGL(tf_count_kernel<true>, dim3((unsigned)min(n, TF_LONG_GROUPS)), dim3(TF_THREADS), 0, st, ptr,
                       code_points, n, min_n, max_n, (unsigned long long*)workspace, slot, out_key, out_count, out_cnt);
    SNX_CHECK_LAUNCH();
  }
  return SNX_OK;
}

extern "C" int snx_tfidf_weights(const int64_t* row_ptr, const int64_t* key, const int32_t* count, int32_t n,
                                 const int64_t* feat_key, const double* idf, int32_t F, const double* tf_table,
                                 int32_t tmax, int32_t* out_fid, float* out_w, int32_t* out_cnt, hipStream_t st) {
  if (n < 0 || F < 0 || tmax < 1) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!row_ptr || !out_cnt || !tf_table || (F > 0 && (!feat_key || !idf))) return SNX_E_ARG;
  hipLaunchKernelGGL(tf_weight_kernel, dim3((unsigned)n), dim3(64), 0, st, row_ptr, key, count, feat_key, idf, F, tf_table,
                     tmax, out_fid, out_w, out_cnt);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_tfidf_compact_counts(const int64_t* src_ptr, const int64_t* dst_ptr, int32_t n, const int64_t* src_key,
                                        const int32_t* src_count, int64_t* dst_key, int32_t* dst_count, hipStream_t st) {
  if (n < 0) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!src_ptr || !dst_ptr) return SNX_E_ARG;
  hipLaunchKernelGGL((tf_compact_kernel<int64_t, int32_t>), dim3((unsigned)n), dim3(64), 0, st, src_ptr, dst_ptr, src_key,
                     src_count, dst_key, dst_count);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_tfidf_compact_rows(const int64_t* src_ptr, const int64_t* dst_ptr, int32_t n, const int32_t* src_fid,
                                      const float* src_w, int32_t* dst_fid, float* dst_w, hipStream_t st) {
  if (n < 0) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!src_ptr || !dst_ptr) return SNX_E_ARG;
  hipLaunchKernelGGL((tf_compact_kernel<int32_t, float>), dim3((unsigned)n), dim3(64), 0, st, src_ptr, dst_ptr, src_fid,
                     src_w, dst_fid, dst_w);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
