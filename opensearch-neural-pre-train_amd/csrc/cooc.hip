// Co-occurrence counts and PMI (include/snx.h "Co-occurrence and PMI"): the two loops of the reference's src/pmi package
// (ref:src/pmi/cooccurrence.py:206-226, one scipy lil_matrix update per pair of token positions of every window, and
// ref:src/pmi/pmi_calculator.py:142-193, one Python call per stored cell).  Rows arrive as token ids, -1 for a token
// outside the vocabulary; what leaves is records (row term * V + col term, multiplicity[, window length]) that the
// Python layer reduces to a CSR with one device-wide sort, and float64 PMI values.
//
//   co_window_kernel<64, WAVE>    one wave per window of at most 64 tokens (sentences), keys in LDS.
//   co_window_kernel<256, TILE>   one workgroup per window of 65 .. SNX_COOC_LDS_TOKENS tokens, keys in LDS.
//   co_window_kernel<256, LONG>   longer windows: a fixed number of workgroups walks them, each in its workspace slot.
//     All three run co_window: the window's valid tokens become keys (id << 32 | position), sorted ascending (bitonic);
//     a run of equal ids is one distinct term, its start found by a ballot scan.  Every pair of runs is one candidate
//     record whose multiplicity is a product of run lengths (symmetric), or the number of position pairs in order (not
//     symmetric: a binary search per position of the first run in the positions of the second).  Records of multiplicity
//     zero are not emitted; a record's place inside its window comes from an LDS counter (one integer atomic per wave),
//     so the order of the records inside a window is arbitrary -- the reduction that follows is a sort with integer
//     sums and does not see it.  Without rec_ptr the kernel only counts (pass 1); with it, it writes (pass 2).
//   co_norm_kernel                one thread per cell: sum over its (window length m ascending, additions at m) of
//                                 additions / m in float64, rounded to fp32 once.
//   co_pmi_cells_kernel           one thread per stored cell; co_pmi_pairs_kernel one thread per (row, col) pair, the cell
//                                 found by binary search in the row.
// No kernel waits for another workgroup; no float atomics; every result is the same bits from run to run.
#include "sparse_common.h"   // block_sum
#include "text_common.h"
#include "snx.h"

namespace {

constexpr int CO_TILE = SNX_COOC_LDS_TOKENS;        // 32 KiB of keys + 16 KiB of run starts: three workgroups per CU
constexpr int CO_WAVE = 64;                         // tokens of a window that one wave takes
constexpr int CO_LONG_GROUPS = 64;                  // workgroups (and workspace slots) of the long-window form
constexpr unsigned long long CO_NONE = ~0ull;       // no valid token in this slot: sorts behind every key

enum { CO_FORM_WAVE = 0, CO_FORM_TILE = 1, CO_FORM_LONG = 2 };

template <int THREADS>
struct CoShared {
  int wcnt[THREADS / 64];
  int run;
  unsigned long long ctr;
};

// window g -> its first token and its length.  Rows are windows (win_ptr == NULL), or sliding: win_ptr [n_rows + 1] are the
// running window counts of the rows, a row of n <= w tokens is one window, a longer one has n - w + 1 of w tokens each.
__device__ __forceinline__ void co_window_of(const int64_t* __restrict__ ptr, const int64_t* __restrict__ win_ptr,
                                             int32_t n_rows, int64_t w, int64_t g, int64_t& start, int64_t& len) {
  if (!win_ptr) {
    start = ptr[g];
    len = ptr[g + 1] - start;
    return;
  }
  int64_t lo = 0, hi = (int64_t)n_rows - 1;                  // the row r with win_ptr[r] <= g < win_ptr[r + 1]
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (win_ptr[mid + 1] <= g) lo = mid + 1; else hi = mid;
  }
  const int64_t n = ptr[lo + 1] - ptr[lo];
  start = ptr[lo] + (g - win_ptr[lo]);
  len = min(n, w);
  if (start + len > ptr[lo + 1]) len = 0;                    // win_ptr disagrees with ptr (precondition): nothing is read
}

// One window: a[0..P) keys, rs[0..len] run starts.  Returns the number of records; with `write`, record i of the window
// goes to out_*[out_off + i].
template <int THREADS>
__device__ __forceinline__ unsigned long long co_window(const int32_t* __restrict__ ids, int64_t start, int64_t len,
                                                        int64_t V, bool symmetric, unsigned long long* a, int32_t* rs,
                                                        int64_t P, CoShared<THREADS>& sh, bool write,
                                                        int64_t* __restrict__ out_key, int64_t* __restrict__ out_mult,
                                                        int32_t* __restrict__ out_m, int64_t out_off) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t e = tid; e < P; e += THREADS) {
    unsigned long long k = CO_NONE;
    if (e < len) {
      const int32_t id = ids[start + e];
      if (id >= 0 && (int64_t)id < V) k = (unsigned long long)(uint32_t)id << 32 | (unsigned long long)(uint32_t)e;
    }
    a[e] = k;
  }
  if (tid == 0) { sh.run = 0; sh.ctr = 0ull; }
  __syncthreads();
  text_bitonic_asc<THREADS>(a, P);
  for (int64_t base = 0; base < len; base += THREADS) {      // block-uniform bounds: the starts of the runs, in order
    const int64_t i = base + tid;
    const unsigned long long k = i < len ? a[i] : CO_NONE;
    const bool head = k != CO_NONE && (i == 0 || (a[i - 1] >> 32) != (k >> 32));
    const unsigned long long hm = __ballot(head);
    if (lane == 0) sh.wcnt[wave] = __popcll(hm);
    __syncthreads();
    if (head) {
      int pos = sh.run + __popcll(hm & below);
      for (int w = 0; w < wave; ++w) pos += sh.wcnt[w];
      rs[pos] = (int32_t)i;
    }
    __syncthreads();
    if (tid == 0) {
      int r = sh.run;
      for (int w = 0; w < THREADS / 64; ++w) r += sh.wcnt[w];
      sh.run = r;
    }
    __syncthreads();
  }
  const int64_t m = lower_bound(a, (int64_t)0, len, CO_NONE);   // the valid tokens: every thread finds the same m
  const int64_t D = sh.run;
  if (tid == 0) rs[D] = (int32_t)m;
  __syncthreads();
  if (m >= 2) {
    const int64_t NP = D * D;
    for (int64_t pb = 0; pb < NP; pb += THREADS) {           // block-uniform bounds
      const int64_t p = pb + tid;
      long long mult = 0;
      int64_t da = 0, db = 0;
      if (p < NP) {
        da = p / D;
        db = p - da * D;
        const int64_t a0 = rs[da], a1 = rs[da + 1], b0 = rs[db], b1 = rs[db + 1];
        if (da == db) {
          const long long r = a1 - a0;
          mult = symmetric ? r * (r - 1) : r * (r - 1) / 2;
        } else if (symmetric) {
          if (da < db) mult = (long long)(a1 - a0) * (long long)(b1 - b0);   // mirrored by the caller
        } else {
          for (int64_t i = a0; i < a1; ++i) {                // positions of b behind this position of a
            const uint32_t pa = (uint32_t)a[i];
            int64_t lo = b0, hi = b1;
            while (lo < hi) {
              const int64_t mid = lo + ((hi - lo) >> 1);
              if ((uint32_t)a[mid] <= pa) lo = mid + 1; else hi = mid;
            }
            mult += b1 - lo;
          }
        }
      }
      const bool has = mult > 0;
      const unsigned long long bm = __ballot(has);
      long long first = 0;
      if (lane == 0 && bm) first = (long long)atomicAdd(&sh.ctr, (unsigned long long)__popcll(bm));
      first = __shfl(first, 0, 64);
      if (write && has) {
        const int64_t o = out_off + first + __popcll(bm & below);
        out_key[o] = (int64_t)(a[rs[da]] >> 32) * V + (int64_t)(a[rs[db]] >> 32);
        out_mult[o] = mult;
        if (out_m) out_m[o] = (int32_t)m;
      }
    }
  }
  __syncthreads();
  const unsigned long long total = sh.ctr;
  __syncthreads();                                           // the long form goes on to its next window
  return total;
}

template <int THREADS, int FORM>
__global__ __launch_bounds__(THREADS) void co_window_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ ids,
                                                            const int64_t* __restrict__ win_ptr, int32_t n_rows, int64_t w,
                                                            int64_t g0, int64_t ng, int64_t V, int32_t symmetric,
                                                            unsigned char* __restrict__ ws, int64_t ws_tokens,
                                                            int64_t slot_bytes, const int64_t* __restrict__ rec_ptr,
                                                            int64_t* __restrict__ out_cnt, int64_t* __restrict__ out_key,
                                                            int64_t* __restrict__ out_mult, int32_t* __restrict__ out_m) {
  __shared__ CoShared<THREADS> sh;
  const bool write = rec_ptr != nullptr;
  if constexpr (FORM != CO_FORM_LONG) {
    constexpr int TOK = FORM == CO_FORM_WAVE ? CO_WAVE : CO_TILE;
    __shared__ unsigned long long keys[TOK];
    __shared__ int32_t rs[TOK + 1];
    const int64_t i = blockIdx.x;
    int64_t start, len;
    co_window_of(ptr, win_ptr, n_rows, w, g0 + i, start, len);
    if (FORM == CO_FORM_WAVE ? len > CO_WAVE : (len <= CO_WAVE || len > CO_TILE)) return;   // block-uniform: another form's
    if (len < 2) {
      if (!write && threadIdx.x == 0) out_cnt[i] = 0;
      return;
    }
    const unsigned long long c = co_window<THREADS>(ids, start, len, V, symmetric != 0, keys, rs, pow2_at_least(len), sh,
                                                    write, out_key, out_mult, out_m, write ? rec_ptr[i] - rec_ptr[0] : 0);
    if (!write && threadIdx.x == 0) out_cnt[i] = (int64_t)c;
  } else {
    unsigned char* slot = ws + (int64_t)blockIdx.x * slot_bytes;
    unsigned long long* a = (unsigned long long*)slot;
    int32_t* rs = (int32_t*)(slot + pow2_at_least(ws_tokens) * (int64_t)sizeof(unsigned long long));
    for (int64_t i = blockIdx.x; i < ng; i += gridDim.x) {
      int64_t start, len;
      co_window_of(ptr, win_ptr, n_rows, w, g0 + i, start, len);
      if (len <= CO_TILE) continue;                          // block-uniform: an LDS form's window
      if (len > ws_tokens) {                                 // `longest` was understated (precondition): no record
        if (!write && threadIdx.x == 0) out_cnt[i] = 0;
        continue;
      }
      const unsigned long long c = co_window<THREADS>(ids, start, len, V, symmetric != 0, a, rs, pow2_at_least(len), sh,
                                                      write, out_key, out_mult, out_m, write ? rec_ptr[i] - rec_ptr[0] : 0);
      if (!write && threadIdx.x == 0) out_cnt[i] = (int64_t)c;
    }
  }
}

__global__ __launch_bounds__(256) void co_norm_kernel(const int64_t* __restrict__ cell_ptr, const int32_t* __restrict__ m,
                                                      const int64_t* __restrict__ adds, int64_t n, float* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  double s = 0.0;
  for (int64_t i = cell_ptr[c]; i < cell_ptr[c + 1]; ++i) s += (double)adds[i] / (double)m[i];   // m ascending
  out[c] = (float)s;
}

struct CoPmi {
  int64_t V;
  double total, k, min_cooc, ln_base;
  int32_t ppmi, base_mode;
};

__device__ __forceinline__ double co_none(const CoPmi& c) { return c.ppmi ? 0.0 : -__builtin_huge_val(); }

// ref:pmi_calculator.py:142-193, operation for operation
__device__ __forceinline__ double co_pmi(double cell, int64_t row, int64_t col, const double* __restrict__ marginals,
                                         const CoPmi& c) {
  if (cell < c.min_cooc) {
    if (c.k > 0.0) cell = c.k; else return co_none(c);
  }
  const double p_joint = (cell + c.k) / (c.total + c.k * (double)c.V * (double)c.V);
  const double p1 = marginals[row], p2 = marginals[col];
  if (p1 == 0.0 || p2 == 0.0) return co_none(c);
  const double x = p_joint / (p1 * p2);
  double pmi = c.base_mode == SNX_COOC_LOG2 ? log2(x) : c.base_mode == SNX_COOC_LOGE ? log(x) : log(x) / c.ln_base;
  if (c.ppmi) pmi = pmi > 0.0 ? pmi : 0.0;
  return pmi;
}

__global__ __launch_bounds__(256) void co_pmi_cells_kernel(const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices,
                                                           const float* __restrict__ data, int64_t nnz,
                                                           const double* __restrict__ marginals, CoPmi c,
                                                           double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nnz) return;
  int64_t lo = 0, hi = c.V - 1;                              // the row r with indptr[r] <= i < indptr[r + 1]
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (indptr[mid + 1] <= i) lo = mid + 1; else hi = mid;
  }
  const int32_t col = indices[i];
  out[i] = (col < 0 || (int64_t)col >= c.V) ? co_none(c) : co_pmi((double)data[i], lo, col, marginals, c);
}

__global__ __launch_bounds__(256) void co_pmi_pairs_kernel(const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices,
                                                           const float* __restrict__ data,
                                                           const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                           int64_t n, const double* __restrict__ marginals, CoPmi c,
                                                           double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t r = rows[i], q = cols[i];
  if (r < 0 || q < 0 || (int64_t)r >= c.V || (int64_t)q >= c.V) {   // a term outside the vocabulary
    out[i] = co_none(c);
    return;
  }
  const int64_t r0 = indptr[r], r1 = indptr[r + 1];
  const int64_t p = lower_bound(indices, r0, r1, q);
  const double cell = (p < r1 && indices[p] == q) ? (double)data[p] : 0.0;
  out[i] = co_pmi(cell, r, q, marginals, c);
}

// bytes of a workspace slot of the long-window form, 0 when every window fits an LDS form
int64_t co_slot_bytes(int64_t longest) {
  if (longest <= CO_TILE) return 0;
  return (int64_t)align256((size_t)pow2_at_least(longest) * sizeof(unsigned long long) +
                           (size_t)(longest + 1) * sizeof(int32_t));
}

bool co_pmi_ok(int64_t V, int32_t base_mode, double ln_base) {
  if (V < 1 || V > 3037000499ll) return false;               // V * V < 2^63
  if (base_mode != SNX_COOC_LOG2 && base_mode != SNX_COOC_LOGE && base_mode != SNX_COOC_LOGB) return false;
  return base_mode != SNX_COOC_LOGB || ln_base != 0.0;
}

}  // namespace

extern "C" size_t snx_cooc_workspace_bytes(int64_t longest_window) {
  if (longest_window < 0 || longest_window >= (1ll << 31)) return 0;
  return (size_t)co_slot_bytes(longest_window) * CO_LONG_GROUPS;
}

extern "C" int snx_cooc_windows(const int64_t* ptr, const int32_t* ids, int32_t n_rows, const int64_t* win_ptr,
                                int64_t window_size, int64_t first_window, int64_t n_windows, int64_t longest_window,
                                int64_t V, int32_t symmetric, const int64_t* rec_ptr, int64_t* out_cnt, int64_t* out_key,
                                int64_t* out_mult, int32_t* out_m, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (n_rows < 0 || n_windows < 0 || n_windows >= (1ll << 31) || first_window < 0 || longest_window < 0 ||
      longest_window >= (1ll << 31) || V < 1 || V > 3037000499ll || (win_ptr && window_size < 1))
    return SNX_E_SHAPE;
  if (n_windows == 0) return SNX_OK;
  if (!ptr || n_rows == 0) return SNX_E_ARG;                 // ids may be NULL when every row is empty
  if (!win_ptr && first_window + n_windows > (int64_t)n_rows) return SNX_E_SHAPE;
  if (rec_ptr ? (!out_key || !out_mult) : !out_cnt) return SNX_E_ARG;
  const int64_t slot = co_slot_bytes(longest_window);
  if (slot && (!workspace || ws_bytes < (size_t)slot * CO_LONG_GROUPS)) return SNX_E_ARG;
  const dim3 grid((unsigned)n_windows);
  hipLaunchKernelGGL((co_window_kernel<64, CO_FORM_WAVE>), grid, dim3(64), 0, st, ptr, ids, win_ptr, n_rows, window_size,
                     first_window, n_windows, V, symmetric, (unsigned char*)nullptr, (int64_t)0, (int64_t)0, rec_ptr,
                     out_cnt, out_key, out_mult, out_m);
  SNX_CHECK_LAUNCH();
  if (longest_window > CO_WAVE) {
    hipLaunchKernelGGL((co_window_kernel<256, CO_FORM_TILE>), grid, dim3(256), 0, st, ptr, ids, win_ptr, n_rows,
                       window_size, first_window, n_windows, V, symmetric, (unsigned char*)nullptr, (int64_t)0, (int64_t)0,
                       rec_ptr, out_cnt, out_key, out_mult, out_m);
    SNX_CHECK_LAUNCH();
  }
  if (slot) {
    hipLaunchKernelGGL((co_window_kernel<256, CO_FORM_LONG>), dim3((unsigned)(n_windows < CO_LONG_GROUPS ? n_windows : CO_LONG_GROUPS)),
                       dim3(256), 0, st, ptr, ids, win_ptr, n_rows, window_size, first_window, n_windows, V, symmetric,
                       (unsigned char*)workspace, longest_window, slot, rec_ptr, out_cnt, out_key, out_mult, out_m);
    SNX_CHECK_LAUNCH();
  }
  return SNX_OK;
}

extern "C" int snx_cooc_normalized_cells(const int64_t* cell_ptr, const int32_t* m, const int64_t* adds, int64_t n_cells,
                                         float* out, hipStream_t st) {
  if (n_cells < 0 || n_cells >= (1ll << 39)) return SNX_E_SHAPE;
  if (n_cells == 0) return SNX_OK;
  if (!cell_ptr || !m || !adds || !out) return SNX_E_ARG;
  hipLaunchKernelGGL(co_norm_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, st, cell_ptr, m, adds, n_cells,
                     out);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_cooc_pmi_cells(const int64_t* indptr, const int32_t* indices, const float* data, int64_t V, int64_t nnz,
                                  const double* marginals, double total, double laplace, double min_cooccurrence,
                                  int32_t use_ppmi, int32_t base_mode, double ln_base, double* out, hipStream_t st) {
  if (nnz < 0 || nnz >= (1ll << 39) || !co_pmi_ok(V, base_mode, ln_base)) return SNX_E_SHAPE;
  if (nnz == 0) return SNX_OK;
  if (!indptr || !indices || !data || !marginals || !out) return SNX_E_ARG;
  const CoPmi c{V, total, laplace, min_cooccurrence, ln_base, use_ppmi, base_mode};
  hipLaunchKernelGGL(co_pmi_cells_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, indptr, indices, data, nnz,
                     marginals, c, out);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_cooc_pmi_pairs(const int64_t* indptr, const int32_t* indices, const float* data, int64_t V,
                                  const int32_t* rows, const int32_t* cols, int64_t n, const double* marginals, double total,
                                  double laplace, double min_cooccurrence, int32_t use_ppmi, int32_t base_mode,
                                  double ln_base, double* out, hipStream_t st) {
  if (n < 0 || n >= (1ll << 39) || !co_pmi_ok(V, base_mode, ln_base)) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!indptr || !rows || !cols || !marginals || !out) return SNX_E_ARG;   // indices / data may be NULL: an empty matrix
  const CoPmi c{V, total, laplace, min_cooccurrence, ln_base, use_ppmi, base_mode};
  hipLaunchKernelGGL(co_pmi_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, indptr, indices, data, rows,
                     cols, n, marginals, c, out);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
