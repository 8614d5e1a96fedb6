// Sparse-vector pruning and the rescoring half of two-phase search (include/snx.h "pruning and two-phase search"): the
// reference's `rank_features` serving path behind OpenSearch's neural_sparse_two_phase_processor
// (ref:benchmark/index_manager.py:197-238) and the ingest-time prune rules max_ratio | abs_value | top_k | alpha_mass.
// The thresholds are this project's deterministic definitions under OpenSearch's names.
//
//   tp_prune_kernel    a fixed grid of workgroups walking the CSR rows r, r + G, ...; one row per workgroup at a time,
//                      lanes over its entries.  max_ratio / abs_value: a workgroup max and a compare.  top_k: the 8-bit
//                      radix select on the weight bits of sz_prune_kernel, then the ties at the threshold are taken in
//                      row (= term) order by an ordered ballot count.  alpha_mass: keys (weight bits << 32 | ~position)
//                      sorted descending by a bitonic sort, in LDS up to TP_SORT_LDS entries and in the workgroup's
//                      slot of the caller's workspace beyond (a random-init model activates the whole vocabulary), the
//                      fp32 left folds on one lane, then every entry's flag from its sorted position.  Output: one keep
//                      flag per entry and the kept count per row; the caller compacts.
//   tp_rescore_kernel  one workgroup per query, the query row staged in LDS (a row longer than TP_QMAX is read from
//                      memory instead); one lane per candidate merges the query with the candidate's CSR row (the
//                      ascending-term fmaf chain: s(q, d) of the exact index bit for bit); the <= 1024 keys (score bits
//                      << 32 | ~doc) are sorted descending in LDS as sr_merge_kernel does, equal neighbours (a doc given
//                      twice) collapse, and the first k distinct keys are written in order.
// Two-phase search = snx_sparse_search over the pruned query rows with k = W, then tp_rescore_kernel with the full
// rows (snx/retrieval/sparse.py SparseIndex.search_two_phase).  No float atomics: byte-identical from run to run.
#include <math.h>

// row_dot, the rank key and bitonic_desc come from sparse_common.h.
#include "sparse_common.h"
#include "snx.h"

namespace {

constexpr int TP_THREADS = 256;
constexpr int TP_WAVES = TP_THREADS / 64;
constexpr int TP_SORT_LDS = 4096;                // alpha_mass rows up to this length sort in LDS, longer ones in a slot
constexpr int TP_SLOTS = 128;                    // prune workgroups when rows sort in workspace slots
constexpr int TP_GRID = 2048;                    // prune workgroups otherwise
constexpr int TP_QMAX = 1024;                    // query terms staged in LDS by the rescore
constexpr int TP_WMAX = 1024;                    // rescore window cap

// ------------------------------------------------------------------------------------------------ prune
struct PruneSmem {
  unsigned long long sbuf[TP_SORT_LDS];
  int hist[256];
  float wmax[TP_WAVES];
  int wsum[TP_WAVES];
  int sh[2];
  int nkeep;
};

// sum over the workgroup through a per-wave array (two barriers; the select's block_sum keeps its LDS word)
__device__ __forceinline__ int wave_array_sum(int v, int* wsum) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                                           // the previous readers of wsum are done
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
#pragma unroll
  for (int w = 0; w < TP_WAVES; ++w) r += wsum[w];
  return r;
}

__global__ __launch_bounds__(TP_THREADS) void tp_prune_kernel(const int64_t* __restrict__ ptr,
                                                              const float* __restrict__ w, int32_t n, int64_t nnz,
                                                              int32_t type, float value, int32_t topn,
                                                              uint8_t* __restrict__ keep,
                                                              int32_t* __restrict__ kept_cnt, char* ws,
                                                              size_t slot_bytes, long slot_cap) {
  __shared__ PruneSmem S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long* G = ws ? (unsigned long long*)(ws + (size_t)blockIdx.x * slot_bytes) : nullptr;
  for (int r = blockIdx.x; r < n; r += gridDim.x) {
    const int64_t a = min(max(ptr[r], (int64_t)0), nnz);
    const int64_t L = min(max(ptr[r + 1], a), nnz) - a;      // never past the arrays, whatever ptr holds
    const float* rw = w + a;
    uint8_t* rk = keep + a;
    int kept = 0;
    if (type == SNX_PRUNE_MAX_RATIO || type == SNX_PRUNE_ABS_VALUE) {
      float thr = value;
      if (type == SNX_PRUNE_MAX_RATIO) {
        float m = 0.f;
        for (int64_t i = tid; i < L; i += TP_THREADS) m = fmaxf(m, rw[i]);
        m = wave_max(m);
        __syncthreads();                                     // the previous row's readers of wmax are done
        if (lane == 0) S.wmax[wave] = m;
        __syncthreads();
        m = S.wmax[0];
#pragma unroll
        for (int x = 1; x < TP_WAVES; ++x) m = fmaxf(m, S.wmax[x]);
        thr = value * m;                                     // fp32 multiply; r <= 1: the maximum passes
      }
      int local = 0;
      for (int64_t i = tid; i < L; i += TP_THREADS) {
        const bool k = rw[i] >= thr;
        rk[i] = k ? 1 : 0;
        local += k;
      }
      kept = wave_array_sum(local, S.wsum);
    } else if (type == SNX_PRUNE_TOP_K) {
      if (L <= topn) {
        for (int64_t i = tid; i < L; i += TP_THREADS) rk[i] = 1;
        kept = (int)L;
      } else {                                               // the topn largest weight bit patterns (weights > 0)
        uint32_t prefix = 0u, known = 0u;
        int remaining = topn;
        for (int shift = 24; shift >= 0; shift -= 8) {
          for (int i = tid; i < 256; i += TP_THREADS) S.hist[i] = 0;
          __syncthreads();
          for (int64_t i = tid; i < L; i += TP_THREADS) {
            const uint32_t kk = fbits(rw[i]);
            if ((kk & known) == prefix) atomicAdd(&S.hist[(kk >> shift) & 255u], 1);
          }
          __syncthreads();
          if (tid == 0) {
            int rem = remaining, b = 255;
            for (; b > 0; --b) {
              if (S.hist[b] >= rem) break;
              rem -= S.hist[b];
            }
            S.sh[0] = b;
            S.sh[1] = rem;
          }
          __syncthreads();
          prefix |= (uint32_t)S.sh[0] << shift;
          known |= 255u << shift;
          remaining = S.sh[1];
          __syncthreads();
        }
        const uint32_t thr = prefix;
        const int need_eq = remaining;
        int E = 0;                                           // ties at the threshold seen so far, in row (= term) order
        for (int64_t base = 0; base < L; base += TP_THREADS) {
          const int64_t i = base + tid;
          const uint32_t kk = i < L ? fbits(rw[i]) : 0u;
          const bool eq = i < L && kk == thr;
          const unsigned long long me = __ballot(eq);
          __syncthreads();                                   // the previous step's readers of wsum are done
          if (lane == 0) S.wsum[wave] = __popcll(me);
          __syncthreads();
          int before = E;
          for (int x = 0; x < TP_WAVES; ++x) {
            if (x < wave) before += S.wsum[x];
            E += S.wsum[x];
          }
          if (i < L) rk[i] = (kk > thr || (eq && before + __popcll(me & below) < need_eq)) ? 1 : 0;
        }
        kept = topn;
      }
    } else {                                                 // SNX_PRUNE_ALPHA_MASS
      const long P = pow2_at_least((long)L);
      unsigned long long* buf = P <= TP_SORT_LDS ? S.sbuf : G;
      if (P > TP_SORT_LDS && (!G || P > slot_cap)) {         // longer than the caller declared: not pruned
        for (int64_t i = tid; i < L; i += TP_THREADS) rk[i] = 0;
        kept = -1;
      } else {
        for (long i = tid; i < P; i += TP_THREADS)           // (weight desc, position asc); the padding 0 sorts last
          buf[i] = i < L ? rank_key(fbits(rw[i]), (uint32_t)i) : 0ull;
        __syncthreads();
        bitonic_desc<TP_THREADS>(buf, P);
        if (tid == 0) {                                      // the fp32 left folds, in sorted order
          float total = 0.f;
          for (int64_t i = 0; i < L; ++i) total = total + bitsf(rank_bits(buf[i]));
          const float goal = value * total;
          float acc = 0.f;
          int k = 0;
          for (int64_t i = 0; i < L; ++i) {
            acc = acc + bitsf(rank_bits(buf[i]));
            k = (int)i + 1;
            if (acc >= goal) break;
          }
          S.nkeep = k;
        }
        __syncthreads();
        kept = S.nkeep;
        for (int64_t i = tid; i < L; i += TP_THREADS)
          rk[(uint32_t)rank_id(buf[i])] = i < kept ? 1 : 0;
        __syncthreads();                                     // buf and nkeep are rewritten by the next row
      }
    }
    if (tid == 0) kept_cnt[r] = kept;
  }
}

// ------------------------------------------------------------------------------------------------ rescore
struct RescoreSmem {
  int32_t qt[TP_QMAX];
  float qw[TP_QMAX];
  unsigned long long key[TP_WMAX];               // (score bits << 32 | ~doc): descending = the ABI's order
  int wsum[TP_WAVES];
  int found;
};

__global__ __launch_bounds__(TP_THREADS) void tp_rescore_kernel(
    const int64_t* __restrict__ q_ptr, const int32_t* __restrict__ q_term, const float* __restrict__ q_w,
    const int32_t* __restrict__ cand_doc, int32_t W, const int64_t* __restrict__ doc_ptr,
    const int32_t* __restrict__ doc_term, const float* __restrict__ doc_w, int32_t nd,
    const int32_t* __restrict__ target, int32_t k, int32_t* __restrict__ out_doc, float* __restrict__ out_score,
    int32_t* __restrict__ out_rank, float* __restrict__ out_tscore) {
  __shared__ RescoreSmem S;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int64_t qa = q_ptr[q], qb = q_ptr[q + 1];
  const bool staged = qb - qa <= TP_QMAX;                    // uniform; a longer row is merged from memory
  const int nqt = staged ? (int)max(qb - qa, (int64_t)0) : 0;
  for (int i = tid; i < nqt; i += TP_THREADS) { S.qt[i] = q_term[qa + i]; S.qw[i] = q_w[qa + i]; }
  if (tid == 0) S.found = 0;
  const int P = (int)pow2_at_least((long)W);
  __syncthreads();
  const int32_t* cand = cand_doc + (int64_t)q * W;
  for (int c = tid; c < P; c += TP_THREADS) {                // one lane per candidate
    unsigned long long key = 0ull;
    if (c < W) {
      const int d = cand[c];
      if ((unsigned)d < (unsigned)nd) {
        const int64_t d0 = doc_ptr[d], d1 = doc_ptr[d + 1];
        const float s = staged ? row_dot(S.qt, S.qw, 0, nqt, doc_term, doc_w, d0, d1)
                               : row_dot(q_term, q_w, qa, qb, doc_term, doc_w, d0, d1);
        if (s > 0.f) key = rank_key(fbits(s), (uint32_t)d);
      }
    }
    S.key[c] = key;
  }
  __syncthreads();
  bitonic_desc<TP_THREADS>(S.key, (long)P);
  const int tt = target ? target[q] : -1;
  int32_t* od = out_doc + (int64_t)q * k;
  float* os = out_score + (int64_t)q * k;
  int nu = 0;                                                // distinct keys so far (uniform)
  for (int c0 = 0; c0 < P; c0 += TP_THREADS) {
    const int i = c0 + tid;
    const unsigned long long kk = i < P ? S.key[i] : 0ull;
    const bool uniq = kk != 0ull && (i == 0 || S.key[i - 1] != kk);   // a doc given twice: equal neighbours
    const unsigned long long m = __ballot(uniq);
    __syncthreads();                                         // the previous step's readers of wsum are done
    if (lane == 0) S.wsum[wave] = __popcll(m);
    __syncthreads();
    int pos = nu + __popcll(m & below);
    for (int x = 0; x < TP_WAVES; ++x) {
      if (x < wave) pos += S.wsum[x];
      nu += S.wsum[x];
    }
    if (uniq && pos < k) {
      const int d = rank_id(kk);
      os[pos] = bitsf(rank_bits(kk));
      od[pos] = d;
      if (d == tt) S.found = pos + 1;
    }
  }
  for (int i = min(nu, k) + tid; i < k; i += TP_THREADS) {
    os[i] = 0.f;
    od[i] = -1;
  }
  __syncthreads();
  if (tid == 0 && target) {
    out_rank[q] = S.found;
    float ts = 0.f;
    if ((unsigned)tt < (unsigned)nd) {
      const int64_t d0 = doc_ptr[tt], d1 = doc_ptr[tt + 1];
      ts = staged ? row_dot(S.qt, S.qw, 0, nqt, doc_term, doc_w, d0, d1)
                  : row_dot(q_term, q_w, qa, qb, doc_term, doc_w, d0, d1);
    }
    out_tscore[q] = ts;
  }
}

inline bool prune_value_ok(int32_t type, float v) {
  switch (type) {
    case SNX_PRUNE_MAX_RATIO: return v >= 0.f && v <= 1.f;
    case SNX_PRUNE_ABS_VALUE: return v >= 0.f;
    case SNX_PRUNE_TOP_K: return v >= 1.f && v == truncf(v);
    case SNX_PRUNE_ALPHA_MASS: return v > 0.f && v <= 1.f;
    default: return false;
  }
}

inline size_t prune_slot_bytes(int32_t max_row_nnz) { return align256((size_t)pow2_at_least((long)max_row_nnz) * 8); }

}  // namespace

extern "C" size_t snx_sparse_prune_workspace_bytes(int32_t prune_type, int32_t n, int32_t max_row_nnz) {
  if (prune_type != SNX_PRUNE_ALPHA_MASS || n <= 0 || max_row_nnz <= TP_SORT_LDS) return 0;
  return (size_t)(n < TP_SLOTS ? n : TP_SLOTS) * prune_slot_bytes(max_row_nnz);
}

extern "C" int snx_sparse_prune_rows(const int64_t* ptr, const float* w, int32_t n, int64_t nnz, int32_t max_row_nnz,
                                     int32_t prune_type, float value, uint8_t* keep, int32_t* kept_cnt,
                                     void* workspace, size_t ws_bytes, hipStream_t st) {
  if (!prune_value_ok(prune_type, value)) return SNX_E_ARG;   // unknown type, value out of range or NaN
  if (n < 0 || nnz < 0 || max_row_nnz < 0) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!ptr || !kept_cnt || (nnz > 0 && (!w || !keep))) return SNX_E_ARG;
  const size_t need = snx_sparse_prune_workspace_bytes(prune_type, n, max_row_nnz);
  if (need && (!workspace || ws_bytes < need)) return SNX_E_ARG;
  const int cap = need ? TP_SLOTS : TP_GRID;
  const int grid = n < cap ? n : cap;
  const int32_t topn = prune_type == SNX_PRUNE_TOP_K ? (value < 1073741824.f ? (int32_t)value : 1 << 30) : 0;
  hipLaunchKernelGGL(tp_prune_kernel, dim3(grid), dim3(TP_THREADS), 0, st, ptr, w, n, nnz, prune_type, value, topn,
                     keep, kept_cnt, need ? (char*)workspace : (char*)nullptr, need ? prune_slot_bytes(max_row_nnz) : 0,
                     need ? pow2_at_least((long)max_row_nnz) : 0L);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_sparse_rescore(const int64_t* q_ptr, const int32_t* q_term, const float* q_w, int32_t nq,
                                  const int32_t* cand_doc, int32_t W, const int64_t* doc_ptr, const int32_t* doc_term,
                                  const float* doc_w, int32_t nd, const int32_t* target, int32_t k, int32_t* out_doc,
                                  float* out_score, int32_t* out_rank, float* out_tscore, hipStream_t st) {
  if (!q_ptr || !cand_doc || !doc_ptr || !out_doc || !out_score) return SNX_E_ARG;
  if (target && (!out_rank || !out_tscore)) return SNX_E_ARG;
  if (nq < 0 || nd < 0 || W < 1 || W > TP_WMAX || k < 1 || k > W) return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  hipLaunchKernelGGL(tp_rescore_kernel, dim3(nq), dim3(TP_THREADS), 0, st, q_ptr, q_term, q_w, cand_doc, W, doc_ptr,
                     doc_term, doc_w, nd, target, k, out_doc, out_score, out_rank, out_tscore);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
