// Device code shared by the dense-retrieval kernels: dn_search_kernel and dn_merge_kernel (dense.hip), iv_scan_kernel and
// iv_merge_kernel (ivf.hip).  Both files are pinned to one contract (include/snx.h): s(q, d) is the fp32 fmaf chain over
// the dimensions in ascending order from +0, then + 0.0f; results are ordered score descending, then doc ascending, bit
// for bit; and inside one candidate list docs ascend along the walk, so a later doc that only ties the list's threshold
// loses to the k already kept and `key > threshold` is exact.  The tests hold the two searches to each other bit for bit,
// so everything that states that contract for the search kernels -- the order key, the MFMA tile, the admission of a
// score, the compaction of a list -- lives here once.  The merge stage is the sparse searches' too and lives with them
// in sparse_common.h: the merge kernels' view of the lists (RankLists), their output tail (write_ranks, decoding with
// dense_unkey here) and, for dn_merge_kernel, whose lists are met in doc order, the whole merge (merge_lists).
// Not here.  The target-rank count of dn_search_kernel: only that kernel has it.  The selection front of
// iv_merge_kernel: its lists are not in doc order, so it selects the tie by doc id and not by ordered_take as merge_lists
// does; they are two rules, not one.  gemm_f32_128_kernel (f32_path.hip) runs the same MFMA loop over strided operands
// with epilogues, under the training goldens.  infogain.hip is the float64 difference form on a 64-wide tile with
// ascending pair keys: it shares the host's split_plan (sparse_common.h) and nothing on the device.
#pragma once
#include "sparse_common.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int DN_THREADS = 256;
constexpr int DN_TILE = 128;                   // query rows and doc rows of a workgroup's tile
constexpr int DN_KT = 16;                      // K per LDS stage
constexpr int DN_PITCH = 132;                  // LDS row pitch (floats), as the 128-wide tiles of f32_path.hip
constexpr int DN_CAP_MAX = 2048;               // candidate list entries for k = 1024
constexpr int DN_DMAX = 4096;

// entries of a candidate list: a power of two (the sort), room for the k kept and the tiles until the next sort
inline int dn_cap(int32_t k) { return (int)pow2_at_least((long)(2 * k > 512 ? 2 * k : 512)); }

// Order key: the usual monotone map of fp32 bits to uint32 (negatives: all bits flipped; others: sign bit set), since
// every doc is a candidate whatever its sign; it is never 0 for a number, so 0 stays radix_select's "no entry".
__device__ __forceinline__ uint32_t dense_key(float s) {
  const uint32_t b = fbits(s);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dense_unkey(uint32_t key) {
  return bitsf((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// this thread's share of a 128 x 16 operand tile of a row-major [*, D] matrix: tile rows r and r + 64, 4 k each.
// row_of(tile row) is the matrix row, negative for a row that reads as zero; k past D reads as zero.
template <typename RowF>
__device__ __forceinline__ void dn_fetch(const float* __restrict__ P, RowF row_of, int D, int k0, int vec, int t,
                                         float (&v)[8]) {
  const int kk = k0 + (t & 3) * 4;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long row = row_of((t >> 2) + 64 * i);
    if (row >= 0 && vec && kk < D) {                         // vec: D % 4 == 0 and 16-byte aligned rows
      const f32x4 x = *(const f32x4*)(P + row * D + kk);
      v[4 * i] = x[0]; v[4 * i + 1] = x[1]; v[4 * i + 2] = x[2]; v[4 * i + 3] = x[3];
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[4 * i + u] = (row >= 0 && kk + u < D) ? P[row * D + kk + u] : 0.f;
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

// The scores of one 128 x 128 tile by the whole workgroup, A's rows against B's rows over all of D: four waves of 2 x 2
// accumulators, register prefetch, double-buffered LDS.  With wave = 2 wm + wn and lane = 32 h + c,
// acc[i][j][r] = s(A tile row 64 wm + 32 i + (r & 3) + 8 (r >> 2) + 4 h, B tile row 64 wn + 32 j + c).  Ends on a barrier.
template <typename RowA, typename RowB>
__device__ __forceinline__ void dn_tile_scores(const float* __restrict__ A, RowA row_a, int vec_a,
                                               const float* __restrict__ B, RowB row_b, int vec_b, int D,
                                               f32x16 (&acc)[2][2]) {
  __shared__ __attribute__((aligned(16))) float As[2][DN_KT][DN_PITCH];
  __shared__ __attribute__((aligned(16))) float Bs[2][DN_KT][DN_PITCH];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const int nk = (D + DN_KT - 1) / DN_KT;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float va[8], vb[8];
  dn_fetch(A, row_a, D, 0, vec_a, t, va);
  dn_fetch(B, row_b, D, 0, vec_b, t, vb);
  dn_put(t, va, As[0]);
  dn_put(t, vb, Bs[0]);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      dn_fetch(A, row_a, D, (kt + 1) * DN_KT, vec_a, t, va);
      dn_fetch(B, row_b, D, (kt + 1) * DN_KT, vec_b, t, vb);
    }
#pragma unroll
    for (int s = 0; s < DN_KT / 2; ++s) {                    // k ascending: the ABI's chain
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
}

// One finished score s of `doc` against a query row, the whole wave at once: `ok` (the pair exists), above the row's
// threshold key `th`, strictly below its ceiling `cl` when there is one, and not in its exclusion row ex_doc[ex0 .. ex1)
// when there are any -> appended to the row's candidate list at the LDS cursor `cnt`.  An entry past `cap` is counted and
// dropped; the caller compacts before a tile could get there.
__device__ __forceinline__ void dn_admit(bool ok, float s, int32_t doc, uint32_t th, bool has_c, float cl, bool has_x,
                                         const int32_t* __restrict__ ex_doc, const int64_t& ex0, const int64_t& ex1,
                                         int& cnt, unsigned long long* list, int cap) {
  const uint32_t key = dense_key(s);
  const bool pass = ok && key > th && (!has_c || s < cl);    // a NaN ceiling admits nothing
  if (__ballot(pass) != 0ull && pass) {
    bool excluded = false;
    if (has_x) {
      const int64_t e1 = ex1;
      const int64_t p = lower_bound(ex_doc, ex0, e1, doc);
      excluded = p < e1 && ex_doc[p] == doc;
    }
    if (!excluded) {
      const int pos = atomicAdd(&cnt, 1);
      if (pos < cap) list[pos] = rank_key(key, (uint32_t)doc);
    }
  }
}

// sort the candidate list `list` (cnt entries, capacity cap) by the whole workgroup, keep the best k, raise its threshold
__device__ __forceinline__ void dn_compact(unsigned long long* list, int& cnt, uint32_t& thr, int k, int cap) {
  __shared__ unsigned long long sbuf[DN_CAP_MAX];
  const int t = threadIdx.x, n = cnt;
  for (int i = t; i < cap; i += DN_THREADS) sbuf[i] = i < n ? list[i] : 0ull;
  __syncthreads();
  bitonic_desc<DN_THREADS, int>(sbuf, cap);
  const int m = min(n, k);
  for (int i = t; i < m; i += DN_THREADS) list[i] = sbuf[i];
  if (t == 0) {
    cnt = m;
    if (n >= k) thr = rank_bits(sbuf[k - 1]);
  }
  __syncthreads();
}

}  // namespace
