// Pairwise MaxSim over ragged multi-vector rows (include/snx.h "multi-vector teacher scores"): BGE-M3's late-interaction
// score of a (query, document) pair of sequences that live in one unpadded row store,
//
//   maxsim(a, b) = (1 / Lq) * sum_i max_j <mv[a][i], mv[b][j]>,      Lq = rows of a, Ld = rows of b,
//
// as its own MFMA kernel: no [pairs, Lq, Ld] tensor, no padded copy of the rows, no float atomics.
//
// ms_pair_kernel   One workgroup (four waves) per (pair, block of 64 query rows).  It walks the document's rows in tiles
//                  of 64.  A 64 x 64 tile of S = Q D^T is four 32 x 32 accumulators, one per wave (wave = 2 wm + wn owns
//                  query rows 32 wm .. and doc rows 32 wn ..), formed on v_mfma_f32_32x32x16_bf16 for the bf16 store and on
//                  v_mfma_f32_32x32x2_f32 for the fp32 store.  Both operands pass through LDS in K slices (64 bf16 or 32
//                  fp32 per row: 8 KB per operand and stage), fetched into registers one slice ahead and double-buffered,
//                  so a 64-row block at D = 1024 never holds more than its current and next slice.  Each lane keeps the
//                  running maximum of its 16 accumulator rows in registers across the document tiles, from -inf; a doc
//                  row past Ld is masked to -inf in the accumulator (its zero-filled operand never reaches a max).  After
//                  the last tile the maxima are merged over the 32 lanes of a half wave (shuffles) and over the two wn
//                  waves (LDS): a max is exact in any order.  One thread then adds the block's row maxima in ascending
//                  row order and either writes the pair's score (every pair of the call fits one block) or the block's
//                  partial sum.
// ms_finish_kernel One thread per pair: the partial sums of its blocks in ascending block order, one division by Lq.
//
// The K loop of a tile is the same for every pair and block, and the order of every sum is fixed by the rows alone, so a
// score is a pure function of the two sequences' rows: bit-identical from call to call and whatever else is in the list.
// Pairs that share a query do not share its staged rows: the query block is re-read per document tile from the L2,
// which a 64-row block (128 KB at D = 1024 in bf16) fits many times over.
#include "common.h"
#include "runtime.h"
#include "snx.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int MS_THREADS = 256;
constexpr int MS_TILE = 64;                    // query rows of a block and doc rows of a tile
constexpr int MS_DMAX = 1024;

// The operand staging and the MFMA steps of one precision.  fetch: this thread's share of a 64-row K slice into registers
// (rows t >> 3 and 32 + (t >> 3), 16 bytes each; a row index < 0 reads as zero); put: registers -> LDS stage; mma: the
// slice's MFMA steps in ascending k.  Lane 32 h + c of a wave supplies row c of its operand.
struct MsBf16 {
  typedef bf16_t elem;
  static constexpr int KT = 64, PITCH = 72;    // 144-byte rows: 16 rows that differ mod 16 sit on 16 different 16-byte slots
  struct Stage { uint16_t a[MS_TILE][PITCH], b[MS_TILE][PITCH]; };
  struct Regs { u32x4 v[2]; };
  __device__ static __forceinline__ void fetch(const elem* __restrict__ P, long row0, int nrows, int D, int k0, int t,
                                               Regs& r) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (t >> 3) + 32 * i;
      r.v[i] = row < nrows ? *(const u32x4*)(P + (row0 + row) * D + k0 + (t & 7) * 8) : (u32x4){0u, 0u, 0u, 0u};
    }
  }
  __device__ static __forceinline__ void put(int t, const Regs& r, uint16_t (*S)[PITCH]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *(u32x4*)&S[(t >> 3) + 32 * i][(t & 7) * 8] = r.v[i];
  }
  __device__ static __forceinline__ void mma(const Stage& s, int wm, int wn, int c, int h, f32x16& acc) {
#pragma unroll
    for (int u = 0; u < KT / 16; ++u) {
      const int ko = 16 * u + 8 * h;
      const bf16x8 a = *(const bf16x8*)&s.a[wm * 32 + c][ko], b = *(const bf16x8*)&s.b[wn * 32 + c][ko];
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
  }
};

struct MsF32 {
  typedef float elem;
  static constexpr int KT = 32, PITCH = 68;    // k-major stage [KT][rows], as the fp32 tiles of dense_common.h
  struct Stage { float a[KT][PITCH], b[KT][PITCH]; };
  struct Regs { f32x4 v[2]; };
  __device__ static __forceinline__ void fetch(const elem* __restrict__ P, long row0, int nrows, int D, int k0, int t,
                                               Regs& r) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (t >> 3) + 32 * i;
      r.v[i] = row < nrows ? *(const f32x4*)(P + (row0 + row) * D + k0 + (t & 7) * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
  __device__ static __forceinline__ void put(int t, const Regs& r, float (*S)[PITCH]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int u = 0; u < 4; ++u) S[(t & 7) * 4 + u][(t >> 3) + 32 * i] = r.v[i][u];
  }
  __device__ static __forceinline__ void mma(const Stage& s, int wm, int wn, int c, int h, f32x16& acc) {
#pragma unroll
    for (int u = 0; u < KT / 2; ++u)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s.a[2 * u + h][wm * 32 + c], s.b[2 * u + h][wn * 32 + c], acc, 0, 0, 0);
  }
};

// rows [lo, hi) of sequence s of the store; an index outside [0, nseq) (the host refuses it) has no rows
__device__ __forceinline__ void ms_rows(const int64_t* __restrict__ mv_ptr, int nseq, int s, long& lo, int& n) {
  const bool ok = (unsigned)s < (unsigned)nseq;
  lo = ok ? mv_ptr[s] : 0;
  n = ok ? (int)(mv_ptr[s + 1] - lo) : 0;
}

template <typename P>
__global__ __launch_bounds__(MS_THREADS) void ms_pair_kernel(const typename P::elem* __restrict__ mv,
                                                             const int64_t* __restrict__ mv_ptr, int nseq, int D,
                                                             const int32_t* __restrict__ pair_q,
                                                             const int32_t* __restrict__ pair_d, int qblocks,
                                                             float* __restrict__ partial, float* __restrict__ score) {
  __shared__ __attribute__((aligned(16))) typename P::Stage stage[2];
  __shared__ float rmax[2][MS_TILE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const long pair = blockIdx.x;
  const int qb = blockIdx.y;
  long q0, d0;
  int Lq, Ld;
  ms_rows(mv_ptr, nseq, pair_q[pair], q0, Lq);
  ms_rows(mv_ptr, nseq, pair_d[pair], d0, Ld);
  const bool direct = qblocks == 1;            // every pair of the launch fits one block: no second kernel
  if (Lq <= 0 || Ld <= 0) {
    if (direct && t == 0) score[pair] = 0.f;
    return;
  }
  const int nq = min(MS_TILE, Lq - qb * MS_TILE);             // query rows of this block
  if (nq <= 0) return;
  q0 += (long)qb * MS_TILE;
  const int nk = D / P::KT;

  float m[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) m[r] = -INFINITY;
  for (int n0 = 0; n0 < Ld; n0 += MS_TILE) {
    const int nd = min(MS_TILE, Ld - n0);                     // doc rows of this tile
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    typename P::Regs ra, rb;
    P::fetch(mv, q0, nq, D, 0, t, ra);
    P::fetch(mv, d0 + n0, nd, D, 0, t, rb);
    P::put(t, ra, stage[0].a);
    P::put(t, rb, stage[0].b);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {                         // k ascending, the same steps for every tile
      const int cur = kt & 1;
      if (kt + 1 < nk) {
        P::fetch(mv, q0, nq, D, (kt + 1) * P::KT, t, ra);
        P::fetch(mv, d0 + n0, nd, D, (kt + 1) * P::KT, t, rb);
      }
      P::mma(stage[cur], wm, wn, c, h, acc);
      if (kt + 1 < nk) {
        P::put(t, ra, stage[cur ^ 1].a);
        P::put(t, rb, stage[cur ^ 1].b);
      }
      __syncthreads();
    }
    // acc[r] = S(query row 32 wm + (r & 3) + 8 (r >> 2) + 4 h, doc row n0 + 32 wn + c)
    const bool ok = wn * 32 + c < nd;
#pragma unroll
    for (int r = 0; r < 16; ++r) m[r] = fmaxf(m[r], ok ? acc[r] : -INFINITY);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) m[r] = fmaxf(m[r], __shfl_xor(m[r], o, 64));
    if (c == 0) rmax[wn][wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = m[r];
  }
  __syncthreads();
  if (t == 0) {
    float s = 0.f;
    for (int i = 0; i < nq; ++i) s += fmaxf(rmax[0][i], rmax[1][i]);        // ascending rows
    if (direct) score[pair] = s / (float)Lq;
    else partial[pair * qblocks + qb] = s;
  }
}

__global__ __launch_bounds__(MS_THREADS) void ms_finish_kernel(const int64_t* __restrict__ mv_ptr, int nseq,
                                                               const int32_t* __restrict__ pair_q,
                                                               const int32_t* __restrict__ pair_d, int64_t npairs,
                                                               int qblocks, const float* __restrict__ partial,
                                                               float* __restrict__ score) {
  const int64_t p = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
  if (p >= npairs) return;
  long q0, d0;
  int Lq, Ld;
  ms_rows(mv_ptr, nseq, pair_q[p], q0, Lq);
  ms_rows(mv_ptr, nseq, pair_d[p], d0, Ld);
  float out = 0.f;
  if (Lq > 0 && Ld > 0) {
    const int nb = min(qblocks, (Lq + MS_TILE - 1) / MS_TILE);
    float s = partial[p * qblocks];
    for (int b = 1; b < nb; ++b) s += partial[p * qblocks + b];             // ascending blocks
    out = s / (float)Lq;
  }
  score[p] = out;
}

// the device image of the call in the workspace: mv_ptr, pair_q, pair_d, then one partial sum per (pair, block)
struct MsPlan {
  size_t ptr, pq, pd, partial, total;
  int qblocks;
  MsPlan(int32_t nseq, int64_t npairs, int32_t max_rows) {
    Arena a;
    qblocks = max_rows > 0 ? (max_rows + MS_TILE - 1) / MS_TILE : 1;
    ptr = a.take(((size_t)nseq + 1) * 8);
    pq = a.take((size_t)npairs * 4);
    pd = a.take((size_t)npairs * 4);
    partial = a.take(qblocks > 1 ? (size_t)npairs * qblocks * 4 : 0);
    total = a.off;
  }
};

inline bool ms_bad_shape(int32_t nseq, int64_t npairs, int32_t max_rows) {
  return nseq <= 0 || npairs < 0 || npairs > 0x7FFFFFFFL || max_rows < 0 ||
         (int64_t)((max_rows + MS_TILE - 1) / MS_TILE) > 65535;
}

}  // namespace

extern "C" size_t snx_maxsim_workspace_bytes(int32_t nseq, int64_t npairs, int32_t max_rows) {
  return ms_bad_shape(nseq, npairs, max_rows) ? 0 : MsPlan(nseq, npairs, max_rows).total;
}

extern "C" int snx_maxsim_pairs(const void* mv, int32_t mv_f32, int64_t nrows, int32_t D, const int64_t* mv_ptr,
                                int32_t nseq, const int32_t* pair_q, const int32_t* pair_d, int64_t npairs,
                                int32_t max_rows, float* score, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (D <= 0 || (D % 64) != 0 || D > MS_DMAX || ms_bad_shape(nseq, npairs, max_rows) || nrows < 0) return SNX_E_SHAPE;
  if (npairs == 0) return SNX_OK;
  if (!mv_ptr || !pair_q || !pair_d || !score || !workspace || (nrows > 0 && !mv) || ((uintptr_t)mv & 15) != 0 ||
      ((uintptr_t)workspace & 15) != 0)
    return SNX_E_ARG;
  // the three index arrays are host memory: everything a kernel will trust is checked here, before any launch.  They are
  // pageable by contract (snx.h): hipMemcpyAsync below has staged them when it returns, and the caller may free them
  if (mv_ptr[0] != 0 || mv_ptr[nseq] > nrows) return SNX_E_ARG;
  for (int s = 0; s < nseq; ++s)
    if (mv_ptr[s + 1] < mv_ptr[s] || mv_ptr[s + 1] - mv_ptr[s] > max_rows) return SNX_E_ARG;
  for (int64_t p = 0; p < npairs; ++p)
    if ((uint32_t)pair_q[p] >= (uint32_t)nseq || (uint32_t)pair_d[p] >= (uint32_t)nseq) return SNX_E_ARG;
  const MsPlan plan(nseq, npairs, max_rows);
  if (ws_bytes < plan.total) return SNX_E_ARG;
  char* ws = (char*)workspace;
  const struct { size_t off; const void* src; size_t bytes; } up[3] = {
      {plan.ptr, mv_ptr, ((size_t)nseq + 1) * 8}, {plan.pq, pair_q, (size_t)npairs * 4}, {plan.pd, pair_d, (size_t)npairs * 4}};
  for (const auto& u : up) {
    const hipError_t e = hipMemcpyAsync(ws + u.off, u.src, u.bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return (int)e;
  }
  const int64_t* dptr = (const int64_t*)(ws + plan.ptr);
  const int32_t *dq = (const int32_t*)(ws + plan.pq), *dd = (const int32_t*)(ws + plan.pd);
  float* partial = (float*)(ws + plan.partial);
  const dim3 grid((unsigned)npairs, (unsigned)plan.qblocks);
  if (mv_f32)
    hipLaunchKernelGGL(ms_pair_kernel<MsF32>, grid, dim3(MS_THREADS), 0, st, (const float*)mv, dptr, nseq, D, dq, dd,
                       plan.qblocks, partial, score);
  else
    hipLaunchKernelGGL(ms_pair_kernel<MsBf16>, grid, dim3(MS_THREADS), 0, st, (const bf16_t*)mv, dptr, nseq, D, dq, dd,
                       plan.qblocks, partial, score);
  SNX_CHECK_LAUNCH();
  if (plan.qblocks > 1) {
    hipLaunchKernelGGL(ms_finish_kernel, dim3(cdiv(npairs, MS_THREADS)), dim3(MS_THREADS), 0, st, dptr, nseq, dq, dd, npairs,
                       plan.qblocks, (const float*)partial, score);
    SNX_CHECK_LAUNCH();
  }
  return SNX_OK;
}
