// Multi-vector candidate search (include/snx.h "multi-vector candidate search"): the centroid-interaction pass of
// ColBERTv2 / PLAID in front of the exact MaxSim score.  Every document row of the store is replaced by the id of its
// nearest centroid (a uint16 code); a query scores a document through its own table of query-row x centroid products,
//
//   a(q, d) = (1 / Lq) * sum_i max_{j in d} S[i, code[j]],      S[i, c] = bf16(<q_i, centroid_c>),
//
// and only the best ncand documents per query go to the exact scorer, which reads them in place from the store.  The
// candidate pass reads 2 bytes per document row where mv_search.hip reads 2 D.
//
// Order keys       A table entry is the bf16 of the product as a 16-bit ORDER KEY: the monotone map of the bf16 bits to a
//                  signed 16-bit integer (negatives: the low 15 bits flipped).  The max of two entries is then the integer
//                  max of their keys, and v_pk_max_i16 takes two of them per lane and instruction; the map is its own
//                  inverse, so the selection decodes the maxima it adds.  The key of -inf stands for "no row".
// Groups           The query rows of the call lie end to end (mv_search's packing); group g is rows R g .. R g + R - 1 of
//                  them, whichever queries they belong to.  R = 64 / 32 / 16 for nc <= 1024 / 2048 / 4096, so that a
//                  group's [nc][R] table is at most 128 KB and stays in LDS for a whole chunk of documents.
// mvc_table_kernel One workgroup per (64 query rows, 64 centroids): the 64 x 64 tile of S on the store's MFMA with k
//                  ascending (the operand staging of maxsim.hip), written as keys in the walk's layout [group][nc][R].
// mvc_walk_kernel  One workgroup (sixteen waves) per (group, chunk of documents), the group the fast grid index.  The
//                  group's table is copied to LDS once.  R / 8 neighbouring lanes own one document at a time; lane p of
//                  them owns query rows 8 p .. 8 p + 7 of the group, that is one 128-bit LDS read per code (the lanes of a
//                  document read one contiguous table row), and keeps their eight running maxima in four registers from the
//                  document's first code to its last: nothing is carried through memory, whatever the document's length.
//                  The codes come straight from HBM, 16 aligned bytes (eight codes) per lane and load, the next piece
//                  requested before the current one is walked; sixteen waves per CU hide the rest of the latency.  (A
//                  coalesced LDS stage of T codes holds T / Ld documents, so with a document per lane group most groups
//                  would wait for their tile; the register look-ahead keeps all of them busy.)  When a document ends its
//                  lanes write the maxima, still as keys, to part[doc][row of the call]: 16 bytes per lane.
// mvc_select_kernel One workgroup per (query, chunk): a thread adds a document's maxima of the query's rows in ascending
//                  row order from +0 -- one chain per query, counted from the query's own first row, so that the sum does
//                  not depend on where the packing put the query -- divides once by Lq, drops documents without rows and
//                  excluded ones and keeps the chunk's best ncand (dense_key, select_chunk).  mvc_merge_kernel is
//                  merge_lists over the chunks.
// mvc_rescore_kernel  ms_pair_kernel's arithmetic, one workgroup per (query, candidate, 64-row run of the query), with
//                  the query rows read from the query store and the document rows from the index's store through doc_ptr:
//                  no gather.  It writes the run's sum; mvc_order_kernel (one workgroup per query) adds the runs in
//                  ascending order, divides by Lq, sorts the candidates by (score descending, doc ascending) and writes
//                  ranks lo .. hi - 1.  Every bit is snx_maxsim_pairs'.
// part holds a bounded group of chunks; the host walks the groups on the stream.  Nothing of size nq x nd exists, and
// there is no float atomic anywhere.
// The residual-compressed store and its scorer (mvr_* kernels, "multi-vector residual store") follow the rescore below,
// and behind them the centroid inverted lists and the walk over a query's probed documents (mvp_* kernels, "multi-vector
// probed candidates").
#include <vector>

#include "dense_common.h"
#include "snx.h"

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(2))) short s16x2;

constexpr int MVC_THREADS = 256;               // table and rescore: four waves, one 32 x 32 accumulator each
constexpr int MVC_TILE = 64;
constexpr int MVC_DMAX = 1024;
constexpr int MVC_NC_MAX = 4096;
constexpr int MVC_WALK_THREADS = 1024;
constexpr int MVC_TABLE_BYTES = 128 * 1024;    // a group's table at the largest nc of each R
constexpr int MVC_CHUNK_MIN = 64, MVC_CHUNK_DEFAULT = 1024, MVC_CHUNK_MAX = 8192;   // docs per chunk (keys in LDS: 32 KB)
constexpr int MVC_WG_TARGET = 4096;            // workgroups per walk launch that the chunk group aims at
constexpr size_t MVC_PART_BUDGET = (size_t)128 << 20;   // bytes of maxima per launch, beyond one chunk's
constexpr uint32_t MVC_NO_ROW = 0x807Fu;       // the key of -inf
constexpr uint32_t MVC_NO_ROW2 = MVC_NO_ROW | (MVC_NO_ROW << 16);

__host__ __device__ inline int mvc_group_rows(int nc) { return nc <= 1024 ? 64 : (nc <= 2048 ? 32 : 16); }

// fp32 -> the order key of its bf16 (round to nearest even; -0 becomes +0 first), and back: the map is an involution
__device__ __forceinline__ uint32_t mvc_key(float s) {
  const uint32_t b = bf16_bits(s + 0.0f);
  return (b & 0x8000u) ? (b ^ 0x7FFFu) : b;
}
__device__ __forceinline__ float mvc_unkey(uint32_t k) { return bits_to_f32((k & 0x8000u) ? (k ^ 0x7FFFu) : k); }

__device__ __forceinline__ uint32_t mvc_max2(uint32_t a, uint32_t b) {       // v_pk_max_i16
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}

// The operand staging and the MFMA steps of one precision: MsBf16 / MsF32 of maxsim.hip restated (same slices, same
// steps, so a score element is the same chain of the same two rows).  fetch: this thread's share of a 64-row K slice
// (rows t >> 3 and 32 + (t >> 3), 16 bytes each; a row past the count reads as zero); put: registers -> LDS stage; mma:
// the slice's MFMA steps in ascending k.
struct MvcBf16 {
  typedef bf16_t elem;
  static constexpr int KT = 64, PITCH = 72;
  struct Stage { uint16_t a[MVC_TILE][PITCH], b[MVC_TILE][PITCH]; };
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

struct MvcF32 {
  typedef float elem;
  static constexpr int KT = 32, PITCH = 68;
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

// One 64 x 64 tile by the whole workgroup: rows a0 .. a0 + na - 1 of A against rows b0 .. b0 + nb - 1 of B over all of D,
// both operands through the double-buffered K-slice stage, one slice ahead in registers: ms_pair_kernel's loop.  With
// wave = 2 wm + wn and lane = 32 h + c, acc[r] = <A row a0 + 32 wm + (r & 3) + 8 (r >> 2) + 4 h, B row b0 + 32 wn + c>.
// The stage must be free on entry; ends on a barrier.
template <typename P>
__device__ __forceinline__ void mvc_tile(const typename P::elem* __restrict__ A, long a0, int na,
                                         const typename P::elem* __restrict__ B, long b0, int nb, int D,
                                         typename P::Stage* stage, f32x16& acc) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const int nk = D / P::KT;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  typename P::Regs ra, rb;
  P::fetch(A, a0, na, D, 0, t, ra);
  P::fetch(B, b0, nb, D, 0, t, rb);
  P::put(t, ra, stage[0].a);
  P::put(t, rb, stage[0].b);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {                           // k ascending, the same steps for every tile
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      P::fetch(A, a0, na, D, (kt + 1) * P::KT, t, ra);
      P::fetch(B, b0, nb, D, (kt + 1) * P::KT, t, rb);
    }
    P::mma(stage[cur], wm, wn, c, h, acc);
    if (kt + 1 < nk) {
      P::put(t, ra, stage[cur ^ 1].a);
      P::put(t, rb, stage[cur ^ 1].b);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ codes
// *bad = 1 when a code of the store's rows is not a centroid id
__global__ __launch_bounds__(MVC_THREADS) void mvc_check_kernel(const uint16_t* __restrict__ codes, int64_t n, int32_t nc,
                                                                int32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * MVC_THREADS + threadIdx.x;
  if (i < n && (int32_t)codes[i] >= nc) *bad = 1;
}

// codes base .. base + 7 (base % 8 == 0, base < drows) as four registers; a code past the store reads as 0
__device__ __forceinline__ u32x4 mvc_codes8(const uint16_t* __restrict__ codes, long base, long drows) {
  if (base + 8 <= drows) return *(const u32x4*)(codes + base);
  u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int u = 0; u < 8; ++u)
    if (base + u < drows) v[u >> 1] |= (uint32_t)codes[base + u] << (16 * (u & 1));
  return v;
}

// ------------------------------------------------------------------------------------------------ table
// table[(g nc + c) R + i] = key(S[R g + i, c]); a row past the call's query rows holds the key of -inf
template <typename P>
__global__ __launch_bounds__(MVC_THREADS) void mvc_table_kernel(const typename P::elem* __restrict__ Q, int64_t qused,
                                                                int64_t prows, const typename P::elem* __restrict__ Cn,
                                                                int32_t nc, int32_t D, int32_t R,
                                                                uint16_t* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) typename P::Stage stage[2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const long q0 = (long)blockIdx.x * MVC_TILE;
  const int c0 = blockIdx.y * MVC_TILE;
  const int nq = (int)max(0l, min((long)MVC_TILE, qused - q0));
  f32x16 acc;
  mvc_tile<P>(Q, q0, nq, Cn, (long)c0, min(MVC_TILE, nc - c0), D, stage, acc);
  const int cent = c0 + wn * 32 + c;
  if (cent >= nc) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {                               // acc[4 j .. 4 j + 3]: four consecutive query rows
    const long row = q0 + wm * 32 + 8 * j + 4 * h;
    if (row >= prows) continue;                               // prows % 16 == 0: the four rows lie in one group
    uint32_t k[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) k[i] = row + i < qused ? mvc_key(acc[4 * j + i]) : MVC_NO_ROW;
    const long g = row / R;
    const int in = (int)(row - g * R);
    *(u32x2*)(table + (g * nc + cent) * R + in) = (u32x2){k[0] | (k[1] << 16), k[2] | (k[3] << 16)};
  }
}

// ------------------------------------------------------------------------------------------------ walk
template <int R>
__global__ __launch_bounds__(MVC_WALK_THREADS) void mvc_walk_kernel(
    const uint16_t* __restrict__ table, const uint16_t* __restrict__ codes, int64_t drows,
    const int64_t* __restrict__ doc_ptr, int32_t nd, int32_t nc, int32_t ngroups, int32_t chunk, int32_t c_first,
    uint16_t* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int LPD = R / 8;                                  // lanes per document: one 16-byte piece of a table row each
  constexpr int DPW = MVC_WALK_THREADS / LPD;                 // documents the workgroup walks at a time
  const int t = threadIdx.x;
  const int g = (int)(blockIdx.x % (unsigned)ngroups), cg = (int)(blockIdx.x / (unsigned)ngroups);
  const long g0 = (long)c_first * chunk;                      // first doc of the launch's chunk group: part's row 0
  const long c0 = min((long)nd, g0 + (long)cg * chunk), c1 = min((long)nd, c0 + chunk);
  u32x4* T = (u32x4*)smem;
  {                                                           // the group's table, once for the whole chunk
    const u32x4* src = (const u32x4*)(table + (long)g * nc * R);
    const int nvec = nc * LPD;
    for (int i = t; i < nvec; i += MVC_WALK_THREADS) T[i] = src[i];
  }
  __syncthreads();
  const int p = t % LPD, slot = t / LPD;
  const long prows = (long)ngroups * R;
  for (long d = c0 + slot; d < c1; d += DPW) {
    const long a = doc_ptr[d], e = doc_ptr[d + 1];
    u32x4 m = {MVC_NO_ROW2, MVC_NO_ROW2, MVC_NO_ROW2, MVC_NO_ROW2};
    if (e > a) {
      long base = a & ~7l;
      u32x4 cur = mvc_codes8(codes, base, drows);
      for (; base < e; base += 8) {
        u32x4 nxt = {0u, 0u, 0u, 0u};
        if (base + 8 < e) nxt = mvc_codes8(codes, base + 8, drows);          // in flight while this piece is walked
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const long pos = base + u;
          if (pos >= a && pos < e) {
            const int code = min((int)((cur[u >> 1] >> (16 * (u & 1))) & 0xFFFFu), nc - 1);
            const u32x4 x = T[code * LPD + p];
#pragma unroll
            for (int w = 0; w < 4; ++w) m[w] = mvc_max2(m[w], x[w]);
          }
        }
        cur = nxt;
      }
    }
    *(u32x4*)(part + (d - g0) * prows + (long)g * R + p * 8) = m;
  }
}

// ------------------------------------------------------------------------------------------------ selection
__global__ __launch_bounds__(SR_THREADS) void mvc_select_kernel(
    const uint16_t* __restrict__ part, const int64_t* __restrict__ q_ptr, const int64_t* __restrict__ doc_ptr, int32_t nd,
    int64_t prows, int32_t chunk, int32_t c_first, int32_t nch, const int64_t* __restrict__ ex_ptr,
    const int32_t* __restrict__ ex_doc, int32_t ncand, unsigned long long* __restrict__ cand, int32_t* __restrict__ ccount) {
  __shared__ SelectSmem S;
  __shared__ uint32_t keys[MVC_CHUNK_MAX];
  const int tid = threadIdx.x, q = blockIdx.x, cg = blockIdx.y;
  const long c0 = ((long)c_first + cg) * chunk;
  const int n = (int)max(0l, min((long)chunk, (long)nd - c0));
  const long qa = q_ptr[q], qe = q_ptr[q + 1];
  const float lq = (float)(qe - qa);
  const int64_t e0 = ex_ptr ? ex_ptr[q] : 0, e1 = ex_ptr ? ex_ptr[q + 1] : 0;
  for (int i = tid; i < n; i += SR_THREADS) {
    const long d = c0 + i;
    uint32_t key = 0u;                                        // a document without rows, or an excluded one: no entry
    bool ok = doc_ptr[d + 1] > doc_ptr[d];
    if (ok && e1 > e0) {
      const int64_t p = lower_bound(ex_doc, e0, e1, (int32_t)d);
      ok = !(p < e1 && ex_doc[p] == (int32_t)d);
    }
    if (ok) {
      const uint16_t* v = part + ((long)cg * chunk + i) * prows;             // prows % 16 == 0: 16-byte pieces
      float x = 0.f;
      for (long base = qa & ~7l; base < qe; base += 8) {      // the query's rows, ascending: one chain from +0
        const u32x4 w = *(const u32x4*)(v + base);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (base + u >= qa && base + u < qe) x += mvc_unkey((w[u >> 1] >> (16 * (u & 1))) & 0xFFFFu);
      }
      key = dense_key(x / lq);
    }
    keys[i] = key;
  }
  __syncthreads();
  const size_t list = (size_t)q * (size_t)nch + (size_t)(c_first + cg);
  select_chunk([&](long i) -> uint32_t { return keys[i]; }, (int)c0, n, ncand, S, cand + list * (size_t)ncand,
               ccount + list);
}

__global__ __launch_bounds__(SR_THREADS) void mvc_merge_kernel(const unsigned long long* __restrict__ cand,
                                                               const int32_t* __restrict__ ccount, int32_t nch,
                                                               int32_t ncand, int32_t* __restrict__ cand_doc,
                                                               float* __restrict__ cand_score) {
  __shared__ SelectSmem S;
  const int q = blockIdx.x;
  const long base = (long)q * nch;
  const RankLists lists = {cand + (size_t)base * (size_t)ncand, ccount + base, ncand, ncand};
  merge_lists<dense_unkey>(lists, nch, S, q, 0, ncand, cand_doc, cand_score, nullptr);
}

// ------------------------------------------------------------------------------------------------ rescore
// partial[pair qblocks + qb] = the sum, in ascending row order from +0, of the row maxima of the query's run qb against
// candidate `pair`'s rows; a slot of cand_doc that names no document with rows, and a run past the query, write nothing
template <typename P>
__global__ __launch_bounds__(MVC_THREADS) void mvc_rescore_kernel(
    const typename P::elem* __restrict__ E, const typename P::elem* __restrict__ Q, int32_t D,
    const int64_t* __restrict__ doc_ptr, int32_t nd, const int64_t* __restrict__ q_ptr,
    const int32_t* __restrict__ cand_doc, int32_t ncand, int32_t qblocks, float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) typename P::Stage stage[2];
  __shared__ float rmax[2][MVC_TILE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const long pair = blockIdx.x;
  const int qb = blockIdx.y, q = (int)(pair / ncand);
  const int32_t d = cand_doc[pair];
  if ((uint32_t)d >= (uint32_t)nd) return;
  const long d0 = doc_ptr[d], Ld = doc_ptr[d + 1] - d0;
  const long q0 = q_ptr[q] + (long)qb * MVC_TILE;
  const int nq = (int)min((long)MVC_TILE, q_ptr[q + 1] - q0);  // query rows of this run
  if (Ld <= 0 || nq <= 0) return;
  float m[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) m[r] = -INFINITY;
  for (long n0 = 0; n0 < Ld; n0 += MVC_TILE) {
    const int nv = (int)min((long)MVC_TILE, Ld - n0);          // doc rows of this tile
    f32x16 acc;
    mvc_tile<P>(Q, q0, nq, E, d0 + n0, nv, D, stage, acc);
    const bool ok = wn * 32 + c < nv;
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
    partial[pair * qblocks + qb] = s;
  }
}

__global__ __launch_bounds__(SR_THREADS) void mvc_order_kernel(
    const float* __restrict__ partial, const int32_t* __restrict__ cand_doc, const int64_t* __restrict__ q_ptr,
    const int64_t* __restrict__ doc_ptr, int32_t nd, int32_t ncand, int32_t qblocks, int32_t lo, int32_t hi,
    int32_t* __restrict__ out_doc, float* __restrict__ out_score, int32_t* __restrict__ out_found) {
  __shared__ unsigned long long sbuf[SR_KMAX];               // rank keys: descending = the ABI's order
  __shared__ int total;
  const int tid = threadIdx.x, q = blockIdx.x;
  const int Lq = (int)(q_ptr[q + 1] - q_ptr[q]);
  const int nb = (Lq + MVC_TILE - 1) / MVC_TILE;
  const int P = pow2_at_least(ncand);
  int local = 0;
  for (int j = tid; j < P; j += SR_THREADS) {
    unsigned long long key = 0ull;
    const int32_t d = j < ncand ? cand_doc[(long)q * ncand + j] : -1;
    if ((uint32_t)d < (uint32_t)nd && doc_ptr[d + 1] > doc_ptr[d]) {
      const float* v = partial + ((long)q * ncand + j) * qblocks;
      float s = v[0];
      for (int b = 1; b < nb; ++b) s += v[b];                 // ascending runs
      key = rank_key(dense_key(s / (float)Lq), (uint32_t)d);
      ++local;
    }
    sbuf[j] = key;
  }
  const int nsel = min(block_sum(local, total), hi);          // found counts the ranks below hi, as the exact search's
  bitonic_desc<SR_THREADS, int>(sbuf, P);
  write_ranks<dense_unkey>(sbuf, nsel, q, lo, hi, out_doc, out_score, out_found);
}

// ------------------------------------------------------------------------------------------------ host
// ptr [n + 1] ascends from 0 and ends within `rows`; need_rows: every sequence has at least one
inline bool mvc_ptr_ok(const int64_t* ptr, int32_t n, int64_t rows, bool need_rows) {
  if (!ptr || ptr[0] != 0) return false;
  for (int32_t s = 0; s < n; ++s)
    if (ptr[s + 1] < ptr[s] + (need_rows ? 1 : 0)) return false;
  return ptr[n] <= rows;
}

inline int mvc_upload(char* ws, size_t off, const void* src, size_t bytes, hipStream_t st) {
  const hipError_t e = hipMemcpyAsync(ws + off, src, bytes, hipMemcpyHostToDevice, st);
  return e == hipSuccess ? SNX_OK : (int)e;
}

inline bool mvc_bad_cand(int32_t nq, int32_t nd, int32_t nc, int32_t ncand, int32_t chunk_docs) {
  return nq < 0 || nd < 0 || nc < 1 || nc > MVC_NC_MAX || ncand < 1 || ncand > SR_KMAX ||
         (chunk_docs != 0 && (chunk_docs < MVC_CHUNK_MIN || chunk_docs > MVC_CHUNK_MAX));
}

// the candidate pass's workspace: device copies of the pointers, the check's flag, the table, the maxima of one chunk
// group, the candidate lists
struct MvcPlan {
  size_t dptr, qptr, flag, table, part, cand, ccount, total;
  int chunk, nch, group, ngroups, R;
  int64_t prows;
  bool ok;
  MvcPlan(const int64_t* q_ptr, int32_t nq, int32_t nd, int32_t nc, int32_t ncand, int32_t chunk_docs) {
    chunk = chunk_docs > 0 ? chunk_docs : MVC_CHUNK_DEFAULT;
    nch = sr_nch(nd, chunk);
    R = mvc_group_rows(nc);
    const int64_t qused = q_ptr[nq];
    ok = qused <= 0x7FFFFFFFL - MVC_TILE && (int64_t)nq * nch <= 0x7FFFFFFFL;
    ngroups = ok ? (int)((qused + R - 1) / R) : 1;
    prows = (int64_t)ngroups * R;
    const size_t per_chunk = (size_t)chunk * (size_t)prows * 2;
    long g = (MVC_WG_TARGET + (long)ngroups - 1) / ngroups;
    if ((size_t)g * per_chunk > MVC_PART_BUDGET) g = (long)(MVC_PART_BUDGET / (per_chunk ? per_chunk : 1));
    group = (int)(g < 1 ? 1 : (g > nch ? nch : (g > 65535 ? 65535 : g)));
    ok = ok && (long)ngroups * group <= 0x7FFFFFFFL;
    Arena a;
    dptr = a.take(((size_t)nd + 1) * 8);
    qptr = a.take(((size_t)nq + 1) * 8);
    flag = a.take(4);
    table = a.take((size_t)prows * (size_t)nc * 2);
    part = a.take((size_t)group * per_chunk);
    cand = a.take((size_t)nq * (size_t)nch * (size_t)ncand * 8);
    ccount = a.take((size_t)nq * (size_t)nch * 4);
    total = a.off;
  }
};

LdsOptIn g_mvc_lds[3];

template <int R>
int mvc_walk(int which, dim3 grid, hipStream_t st, const uint16_t* table, const uint16_t* codes, int64_t drows,
             const int64_t* dptr, int32_t nd, int32_t nc, int ngroups, int chunk, int c, uint16_t* part) {
  if (const int rc = g_mvc_lds[which].ensure((const void*)mvc_walk_kernel<R>, MVC_TABLE_BYTES)) return rc;
  hipLaunchKernelGGL(mvc_walk_kernel<R>, grid, dim3(MVC_WALK_THREADS), (size_t)nc * R * 2, st, table, codes, drows, dptr, nd,
                     nc, ngroups, chunk, c, part);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

// the rescore's workspace: device copies of the pointers and one partial sum per (query, candidate, run)
struct MvcRescorePlan {
  size_t dptr, qptr, partial, total;
  int qblocks;
  bool ok;
  MvcRescorePlan(const int64_t* q_ptr, int32_t nq, int32_t nd, int32_t ncand) {
    int64_t longest = 1;
    for (int32_t q = 0; q < nq; ++q) longest = q_ptr[q + 1] - q_ptr[q] > longest ? q_ptr[q + 1] - q_ptr[q] : longest;
    const int64_t qb = (longest + MVC_TILE - 1) / MVC_TILE;
    ok = qb <= 65535 && (int64_t)nq * ncand <= 0x7FFFFFFFL;
    qblocks = ok ? (int)qb : 1;
    Arena a;
    dptr = a.take(((size_t)nd + 1) * 8);
    qptr = a.take(((size_t)nq + 1) * 8);
    partial = a.take((size_t)nq * (size_t)ncand * (size_t)qblocks * 4);
    total = a.off;
  }
};

// ------------------------------------------------------------------------------------------------ residual store
// include/snx.h "multi-vector residual store": a bf16 row is kept as its centroid code plus nbits bits per dimension that
// name a bucket of row - centroid, and a candidate is scored from that form.  The product splits,
//   <q_i, centroid[code_j] + w_j> -> fl32(S32[i, code_j] + R(i, j)),
// S32 the fp32 table of query row x centroid products and R the MFMA chain of the query row against the row of bf16
// bucket weights, so that a document row costs D nbits / 8 bytes of bits and 256 bytes of table, never 2 D.
// mvr_encode_kernel  One thread per 32-bit word of the packed store: 32 / nbits dimensions of a row, the residual by one
//                    fp32 subtraction, the bucket by counting cutoffs below it.  Dimension k of a row sits at bit k nbits
//                    of the row's D nbits / 8 bytes, little-endian.
// mvr_table_kernel   mvc_table_kernel's tile, written as fp32: one block [nc][64] per (query, 64-row run), so that a block
//                    does not depend on where the call's packing put the query.  A bounded group of blocks exists at a
//                    time (MVR_TABLE_BUDGET); the host walks the groups on the stream.
// mvr_score_kernel   mvc_rescore_kernel's grid and MFMA loop.  The query run goes through MvcBf16's K-slice stage as
//                    there.  The document operand never exists in memory: thread t owns row t >> 2 of the 64-row tile and
//                    dimensions 16 (t & 3) .. + 15 of every 64-wide K slice, which with the order above is ONE aligned
//                    word of 16 nbits bits (2, 4 or 8 bytes), loaded one slice ahead with the row clamped into the
//                    document -- no branch around a load.  Eight lookups in an LDS table of 2^(2 nbits) weight PAIRS
//                    (two bf16 per entry, at most 1 KB) turn the word into the 32 bytes the thread writes into the stage
//                    in MvcBf16's layout.  The lane's code and its four 16-byte table pieces (accumulator rows
//                    (r & 3) + 8 (r >> 2) + 4 h: four runs of four consecutive query rows) are requested before the K loop
//                    and added after it; columns past the document's end become -inf; maxima and sums as
//                    mvc_rescore_kernel.  mvc_order_kernel ranks; mvr_raw_kernel writes the scores in candidate order.
constexpr size_t MVR_TABLE_BUDGET = (size_t)128 << 20;     // bytes of fp32 table blocks per launch group

__device__ __forceinline__ float mvr_bf16_f32(uint16_t b) { return bits_to_f32((uint32_t)b); }

template <int NB>
__global__ __launch_bounds__(MVC_THREADS) void mvr_encode_kernel(
    const uint16_t* __restrict__ rows, const uint16_t* __restrict__ codes, int64_t n, const uint16_t* __restrict__ Cn,
    int32_t nc, int32_t D, const float* __restrict__ cutoffs, uint32_t* __restrict__ out) {
  constexpr int DPW = 32 / NB, NCUT = (1 << NB) - 1;         // dimensions per word: 32, 16 or 8 (a multiple of 8)
  const int wpr = D / DPW;
  const int64_t idx = (int64_t)blockIdx.x * MVC_THREADS + threadIdx.x;
  if (idx >= n * wpr) return;
  const int64_t row = idx / wpr;
  const int k0 = (int)(idx - row * wpr) * DPW;
  const int code = min((int)codes[row], nc - 1);
  float cut[NCUT];
#pragma unroll
  for (int m = 0; m < NCUT; ++m) cut[m] = cutoffs[m];
  uint32_t word = 0u;
#pragma unroll
  for (int v = 0; v < DPW / 8; ++v) {
    const u32x4 x = *(const u32x4*)(rows + row * D + k0 + 8 * v);
    const u32x4 c = *(const u32x4*)(Cn + (long)code * D + k0 + 8 * v);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const uint32_t sh = 16 * (u & 1);
      const float r = mvr_bf16_f32((uint16_t)(x[u >> 1] >> sh)) - mvr_bf16_f32((uint16_t)(c[u >> 1] >> sh));
      uint32_t bucket = 0u;
#pragma unroll
      for (int m = 0; m < NCUT; ++m) bucket += cut[m] < r ? 1u : 0u;
      word |= bucket << (NB * (8 * v + u));
    }
  }
  out[idx] = word;
}

// the query whose runs hold block `blk`: blk_ptr [nq + 1] ascends from 0, blk_ptr[q + 1] - blk_ptr[q] >= 1
__device__ __forceinline__ int mvr_query_of(const int64_t* __restrict__ blk_ptr, int32_t nq, int64_t blk) {
  int lo = 0, hi = nq;                                       // the last q with blk_ptr[q] <= blk
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (blk_ptr[mid] <= blk) lo = mid; else hi = mid;
  }
  return lo;
}

// table[((blk - b0) nc + c) 64 + i] = S32[row i of the run, c]; a row past the query's end holds the product of a zero row
__global__ __launch_bounds__(MVC_THREADS) void mvr_table_kernel(
    const bf16_t* __restrict__ Q, const int64_t* __restrict__ q_ptr, const int64_t* __restrict__ blk_ptr, int32_t nq,
    int64_t b0, const bf16_t* __restrict__ Cn, int32_t nc, int32_t D, float* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) MvcBf16::Stage stage[2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const int64_t blk = b0 + blockIdx.x;
  const int q = mvr_query_of(blk_ptr, nq, blk);
  const long q0 = q_ptr[q] + (blk - blk_ptr[q]) * MVC_TILE;
  const int nr = (int)max(0l, min((long)MVC_TILE, q_ptr[q + 1] - q0));
  const int c0 = blockIdx.y * MVC_TILE;
  f32x16 acc;
  mvc_tile<MvcBf16>(Q, q0, nr, Cn, (long)c0, min(MVC_TILE, nc - c0), D, stage, acc);
  const int cent = c0 + wn * 32 + c;
  if (cent >= nc) return;
  float* dst = table + ((long)blockIdx.x * nc + cent) * MVC_TILE + wm * 32 + 4 * h;
#pragma unroll
  for (int j = 0; j < 4; ++j) *(f32x4*)(dst + 8 * j) = (f32x4){acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]};
}

template <int NB> struct MvrWord;
template <> struct MvrWord<1> { typedef uint16_t type; };
template <> struct MvrWord<2> { typedef uint32_t type; };
template <> struct MvrWord<4> { typedef unsigned long long type; };

// a thread's word of a K slice -> its 16 bf16 weights in the stage: row t >> 2, columns 16 (t & 3) .. + 15
template <int NB>
__device__ __forceinline__ void mvr_expand(typename MvrWord<NB>::type w, const uint32_t* lut, int t,
                                           uint16_t (*S)[MvcBf16::PITCH]) {
  uint32_t o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = lut[(uint32_t)(w >> (2 * NB * i)) & ((1u << (2 * NB)) - 1u)];
  // All eight lookups land before the first store.  hipcc would overlap the first store with the last four lookups under
  // counted waits that are right only because LDS stores hold slots of the same counter; the build's scan of LDS reads
  // (snx/asmcheck.py) counts reads alone, and the overlap is worth nothing next to the MFMA loop.
  __builtin_amdgcn_s_waitcnt(0xC07F);                         // lgkmcnt(0)
  u32x4* dst = (u32x4*)&S[t >> 2][(t & 3) * 16];
  dst[0] = (u32x4){o[0], o[1], o[2], o[3]};
  dst[1] = (u32x4){o[4], o[5], o[6], o[7]};
}

// partial[pair qblocks + qb] as mvc_rescore_kernel's, from the packed store; the launch covers queries q_first .. and the
// table blocks b0 .. b1 - 1, a run outside them is another launch's
template <int NB>
__global__ __launch_bounds__(MVC_THREADS) void mvr_score_kernel(
    const uint16_t* __restrict__ codes, const unsigned char* __restrict__ bits, const uint16_t* __restrict__ weights,
    const float* __restrict__ table, int32_t nc, const bf16_t* __restrict__ Q, int32_t D,
    const int64_t* __restrict__ doc_ptr, int32_t nd, const int64_t* __restrict__ q_ptr,
    const int64_t* __restrict__ blk_ptr, int64_t b0, int64_t b1, int32_t q_first, const int32_t* __restrict__ cand_doc,
    int32_t ncand, int32_t qblocks, float* __restrict__ partial) {
  typedef typename MvrWord<NB>::type W;
  typedef MvcBf16 P;
  __shared__ __attribute__((aligned(16))) P::Stage stage[2];
  __shared__ float rmax[2][MVC_TILE];
  __shared__ uint32_t lut[1 << (2 * NB)];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const long pair = (long)q_first * ncand + blockIdx.x;
  const int qb = blockIdx.y, q = (int)(pair / ncand);
  const int32_t d = cand_doc[pair];
  if ((uint32_t)d >= (uint32_t)nd) return;
  const long d0 = doc_ptr[d], Ld = doc_ptr[d + 1] - d0;
  const long q0 = q_ptr[q] + (long)qb * MVC_TILE;
  const int nq = (int)min((long)MVC_TILE, q_ptr[q + 1] - q0);  // query rows of this run
  if (Ld <= 0 || nq <= 0) return;
  const int64_t blk = blk_ptr[q] + qb;
  if (blk < b0 || blk >= b1) return;
  if (t < (1 << (2 * NB)))                                    // entry e: the weights of buckets e & mask (low half) and e >> NB
    lut[t] = (uint32_t)weights[t & ((1 << NB) - 1)] | ((uint32_t)weights[t >> NB] << 16);
  __syncthreads();
  const float* tab = table + (blk - b0) * (long)nc * MVC_TILE + wm * 32 + 4 * h;
  const int nk = D / P::KT, wpr = D / 16;                     // words of a row
  float m[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) m[r] = -INFINITY;
  for (long n0 = 0; n0 < Ld; n0 += MVC_TILE) {
    const int nv = (int)min((long)MVC_TILE, Ld - n0);          // doc rows of this tile
    const W* wsrc = (const W*)bits + (d0 + n0 + min(t >> 2, nv - 1)) * wpr + (t & 3);
    const int code = min((int)codes[d0 + n0 + min(wn * 32 + c, nv - 1)], nc - 1);
    f32x4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = *(const f32x4*)(tab + (long)code * MVC_TILE + 8 * j);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    P::Regs ra;
    P::fetch(Q, q0, nq, D, 0, t, ra);
    W w = wsrc[0];
    P::put(t, ra, stage[0].a);
    mvr_expand<NB>(w, lut, t, stage[0].b);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {                         // mvc_tile's loop: k ascending
      const int cur = kt & 1;
      if (kt + 1 < nk) {
        P::fetch(Q, q0, nq, D, (kt + 1) * P::KT, t, ra);
        w = wsrc[4 * (kt + 1)];
      }
      P::mma(stage[cur], wm, wn, c, h, acc);
      if (kt + 1 < nk) {
        P::put(t, ra, stage[cur ^ 1].a);
        mvr_expand<NB>(w, lut, t, stage[cur ^ 1].b);
      }
      __syncthreads();
    }
    const bool ok = wn * 32 + c < nv;
#pragma unroll
    for (int r = 0; r < 16; ++r) m[r] = fmaxf(m[r], ok ? s[r >> 2][r & 3] + acc[r] : -INFINITY);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) m[r] = fmaxf(m[r], __shfl_xor(m[r], o, 64));
    if (c == 0) rmax[wn][wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = m[r];
  }
  __syncthreads();
  if (t == 0) {
    float sum = 0.f;
    for (int i = 0; i < nq; ++i) sum += fmaxf(rmax[0][i], rmax[1][i]);      // ascending rows
    partial[pair * qblocks + qb] = sum;
  }
}

// raw[q ncand + j] = the score mvc_order_kernel ranks for candidate slot j, 0 for a slot it skips
__global__ __launch_bounds__(MVC_THREADS) void mvr_raw_kernel(
    const float* __restrict__ partial, const int32_t* __restrict__ cand_doc, const int64_t* __restrict__ q_ptr,
    const int64_t* __restrict__ doc_ptr, int32_t nd, int64_t npairs, int32_t ncand, int32_t qblocks,
    float* __restrict__ raw) {
  const int64_t i = (int64_t)blockIdx.x * MVC_THREADS + threadIdx.x;
  if (i >= npairs) return;
  const int q = (int)(i / ncand);
  const int32_t d = cand_doc[i];
  float out = 0.f;
  if ((uint32_t)d < (uint32_t)nd && doc_ptr[d + 1] > doc_ptr[d]) {
    const int Lq = (int)(q_ptr[q + 1] - q_ptr[q]);
    const int nb = (Lq + MVC_TILE - 1) / MVC_TILE;
    const float* v = partial + i * qblocks;
    float s = v[0];
    for (int b = 1; b < nb; ++b) s += v[b];                   // ascending runs
    out = s / (float)Lq;
  }
  raw[i] = out;
}

inline bool mvr_bad_nbits(int32_t nbits) { return nbits != 1 && nbits != 2 && nbits != 4; }

// the residual rescore's workspace: MvcRescorePlan's arrays, the first table block of every query, one group of blocks
struct MvrPlan {
  size_t dptr, qptr, bptr, partial, table, total;
  int qblocks;
  int64_t nblocks, group;
  bool ok;
  MvrPlan(const int64_t* q_ptr, int32_t nq, int32_t nd, int32_t nc, int32_t ncand) {
    const MvcRescorePlan base(q_ptr, nq, nd, ncand);
    ok = base.ok;
    qblocks = base.qblocks;
    nblocks = 0;
    for (int32_t q = 0; q < nq; ++q) nblocks += (q_ptr[q + 1] - q_ptr[q] + MVC_TILE - 1) / MVC_TILE;
    const size_t block = (size_t)nc * MVC_TILE * 4;
    const int64_t cap = (int64_t)(MVR_TABLE_BUDGET / block);  // >= 128 blocks at nc = 4096
    group = nblocks < cap ? nblocks : cap;
    Arena a;
    dptr = a.take(((size_t)nd + 1) * 8);
    qptr = a.take(((size_t)nq + 1) * 8);
    bptr = a.take(((size_t)nq + 1) * 8);
    partial = a.take((size_t)nq * (size_t)ncand * (size_t)qblocks * 4);
    table = a.take((size_t)group * block);
    total = a.off;
  }
};

template <int NB>
int mvr_launch_score(dim3 grid, hipStream_t st, const uint16_t* codes, const void* bits, const uint16_t* weights,
                     const float* table, int32_t nc, const bf16_t* q, int32_t D, const int64_t* dptr, int32_t nd,
                     const int64_t* qptr, const int64_t* bptr, int64_t b0, int64_t b1, int32_t q_first,
                     const int32_t* cand_doc, int32_t ncand, int32_t qblocks, float* partial) {
  hipLaunchKernelGGL(mvr_score_kernel<NB>, grid, dim3(MVC_THREADS), 0, st, codes, (const unsigned char*)bits, weights, table,
                     nc, q, D, dptr, nd, qptr, bptr, b0, b1, q_first, cand_doc, ncand, qblocks, partial);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

// ------------------------------------------------------------------------------------------------ probed candidates
// include/snx.h "multi-vector probed candidates": centroid inverted lists in front of the walk (ColBERTv2 / PLAID).  A
// query row looks only at the documents that own a row in one of its nprobe best centroids; a(q, d) of those documents is
// the value above, so the pass costs an unprobed document one bit of a bitmap, not Ld LDS gathers.
// mvp_list_*        The lists.  mvp_list_doc_kernel: one wave per document sets the bits of its codes in an LDS bitmap of
//                   nc bits and, per distinct code, counts (first pass) or takes a place (second pass) in the segment of
//                   (centroid, chunk of 4,096 documents).  mvp_list_scan_kernel turns the counts into segment starts in
//                   (centroid, chunk) order; mvp_list_sort_kernel orders every segment in LDS.  The integer atomics decide
//                   only the place inside a segment, which the sort then fixes: the lists are a function of the codes.
// mvp_probe_kernel  One workgroup per table group, the group's [nc][R] table copied to LDS in 16-byte pieces; a wave per
//                   query row keeps 64 packed (key, ~centroid) values per lane and takes nprobe wave maxima.
// mvp_mark_kernel   One workgroup per (query row, probe slot) walks L[c] and sets the document's bit in the query's row of
//                   the bitmap (atomicOr: idempotent); mvp_unmark_kernel clears the bits of exclude[q].
// mvp_count_kernel  One workgroup per query: pre[q][s] = the set bits in front of the 1,024-id word range s, and the
//                   largest |P(q)| of the launch, which the host reads to size the walk.
// mvp_walk_kernel   One workgroup per (query, table group the query overlaps, block of up to 1,024 PROBED documents).  It
//                   finds its block through pre, scans the block's words into an ascending list of doc ids in LDS, copies
//                   the 8-row pieces of the group's table that hold the query's rows ([nc][pieces]) and walks the list
//                   with `pieces` lanes per document: mvc_walk_kernel's look-ahead of eight codes and packed maxima.  The
//                   maxima go to part[slot][the query's own pieces].
// mvp_select_kernel mvc_select_kernel's fold over a block's slots, radix_select + ordered_take with the slot's doc id.
// Blocks of a query follow each other in doc order, so mvc_merge_kernel (merge_lists) finishes the query.
constexpr int MVP_NPROBE_MAX = 64;
constexpr int MVP_THREADS = 256;
constexpr int MVP_PROBE_THREADS = 512;         // eight waves: a lane keeps 64 keys in registers
constexpr int MVP_SEG_WORDS = 32;              // bitmap words per prefix entry: 1,024 doc ids
constexpr int MVP_BLOCK_MAX = 1024;            // probed documents of a walk workgroup
constexpr int MVP_LIST_CHUNK = 4096;           // documents per segment of a list while it is built (ids in LDS: 16 KB)
constexpr size_t MVP_BITS_BUDGET = (size_t)128 << 20;   // bytes of bitmap per slice of queries
constexpr size_t MVP_PART_BUDGET = (size_t)128 << 20;   // bytes of maxima per walk launch

// the distinct codes of document 4 blockIdx.x + wave as bits; FILL: list_docs[cur[code, chunk]++] = doc, else ++cur[..]
template <bool FILL>
__global__ __launch_bounds__(MVP_THREADS) void mvp_list_doc_kernel(const uint16_t* __restrict__ codes,
                                                                   const int64_t* __restrict__ doc_ptr, int32_t nd, int32_t nc,
                                                                   int32_t nchunks, unsigned long long* __restrict__ cur,
                                                                   int32_t* __restrict__ list_docs) {
  __shared__ uint32_t bm[MVP_THREADS / 64][MVC_NC_MAX / 32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long d = (long)blockIdx.x * (MVP_THREADS / 64) + wave;
  for (int w = lane; w < MVC_NC_MAX / 32; w += 64) bm[wave][w] = 0u;
  __syncthreads();
  if (d < nd) {
    const long e = doc_ptr[d + 1];
    for (long j = doc_ptr[d] + lane; j < e; j += 64) {
      const int c = min((int)codes[j], nc - 1);
      atomicOr(&bm[wave][c >> 5], 1u << (c & 31));
    }
  }
  __syncthreads();
  if (d >= nd) return;
  const long chunk = d / MVP_LIST_CHUNK;
  for (int w = lane; w < MVC_NC_MAX / 32; w += 64) {
    uint32_t x = bm[wave][w];
    while (x) {
      const int c = w * 32 + __ffs((int)x) - 1;
      x &= x - 1u;
      const unsigned long long at = atomicAdd(cur + (long)c * nchunks + chunk, 1ull);
      if (FILL) list_docs[at] = (int32_t)d;
    }
  }
}

// seg[i] (counts, flat over (centroid, chunk)) -> the sum of the counts in front of i, also into cur; list_ptr [nc + 1]
__global__ __launch_bounds__(MVC_WALK_THREADS) void mvp_list_scan_kernel(unsigned long long* __restrict__ seg,
                                                                         unsigned long long* __restrict__ cur, int64_t n,
                                                                         int32_t nc, int32_t nchunks,
                                                                         int64_t* __restrict__ list_ptr) {
  __shared__ unsigned long long wsum[MVC_WALK_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long per = (n + MVC_WALK_THREADS - 1) / MVC_WALK_THREADS;
  const long i0 = min((long)n, t * per), i1 = min((long)n, i0 + per);
  unsigned long long run = 0ull;
  for (long i = i0; i < i1; ++i) run += seg[i];
  unsigned long long incl = run;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  unsigned long long off = 0ull, all = 0ull;
#pragma unroll
  for (int w = 0; w < MVC_WALK_THREADS / 64; ++w) {
    const unsigned long long x = wsum[w];
    off += w < wave ? x : 0ull;
    all += x;
  }
  if (t == 0) list_ptr[nc] = (int64_t)all;
  run = off + incl - run;
  for (long i = i0; i < i1; ++i) {
    const unsigned long long x = seg[i];
    seg[i] = run;
    cur[i] = run;
    if (i % nchunks == 0) list_ptr[i / nchunks] = (int64_t)run;
    run += x;
  }
}

// segment blockIdx.x of list_docs (at most MVP_LIST_CHUNK ids, all different) into ascending order
__global__ __launch_bounds__(MVP_THREADS) void mvp_list_sort_kernel(const unsigned long long* __restrict__ seg, int64_t n,
                                                                    const int64_t* __restrict__ list_ptr, int32_t nc,
                                                                    int32_t* __restrict__ list_docs) {
  __shared__ uint32_t s[MVP_LIST_CHUNK];
  const int t = threadIdx.x;
  const long i = blockIdx.x;
  const long a = (long)seg[i], e = i + 1 < n ? (long)seg[i + 1] : (long)list_ptr[nc];
  const int m = (int)min((long)MVP_LIST_CHUNK, e - a);
  if (m < 2) return;
  const int P = pow2_at_least(m);
  for (int j = t; j < P; j += MVP_THREADS) s[j] = j < m ? (uint32_t)list_docs[a + j] : 0xFFFFFFFFu;
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int k = t; k < (P >> 1); k += MVP_THREADS) {
        const int lo = 2 * k - (k & (stride - 1)), hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const uint32_t x = s[lo], y = s[hi];
        if ((x > y) == asc) { s[lo] = y; s[hi] = x; }
      }
      __syncthreads();
    }
  for (int j = t; j < m; j += MVP_THREADS) list_docs[a + j] = (int32_t)s[j];
}

// probe[row np + r] = the r-th best centroid of query row `row` by (key descending, centroid ascending), r < np <= nc
__global__ __launch_bounds__(MVP_PROBE_THREADS) void mvp_probe_kernel(const uint16_t* __restrict__ table, int64_t qused,
                                                                     int32_t nc, int32_t R, int32_t np,
                                                                     int32_t* __restrict__ probe) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long g = blockIdx.x;
  {
    u32x4* T = (u32x4*)smem;
    const u32x4* src = (const u32x4*)(table + g * nc * R);
    const int nvec = nc * (R / 8);
    for (int i = t; i < nvec; i += MVP_PROBE_THREADS) T[i] = src[i];
  }
  __syncthreads();
  const uint16_t* T16 = (const uint16_t*)smem;
  for (int in = wave; in < R; in += MVP_PROBE_THREADS / 64) {
    const long row = g * R + in;
    if (row >= qused) break;
    uint32_t v[64];                                           // (key as unsigned) << 16 | ~centroid; 0: no centroid
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      const int c = 64 * k + lane;
      v[k] = c < nc ? ((((uint32_t)T16[c * R + in] ^ 0x8000u) << 16) | (0xFFFFu - (uint32_t)c)) : 0u;
    }
    for (int r = 0; r < np; ++r) {
      uint32_t best = 0u;
#pragma unroll
      for (int k = 0; k < 64; ++k) best = max(best, v[k]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o, 64));
      if (lane == 0) probe[row * np + r] = (int32_t)(0xFFFFu - (best & 0xFFFFu));
#pragma unroll
      for (int k = 0; k < 64; ++k) v[k] = v[k] == best ? 0u : v[k];
    }
  }
}

// the bit of every document of L[probe[row, slot]] in the bitmap row of the query that owns `row`
__global__ __launch_bounds__(MVP_THREADS) void mvp_mark_kernel(const int32_t* __restrict__ probe, int32_t np,
                                                               const int64_t* __restrict__ q_ptr, int32_t q0, int32_t nqs,
                                                               const int64_t* __restrict__ list_ptr,
                                                               const int32_t* __restrict__ list_docs, int32_t nd, int64_t wp,
                                                               uint32_t* __restrict__ bits) {
  const long row = q_ptr[q0] + blockIdx.x;
  int lo = q0, hi = q0 + nqs;                                 // the last query with q_ptr[q] <= row
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (q_ptr[mid] <= row) lo = mid; else hi = mid;
  }
  const int c = probe[row * np + blockIdx.y];
  uint32_t* b = bits + (long)(lo - q0) * wp;
  const long e = list_ptr[c + 1];
  for (long i = list_ptr[c] + threadIdx.x; i < e; i += MVP_THREADS) {
    const int32_t d = list_docs[i];
    if ((uint32_t)d >= (uint32_t)nd) continue;
    const uint32_t m = 1u << (d & 31);
    // most rows of a query probe the same lists: look before the atomic (a stale look only repeats an idempotent or)
    if (!(__hip_atomic_load(b + (d >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m)) atomicOr(b + (d >> 5), m);
  }
}

__global__ __launch_bounds__(MVP_THREADS) void mvp_unmark_kernel(const int64_t* __restrict__ ex_ptr,
                                                                 const int32_t* __restrict__ ex_doc, int32_t nd, int64_t wp,
                                                                 uint32_t* __restrict__ bits) {
  const long q = blockIdx.x;
  const int64_t e = ex_ptr[q + 1];
  for (int64_t i = ex_ptr[q] + threadIdx.x; i < e; i += MVP_THREADS) {
    const int32_t d = ex_doc[i];
    if ((uint32_t)d < (uint32_t)nd) atomicAnd(bits + q * wp + (d >> 5), ~(1u << (d & 31)));
  }
}

// the sum of c over the threads in front of this one, by a workgroup of MVC_WALK_THREADS; tot = the sum over all of them
__device__ __forceinline__ int mvp_block_scan(int c, int* wsum, int& tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(incl, o, 64);
    if (lane >= o) incl += y;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int off = 0;
  tot = 0;
#pragma unroll
  for (int w = 0; w < MVC_WALK_THREADS / 64; ++w) {
    const int x = wsum[w];
    off += w < wave ? x : 0;
    tot += x;
  }
  __syncthreads();
  return off + incl - c;
}

// pre[q (nseg + 1) + s] = the set bits of query q's bitmap row in front of word MVP_SEG_WORDS s; [nseg]: all of them
__global__ __launch_bounds__(MVC_WALK_THREADS) void mvp_count_kernel(const uint32_t* __restrict__ bits, int64_t wp,
                                                                     int32_t nseg, int32_t* __restrict__ pre,
                                                                     int32_t* __restrict__ maxtot) {
  __shared__ int wsum[MVC_WALK_THREADS / 64];
  const int t = threadIdx.x;
  const u32x4* src = (const u32x4*)(bits + (long)blockIdx.x * wp);
  int32_t* out = pre + (long)blockIdx.x * (nseg + 1);
  int base = 0;
  for (int s0 = 0; s0 < nseg; s0 += MVC_WALK_THREADS) {
    const int s = s0 + t;
    int c = 0;
    if (s < nseg) {
#pragma unroll
      for (int u = 0; u < MVP_SEG_WORDS / 4; ++u) {
        const u32x4 x = src[(long)s * (MVP_SEG_WORDS / 4) + u];
        c += __popc(x[0]) + __popc(x[1]) + __popc(x[2]) + __popc(x[3]);
      }
    }
    int tot;
    const int off = mvp_block_scan(c, wsum, tot);
    if (s < nseg) out[s] = base + off;
    base += tot;
  }
  if (t == 0) {
    out[nseg] = base;
    atomicMax(maxtot, base);
  }
}

// part[((q bg + bl) blk + i) pitch + 8 (piece - q's first piece) ..] = the maxima of the i-th probed document of block
// b_first + bl of query q0 + q against the eight query rows of the piece; slotdoc[.. + i] = the document
__global__ __launch_bounds__(MVC_WALK_THREADS) void mvp_walk_kernel(
    const uint16_t* __restrict__ table, const uint16_t* __restrict__ codes, int64_t drows,
    const int64_t* __restrict__ doc_ptr, int32_t nc, int32_t R, const int64_t* __restrict__ q_ptr, int32_t q0,
    const uint32_t* __restrict__ bits, int64_t wp, const int32_t* __restrict__ pre, int32_t nseg, int32_t blk,
    int32_t b_first, int32_t bg, int32_t pitch, uint16_t* __restrict__ part, int32_t* __restrict__ slotdoc) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int32_t doclist[MVP_BLOCK_MAX];
  __shared__ int wsum[MVC_WALK_THREADS / 64];
  const int t = threadIdx.x;
  const int bl = blockIdx.x, q = blockIdx.z;
  const long qa = q_ptr[q0 + q], qe = q_ptr[q0 + q + 1];
  const long g = qa / R + blockIdx.y;
  if (g * R >= qe) return;                                    // the query does not reach this group
  const int32_t* pq = pre + (long)q * (nseg + 1);
  const long first = ((long)b_first + bl) * blk;
  if (first >= pq[nseg]) return;                              // no probed document left for this block
  const int n = (int)min((long)blk, pq[nseg] - first);
  int s0 = 0;                                                 // the last word range with pre <= first
  for (int hi = nseg; hi - s0 > 1;) {
    const int mid = s0 + ((hi - s0) >> 1);
    if (pq[mid] <= first) s0 = mid; else hi = mid;
  }
  const uint32_t* b = bits + (long)q * wp;
  long base = pq[s0];
  for (long w0 = (long)s0 * MVP_SEG_WORDS; w0 < wp && base < first + n; w0 += MVC_WALK_THREADS) {
    const long w = w0 + t;
    uint32_t x = w < wp ? b[w] : 0u;
    int tot;
    long ord = base + mvp_block_scan(__popc(x), wsum, tot);
    while (x) {
      const int bit = __ffs((int)x) - 1;
      x &= x - 1u;
      if (ord >= first && ord < first + n) doclist[ord - first] = (int32_t)(w * 32 + bit);
      ++ord;
    }
    base += tot;
  }
  // the 8-row pieces of the group that hold rows of the query: local pieces pl0 .. pl0 + np - 1
  const int LPD = R / 8;
  const long gp = g * LPD, qp = qa >> 3;
  const int pl0 = (int)max(0l, qp - gp), np = (int)min((long)LPD - 1, ((qe - 1) >> 3) - gp) - pl0 + 1;
  u32x4* T = (u32x4*)smem;
  {
    const u32x4* src = (const u32x4*)(table + g * nc * R) + pl0;
    const int nvec = nc * np;
    for (int i = t; i < nvec; i += MVC_WALK_THREADS) {
      const int c = i / np;
      T[i] = src[c * LPD + (i - c * np)];
    }
  }
  __syncthreads();
  const int slot = t / np, p = t - slot * np, DPW = MVC_WALK_THREADS / np;
  if (slot >= DPW) return;
  const long out0 = ((long)q * bg + bl) * blk;
  for (int i = slot; i < n; i += DPW) {
    const int32_t d = doclist[i];
    const long a = doc_ptr[d], e = doc_ptr[d + 1];
    u32x4 m = {MVC_NO_ROW2, MVC_NO_ROW2, MVC_NO_ROW2, MVC_NO_ROW2};
    if (e > a) {
      long cb = a & ~7l;
      u32x4 cur = mvc_codes8(codes, cb, drows);
      for (; cb < e; cb += 8) {
        u32x4 nxt = {0u, 0u, 0u, 0u};
        if (cb + 8 < e) nxt = mvc_codes8(codes, cb + 8, drows);              // in flight while this piece is walked
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const long pos = cb + u;
          if (pos >= a && pos < e) {
            const int code = min((int)((cur[u >> 1] >> (16 * (u & 1))) & 0xFFFFu), nc - 1);
            const u32x4 x = T[code * np + p];
#pragma unroll
            for (int w = 0; w < 4; ++w) m[w] = mvc_max2(m[w], x[w]);
          }
        }
        cur = nxt;
      }
    }
    *(u32x4*)(part + (out0 + i) * pitch + (gp + pl0 + p - qp) * 8) = m;
    if (blockIdx.y == 0 && p == 0) slotdoc[out0 + i] = d;
  }
}

__global__ __launch_bounds__(SR_THREADS) void mvp_select_kernel(
    const uint16_t* __restrict__ part, const int32_t* __restrict__ slotdoc, const int64_t* __restrict__ q_ptr, int32_t q0,
    const int32_t* __restrict__ pre, int32_t nseg, int32_t blk, int32_t b_first, int32_t bg, int32_t pitch, int32_t nlist,
    int32_t ncand, unsigned long long* __restrict__ cand, int32_t* __restrict__ ccount) {
  __shared__ SelectSmem S;
  __shared__ uint32_t keys[MVP_BLOCK_MAX];
  const int tid = threadIdx.x, q = blockIdx.x, bl = blockIdx.y;
  const long b = (long)b_first + bl;
  if (b >= nlist) return;
  const int n = (int)max(0l, min((long)blk, (long)pre[(long)q * (nseg + 1) + nseg] - b * blk));
  const long qa = q_ptr[q0 + q], qe = q_ptr[q0 + q + 1], q8 = qa & ~7l;
  const float lq = (float)(qe - qa);
  const long out0 = ((long)q * bg + bl) * blk;
  for (int i = tid; i < n; i += SR_THREADS) {
    const uint16_t* v = part + (out0 + i) * pitch;
    float x = 0.f;
    for (long base = q8; base < qe; base += 8) {              // the query's rows, ascending: one chain from +0
      const u32x4 w = *(const u32x4*)(v + (base - q8));
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (base + u >= qa && base + u < qe) x += mvc_unkey((w[u >> 1] >> (16 * (u & 1))) & 0xFFFFu);
    }
    keys[i] = dense_key(x / lq);
  }
  __syncthreads();
  const size_t list = (size_t)q * (size_t)nlist + (size_t)b;
  unsigned long long* out = cand + list * (size_t)ncand;
  const int32_t* sd = slotdoc + out0;
  auto key = [&](long i) -> uint32_t { return keys[i]; };
  uint32_t thr;
  int need_eq, nsel;
  radix_select(key, n, ncand, S, thr, need_eq, nsel);          // select_chunk's body with the slot's document as the id
  ordered_take(key, n, thr, need_eq, S, [&](long i, int pos) { out[pos] = rank_key(keys[i], (uint32_t)sd[i]); });
  if (tid == 0) ccount[list] = nsel;
}

struct MvpListPlan {
  size_t dptr, seg, cur, total;
  int nchunks;
  int64_t n;
  bool ok;
  MvpListPlan(int32_t nd, int32_t nc) {
    nchunks = sr_nch(nd, MVP_LIST_CHUNK);
    n = (int64_t)nc * nchunks;
    ok = n <= 0x7FFFFFFFL;
    Arena a;
    dptr = a.take(((size_t)nd + 1) * 8);
    seg = a.take((size_t)n * 8);
    cur = a.take((size_t)n * 8);
    total = a.off;
  }
};

inline bool mvp_bad_probe(int32_t nprobe) { return nprobe < 1 || nprobe > MVP_NPROBE_MAX; }

// the probed pass's workspace.  A slice of qs queries holds a bitmap row, a prefix row and candidate lists each; a walk
// launch covers bg blocks of every query of the slice.
struct MvpPlan {
  size_t dptr, qptr, lptr, flag, table, probe, bits, pre, part, slotdoc, cand, ccount, total;
  int R, ngroups, np, blk, nseg, nblk, maxg, maxnp, pitch, qs, bg;
  int64_t prows, wp;
  bool ok;
  MvpPlan(const int64_t* q_ptr, int32_t nq, int32_t nd, int32_t nc, int32_t ncand, int32_t chunk_docs, int32_t nprobe) {
    R = mvc_group_rows(nc);
    const int64_t qused = q_ptr[nq];
    ok = qused <= 0x7FFFFFFFL - MVC_TILE && nq <= 65535;
    ngroups = ok ? (int)((qused + R - 1) / R) : 1;
    prows = (int64_t)ngroups * R;
    np = nprobe < nc ? nprobe : nc;
    blk = chunk_docs > 0 && chunk_docs < MVP_BLOCK_MAX ? chunk_docs : MVP_BLOCK_MAX;
    nseg = sr_nch(nd, MVP_SEG_WORDS * 32);
    wp = (int64_t)nseg * MVP_SEG_WORDS;
    nblk = sr_nch(nd, blk);
    maxg = maxnp = pitch = 1;
    const int LPD = R / 8;
    for (int32_t q = 0; ok && q < nq; ++q) {                  // groups and 8-row pieces a query reaches
      const int64_t a = q_ptr[q], e = q_ptr[q + 1] - 1;
      const int g = (int)(e / R - a / R + 1), pieces = (int)((e >> 3) - (a >> 3) + 1);
      maxg = g > maxg ? g : maxg;
      pitch = pieces > pitch ? pieces : pitch;
      const int in = pieces < LPD ? pieces : LPD;             // at most a group's pieces, at most the query's
      maxnp = in > maxnp ? in : maxnp;
    }
    pitch *= 8;
    const size_t block = (size_t)blk * pitch * 2;
    size_t s = MVP_BITS_BUDGET / ((size_t)wp * 4), s2 = MVP_PART_BUDGET / block;
    s = s < s2 ? s : s2;
    qs = (int)(s < 1 ? 1 : (s > (size_t)nq ? (size_t)nq : s));
    size_t g = MVP_PART_BUDGET / ((size_t)qs * block);
    bg = (int)(g < 1 ? 1 : (g > (size_t)nblk ? (size_t)nblk : g));
    bg = bg > 65535 ? 65535 : bg;
    ok = ok && (int64_t)qs * nblk <= 0x7FFFFFFFL && maxg <= 65535;
    Arena a;
    dptr = a.take(((size_t)nd + 1) * 8);
    qptr = a.take(((size_t)nq + 1) * 8);
    lptr = a.take(((size_t)nc + 1) * 8);
    flag = a.take(8);
    table = a.take((size_t)prows * (size_t)nc * 2);
    probe = a.take((size_t)prows * (size_t)np * 4);
    bits = a.take((size_t)qs * (size_t)wp * 4);
    pre = a.take((size_t)qs * ((size_t)nseg + 1) * 4);
    part = a.take((size_t)qs * (size_t)bg * block);
    slotdoc = a.take((size_t)qs * (size_t)bg * (size_t)blk * 4);
    cand = a.take((size_t)qs * (size_t)nblk * (size_t)ncand * 8);
    ccount = a.take((size_t)qs * (size_t)nblk * 4);
    total = a.off;
  }
};

LdsOptIn g_mvp_lds[2];

}  // namespace

extern "C" size_t snx_mv_candidates_workspace_bytes(const int64_t* q_ptr, int32_t nq, int32_t nd, int32_t nc, int32_t ncand,
                                                    int32_t chunk_docs) {
  if (nq <= 0 || mvc_bad_cand(nq, nd, nc, ncand, chunk_docs) || !mvc_ptr_ok(q_ptr, nq, 0x7FFFFFFFFFFFFFFFL, true)) return 0;
  const MvcPlan plan(q_ptr, nq, nd, nc, ncand, chunk_docs);
  return plan.ok ? plan.total : 0;
}

extern "C" int snx_mv_candidates(const uint16_t* codes, int64_t drows, const int64_t* doc_ptr, int32_t nd,
                                 const void* centroids, int32_t nc, const void* q, int32_t mv_f32, int32_t D, int64_t qrows,
                                 const int64_t* q_ptr, int32_t nq, const int64_t* ex_ptr, const int32_t* ex_doc,
                                 int32_t ncand, int32_t chunk_docs, int32_t* cand_doc, float* cand_score, void* workspace,
                                 size_t ws_bytes, hipStream_t st) {
  if (D <= 0 || (D % 64) != 0 || D > MVC_DMAX || qrows < 0 || drows < 0) return SNX_E_SHAPE;
  if (mvc_bad_cand(nq, nd, nc, ncand, chunk_docs)) return SNX_E_ARG;
  if (nq == 0) return SNX_OK;
  if (!q || !centroids || !cand_doc || !cand_score || !workspace || (ex_ptr && !ex_doc) || ((uintptr_t)q & 15) != 0 ||
      ((uintptr_t)centroids & 15) != 0 || ((uintptr_t)codes & 15) != 0 || ((uintptr_t)workspace & 15) != 0)
    return SNX_E_ARG;
  // the two pointer arrays are pageable host memory (snx.h): everything a kernel will trust is checked here, before any
  // launch; hipMemcpyAsync below has staged them when it returns
  if (!mvc_ptr_ok(doc_ptr, nd, drows, false) || !mvc_ptr_ok(q_ptr, nq, qrows, true)) return SNX_E_ARG;
  const int64_t dused = doc_ptr[nd], qused = q_ptr[nq];
  if (dused > 0 && !codes) return SNX_E_ARG;
  const MvcPlan plan(q_ptr, nq, nd, nc, ncand, chunk_docs);
  if (!plan.ok) return SNX_E_SHAPE;
  if (ws_bytes < plan.total) return SNX_E_ARG;
  char* ws = (char*)workspace;
  if (dused > 0) {                                            // the codes are a device array: a kernel looks, the host waits
    int32_t* flag = (int32_t*)(ws + plan.flag);
    int32_t bad = 0;
    hipError_t e = hipMemsetAsync(flag, 0, 4, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mvc_check_kernel, dim3((unsigned)((dused + MVC_THREADS - 1) / MVC_THREADS)), dim3(MVC_THREADS), 0, st,
                       codes, dused, nc, flag);
    SNX_CHECK_LAUNCH();
    e = hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    if (bad) return SNX_E_ARG;
  }
  RC(mvc_upload(ws, plan.dptr, doc_ptr, ((size_t)nd + 1) * 8, st));
  RC(mvc_upload(ws, plan.qptr, q_ptr, ((size_t)nq + 1) * 8, st));
  const int64_t* dptr = (const int64_t*)(ws + plan.dptr);
  const int64_t* qptr = (const int64_t*)(ws + plan.qptr);
  uint16_t *table = (uint16_t*)(ws + plan.table), *part = (uint16_t*)(ws + plan.part);
  unsigned long long* cand = (unsigned long long*)(ws + plan.cand);
  int32_t* ccount = (int32_t*)(ws + plan.ccount);
  const int R = plan.R;
  if (dused > 0) {
    const dim3 grid((unsigned)((plan.prows + MVC_TILE - 1) / MVC_TILE), (unsigned)((nc + MVC_TILE - 1) / MVC_TILE));
    if (mv_f32)
      hipLaunchKernelGGL(mvc_table_kernel<MvcF32>, grid, dim3(MVC_THREADS), 0, st, (const float*)q, qused, plan.prows,
                         (const float*)centroids, nc, D, R, table);
    else
      hipLaunchKernelGGL(mvc_table_kernel<MvcBf16>, grid, dim3(MVC_THREADS), 0, st, (const bf16_t*)q, qused, plan.prows,
                         (const bf16_t*)centroids, nc, D, R, table);
    SNX_CHECK_LAUNCH();
  }
  for (int c = 0; c < plan.nch; c += plan.group) {            // one chunk group after the other: part is reused in order
    const int g = plan.nch - c < plan.group ? plan.nch - c : plan.group;
    if (dused > 0) {
      const dim3 grid((unsigned)((long)plan.ngroups * g));    // group fast, chunk slow
      if (R == 64) RC(mvc_walk<64>(0, grid, st, table, codes, drows, dptr, nd, nc, plan.ngroups, plan.chunk, c, part));
      else if (R == 32) RC(mvc_walk<32>(1, grid, st, table, codes, drows, dptr, nd, nc, plan.ngroups, plan.chunk, c, part));
      else RC(mvc_walk<16>(2, grid, st, table, codes, drows, dptr, nd, nc, plan.ngroups, plan.chunk, c, part));
    }
    hipLaunchKernelGGL(mvc_select_kernel, dim3(nq, g), dim3(SR_THREADS), 0, st, (const uint16_t*)part, qptr, dptr, nd,
                       plan.prows, plan.chunk, c, plan.nch, ex_ptr, ex_doc, ncand, cand, ccount);
    SNX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(mvc_merge_kernel, dim3(nq), dim3(SR_THREADS), 0, st, (const unsigned long long*)cand,
                     (const int32_t*)ccount, plan.nch, ncand, cand_doc, cand_score);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" size_t snx_mv_rescore_workspace_bytes(const int64_t* q_ptr, int32_t nq, int32_t nd, int32_t ncand) {
  if (nq <= 0 || nd < 0 || ncand < 1 || ncand > SR_KMAX || !mvc_ptr_ok(q_ptr, nq, 0x7FFFFFFFFFFFFFFFL, true)) return 0;
  const MvcRescorePlan plan(q_ptr, nq, nd, ncand);
  return plan.ok ? plan.total : 0;
}

extern "C" int snx_mv_rescore(const void* docs, const void* q, int32_t mv_f32, int32_t D, int64_t drows,
                              const int64_t* doc_ptr, int32_t nd, int64_t qrows, const int64_t* q_ptr, int32_t nq,
                              const int32_t* cand_doc, int32_t ncand, int32_t lo, int32_t hi, int32_t* out_doc,
                              float* out_score, int32_t* out_found, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (D <= 0 || (D % 64) != 0 || D > MVC_DMAX || qrows < 0 || drows < 0 || nq < 0 || nd < 0) return SNX_E_SHAPE;
  if (ncand < 1 || ncand > SR_KMAX || lo < 0 || hi <= lo || hi > ncand) return SNX_E_ARG;
  if (nq == 0) return SNX_OK;
  if (!q || !cand_doc || !out_doc || !out_score || !out_found || !workspace || ((uintptr_t)q & 15) != 0 ||
      ((uintptr_t)docs & 15) != 0 || ((uintptr_t)workspace & 15) != 0)
    return SNX_E_ARG;
  if (!mvc_ptr_ok(doc_ptr, nd, drows, false) || !mvc_ptr_ok(q_ptr, nq, qrows, true)) return SNX_E_ARG;
  if (doc_ptr[nd] > 0 && !docs) return SNX_E_ARG;
  const MvcRescorePlan plan(q_ptr, nq, nd, ncand);
  if (!plan.ok) return SNX_E_SHAPE;
  if (ws_bytes < plan.total) return SNX_E_ARG;
  char* ws = (char*)workspace;
  RC(mvc_upload(ws, plan.dptr, doc_ptr, ((size_t)nd + 1) * 8, st));
  RC(mvc_upload(ws, plan.qptr, q_ptr, ((size_t)nq + 1) * 8, st));
  const int64_t* dptr = (const int64_t*)(ws + plan.dptr);
  const int64_t* qptr = (const int64_t*)(ws + plan.qptr);
  float* partial = (float*)(ws + plan.partial);
  const dim3 grid((unsigned)((long)nq * ncand), (unsigned)plan.qblocks);
  if (mv_f32)
    hipLaunchKernelGGL(mvc_rescore_kernel<MvcF32>, grid, dim3(MVC_THREADS), 0, st, (const float*)docs, (const float*)q, D,
                       dptr, nd, qptr, cand_doc, ncand, plan.qblocks, partial);
  else
    hipLaunchKernelGGL(mvc_rescore_kernel<MvcBf16>, grid, dim3(MVC_THREADS), 0, st, (const bf16_t*)docs, (const bf16_t*)q, D,
                       dptr, nd, qptr, cand_doc, ncand, plan.qblocks, partial);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(mvc_order_kernel, dim3(nq), dim3(SR_THREADS), 0, st, (const float*)partial, cand_doc, qptr, dptr, nd,
                     ncand, plan.qblocks, lo, hi, out_doc, out_score, out_found);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

// ------------------------------------------------------------------------------------------------ residual store: host
extern "C" int snx_mv_residual_encode(const void* rows, int64_t n, const uint16_t* codes, const void* centroids, int32_t nc,
                                      int32_t D, int32_t nbits, const float* cutoffs, void* bits, hipStream_t st) {
  if (D <= 0 || (D % 64) != 0 || D > MVC_DMAX || n < 0 || n > 0x7FFFFFFFFFFFFFFFL / D) return SNX_E_SHAPE;
  if (mvr_bad_nbits(nbits) || nc < 1 || nc > MVC_NC_MAX) return SNX_E_ARG;
  if (n == 0) return SNX_OK;
  if (!rows || !codes || !centroids || !cutoffs || !bits || ((uintptr_t)rows & 15) != 0 || ((uintptr_t)centroids & 15) != 0 ||
      ((uintptr_t)bits & 15) != 0)
    return SNX_E_ARG;
  const int64_t words = n * (D * nbits / 32), blocks = (words + MVC_THREADS - 1) / MVC_THREADS;
  if (blocks > 0x7FFFFFFFL) return SNX_E_SHAPE;
  const dim3 grid((unsigned)blocks);
  const uint16_t *r = (const uint16_t*)rows, *c = (const uint16_t*)centroids;
  if (nbits == 1)
    hipLaunchKernelGGL(mvr_encode_kernel<1>, grid, dim3(MVC_THREADS), 0, st, r, codes, n, c, nc, D, cutoffs, (uint32_t*)bits);
  else if (nbits == 2)
    hipLaunchKernelGGL(mvr_encode_kernel<2>, grid, dim3(MVC_THREADS), 0, st, r, codes, n, c, nc, D, cutoffs, (uint32_t*)bits);
  else
    hipLaunchKernelGGL(mvr_encode_kernel<4>, grid, dim3(MVC_THREADS), 0, st, r, codes, n, c, nc, D, cutoffs, (uint32_t*)bits);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" size_t snx_mv_rescore_residual_workspace_bytes(const int64_t* q_ptr, int32_t nq, int32_t nd, int32_t nc,
                                                          int32_t ncand) {
  if (nq <= 0 || nd < 0 || nc < 1 || nc > MVC_NC_MAX || ncand < 1 || ncand > SR_KMAX ||
      !mvc_ptr_ok(q_ptr, nq, 0x7FFFFFFFFFFFFFFFL, true))
    return 0;
  const MvrPlan plan(q_ptr, nq, nd, nc, ncand);
  return plan.ok ? plan.total : 0;
}

extern "C" int snx_mv_rescore_residual(const uint16_t* codes, const void* bits, const void* centroids, const uint16_t* weights,
                                       int32_t nc, int32_t nbits, const void* q, int32_t mv_f32, int32_t D, int64_t drows,
                                       const int64_t* doc_ptr, int32_t nd, int64_t qrows, const int64_t* q_ptr, int32_t nq,
                                       const int32_t* cand_doc, int32_t ncand, int32_t lo, int32_t hi, int32_t* out_doc,
                                       float* out_score, int32_t* out_found, float* raw_score, void* workspace,
                                       size_t ws_bytes, hipStream_t st) {
  if (D <= 0 || (D % 64) != 0 || D > MVC_DMAX || qrows < 0 || drows < 0 || nq < 0 || nd < 0) return SNX_E_SHAPE;
  if (mv_f32 || mvr_bad_nbits(nbits) || nc < 1 || nc > MVC_NC_MAX || ncand < 1 || ncand > SR_KMAX || lo < 0 || hi <= lo ||
      hi > ncand)
    return SNX_E_ARG;
  if (nq == 0) return SNX_OK;
  if (!q || !centroids || !weights || !cand_doc || !out_doc || !out_score || !out_found || !workspace ||
      ((uintptr_t)q & 15) != 0 || ((uintptr_t)centroids & 15) != 0 || ((uintptr_t)bits & 15) != 0 ||
      ((uintptr_t)workspace & 15) != 0)
    return SNX_E_ARG;
  if (!mvc_ptr_ok(doc_ptr, nd, drows, false) || !mvc_ptr_ok(q_ptr, nq, qrows, true)) return SNX_E_ARG;
  if (doc_ptr[nd] > 0 && (!codes || !bits)) return SNX_E_ARG;
  const MvrPlan plan(q_ptr, nq, nd, nc, ncand);
  if (!plan.ok) return SNX_E_SHAPE;
  if (ws_bytes < plan.total) return SNX_E_ARG;
  char* ws = (char*)workspace;
  std::vector<int64_t> blk((size_t)nq + 1, 0);                // the first table block of every query
  for (int32_t i = 0; i < nq; ++i) blk[i + 1] = blk[i] + (q_ptr[i + 1] - q_ptr[i] + MVC_TILE - 1) / MVC_TILE;
  RC(mvc_upload(ws, plan.dptr, doc_ptr, ((size_t)nd + 1) * 8, st));
  RC(mvc_upload(ws, plan.qptr, q_ptr, ((size_t)nq + 1) * 8, st));
  RC(mvc_upload(ws, plan.bptr, blk.data(), ((size_t)nq + 1) * 8, st));   // pageable: staged when the call returns
  const int64_t* dptr = (const int64_t*)(ws + plan.dptr);
  const int64_t* qptr = (const int64_t*)(ws + plan.qptr);
  const int64_t* bptr = (const int64_t*)(ws + plan.bptr);
  float *partial = (float*)(ws + plan.partial), *table = (float*)(ws + plan.table);
  const bf16_t* Q = (const bf16_t*)q;
  int32_t qa = 0;                                             // the query that holds block b0
  for (int64_t b0 = 0; b0 < plan.nblocks; b0 += plan.group) {  // one group of table blocks after the other, in order
    const int64_t b1 = b0 + plan.group < plan.nblocks ? b0 + plan.group : plan.nblocks;
    while (blk[qa + 1] <= b0) ++qa;
    int32_t qe = qa;                                          // the query that holds block b1 - 1
    while (blk[qe + 1] < b1) ++qe;
    hipLaunchKernelGGL(mvr_table_kernel, dim3((unsigned)(b1 - b0), (unsigned)((nc + MVC_TILE - 1) / MVC_TILE)),
                       dim3(MVC_THREADS), 0, st, Q, qptr, bptr, nq, b0, (const bf16_t*)centroids, nc, D, table);
    SNX_CHECK_LAUNCH();
    const dim3 grid((unsigned)((long)(qe - qa + 1) * ncand), (unsigned)plan.qblocks);
    if (nbits == 1)
      RC(mvr_launch_score<1>(grid, st, codes, bits, weights, table, nc, Q, D, dptr, nd, qptr, bptr, b0, b1, qa, cand_doc,
                             ncand, plan.qblocks, partial));
    else if (nbits == 2)
      RC(mvr_launch_score<2>(grid, st, codes, bits, weights, table, nc, Q, D, dptr, nd, qptr, bptr, b0, b1, qa, cand_doc,
                             ncand, plan.qblocks, partial));
    else
      RC(mvr_launch_score<4>(grid, st, codes, bits, weights, table, nc, Q, D, dptr, nd, qptr, bptr, b0, b1, qa, cand_doc,
                             ncand, plan.qblocks, partial));
  }
  hipLaunchKernelGGL(mvc_order_kernel, dim3(nq), dim3(SR_THREADS), 0, st, (const float*)partial, cand_doc, qptr, dptr, nd,
                     ncand, plan.qblocks, lo, hi, out_doc, out_score, out_found);
  SNX_CHECK_LAUNCH();
  if (raw_score) {
    const int64_t npairs = (int64_t)nq * ncand;
    hipLaunchKernelGGL(mvr_raw_kernel, dim3((unsigned)((npairs + MVC_THREADS - 1) / MVC_THREADS)), dim3(MVC_THREADS), 0, st,
                       (const float*)partial, cand_doc, qptr, dptr, nd, npairs, ncand, plan.qblocks, raw_score);
    SNX_CHECK_LAUNCH();
  }
  return SNX_OK;
}

// ------------------------------------------------------------------------------------------------ probed candidates: host
extern "C" size_t snx_mv_lists_workspace_bytes(int32_t nd, int32_t nc) {
  if (nd < 0 || nc < 1 || nc > MVC_NC_MAX) return 0;
  const MvpListPlan plan(nd, nc);
  return plan.ok ? plan.total : 0;
}

extern "C" int snx_mv_lists_build(const uint16_t* codes, int64_t drows, const int64_t* doc_ptr, int32_t nd, int32_t nc,
                                  int64_t* list_ptr, int32_t* list_docs, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (drows < 0 || nd < 0) return SNX_E_SHAPE;
  if (nc < 1 || nc > MVC_NC_MAX || !list_ptr || !workspace || ((uintptr_t)workspace & 15) != 0) return SNX_E_ARG;
  if (!mvc_ptr_ok(doc_ptr, nd, drows, false)) return SNX_E_ARG;
  const int64_t dused = doc_ptr[nd];
  if (dused > 0 && (!codes || !list_docs)) return SNX_E_ARG;
  const MvpListPlan plan(nd, nc);
  if (!plan.ok) return SNX_E_SHAPE;
  if (ws_bytes < plan.total) return SNX_E_ARG;
  char* ws = (char*)workspace;
  RC(mvc_upload(ws, plan.dptr, doc_ptr, ((size_t)nd + 1) * 8, st));
  const int64_t* dptr = (const int64_t*)(ws + plan.dptr);
  unsigned long long *seg = (unsigned long long*)(ws + plan.seg), *cur = (unsigned long long*)(ws + plan.cur);
  const hipError_t e = hipMemsetAsync(seg, 0, (size_t)plan.n * 8, st);
  if (e != hipSuccess) return (int)e;
  const dim3 docs((unsigned)((nd + (long)MVP_THREADS / 64 - 1) / (MVP_THREADS / 64)));
  if (dused > 0) {
    hipLaunchKernelGGL(mvp_list_doc_kernel<false>, docs, dim3(MVP_THREADS), 0, st, codes, dptr, nd, nc, plan.nchunks, seg,
                       list_docs);
    SNX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(mvp_list_scan_kernel, dim3(1), dim3(MVC_WALK_THREADS), 0, st, seg, cur, plan.n, nc, plan.nchunks,
                     list_ptr);
  SNX_CHECK_LAUNCH();
  if (dused > 0) {
    hipLaunchKernelGGL(mvp_list_doc_kernel<true>, docs, dim3(MVP_THREADS), 0, st, codes, dptr, nd, nc, plan.nchunks, cur,
                       list_docs);
    SNX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mvp_list_sort_kernel, dim3((unsigned)plan.n), dim3(MVP_THREADS), 0, st,
                       (const unsigned long long*)seg, plan.n, (const int64_t*)list_ptr, nc, list_docs);
    SNX_CHECK_LAUNCH();
  }
  return SNX_OK;
}

extern "C" size_t snx_mv_candidates_probed_workspace_bytes(const int64_t* q_ptr, int32_t nq, int32_t nd, int32_t nc,
                                                           int32_t ncand, int32_t chunk_docs, int32_t nprobe) {
  if (nq <= 0 || mvc_bad_cand(nq, nd, nc, ncand, chunk_docs) || mvp_bad_probe(nprobe) ||
      !mvc_ptr_ok(q_ptr, nq, 0x7FFFFFFFFFFFFFFFL, true))
    return 0;
  const MvpPlan plan(q_ptr, nq, nd, nc, ncand, chunk_docs, nprobe);
  return plan.ok ? plan.total : 0;
}

extern "C" int snx_mv_candidates_probed(const uint16_t* codes, int64_t drows, const int64_t* doc_ptr, int32_t nd,
                                        const void* centroids, int32_t nc, const void* q, int32_t mv_f32, int32_t D,
                                        int64_t qrows, const int64_t* q_ptr, int32_t nq, const int64_t* ex_ptr,
                                        const int32_t* ex_doc, int32_t ncand, int32_t chunk_docs, const int64_t* list_ptr,
                                        const int32_t* list_docs, int64_t list_len, int32_t nprobe, int32_t* cand_doc,
                                        float* cand_score, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (D <= 0 || (D % 64) != 0 || D > MVC_DMAX || qrows < 0 || drows < 0) return SNX_E_SHAPE;
  if (mvc_bad_cand(nq, nd, nc, ncand, chunk_docs) || mvp_bad_probe(nprobe)) return SNX_E_ARG;
  if (nq == 0) return SNX_OK;
  if (!q || !centroids || !cand_doc || !cand_score || !workspace || (ex_ptr && !ex_doc) || ((uintptr_t)q & 15) != 0 ||
      ((uintptr_t)centroids & 15) != 0 || ((uintptr_t)codes & 15) != 0 || ((uintptr_t)workspace & 15) != 0)
    return SNX_E_ARG;
  if (!mvc_ptr_ok(doc_ptr, nd, drows, false) || !mvc_ptr_ok(q_ptr, nq, qrows, true)) return SNX_E_ARG;
  // the lists: a host pointer array as doc_ptr, ending at the length of list_docs; a kernel bounds every id it reads
  if (list_len < 0 || !mvc_ptr_ok(list_ptr, nc, list_len, false) || list_ptr[nc] != list_len || (list_len > 0 && !list_docs))
    return SNX_E_ARG;
  const int64_t dused = doc_ptr[nd], qused = q_ptr[nq];
  if (dused > 0 && !codes) return SNX_E_ARG;
  const MvpPlan plan(q_ptr, nq, nd, nc, ncand, chunk_docs, nprobe);
  if (!plan.ok) return SNX_E_SHAPE;
  if (ws_bytes < plan.total) return SNX_E_ARG;
  char* ws = (char*)workspace;
  int32_t* flag = (int32_t*)(ws + plan.flag);                 // [0]: a bad code, [1]: the largest |P(q)| of a slice
  if (dused > 0) {
    int32_t bad = 0;
    hipError_t e = hipMemsetAsync(flag, 0, 4, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mvc_check_kernel, dim3((unsigned)((dused + MVC_THREADS - 1) / MVC_THREADS)), dim3(MVC_THREADS), 0, st,
                       codes, dused, nc, flag);
    SNX_CHECK_LAUNCH();
    e = hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    if (bad) return SNX_E_ARG;
  }
  RC(mvc_upload(ws, plan.dptr, doc_ptr, ((size_t)nd + 1) * 8, st));
  RC(mvc_upload(ws, plan.qptr, q_ptr, ((size_t)nq + 1) * 8, st));
  RC(mvc_upload(ws, plan.lptr, list_ptr, ((size_t)nc + 1) * 8, st));
  const int64_t* dptr = (const int64_t*)(ws + plan.dptr);
  const int64_t* qptr = (const int64_t*)(ws + plan.qptr);
  const int64_t* lptr = (const int64_t*)(ws + plan.lptr);
  uint16_t *table = (uint16_t*)(ws + plan.table), *part = (uint16_t*)(ws + plan.part);
  int32_t *probe = (int32_t*)(ws + plan.probe), *pre = (int32_t*)(ws + plan.pre), *slotdoc = (int32_t*)(ws + plan.slotdoc);
  uint32_t* bits = (uint32_t*)(ws + plan.bits);
  unsigned long long* cand = (unsigned long long*)(ws + plan.cand);
  int32_t* ccount = (int32_t*)(ws + plan.ccount);
  const int R = plan.R;
  const bool live = dused > 0 && list_len > 0;                // otherwise no document can be probed
  if (live) {
    const dim3 grid((unsigned)((plan.prows + MVC_TILE - 1) / MVC_TILE), (unsigned)((nc + MVC_TILE - 1) / MVC_TILE));
    if (mv_f32)
      hipLaunchKernelGGL(mvc_table_kernel<MvcF32>, grid, dim3(MVC_THREADS), 0, st, (const float*)q, qused, plan.prows,
                         (const float*)centroids, nc, D, R, table);
    else
      hipLaunchKernelGGL(mvc_table_kernel<MvcBf16>, grid, dim3(MVC_THREADS), 0, st, (const bf16_t*)q, qused, plan.prows,
                         (const bf16_t*)centroids, nc, D, R, table);
    SNX_CHECK_LAUNCH();
    RC(g_mvp_lds[0].ensure((const void*)mvp_probe_kernel, MVC_TABLE_BYTES));
    hipLaunchKernelGGL(mvp_probe_kernel, dim3((unsigned)plan.ngroups), dim3(MVP_PROBE_THREADS), (size_t)nc * R * 2, st,
                       (const uint16_t*)table, qused, nc, R, plan.np, probe);
    SNX_CHECK_LAUNCH();
    RC(g_mvp_lds[1].ensure((const void*)mvp_walk_kernel, MVC_TABLE_BYTES));
  }
  for (int32_t q0 = 0; q0 < nq; q0 += plan.qs) {              // one slice of queries after the other: the bitmap is reused
    const int32_t nqs = nq - q0 < plan.qs ? nq - q0 : plan.qs;
    hipError_t e = hipMemsetAsync(bits, 0, (size_t)nqs * (size_t)plan.wp * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(flag + 1, 0, 4, st);
    if (e != hipSuccess) return (int)e;
    if (live) {
      hipLaunchKernelGGL(mvp_mark_kernel, dim3((unsigned)(q_ptr[q0 + nqs] - q_ptr[q0]), (unsigned)plan.np), dim3(MVP_THREADS),
                         0, st, (const int32_t*)probe, plan.np, qptr, q0, nqs, lptr, list_docs, nd, plan.wp, bits);
      SNX_CHECK_LAUNCH();
      if (ex_ptr) {
        hipLaunchKernelGGL(mvp_unmark_kernel, dim3((unsigned)nqs), dim3(MVP_THREADS), 0, st, ex_ptr + q0, ex_doc, nd, plan.wp,
                           bits);
        SNX_CHECK_LAUNCH();
      }
    }
    hipLaunchKernelGGL(mvp_count_kernel, dim3((unsigned)nqs), dim3(MVC_WALK_THREADS), 0, st, (const uint32_t*)bits, plan.wp,
                       plan.nseg, pre, flag + 1);
    SNX_CHECK_LAUNCH();
    int32_t most = 0;                                         // the walk's grid follows the probed documents, not nd
    e = hipMemcpyAsync(&most, flag + 1, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    const int nlist = most > 0 ? (int)((most + (long)plan.blk - 1) / plan.blk) : 1;
    for (int b0 = 0; b0 < nlist; b0 += plan.bg) {             // part is reused in order
      const int nb = nlist - b0 < plan.bg ? nlist - b0 : plan.bg;
      if (most > 0) {
        hipLaunchKernelGGL(mvp_walk_kernel, dim3((unsigned)nb, (unsigned)plan.maxg, (unsigned)nqs), dim3(MVC_WALK_THREADS),
                           (size_t)nc * plan.maxnp * 16, st, (const uint16_t*)table, codes, drows, dptr, nc, R, qptr, q0,
                           (const uint32_t*)bits, plan.wp, (const int32_t*)pre, plan.nseg, plan.blk, b0, plan.bg, plan.pitch,
                           part, slotdoc);
        SNX_CHECK_LAUNCH();
      }
      hipLaunchKernelGGL(mvp_select_kernel, dim3((unsigned)nqs, (unsigned)nb), dim3(SR_THREADS), 0, st, (const uint16_t*)part,
                         (const int32_t*)slotdoc, qptr, q0, (const int32_t*)pre, plan.nseg, plan.blk, b0, plan.bg, plan.pitch,
                         nlist, ncand, cand, ccount);
      SNX_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(mvc_merge_kernel, dim3((unsigned)nqs), dim3(SR_THREADS), 0, st, (const unsigned long long*)cand,
                       (const int32_t*)ccount, nlist, ncand, cand_doc + (size_t)q0 * ncand, cand_score + (size_t)q0 * ncand);
    SNX_CHECK_LAUNCH();
  }
  return SNX_OK;
}

// ------------------------------------------------------------------------------------------------ token retrieval
// include/snx.h "multi-vector token retrieval" (XTR's imputed similarity over the residual store, WARP's shape): a query
// row scores only the document rows that sit in its nprobe best centroids, a document that shows it no such row gets the
// row's next-best centroid product instead, and there is no candidate list and no second pass.  The cost follows the
// probed ROWS.  The work is joined BY CENTROID: the packed rows of a centroid are expanded once for all the query rows of
// the slice that probe it, and the score is an MFMA tile.
// mvt_table_kernel  mvc_tile over (64 query rows, 64 centroids), written as fp32 [row][nc]: S32, for a bounded group of
//                   query rows at a time.
// mvt_probe_kernel  One wave per query row: 64 packed (bf16 key, ~centroid) values per lane from the fp32 row, nprobe + 1
//                   wave maxima: top(i) and c*(i), each with its fp32 product.  The table is not needed after it.
// mvt_mark_kernel   One workgroup per (query row, probe slot) walks the centroid's ROW list and sets the bit of each
//                   row's document in the query's bitmap row (atomicOr: idempotent); mvp_unmark_kernel clears exclude[q].
// mvt_count_kernel  One workgroup per query: the set bits in front of every bitmap WORD (a document's rank inside P(q) is
//                   that plus one popcount), |P(q)|, and the largest of the slice for the host.
// mvt_join_*        count / scan / fill over rows x nprobe entries: per centroid the query rows that probe it, with their
//                   S32.  The scan also lays out the score grid: tiles(c) = ceil(entries / 64) * ceil(rows / 256).  The
//                   integer atomics decide only the place of an entry inside its centroid; every value it leads to goes
//                   through an integer max, so the place reaches no output bit.
// mvt_score_kernel  One workgroup per (centroid, 64 entries, 256 list rows), found by a binary search of the tile prefix.
//                   The A operand is GATHERED: the entries' query rows, through MvcBf16's stage, one K slice ahead.  The
//                   B operand is expanded from the packed words of the list's rows (mvr_expand, the LDS table of weight
//                   pairs), the next word in flight during the MFMA steps.  k ascending, S32 added once at the end: t(i, j)
//                   is mvr_score_kernel's value.  Rows of one document are adjacent in a list, so a segmented max over the
//                   32 columns of a wave half (five shuffle steps keyed by the column's document) leaves one value per
//                   (query row, document run) in the run's last lane, and only that lane issues the atomicMax -- on the
//                   order key of the fp32 value, into cell [query][rank of d in P(q)][row of the query].
// mvt_finish_kernel One thread per (query, document): a probed document's cells become m'(i, d) (an untouched cell: miss(i)),
//                   folded in snx_maxsim_pairs' order, divided once; key and doc go to the rank's slot.
// mvt_select_kernel One workgroup per query: radix_select / ordered_take over the slots (they are in doc order), sorted,
//                   ranks lo .. hi-1 written.
// Nothing of size nq x nd x Lq exists: the cells cover P(q) of a slice of queries under a fixed budget, and the host
// shrinks the slice when the largest P(q) asks for it.
namespace {

constexpr int MVT_THREADS = 256;
constexpr int MVT_STRETCH = 256;               // list rows of a score workgroup: four 64-row tiles
constexpr size_t MVT_TABLE_BUDGET = (size_t)128 << 20;   // bytes of fp32 table per probe launch
constexpr size_t MVT_BITS_BUDGET = (size_t)128 << 20;    // bytes of bitmap and word prefix per slice of queries
constexpr size_t MVT_CELL_BUDGET = (size_t)256 << 20;    // bytes of cells per slice, beyond one query's
constexpr int64_t MVT_ENTRIES = (int64_t)1 << 24;        // (query row, probe) entries of a slice, beyond one query's

// the last query of q0 .. q0 + nqs - 1 with q_ptr[q] <= row
__device__ __forceinline__ int mvt_query_of(const int64_t* __restrict__ q_ptr, int q0, int nqs, long row) {
  int lo = q0, hi = q0 + nqs;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (q_ptr[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}

// table[(row - r0) nc + c] = S32[row, c] for the query rows r0 .. r1 - 1
__global__ __launch_bounds__(MVC_THREADS) void mvt_table_kernel(const bf16_t* __restrict__ Q, int64_t r0, int64_t r1,
                                                                const bf16_t* __restrict__ Cn, int32_t nc, int32_t D,
                                                                float* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) MvcBf16::Stage stage[2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const long a0 = r0 + (long)blockIdx.x * MVC_TILE;
  const int na = (int)max(0l, min((long)MVC_TILE, r1 - a0));
  const int c0 = blockIdx.y * MVC_TILE;
  f32x16 acc;
  mvc_tile<MvcBf16>(Q, a0, na, Cn, (long)c0, min(MVC_TILE, nc - c0), D, stage, acc);
  const int cent = c0 + wn * 32 + c;
  if (cent >= nc) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int ti = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (ti < na) table[(a0 - r0 + ti) * nc + cent] = acc[r];
  }
}

// pc[row np1 + r] = the r-th centroid of `row` by (bf16 key of S32 descending, centroid ascending), r < min(np1, nc), and
// ps[..] its S32; slot np1 - 1 is c*(i), and holds -1 / 0 when every centroid is probed
__global__ __launch_bounds__(MVT_THREADS) void mvt_probe_kernel(const float* __restrict__ table, int64_t r0, int64_t r1,
                                                                int32_t nc, int32_t np1, int32_t* __restrict__ pc,
                                                                float* __restrict__ ps) {
  const int lane = threadIdx.x & 63;
  const long row = r0 + (long)blockIdx.x * (MVT_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= r1) return;
  const float* T = table + (row - r0) * nc;
  uint32_t v[64];                                             // (key as unsigned) << 16 | ~centroid; 0: no centroid
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const int c = 64 * k + lane;
    v[k] = c < nc ? (((mvc_key(T[c]) ^ 0x8000u) << 16) | (0xFFFFu - (uint32_t)c)) : 0u;
  }
  const int take = min(np1, nc);
  for (int r = 0; r < take; ++r) {
    uint32_t best = 0u;
#pragma unroll
    for (int k = 0; k < 64; ++k) best = max(best, v[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o, 64));
    if (lane == 0) {
      const int c = (int)(0xFFFFu - (best & 0xFFFFu));
      pc[row * np1 + r] = c;
      ps[row * np1 + r] = T[c];
    }
#pragma unroll
    for (int k = 0; k < 64; ++k) v[k] = v[k] == best ? 0u : v[k];
  }
  if (take < np1 && lane == 0) {
    pc[row * np1 + np1 - 1] = -1;
    ps[row * np1 + np1 - 1] = 0.f;
  }
}

// the document of list row j when the row is one of centroid c's: a row id outside the store, a code that is not c and a
// document outside [0, nd) give -1
__device__ __forceinline__ int32_t mvt_row_doc(int32_t j, int c, const uint16_t* __restrict__ codes, int64_t drows,
                                               int32_t nc, const int32_t* __restrict__ row_doc, int32_t nd) {
  if (j < 0 || (int64_t)j >= drows || min((int)codes[j], nc - 1) != c) return -1;
  const int32_t d = row_doc[j];
  return (uint32_t)d < (uint32_t)nd ? d : -1;
}

// the bit of the document of every row of centroid pc[row, slot]'s list, in the bitmap row of the query that owns `row`
__global__ __launch_bounds__(MVT_THREADS) void mvt_mark_kernel(
    const int32_t* __restrict__ pc, int32_t np1, const int64_t* __restrict__ q_ptr, int32_t q0, int32_t nqs,
    const int64_t* __restrict__ rlp, const int32_t* __restrict__ row_list, const int32_t* __restrict__ row_doc,
    const uint16_t* __restrict__ codes, int64_t drows, int32_t nc, int32_t nd, int64_t wp, uint32_t* __restrict__ bits) {
  const long row = q_ptr[q0] + blockIdx.x;
  const int q = mvt_query_of(q_ptr, q0, nqs, row);
  const int c = pc[row * np1 + blockIdx.y];
  uint32_t* b = bits + (long)(q - q0) * wp;
  const long e = rlp[c + 1];
  for (long i = rlp[c] + threadIdx.x; i < e; i += MVT_THREADS) {
    const int32_t d = mvt_row_doc(row_list[i], c, codes, drows, nc, row_doc, nd);
    if (d < 0) continue;
    const uint32_t m = 1u << (d & 31);
    // rows of a document are neighbours and rows of a query share lists: look before the atomic (a stale look only
    // repeats an idempotent or)
    if (!(__hip_atomic_load(b + (d >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & m)) atomicOr(b + (d >> 5), m);
  }
}

// prew[q wp + w] = the set bits of query q's bitmap row in front of word w; tot[q] = all of them; *maxtot their maximum
__global__ __launch_bounds__(MVC_WALK_THREADS) void mvt_count_kernel(const uint32_t* __restrict__ bits, int64_t wp,
                                                                     int32_t* __restrict__ prew, int32_t* __restrict__ tot,
                                                                     int32_t* __restrict__ maxtot) {
  __shared__ int wsum[MVC_WALK_THREADS / 64];
  const int t = threadIdx.x;
  const uint32_t* b = bits + (long)blockIdx.x * wp;
  int32_t* out = prew + (long)blockIdx.x * wp;
  int base = 0;
  for (long w0 = 0; w0 < wp; w0 += MVC_WALK_THREADS) {
    const long w = w0 + t;
    int all;
    const int off = mvp_block_scan(w < wp ? __popc(b[w]) : 0, wsum, all);
    if (w < wp) out[w] = base + off;
    base += all;
  }
  if (t == 0) {
    tot[blockIdx.x] = base;
    atomicMax(maxtot, base);
  }
}

// entry i = (query row r0 + i / np, probe slot i % np): ++cnt[its centroid]
__global__ __launch_bounds__(MVT_THREADS) void mvt_join_count_kernel(const int32_t* __restrict__ pc, int32_t np, int32_t np1,
                                                                     int64_t r0, int64_t n, int32_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * MVT_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t row = r0 + i / np;
  atomicAdd(cnt + pc[row * np1 + (int)(i - (i / np) * np)], 1);
}

// cnt -> wl_ptr [nc + 1] (entry starts) and cur (a copy the fill counts up); tile_ptr [nc + 1]: the score workgroups in
// front of centroid c, ceil(cnt[c] / 64) * ceil(list rows of c / MVT_STRETCH) each
__global__ __launch_bounds__(MVC_WALK_THREADS) void mvt_join_scan_kernel(const int32_t* __restrict__ cnt,
                                                                         const int64_t* __restrict__ rlp, int32_t nc,
                                                                         int32_t* __restrict__ wl_ptr, int32_t* __restrict__ cur,
                                                                         int64_t* __restrict__ tile_ptr) {
  __shared__ unsigned long long wsum[2][MVC_WALK_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int per = (nc + MVC_WALK_THREADS - 1) / MVC_WALK_THREADS;              // at most four centroids a thread
  const int c0 = min(nc, t * per), c1 = min(nc, c0 + per);
  unsigned long long x[2] = {0ull, 0ull};                     // entries, tiles
  for (int c = c0; c < c1; ++c) {
    const long n = cnt[c], len = rlp[c + 1] - rlp[c];
    x[0] += (unsigned long long)n;
    x[1] += (unsigned long long)(((n + MVC_TILE - 1) / MVC_TILE) * ((len + MVT_STRETCH - 1) / MVT_STRETCH));
  }
  unsigned long long incl[2] = {x[0], x[1]};
#pragma unroll
  for (int o = 1; o < 64; o <<= 1)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const unsigned long long y = __shfl_up(incl[u], o, 64);
      if (lane >= o) incl[u] += y;
    }
  if (lane == 63) { wsum[0][wave] = incl[0]; wsum[1][wave] = incl[1]; }
  __syncthreads();
  unsigned long long run[2], all[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    unsigned long long off = 0ull;
    all[u] = 0ull;
#pragma unroll
    for (int w = 0; w < MVC_WALK_THREADS / 64; ++w) {
      const unsigned long long y = wsum[u][w];
      off += w < wave ? y : 0ull;
      all[u] += y;
    }
    run[u] = off + incl[u] - x[u];
  }
  for (int c = c0; c < c1; ++c) {
    const long n = cnt[c], len = rlp[c + 1] - rlp[c];
    wl_ptr[c] = (int32_t)run[0];
    cur[c] = (int32_t)run[0];
    tile_ptr[c] = (int64_t)run[1];
    run[0] += (unsigned long long)n;
    run[1] += (unsigned long long)(((n + MVC_TILE - 1) / MVC_TILE) * ((len + MVT_STRETCH - 1) / MVT_STRETCH));
  }
  if (t == 0) {
    wl_ptr[nc] = (int32_t)all[0];
    tile_ptr[nc] = (int64_t)all[1];
  }
}

// entry i takes a place in its centroid's stretch of the work list: the query row and its S32 with that centroid
__global__ __launch_bounds__(MVT_THREADS) void mvt_join_fill_kernel(const int32_t* __restrict__ pc,
                                                                    const float* __restrict__ ps, int32_t np, int32_t np1,
                                                                    int64_t r0, int64_t n, int32_t* __restrict__ cur,
                                                                    int32_t* __restrict__ wl_row, float* __restrict__ wl_s) {
  const int64_t i = (int64_t)blockIdx.x * MVT_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t row = r0 + i / np, at = row * np1 + (i - (i / np) * np);
  const int pos = atomicAdd(cur + pc[at], 1);
  wl_row[pos] = (int32_t)row;
  wl_s[pos] = ps[at];
}

// cells[((q - q0) stride + rank of d in P(q)) pitch + i - q_ptr[q]] = max(.., key(t(i, j))) over the list rows j of the
// workgroup's stretch that belong to d, for the 64 entries (query rows i) of its tile
template <int NB>
__global__ __launch_bounds__(MVC_THREADS) void mvt_score_kernel(
    const uint16_t* __restrict__ codes, const unsigned char* __restrict__ bits, const uint16_t* __restrict__ weights,
    int32_t nc, const bf16_t* __restrict__ Q, int32_t D, int64_t drows, const int64_t* __restrict__ rlp,
    const int32_t* __restrict__ row_list, const int32_t* __restrict__ row_doc, int32_t nd,
    const int64_t* __restrict__ q_ptr, int32_t q0, int32_t nqs, const int32_t* __restrict__ wl_ptr,
    const int32_t* __restrict__ wl_row, const float* __restrict__ wl_s, const int64_t* __restrict__ tile_ptr,
    const uint32_t* __restrict__ pbits, const int32_t* __restrict__ prew, int64_t wp, int64_t stride, int32_t pitch,
    uint32_t* __restrict__ cells) {
  typedef typename MvrWord<NB>::type W;
  typedef MvcBf16 P;
  __shared__ __attribute__((aligned(16))) P::Stage stage[2];
  __shared__ uint32_t lut[1 << (2 * NB)];
  __shared__ int32_t qrow[MVC_TILE], qq[MVC_TILE], qi[MVC_TILE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const int64_t tile = blockIdx.x;
  int cen = 0;                                                // the last centroid with tile_ptr <= tile: it owns the tile
  for (int hi = nc; hi - cen > 1;) {
    const int mid = cen + ((hi - cen) >> 1);
    if (tile_ptr[mid] <= tile) cen = mid; else hi = mid;
  }
  const long la = rlp[cen], len = rlp[cen + 1] - la;
  const long nst = (len + MVT_STRETCH - 1) / MVT_STRETCH, local = tile - tile_ptr[cen];
  if (nst <= 0 || local < 0) return;
  const long qt = local / nst, st = local - qt * nst;
  const long e0 = wl_ptr[cen] + qt * MVC_TILE;
  const int ne = (int)min((long)MVC_TILE, wl_ptr[cen + 1] - e0);
  const long a = la + st * MVT_STRETCH;
  const int nrow = (int)min((long)MVT_STRETCH, len - st * MVT_STRETCH);
  if (ne <= 0 || nrow <= 0) return;
  if (t < (1 << (2 * NB)))                                    // mvr_score_kernel's table of weight pairs
    lut[t] = (uint32_t)weights[t & ((1 << NB) - 1)] | ((uint32_t)weights[t >> NB] << 16);
  if (t < MVC_TILE) {
    int32_t row = -1, ql = 0, in = 0;
    if (t < ne) {
      row = wl_row[e0 + t];
      const int q = mvt_query_of(q_ptr, q0, nqs, row);
      ql = q - q0;
      in = (int)(row - q_ptr[q]);
    }
    qrow[t] = row; qq[t] = ql; qi[t] = in;
  }
  __syncthreads();
  const int ar[2] = {qrow[t >> 3], qrow[(t >> 3) + 32]};       // the gathered A rows of this thread's two 16-byte pieces
  auto fetch = [&](int k0, P::Regs& r) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      r.v[i] = ar[i] >= 0 ? *(const u32x4*)(Q + (long)ar[i] * D + k0 + (t & 7) * 8) : (u32x4){0u, 0u, 0u, 0u};
  };
  const int nk = D / P::KT, wpr = D / 16;                     // words of a row
  const int col = wn * 32 + c;
  float s32[16];                                              // S32 of this lane's sixteen entries with the centroid
#pragma unroll
  for (int r = 0; r < 16; ++r) s32[r] = wl_s[e0 + min(wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, ne - 1)];
  for (int n0 = 0; n0 < nrow; n0 += MVC_TILE) {
    const int nv = min(MVC_TILE, nrow - n0);                  // list rows of this tile
    int32_t br = row_list[a + n0 + min(t >> 2, nv - 1)];       // the row this thread expands; an id outside the store
    br = (br >= 0 && (int64_t)br < drows) ? br : 0;            // reads row 0, and its column is dropped below
    const W* wsrc = (const W*)bits + (long)br * wpr + (t & 3);
    // the document of this lane's column, -1 for a column past the stretch or a row that is not the centroid's
    const int32_t dcol = col < nv ? mvt_row_doc(row_list[a + n0 + col], cen, codes, drows, nc, row_doc, nd) : -1;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    P::Regs ra;
    fetch(0, ra);
    W w = wsrc[0];
    P::put(t, ra, stage[0].a);
    mvr_expand<NB>(w, lut, t, stage[0].b);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {                         // k ascending, mvr_score_kernel's steps
      const int cur = kt & 1;
      if (kt + 1 < nk) {
        fetch((kt + 1) * P::KT, ra);
        w = wsrc[4 * (kt + 1)];
      }
      P::mma(stage[cur], wm, wn, c, h, acc);
      if (kt + 1 < nk) {
        P::put(t, ra, stage[cur ^ 1].a);
        mvr_expand<NB>(w, lut, t, stage[cur ^ 1].b);
      }
      __syncthreads();
    }
    // the run of columns with this lane's document: same[k] = the column 2^k to the left belongs to it too
    bool same[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int od = __shfl_up(dcol, 1 << k, 32);
      same[k] = c >= (1 << k) && od == dcol;
    }
    const int nx = __shfl_down(dcol, 1, 32);
    const bool last = dcol >= 0 && (c == 31 || nx != dcol);   // the run's last lane holds the run's maximum
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      v[r] = s32[r] + acc[r];                                 // S32 once, at the end
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const float ov = __shfl_up(v[r], 1 << k, 32);
        v[r] = same[k] ? fmaxf(v[r], ov) : v[r];
      }
    }
    // The shuffles end here, before the LDS reads of the cells' indices: hipcc would interleave the two under counted
    // waits that are right only because a shuffle holds a slot of the same counter; the build's scan of LDS reads
    // (snx/asmcheck.py) counts reads alone.
    __builtin_amdgcn_s_waitcnt(0xC07F);                       // lgkmcnt(0)
    __builtin_amdgcn_sched_barrier(0);
    int seen = -1, rank = -1;                                 // the query whose rank of dcol is known
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ti = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (last && ti < ne) {
        const int ql = qq[ti];
        if (ql != seen) {
          const long at = (long)ql * wp + (dcol >> 5);
          const uint32_t word = pbits[at], bit = 1u << (dcol & 31);
          rank = (word & bit) ? prew[at] + __popc(word & (bit - 1u)) : -1;    // an excluded document has no rank
          seen = ql;
        }
        if (rank >= 0) atomicMax(cells + ((long)ql * stride + rank) * pitch + qi[ti], dense_key(v[r]));
      }
    }
  }
}

// a probed document's cells -> x(q, d): fkey / fdoc[(q - q0) stride + rank] = its order key and the document
__global__ __launch_bounds__(MVT_THREADS) void mvt_finish_kernel(
    const uint32_t* __restrict__ cells, const uint32_t* __restrict__ pbits, const int32_t* __restrict__ prew, int64_t wp,
    int32_t nd, int64_t stride, int32_t pitch, const int64_t* __restrict__ q_ptr, int32_t q0, const float* __restrict__ ps,
    int32_t np1, int32_t has_miss, uint32_t* __restrict__ fkey, int32_t* __restrict__ fdoc) {
  const long d = (long)blockIdx.x * MVT_THREADS + threadIdx.x;
  const int ql = blockIdx.y;
  if (d >= nd) return;
  const long at = (long)ql * wp + (d >> 5);
  const uint32_t word = pbits[at], bit = 1u << (d & 31);
  if (!(word & bit)) return;
  const long slot = (long)ql * stride + prew[at] + __popc(word & (bit - 1u));
  const uint32_t* v = cells + slot * pitch;
  const long qa = q_ptr[q0 + ql];
  const int Lq = (int)(q_ptr[q0 + ql + 1] - qa);
  const float* miss = ps + qa * np1 + (np1 - 1);              // S32[i, c*(i)], np1 apart
  float total = 0.f;
  for (int b0 = 0; b0 < Lq; b0 += MVC_TILE) {                  // runs of 64 rows from the query's first: ascending rows
    const int b1 = min(Lq, b0 + MVC_TILE);
    float s = 0.f;
    for (int i = b0; i < b1; ++i) {
      const uint32_t key = v[i];
      s += key ? dense_unkey(key) : (has_miss ? miss[(long)i * np1] : 0.f);
    }
    total = b0 == 0 ? s : total + s;                          // ascending runs
  }
  fkey[slot] = dense_key(total / (float)Lq);
  fdoc[slot] = (int32_t)d;
}

// the slots of a query as merge_lists reads a list: in doc order, so ordered_take's tie rule is the ABI's
struct MvtSlots {
  const uint32_t* key;
  const int32_t* doc;
  __device__ __forceinline__ unsigned long long at(long f) const { return rank_key(key[f], (uint32_t)doc[f]); }
  __device__ __forceinline__ uint32_t operator()(long f) const { return key[f]; }
};

__global__ __launch_bounds__(SR_THREADS) void mvt_select_kernel(const uint32_t* __restrict__ fkey,
                                                                const int32_t* __restrict__ fdoc,
                                                                const int32_t* __restrict__ tot, int64_t stride, int32_t lo,
                                                                int32_t hi, int32_t* __restrict__ out_doc,
                                                                float* __restrict__ out_score, int32_t* __restrict__ out_found) {
  __shared__ SelectSmem S;
  __shared__ unsigned long long sbuf[SR_KMAX];               // rank keys: descending = the ABI's order
  const int tid = threadIdx.x, q = blockIdx.x;
  const MvtSlots slots = {fkey + (long)q * stride, fdoc + (long)q * stride};
  const long n = tot[q];
  uint32_t thr;
  int need_eq, nsel;
  radix_select(slots, n, hi, S, thr, need_eq, nsel);          // merge_lists' body over one list of |P(q)| entries
  const int P = pow2_at_least(nsel);
  for (int i = tid; i < P; i += SR_THREADS) sbuf[i] = 0ull;
  __syncthreads();
  ordered_take(slots, n, thr, need_eq, S, [&](long f, int pos) { sbuf[pos] = slots.at(f); });
  bitonic_desc<SR_THREADS, int>(sbuf, P);
  write_ranks<dense_unkey>(sbuf, nsel, q, lo, hi, out_doc, out_score, out_found);
}

inline bool mvt_bad(int32_t nq, int32_t nd, int32_t nc, int32_t nprobe, int32_t lo, int32_t hi) {
  return nq < 0 || nd < 0 || nc < 1 || nc > MVC_NC_MAX || mvp_bad_probe(nprobe) || lo < 0 || hi <= lo || hi > SR_KMAX;
}

// the token search's workspace.  A slice of at most qs queries holds a bitmap row and a word-prefix row each; its cells,
// keys and docs share `slots` (query, probed document) places of `pitch` query rows, its work list `entries` places.
struct MvtPlan {
  size_t qptr, lptr, flag, table, pc, ps, bits, prew, tot, cnt, wlptr, cur, tileptr, wlrow, wls, cells, fkey, fdoc, total;
  int np, np1, pitch, qs;
  int64_t wp, trows, entries, slots;
  bool ok;
  MvtPlan(const int64_t* q_ptr, int32_t nq, int32_t nd, int32_t nc, int32_t nprobe) {
    const int64_t qused = q_ptr[nq];
    int64_t longest = 1;
    for (int32_t q = 0; q < nq; ++q) longest = q_ptr[q + 1] - q_ptr[q] > longest ? q_ptr[q + 1] - q_ptr[q] : longest;
    np = nprobe < nc ? nprobe : nc;
    np1 = np + 1;
    ok = qused <= 0x7FFFFFFFL - MVC_TILE && longest * np <= 0x3FFFFFFFL && longest <= 0x00FFFFFFL;
    pitch = ok ? (int)((longest + 3) & ~3l) : 4;
    wp = (((int64_t)nd + 31) / 32 + 3) & ~3l;
    wp = wp < 4 ? 4 : wp;
    const int64_t tr = (int64_t)(MVT_TABLE_BUDGET / ((size_t)nc * 4)) & ~(int64_t)(MVC_TILE - 1);   // >= 8,192 rows
    trows = qused < tr ? ((qused + MVC_TILE - 1) & ~(int64_t)(MVC_TILE - 1)) : tr;
    trows = trows < MVC_TILE ? MVC_TILE : trows;
    size_t s = MVT_BITS_BUDGET / ((size_t)wp * 8);
    qs = (int)(s < 1 ? 1 : (s > (size_t)nq ? (size_t)nq : s));
    qs = qs > 65535 ? 65535 : qs;                             // a grid's y
    const int64_t e_all = qused * np, e_one = longest * np;
    entries = e_all < MVT_ENTRIES ? e_all : (e_one > MVT_ENTRIES ? e_one : MVT_ENTRIES);
    entries = entries < 1 ? 1 : entries;
    const int64_t budget = (int64_t)(MVT_CELL_BUDGET / ((size_t)pitch * 4));
    const int64_t s_all = (int64_t)nq * nd;                   // every document probed by every query
    slots = s_all < budget ? s_all : (nd > budget ? nd : budget);
    slots = slots < 1 ? 1 : slots;
    Arena a;
    qptr = a.take(((size_t)nq + 1) * 8);
    lptr = a.take(((size_t)nc + 1) * 8);
    flag = a.take(16);
    table = a.take((size_t)trows * (size_t)nc * 4);
    pc = a.take((size_t)qused * (size_t)np1 * 4);
    ps = a.take((size_t)qused * (size_t)np1 * 4);
    bits = a.take((size_t)qs * (size_t)wp * 4);
    prew = a.take((size_t)qs * (size_t)wp * 4);
    tot = a.take((size_t)qs * 4);
    cnt = a.take((size_t)nc * 4);
    wlptr = a.take(((size_t)nc + 1) * 4);
    cur = a.take((size_t)nc * 4);
    tileptr = a.take(((size_t)nc + 1) * 8);
    wlrow = a.take((size_t)entries * 4);
    wls = a.take((size_t)entries * 4);
    cells = a.take((size_t)slots * (size_t)pitch * 4);
    fkey = a.take((size_t)slots * 4);
    fdoc = a.take((size_t)slots * 4);
    total = a.off;
  }
};

template <int NB>
int mvt_launch_score(unsigned grid, hipStream_t st, const uint16_t* codes, const void* bits, const uint16_t* weights,
                     int32_t nc, const bf16_t* q, int32_t D, int64_t drows, const int64_t* lptr, const int32_t* row_list,
                     const int32_t* row_doc, int32_t nd, const int64_t* qptr, int32_t q0, int32_t nqs, const int32_t* wlptr,
                     const int32_t* wlrow, const float* wls, const int64_t* tileptr, const uint32_t* pbits,
                     const int32_t* prew, int64_t wp, int64_t stride, int32_t pitch, uint32_t* cells) {
  hipLaunchKernelGGL(mvt_score_kernel<NB>, dim3(grid), dim3(MVC_THREADS), 0, st, codes, (const unsigned char*)bits, weights, nc,
                     q, D, drows, lptr, row_list, row_doc, nd, qptr, q0, nqs, wlptr, wlrow, wls, tileptr, pbits, prew, wp,
                     stride, pitch, cells);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

}  // namespace

extern "C" size_t snx_mv_token_search_workspace_bytes(const int64_t* q_ptr, int32_t nq, int32_t nd, int64_t drows, int32_t nc,
                                                      int32_t nprobe, int32_t hi) {
  if (nq <= 0 || drows < 0 || mvt_bad(nq, nd, nc, nprobe, 0, hi) || !mvc_ptr_ok(q_ptr, nq, 0x7FFFFFFFFFFFFFFFL, true)) return 0;
  const MvtPlan plan(q_ptr, nq, nd, nc, nprobe);
  return plan.ok ? plan.total : 0;
}

extern "C" int snx_mv_token_search(const uint16_t* codes, const void* bits, const void* centroids, const uint16_t* weights,
                                   int32_t nc, int32_t nbits, const void* q, int32_t mv_f32, int32_t D, int64_t drows,
                                   const int64_t* doc_ptr, int32_t nd, const int64_t* row_list_ptr, const int32_t* row_list,
                                   const int32_t* row_doc, int64_t qrows, const int64_t* q_ptr, int32_t nq,
                                   const int64_t* ex_ptr, const int32_t* ex_doc, int32_t nprobe, int32_t lo, int32_t hi,
                                   int32_t* out_doc, float* out_score, int32_t* out_found, void* workspace, size_t ws_bytes,
                                   hipStream_t st) {
  if (D <= 0 || (D % 64) != 0 || D > MVC_DMAX || qrows < 0 || drows < 0 || drows > 0x7FFFFFFFL) return SNX_E_SHAPE;
  if (mv_f32 || mvr_bad_nbits(nbits) || mvt_bad(nq, nd, nc, nprobe, lo, hi)) return SNX_E_ARG;
  if (nq == 0) return SNX_OK;
  if (!q || !centroids || !weights || !out_doc || !out_score || !out_found || !workspace || (ex_ptr && !ex_doc) ||
      ((uintptr_t)q & 15) != 0 || ((uintptr_t)centroids & 15) != 0 || ((uintptr_t)bits & 15) != 0 ||
      ((uintptr_t)workspace & 15) != 0)
    return SNX_E_ARG;
  // the three pointer arrays are pageable host memory: everything a kernel will trust is checked here, before any launch
  if (!mvc_ptr_ok(doc_ptr, nd, drows, false) || !mvc_ptr_ok(q_ptr, nq, qrows, true)) return SNX_E_ARG;
  const int64_t dused = doc_ptr[nd];
  if (!mvc_ptr_ok(row_list_ptr, nc, dused, false) || row_list_ptr[nc] != dused) return SNX_E_ARG;
  if (dused > 0 && (!codes || !bits || !row_list || !row_doc)) return SNX_E_ARG;
  const MvtPlan plan(q_ptr, nq, nd, nc, nprobe);
  if (!plan.ok) return SNX_E_SHAPE;
  if (ws_bytes < plan.total) return SNX_E_ARG;
  char* ws = (char*)workspace;
  RC(mvc_upload(ws, plan.qptr, q_ptr, ((size_t)nq + 1) * 8, st));
  RC(mvc_upload(ws, plan.lptr, row_list_ptr, ((size_t)nc + 1) * 8, st));
  const int64_t* qptr = (const int64_t*)(ws + plan.qptr);
  const int64_t* lptr = (const int64_t*)(ws + plan.lptr);
  int32_t* flag = (int32_t*)(ws + plan.flag);                 // [0]: the largest |P(q)| of a slice; [2..3]: its score tiles
  float *table = (float*)(ws + plan.table), *ps = (float*)(ws + plan.ps), *wls = (float*)(ws + plan.wls);
  int32_t *pc = (int32_t*)(ws + plan.pc), *prew = (int32_t*)(ws + plan.prew), *tot = (int32_t*)(ws + plan.tot);
  int32_t *cnt = (int32_t*)(ws + plan.cnt), *wlptr = (int32_t*)(ws + plan.wlptr), *cur = (int32_t*)(ws + plan.cur);
  int32_t *wlrow = (int32_t*)(ws + plan.wlrow), *fdoc = (int32_t*)(ws + plan.fdoc);
  int64_t* tileptr = (int64_t*)(ws + plan.tileptr);
  uint32_t *pbits = (uint32_t*)(ws + plan.bits), *cells = (uint32_t*)(ws + plan.cells), *fkey = (uint32_t*)(ws + plan.fkey);
  const bf16_t* Q = (const bf16_t*)q;
  const int64_t qused = q_ptr[nq];
  const int np = plan.np, np1 = plan.np1;
  for (int64_t r0 = 0; r0 < qused; r0 += plan.trows) {        // top(i), c*(i) and their S32 for every query row of the call
    const int64_t r1 = r0 + plan.trows < qused ? r0 + plan.trows : qused;
    hipLaunchKernelGGL(mvt_table_kernel, dim3((unsigned)((r1 - r0 + MVC_TILE - 1) / MVC_TILE), (unsigned)((nc + MVC_TILE - 1) / MVC_TILE)),
                       dim3(MVC_THREADS), 0, st, Q, r0, r1, (const bf16_t*)centroids, nc, D, table);
    SNX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mvt_probe_kernel, dim3((unsigned)((r1 - r0 + MVT_THREADS / 64 - 1) / (MVT_THREADS / 64))),
                       dim3(MVT_THREADS), 0, st, (const float*)table, r0, r1, nc, np1, pc, ps);
    SNX_CHECK_LAUNCH();
  }
  int32_t cap = plan.qs;
  for (int32_t q0 = 0; q0 < nq;) {                            // one slice of queries after the other
    int32_t nqs = nq - q0 < cap ? nq - q0 : cap;
    while (nqs > 1 && (q_ptr[q0 + nqs] - q_ptr[q0]) * np > plan.entries) --nqs;
    const int64_t r0 = q_ptr[q0], rows = q_ptr[q0 + nqs] - r0, entries = rows * np;
    hipError_t e = hipMemsetAsync(pbits, 0, (size_t)nqs * (size_t)plan.wp * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(flag, 0, 16, st);
    if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, (size_t)nc * 4, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mvt_mark_kernel, dim3((unsigned)rows, (unsigned)np), dim3(MVT_THREADS), 0, st, (const int32_t*)pc, np1,
                       qptr, q0, nqs, lptr, row_list, row_doc, codes, drows, nc, nd, plan.wp, pbits);
    SNX_CHECK_LAUNCH();
    if (ex_ptr) {
      hipLaunchKernelGGL(mvp_unmark_kernel, dim3((unsigned)nqs), dim3(MVP_THREADS), 0, st, ex_ptr + q0, ex_doc, nd, plan.wp,
                         pbits);
      SNX_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(mvt_count_kernel, dim3((unsigned)nqs), dim3(MVC_WALK_THREADS), 0, st, (const uint32_t*)pbits, plan.wp,
                       prew, tot, flag);
    SNX_CHECK_LAUNCH();
    const dim3 egrid((unsigned)((entries + MVT_THREADS - 1) / MVT_THREADS));
    hipLaunchKernelGGL(mvt_join_count_kernel, egrid, dim3(MVT_THREADS), 0, st, (const int32_t*)pc, np, np1, r0, entries, cnt);
    SNX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mvt_join_scan_kernel, dim3(1), dim3(MVC_WALK_THREADS), 0, st, (const int32_t*)cnt, lptr, nc, wlptr, cur,
                       tileptr);
    SNX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mvt_join_fill_kernel, egrid, dim3(MVT_THREADS), 0, st, (const int32_t*)pc, (const float*)ps, np, np1, r0,
                       entries, cur, wlrow, wls);
    SNX_CHECK_LAUNCH();
    int32_t most = 0;                                         // the cells follow the probed documents, not nd
    int64_t tiles = 0;
    e = hipMemcpyAsync(&most, flag, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&tiles, tileptr + nc, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return (int)e;
    if (nqs > 1 && (int64_t)nqs * most > plan.slots) {        // the slice's cells do not fit: a smaller slice, from here on
      cap = (int32_t)(plan.slots / most);
      cap = cap < 1 ? 1 : cap;
      continue;
    }
    if (tiles > 0x7FFFFFFFL) return SNX_E_SHAPE;
    const int64_t stride = most > 0 ? most : 1;
    if (most > 0) {
      e = hipMemsetAsync(cells, 0, (size_t)nqs * (size_t)stride * (size_t)plan.pitch * 4, st);
      if (e != hipSuccess) return (int)e;
      if (tiles > 0) {
        if (nbits == 1)
          RC(mvt_launch_score<1>((unsigned)tiles, st, codes, bits, weights, nc, Q, D, drows, lptr, row_list, row_doc, nd, qptr,
                                 q0, nqs, wlptr, wlrow, wls, tileptr, pbits, prew, plan.wp, stride, plan.pitch, cells));
        else if (nbits == 2)
          RC(mvt_launch_score<2>((unsigned)tiles, st, codes, bits, weights, nc, Q, D, drows, lptr, row_list, row_doc, nd, qptr,
                                 q0, nqs, wlptr, wlrow, wls, tileptr, pbits, prew, plan.wp, stride, plan.pitch, cells));
        else
          RC(mvt_launch_score<4>((unsigned)tiles, st, codes, bits, weights, nc, Q, D, drows, lptr, row_list, row_doc, nd, qptr,
                                 q0, nqs, wlptr, wlrow, wls, tileptr, pbits, prew, plan.wp, stride, plan.pitch, cells));
      }
      hipLaunchKernelGGL(mvt_finish_kernel, dim3((unsigned)((nd + MVT_THREADS - 1) / MVT_THREADS), (unsigned)nqs),
                         dim3(MVT_THREADS), 0, st, (const uint32_t*)cells, (const uint32_t*)pbits, (const int32_t*)prew,
                         plan.wp, nd, stride, plan.pitch, qptr, q0, (const float*)ps, np1, (int32_t)(np < nc), fkey, fdoc);
      SNX_CHECK_LAUNCH();
    }
    const size_t w = (size_t)(hi - lo);
    hipLaunchKernelGGL(mvt_select_kernel, dim3((unsigned)nqs), dim3(SR_THREADS), 0, st, (const uint32_t*)fkey,
                       (const int32_t*)fdoc, (const int32_t*)tot, stride, lo, hi, out_doc + (size_t)q0 * w,
                       out_score + (size_t)q0 * w, out_found + q0);
    SNX_CHECK_LAUNCH();
    q0 += nqs;
  }
  return SNX_OK;
}
