// Multi-vector search (include/snx.h "multi-vector search"): exact MaxSim top-k of every query against every document of a
// ragged row store.  maxsim.hip scores pairs the caller already knows, one workgroup per (pair, 64 query rows), and
// re-stages the query block for every document tile; a search reads every document for every query, so the work is split
// the other way round here.
//
// Queries are packed.  The query rows of the call lie end to end, and query block b is rows 64 b .. 64 b + 63 of them,
//                  whichever queries they belong to: a block of 16-row queries holds four of them and its 64 x 64 score
//                  tile is full; a query may straddle a block edge or span several blocks.
// mv_score_kernel  One workgroup (four waves) per (query block, chunk of documents), the query block the fast grid index:
//                  the workgroups that are resident together walk the same chunk, so its rows come from HBM about once per
//                  wave of workgroups.  The bf16 query block is written to LDS once, with a pitch of D + 8 (132 KB at D =
//                  1024), and stays there for the whole walk; only document rows stream through the double-buffered K-slice
//                  stage (18 KB).  At D = 1024 the whole next tile's rows wait in registers meanwhile (see the kernel);
//                  other D fetch one slice ahead, the first slice of the next tile during the epilogue of this one.
//                  The fp32 block does not fit that way at D = 1024: that precision stages both operands in K slices
//                  for every D, as ms_pair_kernel does.  The MFMA steps are ms_pair_kernel's, k ascending: a score
//                  element is the same chain of the same two rows.
//                  The chunk's rows are walked in tiles of 64 whatever documents they belong to.  A tile column's document
//                  comes from a row-to-document map; the epilogue takes, per accumulator row, a segmented max-scan keyed
//                  by document over the 32 lanes that hold a wave's columns (five shuffle steps for every document of the
//                  tile at once).  The lane at a segment's end writes the segment's row maxima to LDS (the stage's memory,
//                  idle then), the second column wave joining the segment that crosses column 32; a document that
//                  continues into the next tile leaves its running maxima in `carry`.  When a document ends, its row
//                  maxima are added per SLOT of the block in ascending row order and written to part[doc][slot].
// Slots            The ABI adds a query's row maxima within runs of 64 rows counted from the query's first row, then the
//                  run sums in order.  A run lies in at most two query blocks.  Its rows in the block where it starts are
//                  one slot: the left fold from +0 of their maxima, a prefix of the run's chain.  Each of its rows in the
//                  next block is a slot of its own, holding the raw maximum, so that mv_select_kernel can continue the
//                  chain where the prefix stopped: the order of every addition is the pair kernel's.  A block has at most
//                  64 slots, aligned queries have one per run.  mv_slots_kernel derives them from q_ptr on the device.
// mv_select_kernel One workgroup per (query, chunk): finishes the chunk's scores from the slots (one division by Lq), drops
//                  documents without rows and excluded ones, and keeps the chunk's top hi as rank keys in document order
//                  (dense_key, select_chunk).  mv_merge_kernel is merge_lists over the chunks, as dn_merge_kernel.
// part holds a bounded group of chunks; the host walks the groups on the stream.  Nothing of size nq x nd exists.
#include "dense_common.h"
#include "snx.h"

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int MV_THREADS = 256;
constexpr int MV_TILE = 64;                    // query rows of a block and doc rows of a tile
constexpr int MV_DMAX = 1024;
constexpr int MV_MPITCH = 65;                  // floats per segment of the epilogue's row maxima
constexpr int MV_CHUNK_MIN = 64, MV_CHUNK_DEFAULT = 512, MV_CHUNK_MAX = 8192;   // docs per chunk (keys in LDS: 32 KB)
constexpr int MV_WG_TARGET = 4096;             // workgroups per score launch that the chunk group aims at
constexpr size_t MV_PART_BUDGET = (size_t)128 << 20;   // bytes of partial sums per launch, beyond one chunk's

// The operand staging and MFMA steps of one precision, after MsBf16 / MsF32 of maxsim.hip (same slices, same steps).
// fetch: this thread's share of a 64-row K slice into registers (rows t >> 3 and 32 + (t >> 3), 16 bytes each; a row past
// the count reads as zero); put: registers -> LDS stage; mma: the slice's MFMA steps in ascending k.
struct MvBf16 {
  typedef bf16_t elem;
  static constexpr bool RESIDENT = true;       // the query block lives in LDS: [64][D + 8]
  static constexpr int KT = 64, PITCH = 72;
  struct Stage { uint16_t b[MV_TILE][PITCH]; };
  struct Regs { u32x4 b[2]; };
  __host__ __device__ static constexpr int q_bytes(int D) { return MV_TILE * (D + 8) * 2; }
  __device__ static __forceinline__ void fetch(const elem* __restrict__, long, int, const elem* __restrict__ E, long d0,
                                               int nd, int D, int k0, int t, Regs& r) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (t >> 3) + 32 * i;
      r.b[i] = row < nd ? *(const u32x4*)(E + (d0 + row) * D + k0 + (t & 7) * 8) : (u32x4){0u, 0u, 0u, 0u};
    }
  }
  // the same share without a branch around the load, so that the deep loop's wait counts stay static: a row past the
  // count (nd >= 1) reads the last row again; the epilogue masks its column
  __device__ static __forceinline__ void fetch_all(const elem* __restrict__ E, long d0, int nd, int D, int k0, int t,
                                                   Regs& r) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
      r.b[i] = *(const u32x4*)(E + (d0 + min((t >> 3) + 32 * i, nd - 1)) * D + k0 + (t & 7) * 8);
  }
  __device__ static __forceinline__ void put(int t, const Regs& r, Stage& s) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *(u32x4*)&s.b[(t >> 3) + 32 * i][(t & 7) * 8] = r.b[i];
  }
  // the operands of a slice as registers: the deep loop reads those of slice k + 1 before it issues the MFMAs of slice k
  __device__ static __forceinline__ void load_a(const uint16_t* Qs, int qp, int k0, int wm, int c, int h,
                                                bf16x8 (&a)[KT / 16]) {
#pragma unroll
    for (int u = 0; u < KT / 16; ++u) a[u] = *(const bf16x8*)&Qs[(wm * 32 + c) * qp + k0 + 16 * u + 8 * h];
  }
  __device__ static __forceinline__ void load_b(const Stage& s, int wn, int c, int h, bf16x8 (&b)[KT / 16]) {
#pragma unroll
    for (int u = 0; u < KT / 16; ++u) b[u] = *(const bf16x8*)&s.b[wn * 32 + c][16 * u + 8 * h];
  }
  __device__ static __forceinline__ void mma_ab(const bf16x8 (&a)[KT / 16], const bf16x8 (&b)[KT / 16], f32x16& acc) {
#pragma unroll
    for (int u = 0; u < KT / 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[u], b[u], acc, 0, 0, 0);
  }
  __device__ static __forceinline__ void mma(const uint16_t* Qs, int qp, int k0, const Stage& s, int wm, int wn, int c,
                                             int h, f32x16& acc) {
    bf16x8 a[KT / 16], b[KT / 16];
    load_a(Qs, qp, k0, wm, c, h, a);
    load_b(s, wn, c, h, b);
    mma_ab(a, b, acc);
  }
};

struct MvF32 {
  typedef float elem;
  static constexpr bool RESIDENT = false;      // both operands pass through the k-major stage
  static constexpr int KT = 32, PITCH = 68;
  struct Stage { float a[KT][PITCH], b[KT][PITCH]; };
  struct Regs { f32x4 a[2], b[2]; };
  __host__ __device__ static constexpr int q_bytes(int) { return 0; }
  __device__ static __forceinline__ void fetch(const elem* __restrict__ Q, long q0, int nq, const elem* __restrict__ E,
                                               long d0, int nd, int D, int k0, int t, Regs& r) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (t >> 3) + 32 * i;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      r.a[i] = row < nq ? *(const f32x4*)(Q + (q0 + row) * D + k0 + (t & 7) * 4) : z;
      r.b[i] = row < nd ? *(const f32x4*)(E + (d0 + row) * D + k0 + (t & 7) * 4) : z;
    }
  }
  __device__ static __forceinline__ void put(int t, const Regs& r, Stage& s) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        s.a[(t & 7) * 4 + u][(t >> 3) + 32 * i] = r.a[i][u];
        s.b[(t & 7) * 4 + u][(t >> 3) + 32 * i] = r.b[i][u];
      }
  }
  __device__ static __forceinline__ void mma(const uint16_t*, int, int, const Stage& s, int wm, int wn, int c, int h,
                                             f32x16& acc) {
#pragma unroll
    for (int u = 0; u < KT / 2; ++u)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s.a[2 * u + h][wm * 32 + c], s.b[2 * u + h][wn * 32 + c], acc, 0, 0, 0);
  }
};

template <typename P>
constexpr int mv_lds_bytes(int D) { return P::q_bytes(D) + 2 * (int)sizeof(typename P::Stage); }
static_assert(2 * sizeof(MvBf16::Stage) >= MV_TILE * MV_MPITCH * 4 && 2 * sizeof(MvF32::Stage) >= MV_TILE * MV_MPITCH * 4,
              "the epilogue's row maxima live in the stage");
static_assert(mv_lds_bytes<MvBf16>(MV_DMAX) + 2048 <= 160 * 1024, "160 KB of LDS per workgroup");

// ------------------------------------------------------------------------------------------------ slots
// A slot as one int: first row in its block | rows << 8 | raw << 16.  rows >= 1, so 0 is "no slot starts here".
__device__ __forceinline__ int slot_row(int pk) { return pk & 255; }
__device__ __forceinline__ int slot_rows(int pk) { return (pk >> 8) & 255; }
__device__ __forceinline__ bool slot_raw(int pk) { return (pk >> 16) != 0; }

// the slot that packed query row r starts (0: none); first_of = the query whose first row r is, or -1
__device__ __forceinline__ int mv_slot_at(const int64_t* __restrict__ q_ptr, int nq, long r, long qused, int& first_of) {
  first_of = -1;
  if (r >= qused) return 0;
  int lo = 0, hi = nq - 1;                                   // the query of row r: every query has rows
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (q_ptr[mid] <= r) lo = mid; else hi = mid - 1;
  }
  const long a = q_ptr[lo], e = q_ptr[lo + 1];
  const long run0 = a + ((r - a) / MV_TILE) * MV_TILE, run1 = min(e, run0 + MV_TILE);
  const long blk0 = (r / MV_TILE) * MV_TILE;
  if (r == a) first_of = lo;
  if (run0 < blk0) return (int)(r - blk0) | (1 << 8) | (1 << 16);          // the run began in the block before: raw
  if (r == run0) return (int)(r - blk0) | ((int)(min(run1, blk0 + MV_TILE) - r) << 8);
  return 0;
}

// write == 0: bcnt[b] = slots of block b.  write != 0 (bslot = their running sums): the slots and each query's first one.
__global__ __launch_bounds__(MV_TILE) void mv_slots_kernel(const int64_t* __restrict__ q_ptr, int32_t nq, int64_t qused,
                                                           int32_t nqb, int32_t write, int32_t* __restrict__ bcnt,
                                                           const int32_t* __restrict__ bslot, int32_t* __restrict__ slots,
                                                           int32_t* __restrict__ q_slot) {
  const int t = threadIdx.x, b = blockIdx.x;
  int first_of;
  const int pk = mv_slot_at(q_ptr, nq, (long)b * MV_TILE + t, qused, first_of);
  const unsigned long long m = __ballot(pk != 0);
  if (!write) {
    if (t == 0) bcnt[b] = __popcll(m);
    return;
  }
  const int at = bslot[b] + __popcll(m & ((1ull << t) - 1ull));
  if (pk != 0) slots[at] = pk;
  if (first_of >= 0) q_slot[first_of] = at;
  if (b == 0 && t == 0) q_slot[nq] = bslot[nqb];
}

__global__ void mv_slot_scan_kernel(const int32_t* __restrict__ bcnt, int32_t nqb, int32_t* __restrict__ bslot) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int s = 0;
  for (int b = 0; b < nqb; ++b) { bslot[b] = s; s += bcnt[b]; }
  bslot[nqb] = s;
}

// row_doc[r] = the document that owns store row r < doc_ptr[nd]
__global__ __launch_bounds__(MV_THREADS) void mv_rowdoc_kernel(const int64_t* __restrict__ doc_ptr, int32_t nd, int64_t dused,
                                                               int32_t* __restrict__ row_doc) {
  const int64_t r = (int64_t)blockIdx.x * MV_THREADS + threadIdx.x;
  if (r >= dused) return;
  int lo = 1, hi = nd;                                       // the first i with doc_ptr[i] > r; doc_ptr[nd] = dused > r
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (doc_ptr[mid] > r) hi = mid; else lo = mid + 1;
  }
  row_doc[r] = lo - 1;
}

// ------------------------------------------------------------------------------------------------ scores
// NK > 0 (= D / KT): the document rows of the whole NEXT tile wait in registers (NK slices of two 16-byte loads each) while
// this tile's slices go through the stage -- one workgroup per CU (the resident query block) has nothing else to hide the
// fetch behind.  The loop is unrolled so that every register index and every wait count is static.  NK == 0: any D, one
// slice ahead.
template <typename P, int NK>
__global__ __launch_bounds__(MV_THREADS) void mv_score_kernel(
    const typename P::elem* __restrict__ E, const typename P::elem* __restrict__ Q, int32_t D, int64_t qused,
    const int64_t* __restrict__ doc_ptr, const int32_t* __restrict__ row_doc, int32_t nd, int32_t nqb,
    const int32_t* __restrict__ bslot, const int32_t* __restrict__ slots, int32_t nslots, int32_t chunk, int32_t c_first,
    float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int docid[MV_TILE + 1], segof[MV_TILE], sdoc[MV_TILE], sl[MV_TILE];
  __shared__ float carry[MV_TILE];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const int qb = (int)(blockIdx.x % (unsigned)nqb), cg = (int)(blockIdx.x / (unsigned)nqb);
  const long g0 = (long)c_first * chunk;                     // first doc of the launch's chunk group: part's row 0
  const long c0 = min((long)nd, g0 + (long)cg * chunk), c1 = min((long)nd, c0 + chunk);
  const long rowB = doc_ptr[c0], rowE = doc_ptr[c1];
  if (rowB >= rowE) return;                                  // a chunk without rows
  const long q0 = (long)qb * MV_TILE;
  const int nqr = (int)min((long)MV_TILE, qused - q0);
  const int s0 = bslot[qb], nsl = bslot[qb + 1] - s0;
  uint16_t* Qs = (uint16_t*)smem;
  const int qp = D + 8;
  typename P::Stage* stage = (typename P::Stage*)(smem + P::q_bytes(D));
  float (*M)[MV_MPITCH] = (float (*)[MV_MPITCH])stage;
  if (t < nsl) sl[t] = slots[s0 + t];
  if (P::RESIDENT) {                                         // the query block, once for the whole walk
    const int vecs = D / 8;
    for (int i = t; i < MV_TILE * vecs; i += MV_THREADS) {
      const int row = i / vecs, cv = i - row * vecs;
      *(u32x4*)&Qs[row * qp + cv * 8] =
          row < nqr ? *(const u32x4*)(Q + (q0 + row) * D + cv * 8) : (u32x4){0u, 0u, 0u, 0u};
    }
  }
  const int nk = D / P::KT;
  const int col = wn * 32 + c;
  typename P::Regs regs, buf[NK > 0 ? NK : 1];
  const int nv0 = (int)min((long)MV_TILE, rowE - rowB);
  if constexpr (NK > 0) {
#pragma unroll
    for (int kt = 0; kt < NK; ++kt) P::fetch_all(E, rowB, nv0, D, kt * P::KT, t, buf[kt]);
  } else {
    P::fetch(Q, q0, nqr, E, rowB, nv0, D, 0, t, regs);
  }
  bool open = false;                                         // the previous tile's last document goes on in this one
  for (long n0 = rowB; n0 < rowE; n0 += MV_TILE) {
    const int nv = (int)min((long)MV_TILE, rowE - n0);       // doc rows of this tile
    const int nvn = (int)max(0l, min((long)MV_TILE, rowE - n0 - MV_TILE));   // and of the next: 0 rows read as zero
    if (t <= MV_TILE) docid[t] = n0 + t < rowE ? row_doc[n0 + t] : -1;     // a chunk ends where a document ends
    auto segments = [&]() {                                  // the tile's segments: column -> segment, segment -> doc
      if (wave == 0) {
        const bool starts = t > 0 && docid[t] != docid[t - 1];
        const unsigned long long m = __ballot(starts);
        const int sg = __popcll(m & ((2ull << t) - 1ull));
        segof[t] = sg;
        if (t == 0 || starts) sdoc[sg] = docid[t];
      }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if constexpr (NK > 0) {
      bf16x8 a[2][P::KT / 16], b[2][P::KT / 16];
      P::put(t, buf[0], stage[0]);
      const long fn0 = nvn > 0 ? n0 + MV_TILE : n0;          // no next tile: this one again, never used
      const int fnv = nvn > 0 ? nvn : nv;
      P::fetch_all(E, fn0, fnv, D, 0, t, buf[0]);
      __syncthreads();
      segments();
      P::load_a(Qs, qp, 0, wm, c, h, a[0]);
      P::load_b(stage[0], wn, c, h, b[0]);
#pragma unroll
      for (int kt = 0; kt < NK; ++kt) {                      // k ascending, the same steps for every tile
        if (kt + 1 < NK) {                                   // slice kt + 1: stage, barrier, LDS reads in flight ...
          P::put(t, buf[kt + 1], stage[(kt + 1) & 1]);
          P::fetch_all(E, fn0, fnv, D, (kt + 1) * P::KT, t, buf[kt + 1]);
          __syncthreads();
          P::load_a(Qs, qp, (kt + 1) * P::KT, wm, c, h, a[(kt + 1) & 1]);
          P::load_b(stage[(kt + 1) & 1], wn, c, h, b[(kt + 1) & 1]);
        }
        P::mma_ab(a[kt & 1], b[kt & 1], acc);                // ... behind the MFMAs of slice kt
      }
      __syncthreads();                                       // the stage is read out: the epilogue may use its memory
    } else {
      P::put(t, regs, stage[0]);
      __syncthreads();
      segments();
      for (int kt = 0; kt < nk; ++kt) {                      // k ascending, the same steps for every tile
        const int cur = kt & 1;
        if (kt + 1 < nk) P::fetch(Q, q0, nqr, E, n0, nv, D, (kt + 1) * P::KT, t, regs);
        P::mma(Qs, qp, kt * P::KT, stage[cur], wm, wn, c, h, acc);
        if (kt + 1 < nk) P::put(t, regs, stage[cur ^ 1]);
        __syncthreads();
      }
      if (nvn > 0)                                           // the next tile's first slice flies during the epilogue
        P::fetch(Q, q0, nqr, E, n0 + MV_TILE, nvn, D, 0, t, regs);
    }
    // acc[r] = S(query row 32 wm + (r & 3) + 8 (r >> 2) + 4 h, doc row n0 + col): segmented max-scan along col, by doc
    const int my = docid[col];
    const bool valid = col < nv;
    unsigned same = 0u;                                      // bit s: lane c - 2^s holds a column of the same document
#pragma unroll
    for (int s = 0; s < 5; ++s)
      if (c >= (1 << s) && docid[col - (1 << s)] == my) same |= 1u << s;
    const bool ends = valid && (c == 31 || docid[col + 1] != my);          // last column of its segment in this wave
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float x = valid ? acc[r] : -INFINITY;
#pragma unroll
      for (int s = 0; s < 5; ++s) {
        const float y = __shfl_up(x, 1u << s, 32);
        if ((same >> s) & 1u) x = fmaxf(x, y);
      }
      v[r] = x;
    }
    // the stage is idle (the K loop ended on a barrier): M[segment][query row]
    if (wn == 0 && ends) {
      const int sg = segof[col];
#pragma unroll
      for (int r = 0; r < 16; ++r) M[sg][wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = v[r];
    }
    __syncthreads();
    if (wn == 1 && ends) {                                   // the segment of column 31 may go on behind it: join
      const int sg = segof[col];
      const bool join = sg == segof[31];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float* p = &M[sg][wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
        *p = join ? fmaxf(v[r], *p) : v[r];
      }
    }
    __syncthreads();
    const int nseg = segof[nv - 1] + 1;
    const bool last_ends = docid[nv] != docid[nv - 1];
    if (t < MV_TILE) {
      if (open) M[0][t] = fmaxf(M[0][t], carry[t]);
      if (!last_ends) carry[t] = M[nseg - 1][t];
    }
    __syncthreads();
    const int nend = nseg - (last_ends ? 0 : 1);             // the documents that end in this tile
    for (int item = t; item < nend * nsl; item += MV_THREADS) {
      const int sg = item / nsl, j = item - sg * nsl;
      const int pk = sl[j], r0 = slot_row(pk), n = slot_rows(pk);
      float x = slot_raw(pk) ? M[sg][r0] : 0.f + M[sg][r0];  // ascending rows: the pair kernel's fold
      for (int i = 1; i < n; ++i) x += M[sg][r0 + i];
      part[((long)sdoc[sg] - g0) * nslots + s0 + j] = x;
    }
    open = !last_ends;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ selection
__global__ __launch_bounds__(SR_THREADS) void mv_select_kernel(
    const float* __restrict__ part, const int32_t* __restrict__ slots, const int32_t* __restrict__ q_slot,
    const int64_t* __restrict__ q_ptr, const int64_t* __restrict__ doc_ptr, int32_t nd, int32_t nslots, int32_t chunk,
    int32_t c_first, int32_t nch, const int64_t* __restrict__ ex_ptr, const int32_t* __restrict__ ex_doc, int32_t hi,
    unsigned long long* __restrict__ cand, int32_t* __restrict__ ccount) {
  __shared__ SelectSmem S;
  __shared__ uint32_t keys[MV_CHUNK_MAX];
  const int tid = threadIdx.x, q = blockIdx.x, cg = blockIdx.y;
  const long c0 = ((long)c_first + cg) * chunk;
  const int n = (int)max(0l, min((long)chunk, (long)nd - c0));
  const int a = q_slot[q], b = q_slot[q + 1];
  const float lq = (float)(q_ptr[q + 1] - q_ptr[q]);
  const int64_t e0 = ex_ptr ? ex_ptr[q] : 0, e1 = ex_ptr ? ex_ptr[q + 1] : 0;
  for (int i = tid; i < n; i += SR_THREADS) {
    const long d = c0 + i;
    uint32_t key = 0u;                                       // a document without rows, or an excluded one: no entry
    bool ok = doc_ptr[d + 1] > doc_ptr[d];
    if (ok && e1 > e0) {
      const int64_t p = lower_bound(ex_doc, e0, e1, (int32_t)d);
      ok = !(p < e1 && ex_doc[p] == (int32_t)d);
    }
    if (ok) {
      const float* v = part + ((long)cg * chunk + i) * nslots;
      float run = v[a], total = 0.f;                         // slot a begins the query's first run
      bool have = false;
      for (int s = a + 1; s < b; ++s) {
        if (slot_raw(slots[s])) {
          run += v[s];                                       // the run's chain goes on
        } else {
          total = have ? total + run : run;                  // run sums in ascending order
          have = true;
          run = v[s];
        }
      }
      total = have ? total + run : run;
      key = dense_key(total / lq);
    }
    keys[i] = key;
  }
  __syncthreads();
  const size_t list = (size_t)q * (size_t)nch + (size_t)(c_first + cg);
  select_chunk([&](long i) -> uint32_t { return keys[i]; }, (int)c0, n, hi, S, cand + list * (size_t)hi, ccount + list);
}

__global__ __launch_bounds__(SR_THREADS) void mv_merge_kernel(const unsigned long long* __restrict__ cand,
                                                              const int32_t* __restrict__ ccount, int32_t nch, int32_t lo,
                                                              int32_t hi, int32_t* __restrict__ out_doc,
                                                              float* __restrict__ out_score,
                                                              int32_t* __restrict__ out_found) {
  __shared__ SelectSmem S;
  const int q = blockIdx.x;
  const long base = (long)q * nch;
  const RankLists lists = {cand + (size_t)base * (size_t)hi, ccount + base, hi, hi};
  merge_lists<dense_unkey>(lists, nch, S, q, lo, hi, out_doc, out_score, out_found);
}

// ------------------------------------------------------------------------------------------------ host
// ptr [n + 1] ascends from 0 and ends within `rows`; need_rows: every sequence has at least one
inline bool mv_ptr_ok(const int64_t* ptr, int32_t n, int64_t rows, bool need_rows) {
  if (!ptr || ptr[0] != 0) return false;
  for (int32_t s = 0; s < n; ++s)
    if (ptr[s + 1] < ptr[s] + (need_rows ? 1 : 0)) return false;
  return ptr[n] <= rows;
}

inline bool mv_bad_shape(int32_t nq, int32_t nd, int64_t drows, int32_t lo, int32_t hi, int32_t chunk_docs) {
  return nq < 0 || nd < 0 || drows < 0 || lo < 0 || hi <= lo || hi > SR_KMAX ||
         (chunk_docs != 0 && (chunk_docs < MV_CHUNK_MIN || chunk_docs > MV_CHUNK_MAX));
}

// the slots of the call: per run one, plus one per row of the run that lies behind a block edge (mv_slot_at's count)
inline int64_t mv_count_slots(const int64_t* q_ptr, int32_t nq) {
  int64_t n = 0;
  for (int32_t q = 0; q < nq; ++q)
    for (int64_t run0 = q_ptr[q]; run0 < q_ptr[q + 1]; run0 += MV_TILE) {
      const int64_t run1 = run0 + MV_TILE < q_ptr[q + 1] ? run0 + MV_TILE : q_ptr[q + 1];
      const int64_t edge = (run0 / MV_TILE + 1) * MV_TILE;
      n += 1 + (run1 > edge ? run1 - edge : 0);
    }
  return n;
}

// the call's workspace: device copies of the pointers, the slot tables, the row-to-document map, the partial sums of one
// chunk group, the candidate lists
struct MvPlan {
  size_t dptr, qptr, qslot, bslot, bcnt, slots, rowdoc, part, cand, ccount, total;
  int chunk, nch, group, nqb;
  int64_t nslots;
  bool ok;
  MvPlan(const int64_t* q_ptr, int32_t nq, int32_t nd, int64_t drows, int32_t hi, int32_t chunk_docs) {
    chunk = chunk_docs > 0 ? chunk_docs : MV_CHUNK_DEFAULT;
    nch = sr_nch(nd, chunk);
    const int64_t qused = q_ptr[nq];
    nslots = mv_count_slots(q_ptr, nq);
    ok = qused <= 0x7FFFFFFFL - MV_TILE && (int64_t)nq * nch <= 0x7FFFFFFFL;
    nqb = ok ? (int)((qused + MV_TILE - 1) / MV_TILE) : 1;
    const size_t per_chunk = (size_t)chunk * (size_t)nslots * 4;
    long g = (MV_WG_TARGET + (long)nqb - 1) / nqb;
    if ((size_t)g * per_chunk > MV_PART_BUDGET) g = (long)(MV_PART_BUDGET / (per_chunk ? per_chunk : 1));
    group = (int)(g < 1 ? 1 : (g > nch ? nch : (g > 65535 ? 65535 : g)));
    ok = ok && (long)nqb * group <= 0x7FFFFFFFL;
    Arena a;
    dptr = a.take(((size_t)nd + 1) * 8);
    qptr = a.take(((size_t)nq + 1) * 8);
    qslot = a.take(((size_t)nq + 1) * 4);
    bslot = a.take(((size_t)nqb + 1) * 4);
    bcnt = a.take((size_t)nqb * 4);
    slots = a.take((size_t)nslots * 4);
    rowdoc = a.take((size_t)drows * 4);
    part = a.take((size_t)group * per_chunk);
    cand = a.take((size_t)nq * (size_t)nch * (size_t)hi * 8);
    ccount = a.take((size_t)nq * (size_t)nch * 4);
    total = a.off;
  }
};

LdsOptIn g_mv_lds[2];

int mv_search(const void* docs, const void* q, int32_t mv_f32, int32_t D, int64_t drows, const int64_t* doc_ptr, int32_t nd,
              int64_t qrows, const int64_t* q_ptr, int32_t nq, const int64_t* ex_ptr, const int32_t* ex_doc, int32_t lo,
              int32_t hi, int32_t chunk_docs, int32_t* out_doc, float* out_score, int32_t* out_found, void* workspace,
              size_t ws_bytes, hipStream_t st) {
  if (D <= 0 || (D % 64) != 0 || D > MV_DMAX || qrows < 0 || mv_bad_shape(nq, nd, drows, lo, hi, chunk_docs))
    return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  if (!q || !out_doc || !out_score || !workspace || (ex_ptr && !ex_doc) || ((uintptr_t)q & 15) != 0 ||
      ((uintptr_t)docs & 15) != 0 || ((uintptr_t)workspace & 15) != 0)
    return SNX_E_ARG;
  // the two pointer arrays are pageable host memory (snx.h): everything a kernel will trust is checked here, before any
  // launch; hipMemcpyAsync below has staged them when it returns
  if (!mv_ptr_ok(doc_ptr, nd, drows, false) || !mv_ptr_ok(q_ptr, nq, qrows, true)) return SNX_E_ARG;
  const int64_t dused = doc_ptr[nd], qused = q_ptr[nq];
  if (dused > 0 && !docs) return SNX_E_ARG;
  const MvPlan plan(q_ptr, nq, nd, drows, hi, chunk_docs);
  if (!plan.ok) return SNX_E_SHAPE;
  if (ws_bytes < plan.total) return SNX_E_ARG;
  char* ws = (char*)workspace;
  const struct { size_t off; const void* src; size_t bytes; } up[2] = {{plan.dptr, doc_ptr, ((size_t)nd + 1) * 8},
                                                                       {plan.qptr, q_ptr, ((size_t)nq + 1) * 8}};
  for (const auto& u : up) {
    const hipError_t e = hipMemcpyAsync(ws + u.off, u.src, u.bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return (int)e;
  }
  const int64_t* dptr = (const int64_t*)(ws + plan.dptr);
  const int64_t* qptr = (const int64_t*)(ws + plan.qptr);
  int32_t *qslot = (int32_t*)(ws + plan.qslot), *bslot = (int32_t*)(ws + plan.bslot), *bcnt = (int32_t*)(ws + plan.bcnt);
  int32_t *slots = (int32_t*)(ws + plan.slots), *rowdoc = (int32_t*)(ws + plan.rowdoc), *ccount = (int32_t*)(ws + plan.ccount);
  float* part = (float*)(ws + plan.part);
  unsigned long long* cand = (unsigned long long*)(ws + plan.cand);
  const int nslots = (int)plan.nslots;
  for (int write = 0; write < 2; ++write) {
    hipLaunchKernelGGL(mv_slots_kernel, dim3(plan.nqb), dim3(MV_TILE), 0, st, qptr, nq, qused, plan.nqb, write, bcnt,
                       (const int32_t*)bslot, slots, qslot);
    SNX_CHECK_LAUNCH();
    if (!write) {
      hipLaunchKernelGGL(mv_slot_scan_kernel, dim3(1), dim3(64), 0, st, (const int32_t*)bcnt, plan.nqb, bslot);
      SNX_CHECK_LAUNCH();
    }
  }
  if (dused > 0) {
    hipLaunchKernelGGL(mv_rowdoc_kernel, dim3((unsigned)((dused + MV_THREADS - 1) / MV_THREADS)), dim3(MV_THREADS), 0, st,
                       dptr, nd, dused, rowdoc);
    SNX_CHECK_LAUNCH();
  }
  const int lds = mv_f32 ? mv_lds_bytes<MvF32>(D) : mv_lds_bytes<MvBf16>(D);
  const bool deep = !mv_f32 && D == MV_DMAX;                  // the whole next tile in registers (mv_score_kernel)
  if (!mv_f32) {
    const void* kern = deep ? (const void*)mv_score_kernel<MvBf16, MV_DMAX / MvBf16::KT> : (const void*)mv_score_kernel<MvBf16, 0>;
    if (const int rc = g_mv_lds[deep ? 1 : 0].ensure(kern, mv_lds_bytes<MvBf16>(MV_DMAX))) return rc;
  }
  for (int c = 0; c < plan.nch; c += plan.group) {           // one chunk group after the other: part is reused in order
    const int g = plan.nch - c < plan.group ? plan.nch - c : plan.group;
    if (dused > 0) {
      const dim3 grid((unsigned)((long)plan.nqb * g));       // query block fast, chunk slow
      if (mv_f32)
        hipLaunchKernelGGL((mv_score_kernel<MvF32, 0>), grid, dim3(MV_THREADS), lds, st, (const float*)docs, (const float*)q, D,
                           qused, dptr, (const int32_t*)rowdoc, nd, plan.nqb, (const int32_t*)bslot,
                           (const int32_t*)slots, nslots, plan.chunk, c, part);
      else if (deep)
        hipLaunchKernelGGL((mv_score_kernel<MvBf16, MV_DMAX / MvBf16::KT>), grid, dim3(MV_THREADS), lds, st,
                           (const bf16_t*)docs, (const bf16_t*)q, D, qused, dptr, (const int32_t*)rowdoc, nd, plan.nqb,
                           (const int32_t*)bslot, (const int32_t*)slots, nslots, plan.chunk, c, part);
      else
        hipLaunchKernelGGL((mv_score_kernel<MvBf16, 0>), grid, dim3(MV_THREADS), lds, st, (const bf16_t*)docs,
                           (const bf16_t*)q, D, qused, dptr, (const int32_t*)rowdoc, nd, plan.nqb, (const int32_t*)bslot,
                           (const int32_t*)slots, nslots, plan.chunk, c, part);
      SNX_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(mv_select_kernel, dim3(nq, g), dim3(SR_THREADS), 0, st, (const float*)part, (const int32_t*)slots,
                       (const int32_t*)qslot, qptr, dptr, nd, nslots, plan.chunk, c, plan.nch, ex_ptr, ex_doc, hi, cand,
                       ccount);
    SNX_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(mv_merge_kernel, dim3(nq), dim3(SR_THREADS), 0, st, (const unsigned long long*)cand,
                     (const int32_t*)ccount, plan.nch, lo, hi, out_doc, out_score, out_found);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

}  // namespace

extern "C" size_t snx_mv_search_workspace_bytes(const int64_t* q_ptr, int32_t nq, int32_t nd, int64_t drows, int32_t hi,
                                                int32_t chunk_docs) {
  if (nq <= 0 || mv_bad_shape(nq, nd, drows, 0, hi, chunk_docs) || !mv_ptr_ok(q_ptr, nq, 0x7FFFFFFFFFFFFFFFL, true)) return 0;
  const MvPlan plan(q_ptr, nq, nd, drows, hi, chunk_docs);
  return plan.ok ? plan.total : 0;
}

extern "C" int snx_mv_search(const void* docs, const void* q, int32_t mv_f32, int32_t D, int64_t drows,
                             const int64_t* doc_ptr, int32_t nd, int64_t qrows, const int64_t* q_ptr, int32_t nq, int32_t k,
                             int32_t chunk_docs, int32_t* out_doc, float* out_score, void* workspace, size_t ws_bytes,
                             hipStream_t st) {
  return mv_search(docs, q, mv_f32, D, drows, doc_ptr, nd, qrows, q_ptr, nq, nullptr, nullptr, 0, k, chunk_docs, out_doc,
                   out_score, nullptr, workspace, ws_bytes, st);
}

extern "C" int snx_mv_search_band(const void* docs, const void* q, int32_t mv_f32, int32_t D, int64_t drows,
                                  const int64_t* doc_ptr, int32_t nd, int64_t qrows, const int64_t* q_ptr, int32_t nq,
                                  const int64_t* ex_ptr, const int32_t* ex_doc, int32_t lo, int32_t hi, int32_t chunk_docs,
                                  int32_t* out_doc, float* out_score, int32_t* out_found, void* workspace, size_t ws_bytes,
                                  hipStream_t st) {
  if (!out_found) return SNX_E_ARG;
  return mv_search(docs, q, mv_f32, D, drows, doc_ptr, nd, qrows, q_ptr, nq, ex_ptr, ex_doc, lo, hi, chunk_docs, out_doc,
                   out_score, out_found, workspace, ws_bytes, st);
}
