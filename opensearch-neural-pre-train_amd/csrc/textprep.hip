// Corpus preparation (include/snx.h "Corpus preparation"): the paragraph segmentation, the SHA-256 of rows and the
// first-occurrence dedup of the reference's MLM data script, over rows of code points.  Integer work only; every output is
// a pure function of the inputs.
//
//   tx_segment_kernel<MODE>  one workgroup per document, walking tiles of TX_TILE code points, a thread per code point.
//                            A code point's blank and separator tests read its neighbours in the document (one back, one
//                            ahead), so they hold across a tile edge by construction.  The piece state is carried from tile
//                            to tile in LDS: position of the last separator and of the last code point that is not white
//                            space, the running counts of emitted code points and of Hangul, the number of pieces begun, and
//                            the counts at the current piece's first and last code point that is not white space.  Inside a
//                            tile the same quantities are workgroup scans (max for the positions, sum for the counts).
//                            A piece is CLOSED by the thread on a separator that has a non-white-space code point since the
//                            separator before it, and by thread 0 at the document's end.
//                            MODE TX_COUNT: pieces and code points of the document.  TX_META: length, document and Hangul
//                            count of every piece, at piece_base[doc] + k.  TX_FILL: the code points; a code point is
//                            written iff a non-white-space code point of its piece stands at or before it and its offset is
//                            below the piece's length (par_ptr), which leaves the trailing white space out.
//   tx_sha256_kernel         one lane per row.  The lane encodes UTF-8 byte by byte into a big-endian word, stores every
//                            fourth byte's word into its 16-word column of LDS and compresses every 64th byte; padding and
//                            the 64-bit bit count go through the same byte path.
//   tx_claim_kernel          a thread per row: linear probing from a hash of all eight words; atomicCAS(-1 -> row) claims a
//                            free slot; a slot whose row has the same digest (all eight words, read from the digest array)
//                            is this row's slot, lowered by atomicMin.  A slot only ever holds rows of one digest, so the
//                            comparison through it is valid at any time.
//   tx_first_kernel          first[i] = the slot's minimum.
#include "sparse_common.h"
#include "snx.h"

namespace {

constexpr int TX_THREADS = 256;
constexpr int TX_TILE = TX_THREADS;      // code points of one tile (snx.textprep.TILE mirrors it)
constexpr int TX_WAVES = TX_THREADS / 64;
constexpr int TX_COUNT = 0, TX_META = 1, TX_FILL = 2;
constexpr int TX_SHA_THREADS = 64;
constexpr int TX_DEDUP_THREADS = 256;

__device__ __forceinline__ bool tx_blank(int32_t c) { return c == 0x20 || c == 0x09; }

// Python's str.isspace over all of Unicode
__device__ __forceinline__ bool tx_space(int32_t c) {
  return (c >= 0x09 && c <= 0x0D) || (c >= 0x1C && c <= 0x20) || c == 0x85 || c == 0xA0 || c == 0x1680 ||
         (c >= 0x2000 && c <= 0x200A) || c == 0x2028 || c == 0x2029 || c == 0x202F || c == 0x205F || c == 0x3000;
}

__device__ __forceinline__ bool tx_hangul(int32_t c) { return c >= 0xAC00 && c <= 0xD7AF; }

// four scans at once: fields a and b by max, c and d by sum
struct TxQ {
  int a, b, c, d;
};

__device__ __forceinline__ TxQ tx_join(TxQ lo, TxQ hi) {
  return TxQ{max(lo.a, hi.a), max(lo.b, hi.b), lo.c + hi.c, lo.d + hi.d};
}

// inclusive scan over the workgroup; wtot is LDS [TX_WAVES], free again on return
__device__ __forceinline__ TxQ tx_scan(TxQ v, TxQ* wtot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    TxQ o{__shfl_up(v.a, d, 64), __shfl_up(v.b, d, 64), __shfl_up(v.c, d, 64), __shfl_up(v.d, d, 64)};
    if (lane >= d) v = tx_join(o, v);
  }
  if (lane == 63) wtot[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v = tx_join(wtot[w], v);
  __syncthreads();
  return v;
}

// the state a tile hands to the next one; positions are indices into the document, -1 = none yet
struct TxCarry {
  int ls;        // last separator code point
  int ln;        // last code point that is not white space
  int fi;        // first non-white-space code point of the piece begun last
  int E, H;      // emitted code points / Hangul so far (inclusive)
  int np;        // pieces begun so far
  int e_first;   // E at fi
  int hx_first;  // H in front of fi
  int e_last;    // E at ln
  int h_last;    // H at ln
};

template <int MODE>
__global__ __launch_bounds__(TX_THREADS) void tx_segment_kernel(const int64_t* __restrict__ ptr,
                                                                const int32_t* __restrict__ cps,
                                                                const int64_t* __restrict__ piece_base,
                                                                const int64_t* __restrict__ par_ptr,
                                                                int64_t* __restrict__ out_a,     // doc_pieces | par_len
                                                                int64_t* __restrict__ out_b,     // doc_cps
                                                                int32_t* __restrict__ par_doc,
                                                                int32_t* __restrict__ par_hangul,
                                                                int32_t* __restrict__ par_cps) {
  __shared__ TxQ wtot[TX_WAVES];
  __shared__ TxCarry carry;
  __shared__ int sE[TX_TILE], sH[TX_TILE], sHx[TX_TILE];
  __shared__ unsigned long long total;
  const int tid = threadIdx.x;
  const int64_t doc = blockIdx.x;
  const int64_t a0 = ptr[doc];
  const int len = (int)(ptr[doc + 1] - a0);
  const int64_t pb = MODE == TX_COUNT ? 0 : piece_base[doc];
  if (tid == 0) {
    carry = TxCarry{-1, -1, -1, 0, 0, 0, 0, 0, 0, 0};
    total = 0;
  }
  __syncthreads();
  int64_t my_cps = 0;                                        // TX_COUNT: code points of the pieces this thread closed

  auto close = [&](int piece, int n_cps, int n_hangul) {     // piece: its number in the document
    if (MODE == TX_COUNT) my_cps += n_cps;
    if (MODE == TX_META) {
      out_a[pb + piece] = n_cps;
      par_doc[pb + piece] = (int32_t)doc;
      par_hangul[pb + piece] = n_hangul;
    }
  };

  for (int base = 0; base < len; base += TX_TILE) {          // block-uniform bounds
    const TxCarry C = carry;
    const int i = base + tid;
    const bool in = i < len;
    const int32_t c = in ? cps[a0 + i] : 0;
    const int32_t prev = in && i > 0 ? cps[a0 + i - 1] : 0;  // 0 is neither a blank nor U+000A
    const int32_t next = in && i + 1 < len ? cps[a0 + i + 1] : 0;
    const bool sep = in && c == 0x0A && (prev == 0x0A || next == 0x0A);
    const bool emit = in && !sep && !(tx_blank(c) && tx_blank(prev));
    const bool nonws = in && !sep && !tx_space(c);
    const bool han = in && tx_hangul(c);                     // Hangul is not white space: han implies nonws
    const TxQ s1 = tx_scan(TxQ{sep ? i : -1, nonws ? i : -1, emit ? 1 : 0, han ? 1 : 0}, wtot);
    // exclusive positions: what stands in front of i
    const int ls_up = __shfl_up(s1.a, 1, 64), ln_up = __shfl_up(s1.b, 1, 64);
    sE[tid] = s1.a;                                          // borrowed for the wave edges
    sH[tid] = s1.b;
    __syncthreads();
    const int lsx = max(C.ls, tid == 0 ? -1 : ((tid & 63) ? ls_up : sE[tid - 1]));
    const int lnx = max(C.ln, tid == 0 ? -1 : ((tid & 63) ? ln_up : sH[tid - 1]));
    __syncthreads();
    const int E = C.E + s1.c, H = C.H + s1.d;
    sE[tid] = E;
    sH[tid] = H;
    sHx[tid] = H - (han ? 1 : 0);
    const bool first = nonws && lnx <= lsx;                  // no non-white-space code point since the last separator
    const TxQ s2 = tx_scan(TxQ{first ? i : -1, -1, first ? 1 : 0, 0}, wtot);   // its syncs publish sE, sH, sHx
    const int fi = max(C.fi, s2.a);                          // first code point of the piece begun last, at or before i
    const int np = C.np + s2.c;
    const int e_first = fi >= base ? sE[fi - base] : C.e_first;
    const int hx_first = fi >= base ? sHx[fi - base] : C.hx_first;
    if (sep && lnx > lsx) {                                  // this separator ends a piece with text
      const int e_last = lnx >= base ? sE[lnx - base] : C.e_last;
      const int h_last = lnx >= base ? sH[lnx - base] : C.h_last;
      close(np - 1, e_last - e_first + 1, h_last - hx_first);
    }
    if (MODE == TX_FILL && emit && (nonws || lnx > lsx)) {   // at or behind the piece's first code point
      const int64_t p = pb + np - 1;
      const int64_t o0 = par_ptr[p];
      const int off = E - e_first;
      if (off < par_ptr[p + 1] - o0) par_cps[o0 + off] = tx_blank(c) ? 0x20 : c;
    }
    if (tid == TX_THREADS - 1) {                             // inclusive values of the tile's last place
      const int ln = nonws ? i : lnx;
      TxCarry N;
      N.ls = sep ? i : lsx;
      N.ln = ln;
      N.fi = fi;
      N.E = E;
      N.H = H;
      N.np = np;
      N.e_first = e_first;
      N.hx_first = hx_first;
      N.e_last = ln >= base ? sE[ln - base] : C.e_last;
      N.h_last = ln >= base ? sH[ln - base] : C.h_last;
      carry = N;
    }
    __syncthreads();
  }
  const TxCarry C = carry;
  if (tid == 0 && C.ln > C.ls) close(C.np - 1, C.e_last - C.e_first + 1, C.h_last - C.hx_first);   // the document's end
  if (MODE == TX_COUNT) {
    if (my_cps) atomicAdd(&total, (unsigned long long)my_cps);   // integer: the order does not show
    __syncthreads();
    if (tid == 0) {
      out_a[doc] = C.np;
      out_b[doc] = (int64_t)total;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ SHA-256
__device__ __forceinline__ uint32_t tx_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

__constant__ uint32_t TX_K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
    0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
    0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
    0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

struct TxSha {
  uint32_t h[8];
  uint32_t cur;        // the bytes of the word being filled, big-endian
  uint64_t nbytes;     // bytes pushed so far
};

// one block from the lane's column of W (LDS [16][TX_SHA_THREADS])
__device__ __forceinline__ void tx_compress(TxSha& S, uint32_t (*W)[TX_SHA_THREADS], int lane) {
  uint32_t w[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) w[j] = W[j][lane];
  uint32_t a = S.h[0], b = S.h[1], c = S.h[2], d = S.h[3], e = S.h[4], f = S.h[5], g = S.h[6], h = S.h[7];
#pragma unroll
  for (int r = 0; r < 64; ++r) {
    if (r >= 16) {
      const uint32_t w15 = w[(r + 1) & 15], w2 = w[(r + 14) & 15];
      const uint32_t s0 = tx_rotr(w15, 7) ^ tx_rotr(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = tx_rotr(w2, 17) ^ tx_rotr(w2, 19) ^ (w2 >> 10);
      w[r & 15] = w[r & 15] + s0 + w[(r + 9) & 15] + s1;
    }
    const uint32_t S1 = tx_rotr(e, 6) ^ tx_rotr(e, 11) ^ tx_rotr(e, 25);
    const uint32_t ch = (e & f) ^ (~e & g);
    const uint32_t t1 = h + S1 + ch + TX_K[r] + w[r & 15];
    const uint32_t S0 = tx_rotr(a, 2) ^ tx_rotr(a, 13) ^ tx_rotr(a, 22);
    const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
    const uint32_t t2 = S0 + mj;
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  S.h[0] += a; S.h[1] += b; S.h[2] += c; S.h[3] += d; S.h[4] += e; S.h[5] += f; S.h[6] += g; S.h[7] += h;
}

__device__ __forceinline__ void tx_push(TxSha& S, uint32_t byte, uint32_t (*W)[TX_SHA_THREADS], int lane) {
  S.cur = (S.cur << 8) | byte;
  ++S.nbytes;
  if ((S.nbytes & 3) == 0) {
    W[((S.nbytes - 1) >> 2) & 15][lane] = S.cur;             // the lane's own column: no other lane reads it
    if ((S.nbytes & 63) == 0) tx_compress(S, W, lane);
  }
}

__global__ __launch_bounds__(TX_SHA_THREADS) void tx_sha256_kernel(const int64_t* __restrict__ ptr,
                                                                   const int32_t* __restrict__ cps, int32_t n,
                                                                   uint32_t* __restrict__ digest) {
  __shared__ uint32_t W[16][TX_SHA_THREADS];
  const int lane = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * TX_SHA_THREADS + lane;
  if (row >= n) return;                                      // no workgroup barrier below
  TxSha S{{0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19}, 0, 0};
  const int64_t a0 = ptr[row], a1 = ptr[row + 1];
  for (int64_t i = a0; i < a1; ++i) {
    const uint32_t c = (uint32_t)cps[i];
    if (c < 0x80) {
      tx_push(S, c, W, lane);
    } else if (c < 0x800) {
      tx_push(S, 0xC0 | (c >> 6), W, lane);
      tx_push(S, 0x80 | (c & 0x3F), W, lane);
    } else if (c < 0x10000) {
      tx_push(S, 0xE0 | (c >> 12), W, lane);
      tx_push(S, 0x80 | ((c >> 6) & 0x3F), W, lane);
      tx_push(S, 0x80 | (c & 0x3F), W, lane);
    } else {
      tx_push(S, 0xF0 | ((c >> 18) & 0x07), W, lane);
      tx_push(S, 0x80 | ((c >> 12) & 0x3F), W, lane);
      tx_push(S, 0x80 | ((c >> 6) & 0x3F), W, lane);
      tx_push(S, 0x80 | (c & 0x3F), W, lane);
    }
  }
  const uint64_t bits = S.nbytes * 8;
  tx_push(S, 0x80, W, lane);
  while ((S.nbytes & 63) != 56) tx_push(S, 0, W, lane);
#pragma unroll 1
  for (int s = 56; s >= 0; s -= 8) tx_push(S, (uint32_t)(bits >> s) & 0xFF, W, lane);   // the last push compresses
#pragma unroll
  for (int j = 0; j < 8; ++j) digest[row * 8 + j] = S.h[j];
}

// -------------------------------------------------------------------------------------------- first-occurrence dedup
__device__ __forceinline__ uint32_t tx_slot_hash(const uint32_t* __restrict__ d) {
  uint32_t h = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) h = (h ^ d[j]) * 0x9E3779B1u + 0x7F4A7C15u;
  h ^= h >> 16;
  h *= 0x7FEB352Du;
  h ^= h >> 15;
  h *= 0x846CA68Bu;
  h ^= h >> 16;
  return h;
}

__global__ __launch_bounds__(TX_DEDUP_THREADS) void tx_claim_kernel(const uint32_t* __restrict__ digest, int32_t n,
                                                                    int32_t* slots, uint32_t mask,
                                                                    uint32_t* __restrict__ slot_of) {
  const int64_t i = (int64_t)blockIdx.x * TX_DEDUP_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint32_t* mine = digest + i * 8;
  uint32_t s = tx_slot_hash(mine) & mask;
  for (uint32_t step = 0; step <= mask; ++step, s = (s + 1) & mask) {   // at most one round: the table has free slots
    const int32_t seen = atomicCAS(&slots[s], -1, (int32_t)i);
    bool same = seen < 0;
    if (!same) {
      const uint32_t* other = digest + (int64_t)seen * 8;
      same = true;
#pragma unroll
      for (int j = 0; j < 8; ++j) same = same && other[j] == mine[j];
    }
    if (same) {
      if (seen >= 0 && (int32_t)i < seen) atomicMin(&slots[s], (int32_t)i);
      slot_of[i] = s;
      return;
    }
  }
  slot_of[i] = 0xFFFFFFFFu;                                  // unreachable with n <= slots / 2
}

__global__ __launch_bounds__(TX_DEDUP_THREADS) void tx_first_kernel(const int32_t* __restrict__ slots,
                                                                    const uint32_t* __restrict__ slot_of, int32_t n,
                                                                    uint32_t mask, int32_t* __restrict__ first) {
  const int64_t i = (int64_t)blockIdx.x * TX_DEDUP_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = slot_of[i];
  first[i] = s <= mask ? slots[s] : (int32_t)i;
}

constexpr int64_t TX_DEDUP_MAX = 1ll << 29;

inline int64_t tx_slots(int64_t n) {
  int64_t m = 64;
  while (m < 2 * n) m <<= 1;
  return m;
}

template <int MODE>
int tx_segment(const int64_t* ptr, const int32_t* cps, int32_t n, const int64_t* piece_base, const int64_t* par_ptr,
               int64_t* out_a, int64_t* out_b, int32_t* par_doc, int32_t* par_hangul, int32_t* par_cps, hipStream_t st) {
  hipLaunchKernelGGL(tx_segment_kernel<MODE>, dim3((unsigned)n), dim3(TX_THREADS), 0, st, ptr, cps, piece_base, par_ptr,
                     out_a, out_b, par_doc, par_hangul, par_cps);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

}  // namespace

extern "C" int snx_tx_segment_count(const int64_t* ptr, const int32_t* code_points, int32_t n, int64_t* doc_pieces,
                                    int64_t* doc_cps, hipStream_t st) {
  if (n < 0) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!ptr || !doc_pieces || !doc_cps) return SNX_E_ARG;       // code_points may be NULL when every document is empty
  return tx_segment<TX_COUNT>(ptr, code_points, n, nullptr, nullptr, doc_pieces, doc_cps, nullptr, nullptr, nullptr, st);
}

extern "C" int snx_tx_segment_meta(const int64_t* ptr, const int32_t* code_points, int32_t n, const int64_t* piece_base,
                                   int64_t* par_len, int32_t* par_doc, int32_t* par_hangul, hipStream_t st) {
  if (n < 0) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!ptr || !piece_base || !par_len || !par_doc || !par_hangul) return SNX_E_ARG;
  return tx_segment<TX_META>(ptr, code_points, n, piece_base, nullptr, par_len, nullptr, par_doc, par_hangul, nullptr, st);
}

extern "C" int snx_tx_segment_fill(const int64_t* ptr, const int32_t* code_points, int32_t n, const int64_t* piece_base,
                                   const int64_t* par_ptr, int32_t* par_cps, hipStream_t st) {
  if (n < 0) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!ptr || !piece_base || !par_ptr || !par_cps) return SNX_E_ARG;
  return tx_segment<TX_FILL>(ptr, code_points, n, piece_base, par_ptr, nullptr, nullptr, nullptr, nullptr, par_cps, st);
}

extern "C" int snx_tx_sha256_rows(const int64_t* ptr, const int32_t* code_points, int32_t n, uint32_t* digest,
                                  hipStream_t st) {
  if (n < 0) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!ptr || !digest) return SNX_E_ARG;                       // code_points may be NULL when every row is empty
  hipLaunchKernelGGL(tx_sha256_kernel, dim3((unsigned)cdiv(n, TX_SHA_THREADS)), dim3(TX_SHA_THREADS), 0, st, ptr,
                     code_points, n, digest);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" size_t snx_tx_first_equal_workspace_bytes(int64_t n) {
  if (n <= 0 || n > TX_DEDUP_MAX) return 0;
  return (size_t)((tx_slots(n) + n) * 4);
}

extern "C" int snx_tx_first_equal(const uint32_t* digest, int32_t n, int32_t* first, void* workspace, size_t ws_bytes,
                                  hipStream_t st) {
  if (n < 0 || n > TX_DEDUP_MAX) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!digest || !first || !workspace || ws_bytes < snx_tx_first_equal_workspace_bytes(n)) return SNX_E_ARG;
  const int64_t m = tx_slots(n);
  int32_t* slots = (int32_t*)workspace;
  uint32_t* slot_of = (uint32_t*)(slots + m);
  hipError_t e = hipMemsetAsync(slots, 0xFF, (size_t)m * 4, st);   // -1: free
  if (e != hipSuccess) return (int)e;
  const unsigned grid = (unsigned)cdiv(n, TX_DEDUP_THREADS);
  hipLaunchKernelGGL(tx_claim_kernel, dim3(grid), dim3(TX_DEDUP_THREADS), 0, st, digest, n, slots, (uint32_t)(m - 1),
                     slot_of);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(tx_first_kernel, dim3(grid), dim3(TX_DEDUP_THREADS), 0, st, slots, slot_of, n, (uint32_t)(m - 1),
                     first);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
