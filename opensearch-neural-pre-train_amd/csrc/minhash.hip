// MinHash near-duplicate removal (include/snx.h "MinHash near-duplicate removal"): the reference's MinHashDeduplicator
// (ref:src/preprocessing/cleaners/deduplicator.py:10-187) computes 128 MD5 digests per character n-gram in a Python loop
// and compares every new row with every kept row in a second one.  Both loops are integer work; here they are kernels
// and the answer is the reference's, row for row.
//
//   mh_sig_kernel       one workgroup per row.  64 n-grams at a time are encoded to UTF-8 into LDS slots (one thread per
//                       n-gram, byte stores), with the 0x80 of the MD5 padding behind them.  Then thread (slice, i) hashes
//                       the slice's n-grams under permutation i: the message words are the slot's words shifted behind the
//                       prefix "<i>_" by v_alignbyte, the length goes into word 14, one 64-step MD5, a 128-bit minimum.
//                       All message indices are compile-time: the block stays in registers.  Slices are folded in LDS.
//   mh_stage_kernel     the least significant digest words of a block of MH_B rows, transposed ([perm][row]), and the
//                       block's match state reset.
//   mh_match_kernel     one workgroup per (32 rows of the block, 256 columns).  Columns are the rows KEPT from earlier
//                       blocks (compacted, transposed: coalesced) and then the block's own rows.  A thread owns a column
//                       and counts, for each of the 32 rows (in LDS, broadcast reads), the positions whose low words are
//                       equal; every 32 positions it stops once no row can reach `need` any more.  A count that reaches
//                       `need` is only a candidate: the pair is then compared on all 128 bits, and that count decides.
//                       Kept columns: atomicMin of the kept row's index; own columns: a bit of the block's match matrix.
//   mh_resolve_kernel   one workgroup, the order dependence of one block: one wave walks the rows in order with the
//                       match matrix, the candidates and the exact-key keepers in LDS (a few LDS reads and a ballot per
//                       row); the others then number the kept rows.  No kernel waits for another workgroup.
//   mh_append_kernel    the kept rows' low words join the compacted columns.
//   mh_first_kernel     the incremental form: rows against a plain list of kept signatures, first match per row.
#include "sparse_common.h"
#include "snx.h"

namespace {

constexpr int MH_THREADS = 256;
constexpr int MH_GC = 64;                      // n-grams staged per pass
constexpr int MH_SLOT = 16;                    // words of an n-gram slot: one zero word, then the bytes and their 0x80
constexpr int MH_GRAM_BYTES = SNX_MINHASH_MSG_MAX - 2;   // the shortest prefix is "0_"
constexpr int MH_PERM_MAX = SNX_MINHASH_PERM_MAX;
constexpr int MH_B = 512;                      // rows resolved per block
constexpr int MH_R = 32;                       // rows per workgroup of the match kernel
constexpr int MH_C = 256;                      // columns per workgroup of the match kernel (its threads)
constexpr int MH_W = MH_B / 32;                // words of a row of the match matrix
constexpr int MH_NONE = 0x7fffffff;

// ------------------------------------------------------------------------------------------------ MD5, one block
#define MH_F(x, y, z) ((z) ^ ((x) & ((y) ^ (z))))
#define MH_G(x, y, z) ((y) ^ ((z) & ((x) ^ (y))))
#define MH_H(x, y, z) ((x) ^ (y) ^ (z))
#define MH_I(x, y, z) ((y) ^ ((x) | ~(z)))
#define MH_STEP(f, a, b, c, d, k, s, t)                      \
  do {                                                       \
    (a) += f((b), (c), (d)) + m[k] + (t);                    \
    (a) = (((a) << (s)) | ((a) >> (32 - (s)))) + (b);        \
  } while (0)

struct U128 {
  uint32_t w[4];                               // most significant word first
};

__device__ __forceinline__ bool less128(const U128& x, const U128& y) {
  if (x.w[0] != y.w[0]) return x.w[0] < y.w[0];
  if (x.w[1] != y.w[1]) return x.w[1] < y.w[1];
  if (x.w[2] != y.w[2]) return x.w[2] < y.w[2];
  return x.w[3] < y.w[3];
}

// the digest of the padded block m[0..15], as the integer int(hexdigest, 16): digest bytes big-endian
__device__ __forceinline__ U128 md5_block(const uint32_t (&m)[16]) {
  uint32_t a = 0x67452301u, b = 0xefcdab89u, c = 0x98badcfeu, d = 0x10325476u;
  MH_STEP(MH_F, a, b, c, d, 0, 7, 0xd76aa478u);
  MH_STEP(MH_F, d, a, b, c, 1, 12, 0xe8c7b756u);
  MH_STEP(MH_F, c, d, a, b, 2, 17, 0x242070dbu);
  MH_STEP(MH_F, b, c, d, a, 3, 22, 0xc1bdceeeu);
  MH_STEP(MH_F, a, b, c, d, 4, 7, 0xf57c0fafu);
  MH_STEP(MH_F, d, a, b, c, 5, 12, 0x4787c62au);
  MH_STEP(MH_F, c, d, a, b, 6, 17, 0xa8304613u);
  MH_STEP(MH_F, b, c, d, a, 7, 22, 0xfd469501u);
  MH_STEP(MH_F, a, b, c, d, 8, 7, 0x698098d8u);
  MH_STEP(MH_F, d, a, b, c, 9, 12, 0x8b44f7afu);
  MH_STEP(MH_F, c, d, a, b, 10, 17, 0xffff5bb1u);
  MH_STEP(MH_F, b, c, d, a, 11, 22, 0x895cd7beu);
  MH_STEP(MH_F, a, b, c, d, 12, 7, 0x6b901122u);
  MH_STEP(MH_F, d, a, b, c, 13, 12, 0xfd987193u);
  MH_STEP(MH_F, c, d, a, b, 14, 17, 0xa679438eu);
  MH_STEP(MH_F, b, c, d, a, 15, 22, 0x49b40821u);
  MH_STEP(MH_G, a, b, c, d, 1, 5, 0xf61e2562u);
  MH_STEP(MH_G, d, a, b, c, 6, 9, 0xc040b340u);
  MH_STEP(MH_G, c, d, a, b, 11, 14, 0x265e5a51u);
  MH_STEP(MH_G, b, c, d, a, 0, 20, 0xe9b6c7aau);
  MH_STEP(MH_G, a, b, c, d, 5, 5, 0xd62f105du);
  MH_STEP(MH_G, d, a, b, c, 10, 9, 0x02441453u);
  MH_STEP(MH_G, c, d, a, b, 15, 14, 0xd8a1e681u);
  MH_STEP(MH_G, b, c, d, a, 4, 20, 0xe7d3fbc8u);
  MH_STEP(MH_G, a, b, c, d, 9, 5, 0x21e1cde6u);
  MH_STEP(MH_G, d, a, b, c, 14, 9, 0xc33707d6u);
  MH_STEP(MH_G, c, d, a, b, 3, 14, 0xf4d50d87u);
  MH_STEP(MH_G, b, c, d, a, 8, 20, 0x455a14edu);
  MH_STEP(MH_G, a, b, c, d, 13, 5, 0xa9e3e905u);
  MH_STEP(MH_G, d, a, b, c, 2, 9, 0xfcefa3f8u);
  MH_STEP(MH_G, c, d, a, b, 7, 14, 0x676f02d9u);
  MH_STEP(MH_G, b, c, d, a, 12, 20, 0x8d2a4c8au);
  MH_STEP(MH_H, a, b, c, d, 5, 4, 0xfffa3942u);
  MH_STEP(MH_H, d, a, b, c, 8, 11, 0x8771f681u);
  MH_STEP(MH_H, c, d, a, b, 11, 16, 0x6d9d6122u);
  MH_STEP(MH_H, b, c, d, a, 14, 23, 0xfde5380cu);
  MH_STEP(MH_H, a, b, c, d, 1, 4, 0xa4beea44u);
  MH_STEP(MH_H, d, a, b, c, 4, 11, 0x4bdecfa9u);
  MH_STEP(MH_H, c, d, a, b, 7, 16, 0xf6bb4b60u);
  MH_STEP(MH_H, b, c, d, a, 10, 23, 0xbebfbc70u);
  MH_STEP(MH_H, a, b, c, d, 13, 4, 0x289b7ec6u);
  MH_STEP(MH_H, d, a, b, c, 0, 11, 0xeaa127fau);
  MH_STEP(MH_H, c, d, a, b, 3, 16, 0xd4ef3085u);
  MH_STEP(MH_H, b, c, d, a, 6, 23, 0x04881d05u);
  MH_STEP(MH_H, a, b, c, d, 9, 4, 0xd9d4d039u);
  MH_STEP(MH_H, d, a, b, c, 12, 11, 0xe6db99e5u);
  MH_STEP(MH_H, c, d, a, b, 15, 16, 0x1fa27cf8u);
  MH_STEP(MH_H, b, c, d, a, 2, 23, 0xc4ac5665u);
  MH_STEP(MH_I, a, b, c, d, 0, 6, 0xf4292244u);
  MH_STEP(MH_I, d, a, b, c, 7, 10, 0x432aff97u);
  MH_STEP(MH_I, c, d, a, b, 14, 15, 0xab9423a7u);
  MH_STEP(MH_I, b, c, d, a, 5, 21, 0xfc93a039u);
  MH_STEP(MH_I, a, b, c, d, 12, 6, 0x655b59c3u);
  MH_STEP(MH_I, d, a, b, c, 3, 10, 0x8f0ccc92u);
  MH_STEP(MH_I, c, d, a, b, 10, 15, 0xffeff47du);
  MH_STEP(MH_I, b, c, d, a, 1, 21, 0x85845dd1u);
  MH_STEP(MH_I, a, b, c, d, 8, 6, 0x6fa87e4fu);
  MH_STEP(MH_I, d, a, b, c, 15, 10, 0xfe2ce6e0u);
  MH_STEP(MH_I, c, d, a, b, 6, 15, 0xa3014314u);
  MH_STEP(MH_I, b, c, d, a, 13, 21, 0x4e0811a1u);
  MH_STEP(MH_I, a, b, c, d, 4, 6, 0xf7537e82u);
  MH_STEP(MH_I, d, a, b, c, 11, 10, 0xbd3af235u);
  MH_STEP(MH_I, c, d, a, b, 2, 15, 0x2ad7d2bbu);
  MH_STEP(MH_I, b, c, d, a, 9, 21, 0xeb86d391u);
  U128 r;
  r.w[0] = __builtin_bswap32(a + 0x67452301u);
  r.w[1] = __builtin_bswap32(b + 0xefcdab89u);
  r.w[2] = __builtin_bswap32(c + 0x98badcfeu);
  r.w[3] = __builtin_bswap32(d + 0x10325476u);
  return r;
}

// ------------------------------------------------------------------------------------------------ signatures
__global__ __launch_bounds__(MH_THREADS) void mh_sig_kernel(const int64_t* __restrict__ ptr,
                                                            const int32_t* __restrict__ cps, int32_t ngram, int32_t P,
                                                            uint32_t* __restrict__ sig) {
  __shared__ __attribute__((aligned(16))) uint32_t slot[MH_GC * MH_SLOT];   // 4 KiB: the staged n-grams
  __shared__ int glen[MH_GC];                                               // their UTF-8 lengths
  __shared__ __attribute__((aligned(16))) uint32_t red[MH_THREADS * 4];     // 4 KiB: the slices' minima
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t a = ptr[row];
  const int64_t len = ptr[row + 1] - a;
  const int64_t G = len < ngram ? 1 : len - ngram + 1;     // a text shorter than ngram is its own single n-gram
  unsigned char* const sbytes = (unsigned char*)slot;
  for (int i0 = 0; i0 < P; i0 += MH_THREADS) {
    const int Pc = min(MH_THREADS, P - i0);                // permutations of this pass
    const int S = MH_THREADS / Pc;                         // slices of the n-grams, folded below
    const bool active = tid < S * Pc;
    const int i = i0 + tid % Pc, s = tid / Pc;
    // the prefix "<i>_" as the low bytes of message word 0 (i < 1000: at most 4 bytes)
    uint32_t pre;
    int plen;
    if (i >= 100) {
      pre = (uint32_t)('0' + i / 100) | (uint32_t)('0' + (i / 10) % 10) << 8 | (uint32_t)('0' + i % 10) << 16 | (uint32_t)'_' << 24;
      plen = 4;
    } else if (i >= 10) {
      pre = (uint32_t)('0' + i / 10) | (uint32_t)('0' + i % 10) << 8 | (uint32_t)'_' << 16;
      plen = 3;
    } else {
      pre = (uint32_t)('0' + i) | (uint32_t)'_' << 8;
      plen = 2;
    }
    const uint32_t sh = (uint32_t)(4 - plen);              // bytes the slot's words are read ahead of the message's
    U128 best;
    best.w[0] = best.w[1] = best.w[2] = best.w[3] = 0xffffffffu;
    for (int64_t c0 = 0; c0 < G; c0 += MH_GC) {
      const int ng = (int)min((int64_t)MH_GC, G - c0);
      __syncthreads();                                     // the previous pass has read its slots
      if (tid < ng) {
#pragma unroll
        for (int k = 0; k < MH_SLOT; ++k) slot[tid * MH_SLOT + k] = 0u;
        unsigned char* out = sbytes + tid * (MH_SLOT * 4) + 4;
        const int64_t g0 = a + c0 + tid;
        const int nc = (int)min((int64_t)ngram, len);
        int pos = 0;
        for (int j = 0; j < nc; ++j) {
          const uint32_t cp = (uint32_t)cps[g0 + j];
          const int nbytes = cp < 0x80u ? 1 : cp < 0x800u ? 2 : cp < 0x10000u ? 3 : 4;
          if (pos + nbytes > MH_GRAM_BYTES) break;         // over-long (precondition of the header): truncated, in bounds
          if (nbytes == 1) {
            out[pos] = (unsigned char)cp;
          } else if (nbytes == 2) {
            out[pos] = (unsigned char)(0xC0u | (cp >> 6));
            out[pos + 1] = (unsigned char)(0x80u | (cp & 0x3Fu));
          } else if (nbytes == 3) {
            out[pos] = (unsigned char)(0xE0u | (cp >> 12));
            out[pos + 1] = (unsigned char)(0x80u | ((cp >> 6) & 0x3Fu));
            out[pos + 2] = (unsigned char)(0x80u | (cp & 0x3Fu));
          } else {
            out[pos] = (unsigned char)(0xF0u | ((cp >> 18) & 0x07u));
            out[pos + 1] = (unsigned char)(0x80u | ((cp >> 12) & 0x3Fu));
            out[pos + 2] = (unsigned char)(0x80u | ((cp >> 6) & 0x3Fu));
            out[pos + 3] = (unsigned char)(0x80u | (cp & 0x3Fu));
          }
          pos += nbytes;
        }
        out[pos] = 0x80u;                                  // MD5 padding: the bit behind the message
        glen[tid] = pos;
      }
      __syncthreads();
      if (active) {
        for (int g = s; g < ng; g += S) {
          const uint4* sw = (const uint4*)(slot + g * MH_SLOT);
          const uint4 q0 = sw[0], q1 = sw[1], q2 = sw[2], q3 = sw[3];
          const uint32_t w[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                                  q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
          uint32_t m[16];
#pragma unroll
          for (int k = 0; k < 14; ++k) m[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
          m[0] |= pre;
          m[14] = (uint32_t)(plen + glen[g]) * 8u;
          m[15] = 0u;
          const U128 h = md5_block(m);
          if (less128(h, best)) best = h;
        }
      }
    }
    __syncthreads();                                       // red is free again (second pass over i0)
    *(uint4*)(red + tid * 4) = make_uint4(best.w[0], best.w[1], best.w[2], best.w[3]);
    __syncthreads();
    if (tid < Pc) {
      for (int j = 1; j < S; ++j) {
        const uint4 o = *(const uint4*)(red + (j * Pc + tid) * 4);
        U128 x;
        x.w[0] = o.x; x.w[1] = o.y; x.w[2] = o.z; x.w[3] = o.w;
        if (less128(x, best)) best = x;
      }
      *(uint4*)(sig + (row * P + i) * 4) = make_uint4(best.w[0], best.w[1], best.w[2], best.w[3]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ greedy matcher
// positions at which two signatures are equal on all 128 bits
__device__ __forceinline__ int exact_matches(const uint32_t* __restrict__ x, const uint32_t* __restrict__ y, int P) {
  const uint4* a = (const uint4*)x;
  const uint4* b = (const uint4*)y;
  int n = 0;
  for (int p = 0; p < P; ++p) {
    const uint4 u = a[p], v = b[p];
    n += (u.x == v.x) & (u.y == v.y) & (u.z == v.z) & (u.w == v.w);
  }
  return n;
}

__global__ __launch_bounds__(256) void mh_stage_kernel(const uint32_t* __restrict__ sig, int64_t row0, int32_t nb, int32_t P,
                                                       uint32_t* __restrict__ blkT, int32_t* __restrict__ cand,
                                                       uint32_t* __restrict__ M) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < P * MH_B) {
    const int p = idx / MH_B, j = idx % MH_B;
    blkT[idx] = j < nb ? sig[((row0 + j) * P + p) * 4 + 3] : 0u;
  }
  if (idx < MH_B) cand[idx] = MH_NONE;
  if (idx < MH_B * MH_W) M[idx] = 0u;
}

__global__ __launch_bounds__(MH_C) void mh_match_kernel(
    const uint32_t* __restrict__ sig, const uint32_t* __restrict__ lowT, int64_t cap, const int32_t* __restrict__ kept_idx,
    const int32_t* __restrict__ nk_ptr, const uint32_t* __restrict__ blkT, int64_t row0, int32_t nb, int32_t P,
    int32_t need, int32_t ncross, int32_t* __restrict__ cand, uint32_t* __restrict__ M) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sR[];   // [P][MH_R]: the low words of this workgroup's rows
  const int tid = threadIdx.x;
  const int r0 = blockIdx.y * MH_R;
  if (r0 >= nb) return;
  const int nk = *nk_ptr;                                    // rows kept from the earlier blocks
  const bool cross = (int)blockIdx.x < ncross;
  const int c0 = (cross ? (int)blockIdx.x : (int)blockIdx.x - ncross) * MH_C;
  if (cross ? c0 >= nk : (c0 >= nb || c0 >= r0 + MH_R - 1)) return;   // block-uniform: no column (in front of a row) here
  for (int idx = tid; idx < P * MH_R; idx += MH_C) {
    const int p = idx / MH_R, r = idx % MH_R;
    sR[idx] = r0 + r < nb ? blkT[p * MH_B + r0 + r] : 0u;
  }
  __syncthreads();
  const int c = c0 + tid;
  if (c >= (cross ? nk : nb)) return;
  const uint32_t* col = cross ? lowT + c : blkT + c;
  const int64_t stride = cross ? cap : MH_B;
  int cnt[MH_R];
#pragma unroll
  for (int r = 0; r < MH_R; ++r) cnt[r] = 0;
  for (int p0 = 0; p0 < P; p0 += 32) {
    const int pe = min(P, p0 + 32);
    for (int p = p0; p < pe; ++p) {
      const uint32_t x = col[p * stride];
      const uint4* s4 = (const uint4*)(sR + p * MH_R);
#pragma unroll
      for (int q = 0; q < MH_R / 4; ++q) {
        const uint4 v = s4[q];
        cnt[4 * q] += x == v.x;
        cnt[4 * q + 1] += x == v.y;
        cnt[4 * q + 2] += x == v.z;
        cnt[4 * q + 3] += x == v.w;
      }
    }
    int mx = 0;
#pragma unroll
    for (int r = 0; r < MH_R; ++r) mx = max(mx, cnt[r]);
    if (mx + (P - pe) < need) return;                        // no row can reach `need` against this column any more
  }
  uint32_t hits = 0u;                                        // low-word counts can only exceed the 128-bit ones
#pragma unroll
  for (int r = 0; r < MH_R; ++r) hits |= cnt[r] >= need ? 1u << r : 0u;
  if (!hits) return;
  const int orig = cross ? kept_idx[c] : (int)(row0 + c);
  while (hits) {
    const int rr = r0 + __builtin_ctz(hits);
    hits &= hits - 1u;
    if (rr >= nb || (!cross && c >= rr)) continue;           // only an earlier row can take a later one
    if (exact_matches(sig + (row0 + rr) * P * 4, sig + (int64_t)orig * P * 4, P) < need) continue;
    if (cross) atomicMin(&cand[rr], orig);
    else atomicOr(&M[rr * MH_W + (c >> 5)], 1u << (c & 31));
  }
}

__global__ __launch_bounds__(256) void mh_resolve_kernel(
    const int32_t* __restrict__ group, int32_t* __restrict__ group_kept, const int32_t* __restrict__ cand,
    const uint32_t* __restrict__ M, int64_t row0, int32_t nb, int32_t n, int32_t* __restrict__ nk_ptr,
    int32_t* __restrict__ kept_idx, int32_t* __restrict__ pos, int32_t* __restrict__ dup_of) {
  __shared__ uint32_t Ms[MH_B * MH_W];                       // 32 KiB: the block's match matrix
  __shared__ int grp[MH_B], slotof[MH_B], cnd[MH_B];
  __shared__ int keeper[MH_B];                               // per exact-key slot: the kept row with that key, or -1
  __shared__ uint32_t keptbits[MH_W];
  const int tid = threadIdx.x;
  const int nk = *nk_ptr;
  for (int i = tid; i < MH_B * MH_W; i += 256) Ms[i] = M[i];
  for (int j = tid; j < MH_B; j += 256) {
    cnd[j] = j < nb ? cand[j] : MH_NONE;
    const int g = group && j < nb ? group[row0 + j] : -1;
    grp[j] = (unsigned)g < (unsigned)n ? g : -1;             // an id out of range (precondition) is no key at all
  }
  __syncthreads();
  for (int j = tid; j < nb; j += 256) {                      // slot: the first row of the block with the same exact key
    int s = j;
    const int g = grp[j];
    if (g >= 0) {
      for (int c = 0; c < j; ++c)
        if (grp[c] == g) { s = c; break; }
    }
    slotof[j] = s;
    keeper[j] = g >= 0 && s == j ? group_kept[g] : -1;
  }
  __syncthreads();
  if (tid < 64) {                                            // one wave walks the rows in order; lane l owns kept word l
    volatile int* vkeeper = keeper;
    uint32_t keptw = 0u;
    for (int r = 0; r < nb; ++r) {
      const int sl = slotof[r];
      const int ks = vkeeper[sl];
      const uint32_t x = tid < MH_W ? Ms[r * MH_W + tid] & keptw : 0u;
      const unsigned long long bal = __ballot(x != 0u);
      int d;
      if (ks >= 0) {                                         // a kept row has the same exact key: the reference's first test
        d = ks;
      } else if (cnd[r] != MH_NONE) {                        // kept rows of earlier blocks come before the block's own
        d = cnd[r];
      } else if (bal) {
        const int fw = __builtin_ctzll(bal);
        const uint32_t xv = (uint32_t)__shfl((int)x, fw, 64);
        d = (int)(row0 + fw * 32 + __builtin_ctz(xv));
      } else {
        d = -1;
        if (tid == (r >> 5)) keptw |= 1u << (r & 31);
        if (tid == 0) vkeeper[sl] = (int)(row0 + r);
      }
      if (tid == 0) dup_of[row0 + r] = d;
    }
    if (tid < MH_W) keptbits[tid] = keptw;
  }
  __syncthreads();
  for (int j = tid; j < MH_B; j += 256) {
    int p = -1;
    if (j < nb && (keptbits[j >> 5] >> (j & 31) & 1u)) {
      int rank = __popc(keptbits[j >> 5] & ((1u << (j & 31)) - 1u));
      for (int w = 0; w < (j >> 5); ++w) rank += __popc(keptbits[w]);
      p = nk + rank;
      kept_idx[p] = (int)(row0 + j);
      if (grp[j] >= 0) group_kept[grp[j]] = (int)(row0 + j);
    }
    pos[j] = p;
  }
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < MH_W; ++w) total += __popc(keptbits[w]);
    *nk_ptr = nk + total;
  }
}

__global__ __launch_bounds__(256) void mh_append_kernel(const uint32_t* __restrict__ blkT, const int32_t* __restrict__ pos,
                                                        int32_t nb, int32_t P, int64_t cap, uint32_t* __restrict__ lowT) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= P * MH_B) return;
  const int p = idx / MH_B, j = idx % MH_B;
  if (j >= nb) return;
  const int pp = pos[j];
  if (pp >= 0) lowT[p * cap + pp] = blkT[idx];
}

// one wave per 16 kept rows of a query row: the first kept row (ascending) that reaches `need` on all 128 bits
__global__ __launch_bounds__(256) void mh_first_kernel(const uint32_t* __restrict__ q_sig, const uint32_t* __restrict__ k_sig,
                                                       int32_t nk, int32_t P, int32_t need, uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t q = blockIdx.y;
  const int k0 = blockIdx.x * 64 + (threadIdx.x >> 6) * 16;
  const uint4* qs = (const uint4*)(q_sig + q * P * 4);
  for (int k = k0; k < min(nk, k0 + 16); ++k) {              // wave-uniform
    const uint4* ks = (const uint4*)(k_sig + (int64_t)k * P * 4);
    int n = 0;
    for (int p = lane; p < P; p += 64) {
      const uint4 u = qs[p], v = ks[p];
      n += (u.x == v.x) & (u.y == v.y) & (u.z == v.z) & (u.w == v.w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (n >= need) {
      if (lane == 0) atomicMin(&out[q], (uint32_t)k);
      return;
    }
  }
}

struct DedupWs {
  size_t lowT, kept_idx, group_kept, blkT, cand, M, pos, nk, total;
  int64_t cap;
};

DedupWs dedup_ws(int64_t n, int P) {
  DedupWs w;
  w.cap = (n + 63) / 64 * 64;
  size_t o = 0;
  w.lowT = o;       o += align256((size_t)P * (size_t)w.cap * 4);
  w.kept_idx = o;   o += align256((size_t)n * 4);
  w.group_kept = o; o += align256((size_t)n * 4);
  w.blkT = o;       o += align256((size_t)P * MH_B * 4);
  w.cand = o;       o += align256((size_t)MH_B * 4);
  w.M = o;          o += align256((size_t)MH_B * MH_W * 4);
  w.pos = o;        o += align256((size_t)MH_B * 4);
  w.nk = o;         o += 256;
  w.total = o;
  return w;
}

}  // namespace

extern "C" int snx_minhash_signatures(const int64_t* ptr, const int32_t* code_points, int32_t n, int32_t ngram_size,
                                      int32_t num_perm, uint32_t* sig, hipStream_t st) {
  if (n < 0 || ngram_size < 1 || num_perm < 1 || num_perm > MH_PERM_MAX) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!ptr || !sig) return SNX_E_ARG;                        // code_points may be NULL when every row is empty
  hipLaunchKernelGGL(mh_sig_kernel, dim3((unsigned)n), dim3(MH_THREADS), 0, st, ptr, code_points, ngram_size, num_perm, sig);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" size_t snx_minhash_dedup_workspace_bytes(int32_t n, int32_t num_perm) {
  if (n <= 0 || num_perm < 1 || num_perm > MH_PERM_MAX) return 0;
  return dedup_ws(n, num_perm).total;
}

extern "C" int snx_minhash_dedup(const uint32_t* sig, int32_t n, int32_t num_perm, int32_t need, const int32_t* group,
                                 int32_t* duplicate_of, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (n < 0 || num_perm < 1 || num_perm > MH_PERM_MAX) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!sig || !duplicate_of) return SNX_E_ARG;
  const int P = num_perm;
  const DedupWs w = dedup_ws(n, P);
  if (!workspace || ws_bytes < w.total) return SNX_E_ARG;
  char* base = (char*)workspace;
  uint32_t* lowT = (uint32_t*)(base + w.lowT);
  int32_t* kept_idx = (int32_t*)(base + w.kept_idx);
  int32_t* group_kept = (int32_t*)(base + w.group_kept);
  uint32_t* blkT = (uint32_t*)(base + w.blkT);
  int32_t* cand = (int32_t*)(base + w.cand);
  uint32_t* M = (uint32_t*)(base + w.M);
  int32_t* pos = (int32_t*)(base + w.pos);
  int32_t* nk = (int32_t*)(base + w.nk);
  hipError_t e = hipMemsetAsync(nk, 0, 256, st);
  if (e != hipSuccess) return (int)e;
  if (group) {
    e = hipMemsetAsync(group_kept, 0xFF, (size_t)n * 4, st);   // -1: no kept row has this exact key yet
    if (e != hipSuccess) return (int)e;
  }
  const int stage_blocks = cdiv((long)max(P, MH_W) * MH_B, 256);
  const size_t lds = (size_t)P * MH_R * sizeof(uint32_t);
  for (int64_t row0 = 0; row0 < n; row0 += MH_B) {
    const int nb = (int)min((int64_t)MH_B, (int64_t)n - row0);
    const int ncross = cdiv(row0, MH_C);                     // at most row0 rows are kept so far; empty tiles leave at once
    hipLaunchKernelGGL(mh_stage_kernel, dim3(stage_blocks), dim3(256), 0, st, sig, row0, nb, P, blkT, cand, M);
    SNX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mh_match_kernel, dim3(ncross + cdiv(nb, MH_C), cdiv(nb, MH_R)), dim3(MH_C), lds, st, sig,
                       (const uint32_t*)lowT, w.cap, (const int32_t*)kept_idx, (const int32_t*)nk, (const uint32_t*)blkT,
                       row0, nb, P, need, ncross, cand, M);
    SNX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mh_resolve_kernel, dim3(1), dim3(256), 0, st, group, group_kept, (const int32_t*)cand,
                       (const uint32_t*)M, row0, nb, n, nk, kept_idx, pos, duplicate_of);
    SNX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mh_append_kernel, dim3(cdiv((long)P * MH_B, 256)), dim3(256), 0, st, (const uint32_t*)blkT,
                       (const int32_t*)pos, nb, P, w.cap, lowT);
    SNX_CHECK_LAUNCH();
  }
  return SNX_OK;
}

extern "C" int snx_minhash_first_match(const uint32_t* q_sig, int32_t nq, const uint32_t* kept_sig, int32_t nk,
                                       int32_t num_perm, int32_t need, int32_t* out, hipStream_t st) {
  if (nq < 0 || nk < 0 || num_perm < 1 || num_perm > MH_PERM_MAX) return SNX_E_SHAPE;
  if (nq == 0) return SNX_OK;
  if (!q_sig || !out || (nk > 0 && !kept_sig)) return SNX_E_ARG;
  if (nq > 65535) return SNX_E_SHAPE;                        // one launch: the rows are the grid's y
  const hipError_t e = hipMemsetAsync(out, 0xFF, (size_t)nq * 4, st);   // -1: no match
  if (e != hipSuccess) return (int)e;
  if (nk == 0) return SNX_OK;
  hipLaunchKernelGGL(mh_first_kernel, dim3(cdiv(nk, 64), nq), dim3(256), 0, st, q_sig, kept_sig, nk, num_perm, need,
                     (uint32_t*)out);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
