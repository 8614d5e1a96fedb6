// Unigram tokenizer (include/snx.h "Unigram tokenizer"): the Precompiled normalizer, WhitespaceSplit + Metaspace and the
// Unigram model of XLM-RoBERTa's tokenizer.json over rows of code points that normalize code point by code point, bit for
// bit what the `tokenizers` library returns.
//
//   ug_norm_count_kernel   one workgroup per row: 1 + the sum of the replacement lengths of its code points.
//   ug_norm_fill_kernel    one workgroup per row: a white-space slot, then every code point's replacement (or itself) at
//                          the place a workgroup scan of the lengths gives it.
//   ug_pieces_kernel<CPS>  one workgroup per row of at most CPS + 1 entries, all state in LDS.  A UNIT is a U+2581, or the
//                          white space in front of a word that does not begin with one (read as U+2581), and the word
//                          characters behind it.  Phase A: the thread on a unit's first entry hashes its prefixes.  Phase
//                          B: a thread per start probes every length up to the longest piece against the open-addressed
//                          vocabulary table (a lookup compares the stored code points) and leaves the bitmask of hit
//                          lengths.  Phase C: the thread on a unit's first entry runs the Viterbi recurrence in float64 over
//                          the hits only, end by end, pulling candidates from the longest length down (so the earliest start
//                          is offered first and a strict > keeps it on a tie), the unknown last; then walks back, fuses
//                          consecutive unknowns and writes the id of every piece onto the entry the piece starts at, -1 onto
//                          the others.  Every entry is written by exactly one thread.  Two sizes: CPS = 512 and 4096.
//   ug_pieces_long_kernel  the same code for longer rows: entries read from memory, the state in the workgroup's workspace
//                          slot; a fixed number of workgroups walks the rows.
// No atomic and no sort decides an id or a place; the float64 additions are single adds in a fixed order (there is no
// multiplication to contract with): the result is a pure function of the input.  snx_wp_fill / snx_wp_pad
// (wordpiece.hip) do the compaction behind bos and the padding.
#include "sparse_common.h"   // block_sum
#include "text_common.h"
#include "snx.h"

namespace {

constexpr int UG_THREADS = 256;
constexpr int UG_WAVES = UG_THREADS / 64;
constexpr int UG_MAX_PIECE = 32;                    // longest piece in code points: a start's hit lengths are one uint32
constexpr int UG_LDS_CPS = 4096;                    // 25 bytes an entry: 100 KiB, one workgroup per CU of 160 KiB
constexpr int UG_SMALL_CPS = 512;                   // 12.7 KiB: LDS admits 12 workgroups per CU, the compiler's occupancy 7
constexpr int UG_LONG_GROUPS = 64;                  // workgroups (and workspace slots) of the long-row form
constexpr int32_t UG_META = 0x2581;

struct UgVocab {
  const int32_t* slots;
  const int32_t* ent_ptr;
  const int32_t* ent_cps;
  const int32_t* ent_id;
  const double* ent_score;
  int32_t n_slots, n_entries, max_entry, unk_id;
  double unk_score;
};

// one row's state: LDS, or the workgroup's workspace slot
struct UgState {
  uint32_t* hx;       // the hash of the unit's prefix that ends at an entry
  uint32_t* mask;     // bit L-1: a piece of L code points starts at the entry
  double* best;       // the best score of a path that ends behind the entry
  int32_t* bid;       // ... the id of its last piece
  uint8_t* blen;      // ... and that piece's length
};

// Rust's char::is_whitespace (White_Space)
__device__ __forceinline__ bool ug_space(int32_t c) {
  return (c >= 0x09 && c <= 0x0D) || c == 0x20 || c == 0x85 || c == 0xA0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200A) ||
         c == 0x2028 || c == 0x2029 || c == 0x202F || c == 0x205F || c == 0x3000;
}
__device__ __forceinline__ bool ug_word(int32_t c) { return c != UG_META && !ug_space(c); }

// the replacement of code point c: nmap's entry, -1 when c is kept
__device__ __forceinline__ int32_t ug_map(const int32_t* __restrict__ nmap, int32_t c) {
  return (uint32_t)c < 0x110000u ? nmap[c] : -1;
}

// the entry whose code points are first, w[1..L) and whose polynomial hash is h, -1 when the vocabulary has none
__device__ __forceinline__ int32_t ug_find(const UgVocab& V, uint32_t h, int32_t first, const int32_t* w, int L) {
  const uint32_t x = text_hash_mix(h ^ ((uint32_t)L * 0xC2B2AE35u));
  return text_probe(V.slots, V.ent_ptr, V.n_slots, V.n_entries, x, L, [&](int32_t, int32_t b) {
    if (V.ent_cps[b] != first) return false;
    int k = 1;
    while (k < L && V.ent_cps[b + k] == w[k]) ++k;
    return k == L;
  });
}

// does a unit start at entry i of the row t[0..len)?
__device__ __forceinline__ bool ug_starts(const int32_t* t, int64_t len, int64_t i, int32_t c) {
  return c == UG_META || (ug_space(c) && i + 1 < len && ug_word(t[i + 1]));
}

// the unit that starts at entry s: Viterbi over the hit masks, then the walk back; its pieces onto out[s..e), -> their number
__device__ __forceinline__ int ug_unit(const UgVocab& V, const uint32_t* pw, const int32_t* t, const UgState& S, int64_t len,
                                       int64_t s, int32_t* __restrict__ out) {
  int64_t e = s + 1;
  while (e < len && ug_word(t[e])) ++e;
  for (int64_t k = s; k < e; ++k) {                          // the path that ends behind entry k
    const int64_t en = k + 1;
    bool found = false;
    double bb = 0.0;
    int32_t bi = V.unk_id;
    int bl = 1;
    for (int L = (int)min((int64_t)V.max_entry, en - s); L >= 1; --L) {      // earliest start first
      const int64_t st = en - L;
      if (!((S.mask[st] >> (L - 1)) & 1u)) continue;
      const uint32_t hb = st > s ? S.hx[st - 1] : 0u;
      const int32_t ent = ug_find(V, S.hx[k] - hb * pw[L], st > s ? t[st] : UG_META, t + st, L);
      if (ent < 0) continue;                                 // cannot happen: phase B found it
      const double cand = V.ent_score[ent] + (st > s ? S.best[st - 1] : 0.0);
      if (!found || cand > bb) { found = true; bb = cand; bi = V.ent_id[ent]; bl = L; }
    }
    if (!(S.mask[k] & 1u)) {                                 // no piece of one code point here: the unknown competes, last
      const double cand = V.unk_score + (k > s ? S.best[k - 1] : 0.0);
      if (!found || cand > bb) { found = true; bb = cand; bi = V.unk_id; bl = 1; }
    }
    S.best[k] = bb;
    S.bid[k] = bi;
    S.blen[k] = (uint8_t)bl;
  }
  int n = 0;
  int64_t en = e;
  while (en > s) {
    const int64_t st = en - S.blen[en - 1];
    const int32_t id = S.bid[en - 1];
    const bool fused = id == V.unk_id && st > s && S.bid[st - 1] == V.unk_id;  // the run's first unknown carries the id
    out[st] = fused ? -1 : id;
    for (int64_t k = st + 1; k < en; ++k) out[k] = -1;
    n += fused ? 0 : 1;
    en = st;
  }
  return n;
}

// one row: t its entries (LDS or memory), S room for len entries of state
__device__ __forceinline__ void ug_row(const UgVocab& V, const uint32_t* pw, const int32_t* t, const UgState& S, int64_t len,
                                       int64_t max_pieces, int32_t* __restrict__ out, int64_t* __restrict__ out_cnt,
                                       int64_t row, int& slot) {
  // phase A: prefix hashes, a unit by the thread on its first entry; white space that starts nothing is no piece
  for (int64_t base = 0; base < len; base += UG_THREADS) {
    const int64_t i = base + threadIdx.x;
    if (i < len) {
      const int32_t c = t[i];
      if (ug_starts(t, len, i, c)) {
        uint32_t h = (uint32_t)(UG_META + 1);
        S.hx[i] = h;
        for (int64_t k = i + 1; k < len && ug_word(t[k]); ++k) {
          h = h * TEXT_HASH_BASE + (uint32_t)(t[k] + 1);
          S.hx[k] = h;
        }
      } else if (!ug_word(c)) {
        out[i] = -1;
      }
    }
  }
  __syncthreads();
  // phase B: the hit lengths of every start
  for (int64_t base = 0; base < len; base += UG_THREADS) {
    const int64_t i = base + threadIdx.x;
    if (i < len) {
      const int32_t c = t[i];
      const bool start = ug_starts(t, len, i, c);
      uint32_t m = 0u;
      if (start || ug_word(c)) {
        const uint32_t hb = start || i == 0 ? 0u : S.hx[i - 1];   // a word character has its unit's start in front of it
        const int32_t first = start ? UG_META : c;
        uint32_t p = 1u;
        for (int L = 1; L <= V.max_entry; ++L) {
          const int64_t k = i + L - 1;
          if (L > 1 && (k >= len || !ug_word(t[k]))) break;
          p *= TEXT_HASH_BASE;
          if (ug_find(V, S.hx[k] - hb * p, first, t + i, L) >= 0) m |= 1u << (L - 1);
        }
      }
      S.mask[i] = m;
    }
  }
  __syncthreads();
  // phase C: the recurrence and the walk back, a unit by the thread on its first entry
  int cnt = 0;
  for (int64_t base = 0; base < len; base += UG_THREADS) {
    const int64_t i = base + threadIdx.x;
    if (i < len && ug_starts(t, len, i, t[i])) cnt += ug_unit(V, pw, t, S, len, i, out);
  }
  const int total = block_sum(cnt, slot);
  if (threadIdx.x == 0) out_cnt[row] = (max_pieces >= 0 ? min((int64_t)total, max_pieces) : (int64_t)total) + 2;
}

// rows of MIN_LEN < len <= CPS + 1 entries (the white-space slot and CPS normalized code points)
template <int CPS, int MIN_LEN>
__global__ __launch_bounds__(UG_THREADS) void ug_pieces_kernel(const int64_t* __restrict__ ptr,
                                                               const int32_t* __restrict__ norm, UgVocab V,
                                                               int64_t max_pieces, int32_t* __restrict__ pieces,
                                                               int64_t* __restrict__ out_cnt) {
  __shared__ double best[CPS + 1];
  __shared__ int32_t t[CPS + 1];
  __shared__ uint32_t hx[CPS + 1];
  __shared__ uint32_t mask[CPS + 1];
  __shared__ int32_t bid[CPS + 1];
  __shared__ uint8_t blen[CPS + 1];
  __shared__ uint32_t pw[UG_MAX_PIECE + 1];                  // pw[L] = TEXT_HASH_BASE^L
  __shared__ int slot;
  const int64_t row = blockIdx.x;
  const int64_t a0 = ptr[row], len = ptr[row + 1] - a0;
  if (len <= MIN_LEN || len > CPS + 1) return;               // block-uniform: another form's row
  for (int64_t i = threadIdx.x; i < len; i += UG_THREADS) t[i] = norm[a0 + i];
  text_hash_powers(pw, V.max_entry);
  __syncthreads();
  const UgState S{hx, mask, best, bid, blen};
  ug_row(V, pw, t, S, len, max_pieces, pieces + a0, out_cnt, row, slot);
}

// entries of a workspace slot of the long-row form (a multiple of 8, so that every array of the slot is aligned)
__host__ __device__ inline int64_t ug_slot_entries(int64_t longest_row) {
  return longest_row <= UG_LDS_CPS + 1 ? 0 : (longest_row + 7) / 8 * 8;
}
constexpr int64_t UG_SLOT_BYTES = 8 + 4 + 4 + 4 + 1;         // best, hx, mask, bid, blen of an entry

__global__ __launch_bounds__(UG_THREADS) void ug_pieces_long_kernel(const int64_t* __restrict__ ptr,
                                                                    const int32_t* __restrict__ norm, int32_t n, UgVocab V,
                                                                    int64_t max_pieces, uint8_t* __restrict__ ws,
                                                                    int64_t slot_entries, int32_t* __restrict__ pieces,
                                                                    int64_t* __restrict__ out_cnt) {
  __shared__ uint32_t pw[UG_MAX_PIECE + 1];
  __shared__ int slot;
  text_hash_powers(pw, V.max_entry);
  __syncthreads();
  uint8_t* base = ws + (int64_t)blockIdx.x * slot_entries * UG_SLOT_BYTES;
  UgState S;
  S.best = (double*)base;
  S.hx = (uint32_t*)(base + 8 * slot_entries);
  S.mask = (uint32_t*)(base + 12 * slot_entries);
  S.bid = (int32_t*)(base + 16 * slot_entries);
  S.blen = base + 20 * slot_entries;
  for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
    const int64_t a0 = ptr[row], len = ptr[row + 1] - a0;
    if (len <= UG_LDS_CPS + 1) continue;                     // block-uniform: an LDS form's row
    if (len > slot_entries) {                                // `longest_row` was understated (precondition): bos, eos
      for (int64_t i = threadIdx.x; i < len; i += UG_THREADS) pieces[a0 + i] = -1;
      if (threadIdx.x == 0) out_cnt[row] = 2;
      continue;
    }
    ug_row(V, pw, norm + a0, S, len, max_pieces, pieces + a0, out_cnt, row, slot);
    __syncthreads();                                         // the next row reuses the slot
  }
}

__global__ __launch_bounds__(UG_THREADS) void ug_norm_count_kernel(const int64_t* __restrict__ ptr,
                                                                   const int32_t* __restrict__ cps,
                                                                   const int32_t* __restrict__ nmap,
                                                                   int64_t* __restrict__ out_len) {
  __shared__ int slot;
  const int64_t row = blockIdx.x;
  const int64_t a0 = ptr[row], len = ptr[row + 1] - a0;
  int sum = 0;
  for (int64_t i = threadIdx.x; i < len; i += UG_THREADS) {
    const int32_t m = ug_map(nmap, cps[a0 + i]);
    sum += m < 0 ? 1 : (m & 31);
  }
  const int total = block_sum(sum, slot);
  if (threadIdx.x == 0) out_len[row] = (int64_t)total + 1;
}

__global__ __launch_bounds__(UG_THREADS) void ug_norm_fill_kernel(const int64_t* __restrict__ ptr,
                                                                  const int32_t* __restrict__ cps,
                                                                  const int32_t* __restrict__ nmap,
                                                                  const int32_t* __restrict__ pool,
                                                                  const int64_t* __restrict__ norm_ptr,
                                                                  int32_t* __restrict__ norm) {
  __shared__ int wsum[UG_WAVES];
  __shared__ int64_t run;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const int64_t a0 = ptr[row], len = ptr[row + 1] - a0;
  const int64_t o0 = norm_ptr[row], room = norm_ptr[row + 1] - o0;
  if (room < 1) return;                                      // no room for the slot (precondition): nothing written
  if (tid == 0) {
    norm[o0] = 0x20;
    run = 1;
  }
  __syncthreads();
  for (int64_t base = 0; base < len; base += UG_THREADS) {   // block-uniform bounds
    const int64_t i = base + tid;
    const int32_t c = i < len ? cps[a0 + i] : 0;
    const int32_t m = i < len ? ug_map(nmap, c) : 0;         // 0: a replacement of length 0
    const int v = m < 0 ? 1 : (m & 31);
    int x = v;                                               // inclusive scan of the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int64_t pos = run + x - v;
    for (int w = 0; w < wave; ++w) pos += wsum[w];
    if (pos + v <= room) {                                   // inside the row's span (it is, when norm_ptr is the count's scan)
      if (m < 0) {
        norm[o0 + pos] = c;
      } else {
        const int32_t* src = pool + (m >> 5);
        for (int j = 0; j < v; ++j) norm[o0 + pos + j] = src[j];
      }
    }
    __syncthreads();
    if (tid == 0) {
      int64_t r = run;
      for (int w = 0; w < UG_WAVES; ++w) r += wsum[w];
      run = r;
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" size_t snx_ug_workspace_bytes(int64_t longest_row) {
  if (longest_row < 0 || longest_row >= (1ll << 31)) return 0;
  return (size_t)(ug_slot_entries(longest_row) * UG_SLOT_BYTES * UG_LONG_GROUPS);
}

extern "C" int snx_ug_norm_count(const int64_t* ptr, const int32_t* code_points, int32_t n, const int32_t* nmap,
                                 int64_t* out_len, hipStream_t st) {
  if (n < 0) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!ptr || !nmap || !out_len) return SNX_E_ARG;             // code_points may be NULL when every row is empty
  hipLaunchKernelGGL(ug_norm_count_kernel, dim3((unsigned)n), dim3(UG_THREADS), 0, st, ptr, code_points, nmap, out_len);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_ug_norm_fill(const int64_t* ptr, const int32_t* code_points, int32_t n, const int32_t* nmap,
                                const int32_t* pool, const int64_t* norm_ptr, int32_t* norm, hipStream_t st) {
  if (n < 0) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!ptr || !nmap || !norm_ptr || !norm) return SNX_E_ARG;   // pool may be NULL when the map replaces nothing by text
  hipLaunchKernelGGL(ug_norm_fill_kernel, dim3((unsigned)n), dim3(UG_THREADS), 0, st, ptr, code_points, nmap, pool, norm_ptr,
                     norm);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_ug_pieces(const int64_t* norm_ptr, const int32_t* norm, int32_t n, int64_t longest_row,
                             const int32_t* slots, int32_t n_slots, const int32_t* ent_ptr, const int32_t* ent_cps,
                             const int32_t* ent_id, const double* ent_score, int32_t n_entries, int32_t max_entry,
                             int32_t unk_id, double unk_score, int64_t max_pieces, int32_t* pieces, int64_t* out_cnt,
                             void* workspace, size_t ws_bytes, hipStream_t st) {
  if (n < 0 || longest_row < 0 || longest_row >= (1ll << 31)) return SNX_E_SHAPE;
  if (n_slots < 1 || (n_slots & (n_slots - 1)) != 0 || n_entries < 0 || n_entries > n_slots) return SNX_E_SHAPE;
  if (max_entry < 1 || max_entry > UG_MAX_PIECE) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!norm_ptr || !slots || !ent_ptr || !out_cnt || (n_entries > 0 && (!ent_cps || !ent_id || !ent_score))) return SNX_E_ARG;
  if (longest_row > 0 && (!norm || !pieces)) return SNX_E_ARG;
  const int64_t slot = ug_slot_entries(longest_row);
  if (slot && (!workspace || ws_bytes < (size_t)(slot * UG_SLOT_BYTES * UG_LONG_GROUPS))) return SNX_E_ARG;
  const UgVocab V{slots, ent_ptr, ent_cps, ent_id, ent_score, n_slots, n_entries, max_entry, unk_id, unk_score};
  hipLaunchKernelGGL((ug_pieces_kernel<UG_SMALL_CPS, -1>), dim3((unsigned)n), dim3(UG_THREADS), 0, st, norm_ptr, norm, V,
                     max_pieces, pieces, out_cnt);
  SNX_CHECK_LAUNCH();
  if (longest_row > UG_SMALL_CPS + 1) {
    hipLaunchKernelGGL((ug_pieces_kernel<UG_LDS_CPS, UG_SMALL_CPS + 1>), dim3((unsigned)n), dim3(UG_THREADS), 0, st, norm_ptr,
                       norm, V, max_pieces, pieces, out_cnt);
    SNX_CHECK_LAUNCH();
  }
  if (slot) {
    hipLaunchKernelGGL(ug_pieces_long_kernel, dim3((unsigned)min(n, UG_LONG_GROUPS)), dim3(UG_THREADS), 0, st, norm_ptr, norm,
                       n, V, max_pieces, (uint8_t*)workspace, slot, pieces, out_cnt);
    SNX_CHECK_LAUNCH();
  }
  return SNX_OK;
}
