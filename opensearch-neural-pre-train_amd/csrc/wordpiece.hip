// WordPiece tokenizer (include/snx.h "WordPiece tokenizer"): BertPreTokenizer and WordPiece of the model's tokenizer.json
// over rows of NFC code points, bit for bit what the `tokenizers` library returns.
//
//   wp_pieces_kernel<false>  one workgroup per row, the row's code points and the prefix hashes of its words in LDS.  A
//                            thread owns a code point; the thread on a word's FIRST code point walks that word: finds its
//                            end, hashes its prefixes once, matches greedily longest-first against the open-addressed
//                            vocabulary table (a lookup compares the stored code points) and writes the id of every piece
//                            onto the code point the piece starts at, -1 onto the others.  Each code point is written by
//                            exactly one thread.  The row's count is a workgroup sum.  Rows of more than WP_LDS_CPS code
//                            points are left alone.
//   wp_pieces_kernel<true>   the same code for the rows the LDS form leaves alone: code points read from memory, prefix
//                            hashes in the workgroup's workspace slot; a fixed number of workgroups walks the rows.
//   wp_fill_kernel           one workgroup per row: the pieces >= 0 in text order move behind bos (ballot scan), cut at the
//                            row's span in out_ptr, eos behind them.
//   wp_pad_kernel            the CSR of ids as right-padded input_ids / attention_mask.
// No atomic decides a place, no kernel waits for another workgroup: the result is a pure function of the input.
#include "sparse_common.h"   // block_sum
#include "text_common.h"
#include "snx.h"

namespace {

constexpr int WP_THREADS = 256;
constexpr int WP_WAVES = WP_THREADS / 64;
constexpr int WP_LDS_CPS = 4096;                    // 16 KiB of code points + 16 KiB of prefix hashes
constexpr int WP_LONG_GROUPS = 64;                  // workgroups (and workspace slots) of the long-row form
constexpr int WP_WORD_MAX = 128;                    // bound of max_word / max_entry: the power table in LDS
constexpr uint8_t WP_SPACE = 1, WP_PUNCT = 2;       // class 0: a word character

struct WpVocab {
  const uint8_t* cls;
  const int32_t* slots;
  const int32_t* ent_ptr;
  const int32_t* ent_cps;
  const int32_t* ent_cont;
  const int32_t* ent_id;
  int32_t n_slots, n_entries, max_entry, max_word, unk_id;
};

__device__ __forceinline__ uint8_t wp_class(const WpVocab& V, int32_t c) {
  return (uint32_t)c < 0x110000u ? V.cls[c] : (uint8_t)0;
}

// the id of the entry (cont, w[0..L)) whose polynomial hash is h, -1 when the vocabulary has none
__device__ __forceinline__ int32_t wp_lookup(const WpVocab& V, uint32_t h, int cont, const int32_t* w, int L) {
  const uint32_t x = text_hash_mix(h ^ (cont ? 0x85EBCA6Bu : 0u) ^ ((uint32_t)L * 0xC2B2AE35u));
  // text_probe's loop, written out: with the shared one (ent_cont in the predicate, ent_id read behind the probe), and
  // likewise with text_hash_powers, wp_pieces_kernel compiles to other code (profiles/text_front_refactor.txt)
  const uint32_t mask = (uint32_t)V.n_slots - 1u;
  uint32_t s = x & mask;
  for (int32_t probe = 0; probe < V.n_slots; ++probe) {      // bounded: a full table has no free slot to stop at
    const int32_t e = V.slots[s];
    if (e < 0 || e >= V.n_entries) return -1;
    const int32_t b = V.ent_ptr[e];
    if (V.ent_ptr[e + 1] - b == L && V.ent_cont[e] == cont) {
      int k = 0;
      while (k < L && V.ent_cps[b + k] == w[k]) ++k;
      if (k == L) return V.ent_id[e];
    }
    s = (s + 1u) & mask;
  }
  return -1;
}

// the word that starts at code point s of the row t[0..len): its pieces onto out[s..e), -> their number
__device__ __forceinline__ int wp_word(const WpVocab& V, const uint32_t* pw, const int32_t* t, uint32_t* hx, int64_t len,
                                       int64_t s, uint8_t c, int32_t* __restrict__ out) {
  int64_t e = s + 1;
  if (c == 0)
    while (e < len && wp_class(V, t[e]) == 0) ++e;
  bool ok = e - s <= V.max_word;
  int n = 0;
  if (ok) {
    uint32_t h = 0;
    for (int64_t k = s; k < e; ++k) {
      h = h * TEXT_HASH_BASE + (uint32_t)(t[k] + 1);
      hx[k] = h;                                             // the hash of t[s..k]
    }
    int64_t st = s;
    while (st < e) {
      const uint32_t hb = st > s ? hx[st - 1] : 0u;
      int64_t en = min(e, st + (int64_t)V.max_entry);
      int32_t found = -1;
      for (; en > st; --en) {
        const int L = (int)(en - st);
        found = wp_lookup(V, hx[en - 1] - hb * pw[L], st > s, t + st, L);
        if (found >= 0) break;
      }
      if (found < 0) { ok = false; break; }
      out[st] = found;
      for (int64_t k = st + 1; k < en; ++k) out[k] = -1;
      ++n;
      st = en;
    }
  }
  if (!ok) {                                                 // too long, or an offset without a hit: the whole word is unk
    out[s] = V.unk_id;
    for (int64_t k = s + 1; k < e; ++k) out[k] = -1;
    n = 1;
  }
  return n;
}

// one row: t its code points (LDS or memory), hx room for len prefix hashes (LDS or the workspace slot)
__device__ __forceinline__ void wp_row(const WpVocab& V, const uint32_t* pw, const int32_t* t, uint32_t* hx, int64_t len,
                                       int64_t max_pieces, int32_t* __restrict__ out, int64_t* __restrict__ out_cnt,
                                       int64_t row, int& slot) {
  int cnt = 0;
  for (int64_t base = 0; base < len; base += WP_THREADS) {
    const int64_t i = base + threadIdx.x;
    if (i < len) {
      const uint8_t c = wp_class(V, t[i]);
      if (c == WP_SPACE) out[i] = -1;
      else if (c == WP_PUNCT || i == 0 || wp_class(V, t[i - 1]) != 0) cnt += wp_word(V, pw, t, hx, len, i, c, out);
    }
  }
  const int total = block_sum(cnt, slot);
  if (threadIdx.x == 0) out_cnt[row] = (max_pieces >= 0 ? min((int64_t)total, max_pieces) : (int64_t)total) + 2;
}

template <bool LONG>
__global__ __launch_bounds__(WP_THREADS) void wp_pieces_kernel(const int64_t* __restrict__ ptr,
                                                               const int32_t* __restrict__ cps, int32_t n, WpVocab V,
                                                               int64_t max_pieces, uint32_t* __restrict__ ws,
                                                               int64_t ws_cps, int32_t* __restrict__ pieces,
                                                               int64_t* __restrict__ out_cnt) {
  __shared__ uint32_t pw[WP_WORD_MAX + 1];                   // pw[L] = TEXT_HASH_BASE^L
  __shared__ int slot;
  if constexpr (!LONG) {
    __shared__ int32_t t[WP_LDS_CPS];
    __shared__ uint32_t hx[WP_LDS_CPS];
    const int64_t row = blockIdx.x;
    const int64_t a0 = ptr[row], len = ptr[row + 1] - a0;
    if (len > WP_LDS_CPS) return;                            // block-uniform: the long form's row
    for (int64_t i = threadIdx.x; i < len; i += WP_THREADS) t[i] = cps[a0 + i];
    if (threadIdx.x == 0) {                                  // text_hash_powers written out, as wp_lookup's probe
      uint32_t p = 1u;
      for (int L = 0; L <= V.max_entry; ++L) { pw[L] = p; p *= TEXT_HASH_BASE; }
    }
    __syncthreads();
    wp_row(V, pw, t, hx, len, max_pieces, pieces + a0, out_cnt, row, slot);
  } else {
    if (threadIdx.x == 0) {                                  // text_hash_powers written out, as wp_lookup's probe
      uint32_t p = 1u;
      for (int L = 0; L <= V.max_entry; ++L) { pw[L] = p; p *= TEXT_HASH_BASE; }
    }
    __syncthreads();
    uint32_t* hx = ws + (int64_t)blockIdx.x * ws_cps;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
      const int64_t a0 = ptr[row], len = ptr[row + 1] - a0;
      if (len <= WP_LDS_CPS) continue;                       // block-uniform: the LDS form's row
      if (len > ws_cps) {                                    // `longest_row` was understated (precondition): bos, eos
        for (int64_t i = threadIdx.x; i < len; i += WP_THREADS) pieces[a0 + i] = -1;
        if (threadIdx.x == 0) out_cnt[row] = 2;
        continue;
      }
      wp_row(V, pw, cps + a0, hx, len, max_pieces, pieces + a0, out_cnt, row, slot);
    }
  }
}

__global__ __launch_bounds__(WP_THREADS) void wp_fill_kernel(const int64_t* __restrict__ ptr,
                                                             const int32_t* __restrict__ pieces,
                                                             const int64_t* __restrict__ out_ptr, int32_t bos_id,
                                                             int32_t eos_id, int64_t* __restrict__ out_ids) {
  __shared__ int wcnt[WP_WAVES];
  __shared__ int64_t run;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = blockIdx.x;
  const int64_t a0 = ptr[row], len = ptr[row + 1] - a0;
  const int64_t o0 = out_ptr[row], keep = out_ptr[row + 1] - o0 - 2;
  if (keep < 0) return;                                      // no room for the frame (precondition): nothing written
  if (tid == 0) {
    out_ids[o0] = bos_id;
    out_ids[o0 + 1 + keep] = eos_id;
    run = 0;
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t base = 0; base < len; base += WP_THREADS) {   // block-uniform bounds
    if (run >= keep) break;                                  // block-uniform: read behind the barrier that follows its update
    const int64_t i = base + tid;
    const int32_t p = i < len ? pieces[a0 + i] : -1;
    const unsigned long long m = __ballot(p >= 0);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();
    if (p >= 0) {
      int64_t pos = run + __popcll(m & below);
      for (int w = 0; w < wave; ++w) pos += wcnt[w];
      if (pos < keep) out_ids[o0 + 1 + pos] = p;
    }
    __syncthreads();
    if (tid == 0) {
      int64_t r = run;
      for (int w = 0; w < WP_WAVES; ++w) r += wcnt[w];
      run = r;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(WP_THREADS) void wp_pad_kernel(const int64_t* __restrict__ out_ptr,
                                                            const int64_t* __restrict__ out_ids, int64_t total, int64_t L,
                                                            int64_t pad_id, int64_t* __restrict__ input_ids,
                                                            int64_t* __restrict__ attention_mask) {
  for (int64_t idx = (int64_t)blockIdx.x * WP_THREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * WP_THREADS) {
    const int64_t r = idx / L, j = idx - r * L;
    const int64_t o0 = out_ptr[r];
    const bool in = j < out_ptr[r + 1] - o0;
    input_ids[idx] = in ? out_ids[o0 + j] : pad_id;
    attention_mask[idx] = in ? 1 : 0;
  }
}

// code points of a workspace slot of the long-row form, 0 when every row fits the LDS form
int64_t long_slot_cps(int64_t longest_row) { return longest_row <= WP_LDS_CPS ? 0 : longest_row; }

}  // namespace

extern "C" size_t snx_wp_workspace_bytes(int64_t longest_row) {
  if (longest_row < 0 || longest_row >= (1ll << 31)) return 0;
  return (size_t)long_slot_cps(longest_row) * sizeof(uint32_t) * WP_LONG_GROUPS;
}

extern "C" int snx_wp_pieces(const int64_t* ptr, const int32_t* code_points, int32_t n, int64_t longest_row,
                             const uint8_t* cls, const int32_t* slots, int32_t n_slots, const int32_t* ent_ptr,
                             const int32_t* ent_cps, const int32_t* ent_cont, const int32_t* ent_id, int32_t n_entries,
                             int32_t max_entry, int32_t max_word, int32_t unk_id, int64_t max_pieces, int32_t* pieces,
                             int64_t* out_cnt, void* workspace, size_t ws_bytes, hipStream_t st) {
  if (n < 0 || longest_row < 0 || longest_row >= (1ll << 31)) return SNX_E_SHAPE;
  if (n_slots < 1 || (n_slots & (n_slots - 1)) != 0 || n_entries < 0 || n_entries > n_slots) return SNX_E_SHAPE;
  if (max_entry < 1 || max_entry > max_word || max_word > WP_WORD_MAX) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  // code_points and pieces may be NULL when every row is empty, ent_cps when every entry is
  if (!ptr || !cls || !slots || !ent_ptr || !out_cnt || (n_entries > 0 && (!ent_cont || !ent_id))) return SNX_E_ARG;
  if (longest_row > 0 && (!code_points || !pieces)) return SNX_E_ARG;
  const int64_t slot = long_slot_cps(longest_row);
  if (slot && (!workspace || ws_bytes < (size_t)slot * sizeof(uint32_t) * WP_LONG_GROUPS)) return SNX_E_ARG;
  const WpVocab V{cls, slots, ent_ptr, ent_cps, ent_cont, ent_id, n_slots, n_entries, max_entry, max_word, unk_id};
  hipLaunchKernelGGL(wp_pieces_kernel<false>, dim3((unsigned)n), dim3(WP_THREADS), 0, st, ptr, code_points, n, V, max_pieces,
                     (uint32_t*)nullptr, (int64_t)0, pieces, out_cnt);
  SNX_CHECK_LAUNCH();
  if (slot) {
    hipLaunchKernelGGL(wp_pieces_kernel<true>, dim3((unsigned)min(n, WP_LONG_GROUPS)), dim3(WP_THREADS), 0, st, ptr,
                       code_points, n, V, max_pieces, (uint32_t*)workspace, slot, pieces, out_cnt);
    SNX_CHECK_LAUNCH();
  }
  return SNX_OK;
}

extern "C" int snx_wp_fill(const int64_t* ptr, const int32_t* pieces, int32_t n, const int64_t* out_ptr, int32_t bos_id,
                           int32_t eos_id, int64_t* out_ids, hipStream_t st) {
  if (n < 0) return SNX_E_SHAPE;
  if (n == 0) return SNX_OK;
  if (!ptr || !out_ptr || !out_ids) return SNX_E_ARG;          // pieces may be NULL when every row is empty
  hipLaunchKernelGGL(wp_fill_kernel, dim3((unsigned)n), dim3(WP_THREADS), 0, st, ptr, pieces, out_ptr, bos_id, eos_id,
                     out_ids);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_wp_pad(const int64_t* out_ptr, const int64_t* out_ids, int32_t n, int64_t L, int64_t pad_id,
                          int64_t* input_ids, int64_t* attention_mask, hipStream_t st) {
  if (n < 0 || L < 0) return SNX_E_SHAPE;
  const int64_t total = (int64_t)n * L;
  if (total == 0) return SNX_OK;
  if (!out_ptr || !out_ids || !input_ids || !attention_mask) return SNX_E_ARG;
  const int64_t blocks = min((total + WP_THREADS - 1) / WP_THREADS, (int64_t)1 << 20);
  hipLaunchKernelGGL(wp_pad_kernel, dim3((unsigned)blocks), dim3(WP_THREADS), 0, st, out_ptr, out_ids, total, L, pad_id,
                     input_ids, attention_mask);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
