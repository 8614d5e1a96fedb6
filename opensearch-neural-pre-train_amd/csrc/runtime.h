// Host plumbing shared by the model runtimes (model.hip, f32_path.hip, teacher.hip) and the arena plans of the sparse
// kernels (sparse_common.h): 256-byte arena offsets, early return on an error code, the ModernBERT parameter order.
// Host-only: nothing here is device code.
#pragma once
#include <stddef.h>

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// bump allocator over a caller-owned buffer: every block starts on a 256-byte boundary; `off` is the size so far
struct Arena {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t at = off;
    off = align256(off + bytes);
    return at;
  }
};

#define RC(call)            \
  do {                      \
    int rc__ = (call);      \
    if (rc__) return rc__;  \
  } while (0)

namespace modernbert {

// canonical parameter order of `params` (== state-dict order with the tied decoder weight listed once; include/snx.h)
struct PIdx {
  int L;
  int tok_emb() const { return 0; }
  int emb_norm() const { return 1; }
  int base(int l) const { return l == 0 ? 2 : 7 + 6 * (l - 1); }
  int attn_norm(int l) const { return base(l); }                 // l >= 1 only: layer 0 has no attn_norm
  int wqkv(int l) const { return base(l) + (l == 0 ? 0 : 1); }
  int wo(int l) const { return wqkv(l) + 1; }
  int mlp_norm(int l) const { return wqkv(l) + 2; }
  int wi(int l) const { return wqkv(l) + 3; }
  int wo_mlp(int l) const { return wqkv(l) + 4; }
  int tail() const { return 7 + 6 * (L - 1); }
  int final_norm() const { return tail(); }
  int head_dense() const { return tail() + 1; }
  int head_norm() const { return tail() + 2; }
  int dec_bias() const { return tail() + 3; }
  int count() const { return tail() + 4; }
};

}  // namespace modernbert
