// Masked-language-model pre-training: token masking and the cross-entropy of the masked rows against the tied
// decoder (what ModernBertForMaskedLM computes with sparse_prediction: the decoder runs on the masked rows only).
//
//   mask kernel   one thread per token; the draws are Philox4x32-10 outputs keyed by the token's identity
//                 (sample index, position, epoch), so a result depends neither on the batch nor on the launch shape
//   tile kernel   GemmCore 128x128 over h [M,H] x E [V,H]^T with an epilogue that rounds the logit as nn.Linear under
//                 autocast does, stores it (bf16, [M,Vp], pad columns zero), and leaves the row's (max, sum exp) over the
//                 tile's REAL columns and, in the tile that holds the label, the target logit
//   merge kernel  one wave per row: the tiles' partials -> lse and the row's loss, in a fixed order
//   backward      z -> g in place (elementwise); dh = g E over K = Vp against E^T [H,Vp] (built here when the weights
//                 change) as a K-split GemmCore kernel with an ordered reduction; dE by the library's weight-gradient
//                 GEMM through a padded fp32 scratch (it writes whole 128-row tiles); dbias by an ordered two-stage
//                 column sum.  No float atomics anywhere.
#include "common.h"
#include "gemm_core.h"
#include "snx.h"

namespace {

constexpr int MLM_TILE = 128;
using MlmCore = GemmCore<MLM_TILE, MLM_TILE, 4, 1>;

inline long vpad(long V) { return (V + MLM_TILE - 1) / MLM_TILE * MLM_TILE; }

#define RC(x)                     \
  do {                            \
    const int rc__ = (x);         \
    if (rc__ != SNX_OK) return rc__; \
  } while (0)

// ---- masking -----------------------------------------------------------------------------------------------------
struct Specials {
  int64_t id[16];
  int n;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__global__ void mlm_mask_kernel(const int64_t* __restrict__ ids, const int64_t* __restrict__ mask,
                                const int64_t* __restrict__ sample, int64_t* __restrict__ out_ids,
                                int64_t* __restrict__ labels, long n, int S, Specials sp, int64_t mask_id, uint32_t vocab,
                                uint32_t k0, uint32_t k1, uint32_t epoch, double p, double p_mask, double p_mr) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long b = i / S;
  const int pos = (int)(i - b * S);
  const int64_t id = ids[i];
  bool can = mask[i] != 0;
  for (int k = 0; k < sp.n; ++k) can = can && id != sp.id[k];
  const uint64_t t = (uint64_t)sample[b] * 65536ull + (uint64_t)pos;
  uint32_t r[4];
  philox4x32_10((uint32_t)t, (uint32_t)(t >> 32), epoch, 0u, k0, k1, r);
  const double two32 = 1.0 / 4294967296.0;
  int64_t o = id, lab = -100;
  if (can && (double)r[0] * two32 < p) {
    lab = id;
    const double u = (double)r[1] * two32;
    if (u < p_mask) o = mask_id;
    else if (u < p_mr) o = (int64_t)(((uint64_t)r[2] * (uint64_t)vocab) >> 32);
  }
  out_ids[i] = o;
  labels[i] = lab;
}

// ---- forward -----------------------------------------------------------------------------------------------------
// The epilogue of one 32-row x 128-column wave tile.  Transposed accumulators: acc[i][j][r] = C[wave*32 + i*16 + li]
// [j*16 + 4g + r]; a row's 128 columns are held by the four lanes li, li + 16, li + 32, li + 48.  TAIL: the tile that
// holds column V - 1 and the pad columns behind it; every other tile skips the column bounds.  The epilogue is VALU work
// of the order of the tile's MFMA time (K = H is only 4 to 16 K-steps), hence the fast exp: its relative error (about
// 2^-22 per term) is far inside what the merge's fp32 log and the row's sum already carry.
template <bool TAIL>
__device__ __forceinline__ void mlm_ce_epilogue(const f32x4 (&acc)[MlmCore::MI][MlmCore::NI], const float* __restrict__ bias,
                                                const int64_t* __restrict__ labels, bf16_t* __restrict__ Z,
                                                float* __restrict__ pmax, float* __restrict__ psum, float* __restrict__ tgt,
                                                int m0, int n0, int M, int V, long Vp) {
  using Core = MlmCore;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g4 = (lane >> 4) * 4;
  float b[Core::NI][4];
#pragma unroll
  for (int j = 0; j < Core::NI; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = n0 + j * 16 + g4 + r;
      b[j][r] = (!TAIL || c < V) ? rbf(bias[c]) : 0.f;
    }
#pragma unroll
  for (int i = 0; i < Core::MI; ++i) {
    const int row = m0 + wave * Core::WTM + i * 16 + li;
    const bool live = row < M;
    float z[Core::NI][4];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < Core::NI; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = rbf(acc[i][j][r] + b[j][r]);
        if (TAIL) {
          const bool in = n0 + j * 16 + g4 + r < V;
          z[j][r] = in ? v : 0.f;
          if (in) mx = fmaxf(mx, v);
        } else {
          z[j][r] = v;
          mx = fmaxf(mx, v);
        }
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < Core::NI; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (!TAIL || n0 + j * 16 + g4 + r < V) s += __expf(z[j][r] - mx);
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (live) {
      if (g4 == 0) {
        pmax[(long)blockIdx.y * M + row] = mx;
        psum[(long)blockIdx.y * M + row] = s;
      }
      // the target logit: only the lanes of a row whose label falls into this tile look for it (one tile in V / 128)
      const long d = (long)labels[row] - n0 - g4;
      if (d >= 0 && d < MLM_TILE && (d & 15) < 4 && (!TAIL || d + n0 + g4 < V)) {
#pragma unroll
        for (int j = 0; j < Core::NI; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (d == j * 16 + r) tgt[row] = z[j][r];
      }
      bf16_t* zr = Z + (long)row * Vp + n0 + g4;
#pragma unroll
      for (int j = 0; j < Core::NI; ++j)
        *(bf16x4*)(zr + j * 16) = (bf16x4){f2bf(z[j][0]), f2bf(z[j][1]), f2bf(z[j][2]), f2bf(z[j][3])};
    }
  }
}

// grid (row tiles, column tiles): the workgroups that run at one time share a few tiles of E and walk the row panels of
// h, which stay in L2 (M x H bf16 is a few MB).
__global__ __launch_bounds__(MlmCore::NTHREADS) void mlm_ce_tile_kernel(
    const bf16_t* __restrict__ h, const bf16_t* __restrict__ E, const float* __restrict__ bias,
    const int64_t* __restrict__ labels, bf16_t* __restrict__ Z, float* __restrict__ pmax, float* __restrict__ psum,
    float* __restrict__ tgt, int M, int V, int H, long Vp) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  using Core = MlmCore;
  const int m0 = blockIdx.x * MLM_TILE, n0 = blockIdx.y * MLM_TILE;
  f32x4 acc[Core::MI][Core::NI];
#pragma unroll
  for (int i = 0; i < Core::MI; ++i)
#pragma unroll
    for (int j = 0; j < Core::NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  Core::template mainloop<true>(h, H, m0, M, E, H, n0, V, H, smem, acc);
  if (n0 + MLM_TILE <= V) mlm_ce_epilogue<false>(acc, bias, labels, Z, pmax, psum, tgt, m0, n0, M, V, Vp);
  else mlm_ce_epilogue<true>(acc, bias, labels, Z, pmax, psum, tgt, m0, n0, M, V, Vp);
}

// one wave per row: lane l takes tiles l, l + 64, ...; the wave reductions add in a fixed order
__global__ __launch_bounds__(256) void mlm_ce_merge_kernel(const float* __restrict__ pmax, const float* __restrict__ psum,
                                                           const float* __restrict__ tgt, float* __restrict__ lse,
                                                           float* __restrict__ row_loss, int M, int nt) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  float mx = -INFINITY;
  for (int t = lane; t < nt; t += 64) mx = fmaxf(mx, pmax[(long)t * M + row]);
  mx = wave_max(mx);
  float s = 0.f;
  for (int t = lane; t < nt; t += 64) s += psum[(long)t * M + row] * expf(pmax[(long)t * M + row] - mx);
  s = wave_sum(s);
  if (lane == 0) {
    const float ls = logf(s);
    lse[row] = mx + ls;
    row_loss[row] = (mx - tgt[row]) + ls;      // the difference of two bf16 logits is exact in fp32
  }
}

// loss = sum of the rows' losses / M, one workgroup, fixed order
__global__ __launch_bounds__(256) void mlm_loss_kernel(const float* __restrict__ row_loss, float* __restrict__ loss, int M) {
  __shared__ float part[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < M; i += 256) s += row_loss[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = part[0] / (float)M;
}

// ---- backward ----------------------------------------------------------------------------------------------------
// z -> g = bf16((exp(z - lse) - [v == y]) * upstream / M), in place, 8 columns per thread; pad columns stay zero
__global__ __launch_bounds__(256) void mlm_ce_grad_kernel(bf16_t* __restrict__ Z, const float* __restrict__ lse,
                                                          const int64_t* __restrict__ labels,
                                                          const float* __restrict__ upstream, int M, int V, long Vp) {
  const long per_row = Vp / 8;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * per_row) return;
  const long row = i / per_row;
  const int c0 = (int)(i - row * per_row) * 8;
  const float scale = upstream[0] / (float)M, l = lse[row];
  const long lab = (long)labels[row];
  bf16_t* p = Z + row * Vp + c0;
  bf16x8 v = *(const bf16x8*)p;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = c0 + k;
    const float e = expf(bf2f(v[k]) - l) - (c == lab ? 1.f : 0.f);
    v[k] = c < V ? f2bf(e * scale) : f2bf(0.f);
  }
  *(bf16x8*)p = v;
}

// dbias[c] += sum over the rows of g[., c] in two ordered stages: chunk `y` of `rows` consecutive rows leaves its column
// sums in part[y][.] (8 columns per thread), then one thread per column adds the chunks in ascending order
__global__ __launch_bounds__(256) void mlm_dbias_part_kernel(const bf16_t* __restrict__ G, float* __restrict__ part, int M,
                                                             long Vp, int rows) {
  const long c8 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c8 >= Vp / 8) return;
  const int r0 = blockIdx.y * rows, r1 = min(M, r0 + rows);
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int m = r0; m < r1; ++m) {
    const bf16x8 v = *(const bf16x8*)(G + (long)m * Vp + c8 * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] += bf2f(v[k]);
  }
  float* o = part + (long)blockIdx.y * Vp + c8 * 8;
  *(f32x4*)o = (f32x4){a[0], a[1], a[2], a[3]};
  *(f32x4*)(o + 4) = (f32x4){a[4], a[5], a[6], a[7]};
}

__global__ __launch_bounds__(256) void mlm_dbias_sum_kernel(const float* __restrict__ part, float* __restrict__ dbias,
                                                            int nchunk, int V, long Vp) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= V) return;
  float s = 0.f;
  for (int y = 0; y < nchunk; ++y) s += part[(long)y * Vp + c];
  dbias[c] += s;
}

// dh = bf16(g E): M x H outputs over K = Vp are far fewer tiles than the device has CUs, so K is split: workgroup
// (row tile, column tile, z) multiplies K-steps [z steps, (z + 1) steps) and stores its fp32 tile into part[z]; a second
// kernel adds the splits in ascending order and rounds once.  The split is a function of (M, H, V) alone.
using DhCore = GemmCore<MLM_TILE, MLM_TILE, 2, 2>;

__global__ __launch_bounds__(DhCore::NTHREADS) void mlm_dh_splitk_kernel(const bf16_t* __restrict__ G,
                                                                         const bf16_t* __restrict__ ET,
                                                                         float* __restrict__ part, int M, int H, long Vp,
                                                                         int steps) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  using Core = DhCore;
  const int m0 = blockIdx.x * MLM_TILE, n0 = blockIdx.y * MLM_TILE;
  const long k0 = (long)blockIdx.z * steps * Core::BK;
  const int K = (int)min((long)steps * Core::BK, Vp - k0);
  f32x4 acc[Core::MI][Core::NI];
#pragma unroll
  for (int i = 0; i < Core::MI; ++i)
#pragma unroll
    for (int j = 0; j < Core::NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  Core::template mainloop<true>(G + k0, Vp, m0, M, ET + k0, Vp, n0, H, K, smem, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, g4 = (lane >> 4) * 4;
  const int wm = wave / 2, wn = wave % 2;
#pragma unroll
  for (int i = 0; i < Core::MI; ++i) {
    const int row = m0 + wm * Core::WTM + i * 16 + li;
    if (row >= M) continue;
    float* o = part + ((long)blockIdx.z * M + row) * H + n0 + wn * Core::WTN + g4;
#pragma unroll
    for (int j = 0; j < Core::NI; ++j) *(f32x4*)(o + j * 16) = acc[i][j];
  }
}

__global__ __launch_bounds__(256) void mlm_dh_reduce_kernel(const float* __restrict__ part, bf16_t* __restrict__ dh,
                                                            long n4, int nsplit) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  f32x4 a = *(const f32x4*)(part + i * 4);
  for (int z = 1; z < nsplit; ++z) {
    const f32x4 b = *(const f32x4*)(part + ((long)z * n4 + i) * 4);
    a[0] += b[0]; a[1] += b[1]; a[2] += b[2]; a[3] += b[3];
  }
  *(bf16x4*)(dh + i * 4) = (bf16x4){f2bf(a[0]), f2bf(a[1]), f2bf(a[2]), f2bf(a[3])};
}

__global__ __launch_bounds__(256) void mlm_add_kernel(float* __restrict__ dst, const float* __restrict__ src, long n4) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  f32x4 a = *(f32x4*)(dst + i * 4);
  const f32x4 b = *(const f32x4*)(src + i * 4);
  a[0] += b[0]; a[1] += b[1]; a[2] += b[2]; a[3] += b[3];
  *(f32x4*)(dst + i * 4) = a;
}

// E [V,H] bf16 -> E^T [H,Vp] bf16, pad columns zero; 64 x 64 tiles through LDS
__global__ __launch_bounds__(256) void mlm_transpose_kernel(const bf16_t* __restrict__ E, bf16_t* __restrict__ ET, int V,
                                                            int H, long Vp) {
  __shared__ bf16_t tile[64][66];
  const int v0 = blockIdx.x * 64, h0 = blockIdx.y * 64;
  const int c = threadIdx.x & 63, r4 = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int r = r4 + 4 * k;
    tile[r][c] = (v0 + r < V) ? E[(long)(v0 + r) * H + h0 + c] : f2bf(0.f);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int r = r4 + 4 * k;
    ET[(long)(h0 + r) * Vp + v0 + c] = tile[c][r];
  }
}

bool ce_shape_ok(int M, int V, int H) { return M > 0 && V > 0 && H > 0 && H % 128 == 0 && H <= 1024; }

size_t tn_ws_bytes(int M, int V, int H) {
  const snx_tn_problem pr = {nullptr, nullptr, nullptr, (int32_t)vpad(V), H, 0, 0};
  return snx_gemm_tn_workspace_bytes(&pr, 1, M);
}

inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }

// K split of the dh GEMM: about two workgroups per CU of a 256-CU device, at most 16 splits, whole K-steps
struct DhSplit { int nsplit, steps; };
DhSplit dh_split(int M, int V, int H) {
  const int nk = (int)(vpad(V) / DhCore::BK), tiles = cdiv(M, MLM_TILE) * (H / MLM_TILE);
  int want = cdiv(512, tiles);
  want = want < 1 ? 1 : (want > 16 ? 16 : want);
  want = want > nk ? nk : want;
  DhSplit s;
  s.steps = cdiv(nk, want);
  s.nsplit = cdiv(nk, s.steps);
  return s;
}

// row chunks of the bias sum: 32 rows, more when that many chunks would not fit the padded dE scratch they are kept in
int dbias_rows(int M, int H) { const int r = cdiv(M, H); return r > 32 ? r : 32; }

}  // namespace

extern "C" int snx_mlm_mask_tokens(const int64_t* input_ids, const int64_t* attention_mask, const int64_t* sample_index,
                                   int64_t* masked_ids, int64_t* labels, int32_t B, int32_t S, const int64_t* special_ids,
                                   int32_t n_special, int64_t mask_id, int32_t vocab, int64_t seed, int32_t epoch, double p,
                                   double p_mask, double p_random, hipStream_t st) {
  if (B < 0 || S < 1 || S > 65535 || vocab < 1 || n_special < 0 || n_special > 16 || epoch < 0) return SNX_E_SHAPE;
  if (mask_id < 0 || mask_id >= vocab) return SNX_E_ARG;
  if (B == 0) return SNX_OK;
  if (!input_ids || !attention_mask || !sample_index || !masked_ids || !labels || (n_special > 0 && !special_ids))
    return SNX_E_ARG;
  Specials sp{};
  sp.n = n_special;
  for (int k = 0; k < n_special; ++k) sp.id[k] = special_ids[k];
  const long n = (long)B * S;
  const uint64_t key = (uint64_t)seed;
  hipLaunchKernelGGL(mlm_mask_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, input_ids, attention_mask, sample_index,
                     masked_ids, labels, n, (int)S, sp, mask_id, (uint32_t)vocab, (uint32_t)key, (uint32_t)(key >> 32),
                     (uint32_t)epoch, p, p_mask, p_mask + p_random);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int64_t snx_mlm_vocab_padded(int32_t V) { return V > 0 ? (int64_t)vpad(V) : 0; }

extern "C" int snx_mlm_transpose_embeddings(const void* E, void* ET, int32_t V, int32_t H, hipStream_t st) {
  if (V <= 0 || H <= 0 || H % 64) return SNX_E_SHAPE;
  if (!E || !ET) return SNX_E_ARG;
  const long Vp = vpad(V);
  hipLaunchKernelGGL(mlm_transpose_kernel, dim3((unsigned)(Vp / 64), H / 64), dim3(256), 0, st, (const bf16_t*)E,
                     (bf16_t*)ET, (int)V, (int)H, Vp);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_mlm_ce_fwd(const void* h, const void* E, const float* bias, const int64_t* labels, void* z, float* part,
                              float* lse, float* row_loss, float* loss, int32_t M, int32_t V, int32_t H, hipStream_t st) {
  if (M == 0) return SNX_OK;                                 // nothing to launch: the caller reports loss 0
  if (!ce_shape_ok(M, V, H)) return SNX_E_SHAPE;
  if (!h || !E || !bias || !labels || !z || !part || !lse || !row_loss || !loss) return SNX_E_ARG;
  const long Vp = vpad(V);
  const int nt = (int)(Vp / MLM_TILE), tm = cdiv(M, MLM_TILE);
  if (nt > 65535) return SNX_E_SHAPE;
  float* pmax = part;
  float* psum = part + (size_t)nt * M;
  float* tgt = part + 2 * (size_t)nt * M;
  // a label outside [0, V) leaves its row's target unwritten: NaN, so the loss says so
  if (hipMemsetAsync(tgt, 0xFF, (size_t)M * 4, st) != hipSuccess) return SNX_E_ARG;
  hipLaunchKernelGGL(mlm_ce_tile_kernel, dim3(tm, nt), dim3(MlmCore::NTHREADS), MlmCore::LDS_BYTES, st, (const bf16_t*)h,
                     (const bf16_t*)E, bias, labels, (bf16_t*)z, pmax, psum, tgt, (int)M, (int)V, (int)H, Vp);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(mlm_ce_merge_kernel, dim3(cdiv(M, 4)), dim3(256), 0, st, pmax, psum, tgt, lse, row_loss, (int)M, nt);
  SNX_CHECK_LAUNCH();
  hipLaunchKernelGGL(mlm_loss_kernel, dim3(1), dim3(256), 0, st, row_loss, loss, (int)M);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" size_t snx_mlm_ce_bwd_workspace_bytes(int32_t M, int32_t V, int32_t H) {
  if (!ce_shape_ok(M, V, H)) return 0;
  return up256((size_t)vpad(V) * H * 4) + up256(tn_ws_bytes(M, V, H)) +
         up256((size_t)dh_split(M, V, H).nsplit * M * H * 4);
}

extern "C" int snx_mlm_ce_bwd(void* z, const float* lse, const int64_t* labels, const float* upstream, const void* h,
                              const void* ET, void* dh, float* dE, float* dbias, void* ws, size_t ws_bytes, int32_t M,
                              int32_t V, int32_t H, hipStream_t st) {
  if (M == 0) return SNX_OK;
  if (!ce_shape_ok(M, V, H)) return SNX_E_SHAPE;
  if (!z || !lse || !labels || !upstream || !h || !ET || !dh || !dE || !dbias || !ws) return SNX_E_ARG;
  if (ws_bytes < snx_mlm_ce_bwd_workspace_bytes(M, V, H)) return SNX_E_ARG;
  const long Vp = vpad(V);
  const size_t pad_bytes = up256((size_t)Vp * H * 4), tn_bytes = up256(tn_ws_bytes(M, V, H));
  float* dEpad = (float*)ws;
  char* tnws = (char*)ws + pad_bytes;
  float* dhpart = (float*)((char*)ws + pad_bytes + tn_bytes);
  const long n8 = (long)M * (Vp / 8);
  hipLaunchKernelGGL(mlm_ce_grad_kernel, dim3(cdiv(n8, 256)), dim3(256), 0, st, (bf16_t*)z, lse, labels, upstream, (int)M,
                     (int)V, Vp);
  SNX_CHECK_LAUNCH();
  {                                                                             // dh = bf16(g E), K split
    const DhSplit sp = dh_split(M, V, H);
    hipLaunchKernelGGL(mlm_dh_splitk_kernel, dim3(cdiv(M, MLM_TILE), H / MLM_TILE, sp.nsplit), dim3(DhCore::NTHREADS),
                       DhCore::LDS_BYTES, st, (const bf16_t*)z, (const bf16_t*)ET, dhpart, (int)M, (int)H, Vp, sp.steps);
    SNX_CHECK_LAUNCH();
    const long n4 = (long)M * H / 4;
    hipLaunchKernelGGL(mlm_dh_reduce_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, st, (const float*)dhpart, (bf16_t*)dh, n4,
                       sp.nsplit);
    SNX_CHECK_LAUNCH();
  }
  if (hipMemsetAsync(dEpad, 0, (size_t)Vp * H * 4, st) != hipSuccess) return SNX_E_ARG;
  RC(snx_gemm_tn_accum(z, h, dEpad, M, (int32_t)Vp, H, tnws, tn_bytes, st));   // g^T h, whole tiles
  const long n4 = (long)V * H / 4;
  hipLaunchKernelGGL(mlm_add_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, st, dE, (const float*)dEpad, n4);
  SNX_CHECK_LAUNCH();
  {                                                                             // the padded scratch is free again
    const int rows = dbias_rows(M, H), nchunk = cdiv(M, rows);
    hipLaunchKernelGGL(mlm_dbias_part_kernel, dim3(cdiv(Vp / 8, 256), nchunk), dim3(256), 0, st, (const bf16_t*)z, dEpad,
                       (int)M, Vp, rows);
    SNX_CHECK_LAUNCH();
    hipLaunchKernelGGL(mlm_dbias_sum_kernel, dim3(cdiv(V, 256)), dim3(256), 0, st, (const float*)dEpad, dbias, nchunk,
                       (int)V, Vp);
    SNX_CHECK_LAUNCH();
  }
  return SNX_OK;
}
