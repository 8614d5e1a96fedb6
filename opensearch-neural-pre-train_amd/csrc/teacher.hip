// Dense teacher encoder: the forward of an XLM-RoBERTa encoder with CLS pooling (BGE-M3's dense head;
// ref:src/model/teachers/bge_m3.py:66-94, ref:scripts/precompute_teacher_scores.py:89-159 -- what sentence-transformers
// runs underneath).  `xr:` = transformers/models/xlm_roberta/modeling_xlm_roberta.py.
//
// The contractions are the tree's GEMMs and attention (snx_gemm_nt_bf16 / snx_attn_fwd, or snx_gemm_f32 and the tiled fp32
// attention forward of f32_path.hip); this file holds the glue between them that ModernBERT does not have: learned absolute
// positions and a token-type row in the embeddings, a bias on every Linear, post-LayerNorm with a bias, erf-GELU on a biased
// Linear, CLS pooling.  Row kernels: one wave per token row, 16 B per lane, on the RowVec toolkit of rows.h (shared with
// elementwise.hip); arena offsets and RC come from runtime.h.
//
// Cast points of the bf16 path: GEMM operands and GEMM outputs are bf16 (a bias added to a bf16 GEMM output that is a GEMM
// or attention operand is rounded to bf16 again); the residual stream h is fp32, GELU and softmax arithmetic are fp32, a
// row's LayerNorm is evaluated in fp64 and stored as fp32.  The fp32 path has no cast point.
#include "common.h"
#include "rows.h"
#include "runtime.h"
#include "snx.h"

namespace {

constexpr int EW_MAX_BLOCKS = 2048; // elementwise kernels: grid-stride beyond this

// A row's LayerNorm input in fp64.  These kernels are bound by their 16-byte loads and stores, the fp64 vector rate is far
// from a limit at <= 16 elements per lane, and it buys outputs that are the correctly rounded LayerNorm also where
// w * xhat + b cancels to a value orders of magnitude below the row's scale (an fp32 xhat is good to ~1e-7 of the ROW's
// scale, which is many bf16 steps of such an element).
template <int NV>
struct RowF64 {
  double v[NV][4];
  __device__ __forceinline__ void set(const RowVec<NV>& a) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] = (double)a.v[i][e];
  }
  __device__ __forceinline__ void add(const RowVec<NV>& a) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[i][e] += (double)a.v[i][e];
  }
};

// LN(x) * w + b -> h_out fp32 and (x_out != null) bf16(h_out)
template <int NV>
__device__ __forceinline__ void ln_affine_store(RowF64<NV>& x, const float* __restrict__ w, const float* __restrict__ b,
                                                float* h_out, bf16_t* x_out, int lane, int H, float eps) {
  RowVec<NV> wv, bv, o;
  wv.load_f32(w, lane);
  bv.load_f32(b, lane);
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < NV; ++i) s += (x.v[i][0] + x.v[i][1]) + (x.v[i][2] + x.v[i][3]);
  const double mean = wave_sum_f64(s) / (double)H;
  s = 0.0;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x.v[i][e] -= mean;
      s += x.v[i][e] * x.v[i][e];
    }
  const double rstd = 1.0 / sqrt(wave_sum_f64(s) / (double)H + (double)eps);
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) o.v[i][e] = (float)(x.v[i][e] * rstd * (double)wv.v[i][e] + (double)bv.v[i][e]);
  o.store_f32(h_out, lane);
  if (x_out) o.store_bf16(x_out, lane);
}

// XLMRobertaEmbeddings.forward (xr: word + token_type, then + position, LayerNorm; dropout is the identity in eval).
// ids and pos_ids are clamped into their tables: the binding validates them on the host, a stray id must not read outside.
template <int NV>
__global__ __launch_bounds__(256) void teacher_embed_ln_kernel(const int64_t* __restrict__ ids,
                                                               const int32_t* __restrict__ pos_ids,
                                                               const float* __restrict__ word, const float* __restrict__ pos,
                                                               const float* __restrict__ type0, const float* __restrict__ w,
                                                               const float* __restrict__ b, float* __restrict__ h_out,
                                                               bf16_t* __restrict__ x_out, int T, int H, int V, int P,
                                                               float eps) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (t >= T) return;
  long id = ids[t];
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);
  int p = pos_ids[t];
  p = p < 0 ? 0 : (p >= P ? P - 1 : p);
  RowVec<NV> a, y, z;
  a.load_f32(word + id * (long)H, lane);
  y.load_f32(pos + p * (long)H, lane);
  z.load_f32(type0, lane);
  RowF64<NV> x;
  x.set(a);
  x.add(z);
  x.add(y);
  ln_affine_store<NV>(x, w, b, h_out + (long)t * H, x_out ? x_out + (long)t * H : nullptr, lane, H, eps);
}

// XLMRobertaSelfOutput / XLMRobertaOutput (xr: LayerNorm(dense(x) + input_tensor)): h_out = LN((y + bias) + h) * w + b.
// h and h_out may be the same buffer (a wave reads its whole row before it writes it): no __restrict__ on them.
template <int NV, bool YF32>
__global__ __launch_bounds__(256) void teacher_bias_resid_ln_kernel(const float* h, const void* __restrict__ y,
                                                                    const float* __restrict__ bias,
                                                                    const float* __restrict__ w, const float* __restrict__ b,
                                                                    float* h_out, bf16_t* __restrict__ x_out, int T, int H,
                                                                    float eps) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (t >= T) return;
  RowVec<NV> hv, yv, bb;
  hv.load_f32(h + (long)t * H, lane);
  if (YF32) yv.load_f32((const float*)y + (long)t * H, lane);
  else yv.load_bf16((const bf16_t*)y + (long)t * H, lane);
  bb.load_f32(bias, lane);
  RowF64<NV> x;
  x.set(yv);
  x.add(bb);
  x.add(hv);
  ln_affine_store<NV>(x, w, b, h_out + (long)t * H, x_out ? x_out + (long)t * H : nullptr, lane, H, eps);
}

// y[t, :] += bias (GELU = false) or y[t, :] = gelu_erf(y[t, :] + bias) (GELU = true), in place on [T, N]; one item =
// 16 bytes of y (8 bf16 / 4 fp32), N8 / N4 items per row
template <bool GELU>
__global__ __launch_bounds__(256) void teacher_bias_bf16_kernel(bf16_t* __restrict__ y, const float* __restrict__ bias, long n8,
                                                                int N8) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
    const int c = (int)(i % N8) * 8;
    bf16x8 v = *(const bf16x8*)(y + i * 8);
    const f32x4 b0 = *(const f32x4*)(bias + c), b1 = *(const f32x4*)(bias + c + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float s = bf2f(v[e]) + (e < 4 ? b0[e & 3] : b1[e & 3]);
      v[e] = f2bf(GELU ? gelu_f(s) : s);
    }
    *(bf16x8*)(y + i * 8) = v;
  }
}
template <bool GELU>
__global__ __launch_bounds__(256) void teacher_bias_f32_kernel(float* __restrict__ y, const float* __restrict__ bias, long n4,
                                                               int N4) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const int c = (int)(i % N4) * 4;
    f32x4 v = *(const f32x4*)(y + i * 4);
    const f32x4 bb = *(const f32x4*)(bias + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float s = v[e] + bb[e];
      v[e] = GELU ? gelu_f(s) : s;
    }
    *(f32x4*)(y + i * 4) = v;
  }
}

// CLS pooling (sentence-transformers pooling_mode_cls_token) and F.normalize(p=2, eps=1e-12): one wave per sequence
template <int NV>
__global__ __launch_bounds__(256) void teacher_cls_normalize_kernel(const float* __restrict__ h, const int32_t* __restrict__ cu,
                                                                    float* __restrict__ cls, float* __restrict__ emb, int T,
                                                                    int nseq, int H) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (s >= nseq) return;
  int t = cu[s];
  t = t < 0 ? 0 : (t >= T ? T - 1 : t);
  RowVec<NV> x;
  x.load_f32(h + (long)t * H, lane);
  x.store_f32(cls + (long)s * H, lane);
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) ss += x.v[i][e] * x.v[i][e];
  const float nrm = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) x.v[i][e] = x.v[i][e] / nrm;
  x.store_f32(emb + (long)s * H, lane);
}

__global__ void teacher_fill_ones_kernel(int64_t* __restrict__ p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 1;
}

inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
inline int ew_blocks(long items) {
  const long b = (items + 255) / 256;
  return (int)(b < 1 ? 1 : (b > EW_MAX_BLOCKS ? EW_MAX_BLOCKS : b));
}

template <bool GELU>
int bias_launch(void* y, int y_f32, const float* bias, int T, int N, hipStream_t st) {
  if (!y || !bias || T <= 0) return SNX_E_ARG;
  if (N <= 0 || (N % 8) != 0) return SNX_E_SHAPE;
  if (misaligned(y) || misaligned(bias)) return SNX_E_ARG;
  if (y_f32) {
    const long n4 = (long)T * (N / 4);
    hipLaunchKernelGGL(teacher_bias_f32_kernel<GELU>, dim3(ew_blocks(n4)), dim3(256), 0, st, (float*)y, bias, n4, N / 4);
  } else {
    const long n8 = (long)T * (N / 8);
    hipLaunchKernelGGL(teacher_bias_bf16_kernel<GELU>, dim3(ew_blocks(n8)), dim3(256), 0, st, (bf16_t*)y, bias, n8, N / 8);
  }
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

// ---- the model ------------------------------------------------------------------------------------------------------
constexpr int MAX_LAYERS = 128;

bool desc_ok(const snx_teacher_desc* d) {
  return d && d->vocab > 0 && !bad_h(d->hidden) && d->inter > 0 && (d->inter % 64) == 0 && d->layers > 0 &&
         d->layers <= MAX_LAYERS && d->heads > 0 && d->head_dim == 64 && d->heads * 64 == d->hidden && d->max_pos > 0 &&
         d->type_vocab > 0 && d->pad_id >= 0 && d->ln_eps > 0.f;
}

// canonical parameter order of `params` (include/snx.h)
struct PIdx {
  static constexpr int word = 0, pos = 1, type = 2, emb_ln_w = 3, emb_ln_b = 4, per_layer = 16;
  static int base(int l) { return 5 + per_layer * l; }
  static int wq(int l) { return base(l); }
  static int bq(int l) { return base(l) + 1; }
  static int wk(int l) { return base(l) + 2; }
  static int bk(int l) { return base(l) + 3; }
  static int wv(int l) { return base(l) + 4; }
  static int bv(int l) { return base(l) + 5; }
  static int wo(int l) { return base(l) + 6; }
  static int bo(int l) { return base(l) + 7; }
  static int ln1_w(int l) { return base(l) + 8; }
  static int ln1_b(int l) { return base(l) + 9; }
  static int wi(int l) { return base(l) + 10; }
  static int bi(int l) { return base(l) + 11; }
  static int wo2(int l) { return base(l) + 12; }
  static int bo2(int l) { return base(l) + 13; }
  static int ln2_w(int l) { return base(l) + 14; }
  static int ln2_b(int l) { return base(l) + 15; }
};

// weight cache: per layer the bf16 matrices [Wq; Wk; Wv] [3H, H], Wo [H, H], Wi [I, H], Wo2 [H, I], then (after all
// layers) the stacked fp32 bias [bq; bk; bv] [3H] of every layer
struct Cache {
  size_t H, I, per_layer, bias0, total;
  explicit Cache(const snx_teacher_desc* d) : H(d->hidden), I(d->inter) {
    per_layer = align256((4 * H * H + 2 * H * I) * 2);
    bias0 = per_layer * d->layers;
    total = bias0 + align256(3 * H * 4) * d->layers;
  }
  size_t wqkv(int l) const { return per_layer * l; }
  size_t wo(int l) const { return wqkv(l) + 3 * H * H * 2; }
  size_t wi(int l) const { return wo(l) + H * H * 2; }
  size_t wo2(int l) const { return wi(l) + I * H * 2; }
  size_t bqkv(int l) const { return bias0 + align256(3 * H * 4) * l; }
};

// activation arena of one forward
struct Plan {
  size_t h, x, qkv, attn, y, u, lse, mask, total;
  Plan(const snx_teacher_desc* d, int T, int f32) {
    const size_t H = d->hidden, I = d->inter, e = f32 ? 4 : 2;
    Arena a;
    h = a.take((size_t)T * H * 4);
    x = f32 ? 0 : a.take((size_t)T * H * 2);
    qkv = a.take((size_t)T * 3 * H * e);
    attn = a.take((size_t)T * H * e);
    y = a.take((size_t)T * H * e);
    u = a.take((size_t)T * I * e);
    lse = f32 ? 0 : a.take((size_t)d->heads * T * 4);
    mask = f32 ? 0 : a.take((size_t)T * 8);
    total = a.off;
  }
};

}  // namespace

extern "C" int snx_teacher_embed_ln(const int64_t* ids, const int32_t* pos_ids, const float* word, const float* pos,
                                    const float* type0, const float* w, const float* b, float* h_out, void* x_out,
                                    int32_t T, int32_t H, int32_t vocab, int32_t max_pos, float eps, hipStream_t st) {
  if (!ids || !pos_ids || !word || !pos || !type0 || !w || !b || !h_out || T <= 0 || vocab <= 0 || max_pos <= 0)
    return SNX_E_ARG;
  if (bad_h(H)) return SNX_E_SHAPE;
  if (misaligned(word) || misaligned(pos) || misaligned(type0) || misaligned(w) || misaligned(b) || misaligned(h_out) ||
      ((uintptr_t)x_out & 7))
    return SNX_E_ARG;
  DISPATCH_NV(H, hipLaunchKernelGGL((teacher_embed_ln_kernel<NV>), dim3(cdiv(T, ROWS_PER_BLOCK)), dim3(256), 0, st, ids,
                                    pos_ids, word, pos, type0, w, b, h_out, (bf16_t*)x_out, T, H, vocab, max_pos, eps));
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_teacher_bias_resid_ln(const float* h, const void* y, int32_t y_f32, const float* bias, const float* w,
                                         const float* b, float* h_out, void* x_out, int32_t T, int32_t H, float eps,
                                         hipStream_t st) {
  if (!h || !y || !bias || !w || !b || !h_out || T <= 0) return SNX_E_ARG;
  if (bad_h(H)) return SNX_E_SHAPE;
  if (misaligned(h) || (y_f32 ? misaligned(y) : ((uintptr_t)y & 7) != 0) || misaligned(bias) || misaligned(w) ||
      misaligned(b) || misaligned(h_out) || ((uintptr_t)x_out & 7))
    return SNX_E_ARG;
  if (y_f32) {
    DISPATCH_NV(H, hipLaunchKernelGGL((teacher_bias_resid_ln_kernel<NV, true>), dim3(cdiv(T, ROWS_PER_BLOCK)), dim3(256), 0,
                                      st, h, y, bias, w, b, h_out, (bf16_t*)x_out, T, H, eps));
  } else {
    DISPATCH_NV(H, hipLaunchKernelGGL((teacher_bias_resid_ln_kernel<NV, false>), dim3(cdiv(T, ROWS_PER_BLOCK)), dim3(256), 0,
                                      st, h, y, bias, w, b, h_out, (bf16_t*)x_out, T, H, eps));
  }
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_teacher_bias_rows(void* y, int32_t y_f32, const float* bias, int32_t T, int32_t N, hipStream_t st) {
  return bias_launch<false>(y, y_f32, bias, T, N, st);
}

extern "C" int snx_teacher_bias_gelu(void* y, int32_t y_f32, const float* bias, int32_t T, int32_t N, hipStream_t st) {
  return bias_launch<true>(y, y_f32, bias, T, N, st);
}

extern "C" int snx_teacher_cls_normalize(const float* h, const int32_t* cu_seqlens, float* cls, float* emb, int32_t T,
                                         int32_t nseq, int32_t H, hipStream_t st) {
  if (!h || !cu_seqlens || !cls || !emb || T <= 0 || nseq <= 0) return SNX_E_ARG;
  if (bad_h(H)) return SNX_E_SHAPE;
  if (misaligned(h) || misaligned(cls) || misaligned(emb)) return SNX_E_ARG;
  DISPATCH_NV(H, hipLaunchKernelGGL((teacher_cls_normalize_kernel<NV>), dim3(cdiv(nseq, ROWS_PER_BLOCK)), dim3(256), 0, st,
                                    h, cu_seqlens, cls, emb, T, nseq, H));
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" int snx_teacher_attn_f32(const float* qkv, const int32_t* cu_seqlens, float* out, int32_t T, int32_t nseq,
                                    int32_t heads, hipStream_t st) {
  if (!qkv || !cu_seqlens || !out || T <= 0 || nseq <= 0) return SNX_E_ARG;
  if (heads <= 0) return SNX_E_SHAPE;
  if (misaligned(qkv) || misaligned(out)) return SNX_E_ARG;                // 16-byte loads and stores
  // xr: XLMRobertaSelfAttention -> SDPA, no mask inside an unpadded sequence, head_dim 64, every layer global
  return snx_attn_f32_fwd_tiled_x(qkv, cu_seqlens, nullptr, out, nullptr, T, nseq, heads, 64, -1, 0.125f, st);
}

extern "C" int32_t snx_teacher_param_count(const snx_teacher_desc* d) {
  return desc_ok(d) ? 5 + PIdx::per_layer * d->layers : 0;
}

extern "C" size_t snx_teacher_weight_cache_bytes(const snx_teacher_desc* d) { return desc_ok(d) ? Cache(d).total : 0; }

extern "C" int snx_teacher_weight_cache_refresh(const snx_teacher_desc* d, const void* const* params, void* cache,
                                                hipStream_t st) {
  if (!desc_ok(d)) return SNX_E_SHAPE;
  if (!params || !cache || misaligned(cache)) return SNX_E_ARG;
  const int n = snx_teacher_param_count(d);
  for (int i = 0; i < n; ++i)
    if (!params[i] || misaligned(params[i])) return SNX_E_ARG;
  const Cache c(d);
  const long H = d->hidden, I = d->inter;
  char* base = (char*)cache;
  auto F = [&](int i) { return (const float*)params[i]; };
  for (int l = 0; l < d->layers; ++l) {
    bf16_t* wqkv = (bf16_t*)(base + c.wqkv(l));
    RC(snx_cast_bf16(F(PIdx::wq(l)), wqkv, H * H, st));
    RC(snx_cast_bf16(F(PIdx::wk(l)), wqkv + H * H, H * H, st));
    RC(snx_cast_bf16(F(PIdx::wv(l)), wqkv + 2 * H * H, H * H, st));
    RC(snx_cast_bf16(F(PIdx::wo(l)), base + c.wo(l), H * H, st));
    RC(snx_cast_bf16(F(PIdx::wi(l)), base + c.wi(l), I * H, st));
    RC(snx_cast_bf16(F(PIdx::wo2(l)), base + c.wo2(l), H * I, st));
    float* bqkv = (float*)(base + c.bqkv(l));
    const int bsrc[3] = {PIdx::bq(l), PIdx::bk(l), PIdx::bv(l)};
    for (int j = 0; j < 3; ++j) {
      const hipError_t e = hipMemcpyAsync(bqkv + j * H, params[bsrc[j]], (size_t)H * 4, hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) return (int)e;
    }
  }
  return SNX_OK;
}

extern "C" size_t snx_teacher_workspace_bytes(const snx_teacher_desc* d, int32_t T, int32_t nseq, int32_t precision) {
  if (!desc_ok(d) || T <= 0 || nseq <= 0 || (precision != SNX_TEACHER_BF16 && precision != SNX_TEACHER_F32)) return 0;
  return Plan(d, T, precision == SNX_TEACHER_F32).total;
}

extern "C" int snx_teacher_forward(const snx_teacher_desc* d, const void* const* params, const void* wcache,
                                   const int64_t* ids, const int32_t* pos_ids, const int32_t* cu_seqlens, void* workspace,
                                   float* cls_out, float* emb_out, int32_t T, int32_t nseq, int32_t max_seqlen,
                                   int32_t precision, hipStream_t st) {
  if (!desc_ok(d)) return SNX_E_SHAPE;
  if (!params || !wcache || !ids || !pos_ids || !cu_seqlens || !workspace || !cls_out || !emb_out || T <= 0 || nseq <= 0 ||
      nseq > T || max_seqlen <= 0 || max_seqlen > T || misaligned(workspace) || misaligned(wcache))
    return SNX_E_ARG;
  if (precision != SNX_TEACHER_BF16 && precision != SNX_TEACHER_F32) return SNX_E_ARG;
  const int n = snx_teacher_param_count(d);
  for (int i = 0; i < n; ++i)
    if (!params[i]) return SNX_E_ARG;
  const bool f32 = precision == SNX_TEACHER_F32;
  const int H = d->hidden, I = d->inter, L = d->layers;
  const Plan s(d, T, f32);
  const Cache c(d);
  char* ws = (char*)workspace;
  const char* wc = (const char*)wcache;
  auto F = [&](int i) { return (const float*)params[i]; };
  float* h = (float*)(ws + s.h);
  void* x = f32 ? nullptr : (void*)(ws + s.x);
  void *qkv = ws + s.qkv, *attn = ws + s.attn, *y = ws + s.y, *u = ws + s.u;
  RC(snx_teacher_embed_ln(ids, pos_ids, F(PIdx::word), F(PIdx::pos), F(PIdx::type), F(PIdx::emb_ln_w), F(PIdx::emb_ln_b), h, x,
                          T, H, d->vocab, d->max_pos, d->ln_eps, st));
  int64_t* ones = nullptr;
  if (!f32) {
    ones = (int64_t*)(ws + s.mask);                              // snx_attn_fwd's key mask: unpadded rows, all tokens
    hipLaunchKernelGGL(teacher_fill_ones_kernel, dim3(cdiv(T, 256)), dim3(256), 0, st, ones, T);
    SNX_CHECK_LAUNCH();
  }
  // y[T, N] = a[T, K] W[N, K]^T on the precision's GEMM; fp32 weights come from `params`, bf16 ones from the cache
  auto linear = [&](const void* a, int pidx, size_t coff, void* out, int ldc, int N, int K) -> int {
    if (f32) return snx_gemm_f32((const float*)a, K, 1, F(pidx), K, 1, (float*)out, ldc, nullptr, 0, T, N, K, 0, st);
    return snx_gemm_nt_bf16(a, wc + coff, out, T, N, K, st);
  };
  for (int l = 0; l < L; ++l) {
    const float* bqkv = (const float*)(wc + c.bqkv(l));
    if (f32) {                                                   // three Linears into the thirds of qkv [T, 3, heads, 64]
      RC(linear(h, PIdx::wq(l), 0, (float*)qkv, 3 * H, H, H));
      RC(linear(h, PIdx::wk(l), 0, (float*)qkv + H, 3 * H, H, H));
      RC(linear(h, PIdx::wv(l), 0, (float*)qkv + 2 * H, 3 * H, H, H));
    } else {
      RC(linear(x, 0, c.wqkv(l), qkv, 3 * H, 3 * H, H));
    }
    RC(snx_teacher_bias_rows(qkv, f32, bqkv, T, 3 * H, st));
    if (f32) RC(snx_teacher_attn_f32((const float*)qkv, cu_seqlens, (float*)attn, T, nseq, d->heads, st));
    else RC(snx_attn_fwd(qkv, cu_seqlens, ones, attn, (float*)(ws + s.lse), T, nseq, max_seqlen, d->heads, 64, -1, st));
    RC(linear(attn, PIdx::wo(l), c.wo(l), y, H, H, H));
    RC(snx_teacher_bias_resid_ln(h, y, f32, F(PIdx::bo(l)), F(PIdx::ln1_w(l)), F(PIdx::ln1_b(l)), h, x, T, H, d->ln_eps, st));
    RC(linear(f32 ? (const void*)h : x, PIdx::wi(l), c.wi(l), u, I, I, H));
    RC(snx_teacher_bias_gelu(u, f32, F(PIdx::bi(l)), T, I, st));
    RC(linear(u, PIdx::wo2(l), c.wo2(l), y, H, H, I));
    RC(snx_teacher_bias_resid_ln(h, y, f32, F(PIdx::bo2(l)), F(PIdx::ln2_w(l)), F(PIdx::ln2_b(l)), h, x, T, H, d->ln_eps, st));
  }
  return snx_teacher_cls_normalize(h, cu_seqlens, cls_out, emb_out, T, nseq, H, st);
}
