// The row kernel of the dense teacher's multi-vector head (BGE-M3's colbert_linear; include/snx.h "multi-vector teacher
// scores").  snx_teacher_forward_mv (teacher.hip) runs the head's GEMM over the last hidden state and then this kernel,
// which packs the rows that maxsim.hip scores.  One wave per token row, 16 B per lane, on the RowVec toolkit of rows.h, as
// the row kernels of teacher.hip.  The kernel lives in a file of its own because it is built with a flag of its own
// (snx/asmcheck.py FILE_FLAGS); teacher.hip keeps the project's flags and with them the code of its kernels.
#include "common.h"
#include "rows.h"
#include "snx.h"

namespace {

// mv[t - s - 1] = normalize(y[t] + bias) for every token row t of sequence s but its first (CLS), F.normalize's rule
// (x / max(||x||_2, 1e-12)) in fp32; the store has the type of y (one rounding to bf16)
template <int NV, bool F32>
__global__ __launch_bounds__(256) void teacher_mv_rows_kernel(const void* __restrict__ y, const float* __restrict__ bias,
                                                              const int32_t* __restrict__ cu, void* __restrict__ mv, int T,
                                                              int nseq, int H) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (t >= T) return;
  const int s = seq_of_token(cu, nseq, t);
  const long row = (long)t - s - 1;
  // the CLS row has no multi-vector; a cu_seqlens with an empty sequence (the contract rules it out) must not write outside
  if (t == cu[s] || row < 0 || row >= (long)T - nseq) return;
  RowVec<NV> x, b;
  if (F32) x.load_f32((const float*)y + (long)t * H, lane);
  else x.load_bf16((const bf16_t*)y + (long)t * H, lane);
  b.load_f32(bias, lane);
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x.v[i][e] += b.v[i][e];
      ss += x.v[i][e] * x.v[i][e];
    }
  const float nrm = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) x.v[i][e] = x.v[i][e] / nrm;
  if (F32) x.store_f32((float*)mv + row * H, lane);
  else x.store_bf16((bf16_t*)mv + row * H, lane);
}

inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

extern "C" int snx_teacher_mv_rows(const void* y, int32_t y_f32, const float* bias, const int32_t* cu_seqlens, void* mv,
                                   int32_t T, int32_t nseq, int32_t H, hipStream_t st) {
  if (!y || !bias || !cu_seqlens || !mv || T <= 0 || nseq <= 0 || nseq > T) return SNX_E_ARG;
  if (bad_h(H)) return SNX_E_SHAPE;
  if (misaligned(bias) || (y_f32 ? misaligned(y) || misaligned(mv) : (((uintptr_t)y | (uintptr_t)mv) & 7) != 0))
    return SNX_E_ARG;
  if (y_f32) {
    DISPATCH_NV(H, hipLaunchKernelGGL((teacher_mv_rows_kernel<NV, true>), dim3(cdiv(T, ROWS_PER_BLOCK)), dim3(256), 0, st, y,
                                      bias, cu_seqlens, mv, T, nseq, H));
  } else {
    DISPATCH_NV(H, hipLaunchKernelGGL((teacher_mv_rows_kernel<NV, false>), dim3(cdiv(T, ROWS_PER_BLOCK)), dim3(256), 0, st, y,
                                      bias, cu_seqlens, mv, T, nseq, H));
  }
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}
