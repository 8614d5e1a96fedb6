// The one-wave-per-row toolkit of the token-wise kernels (elementwise.hip, teacher.hip): a 256-thread block holds
// ROWS_PER_BLOCK waves, each wave one row of H = NV * 256 elements in registers, 16 bytes per lane and access.
#pragma once
#include "common.h"

constexpr int ROWS_PER_BLOCK = 4;   // 256 threads = 4 waves = 4 token rows

// one row, NV = H / 256 float4 per lane
template <int NV>
struct RowVec {
  f32x4 v[NV];
  __device__ __forceinline__ void load_f32(const float* p, int lane) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = *(const f32x4*)(p + (i * 64 + lane) * 4);
  }
  __device__ __forceinline__ void load_bf16(const bf16_t* p, int lane) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const bf16x4 b = *(const bf16x4*)(p + (i * 64 + lane) * 4);
      v[i] = (f32x4){bf2f(b[0]), bf2f(b[1]), bf2f(b[2]), bf2f(b[3])};
    }
  }
  __device__ __forceinline__ void store_f32(float* p, int lane) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) *(f32x4*)(p + (i * 64 + lane) * 4) = v[i];
  }
  // non-temporal forms ("stream_nt", config.h): rows that are read for the last time / written for a reader tens of
  // milliseconds away should not displace the next GEMM's operands from the L2 and the Infinity Cache
  __device__ __forceinline__ void load_f32_nt(const float* p, int lane) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = __builtin_nontemporal_load((const f32x4*)(p + (i * 64 + lane) * 4));
  }
  __device__ __forceinline__ void load_bf16_nt(const bf16_t* p, int lane) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const bf16x4 b = __builtin_nontemporal_load((const bf16x4*)(p + (i * 64 + lane) * 4));
      v[i] = (f32x4){bf2f(b[0]), bf2f(b[1]), bf2f(b[2]), bf2f(b[3])};
    }
  }
  __device__ __forceinline__ void store_f32_nt(float* p, int lane) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) __builtin_nontemporal_store(v[i], (f32x4*)(p + (i * 64 + lane) * 4));
  }
  __device__ __forceinline__ void store_bf16(bf16_t* p, int lane) const {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      bf16x4 b = {f2bf(v[i][0]), f2bf(v[i][1]), f2bf(v[i][2]), f2bf(v[i][3])};
      *(bf16x4*)(p + (i * 64 + lane) * 4) = b;
    }
  }
  __device__ __forceinline__ float sum() const {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    return wave_sum(s);
  }
};

// CALL with `constexpr int NV = H / 256`; a width the row kernels do not cover returns SNX_E_SHAPE from the caller
#define DISPATCH_NV(H, CALL)                       \
  switch ((H) / 256) {                             \
    case 1: { constexpr int NV = 1; CALL; } break; \
    case 2: { constexpr int NV = 2; CALL; } break; \
    case 3: { constexpr int NV = 3; CALL; } break; \
    case 4: { constexpr int NV = 4; CALL; } break; \
    default: return SNX_E_SHAPE;                   \
  }

static inline bool bad_h(int H) { return H <= 0 || (H % 256) != 0 || H > 1024; }
