// Multi-vector fixed-dimensional encodings (include/snx.h "multi-vector fixed-dimensional encodings"): MUVERA's map of a
// ragged set of bf16 rows to one fp32 vector whose inner products approximate the Chamfer / MaxSim sum.  Per repetition r
// a row x gets a code c_r(x) from the signs of k_sim products with planes[r], and a projected row y_r(x) = proj[r] x; the
// FDE's block (r, b) is the sum (queries) or the mean (documents) of y_r over the sequence's rows with c_r(x) == b, and an
// empty block of a document takes the projected row of its nearest code.  No training, no centroids.
//
// Packed operand   planes and proj become ONE operand, packed once per encoder in the order the MFMA reads it.  A PASS is
//                  64 projection columns, that is 64 / d_proj whole repetitions, plus the sign columns of exactly those
//                  repetitions (at most 4 x 6 = 24, padded to a 32-column tile with zeros): three 32-column tiles per pass.
//                  packed[((pass 3 + tile) D / 16 + kstep) 64 + lane] is the 16 bytes lane 32 h + c feeds to
//                  v_mfma_f32_32x32x16_bf16 as the B operand of that k-step: column c of the tile, k = 16 kstep + 8 h ..
//                  + 7.  A wave's load of a k-step is 1 KB of consecutive bytes, and the sign columns ride in the same K
//                  loop as the projection columns: a row of the store is read once per pass for both.
// Units            The host cuts the sequences of a call into units of whole sequences (about rows / 2,048 rows each, 64 ..
//                  1,024); one workgroup of four waves owns a unit and walks its rows 64 at a time.  A sequence never
//                  spans workgroups, so nothing is combined through memory and there is no atomic on a float anywhere.
// mvf_encode_kernel  Per 64-row tile and pass: the tile's rows go through a double-buffered 64-wide K-slice stage in LDS
//                  (one slice ahead in registers), the packed operand comes straight from L2 into registers (one slice
//                  ahead as well).  Wave 2 wm + wn keeps the 32 x 32 accumulator of rows 32 wm .., projection columns
//                  32 wn ..; the waves wn == 0 also keep the sign tile of their rows.  After the K loop the stage is free
//                  and becomes the park: the tile's [64][64] projected values as fp32, and next to it the rows' codes
//                  (the sign bits or-ed together with integer LDS atomics).
//                  Walk.  Lane l of a wave owns column l of the pass (repetition l / d_proj, component l % d_proj); wave w
//                  owns the buckets b with b % 4 == w.  A lane walks the rows of a sequence's segment of the tile in
//                  ascending order and adds the parked value into sum[(r B + b) d_proj + i] in LDS -- the FDE's own
//                  layout -- from +0 at the bucket's first row.  The state (sum, the bucket's first projected row, its row
//                  count and first row index) covers the whole FDE, at most 2 x 16 KB: a long document carries it across
//                  tiles while the passes take turns, several short documents of a tile use it one after the other.
//                  Finish.  When a segment ends its sequence, one thread per (repetition, bucket) of the pass names the
//                  bucket an empty block is filled from (smallest popcount(b xor c), then the lowest first row), and all
//                  threads write the pass's part of the FDE -- one division and one multiplication per element -- as
//                  16-byte stores.
// mvf_empty_kernel writes the zeros of the sequences without rows; mvf_pack_kernel packs the operand.
#include <cmath>
#include <vector>

#include "dense_common.h"
#include "snx.h"

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int MVF_THREADS = 256;
constexpr int MVF_TILE = 64;                   // store rows of a tile
constexpr int MVF_KT = 64;                     // K of a stage
constexpr int MVF_PITCH = 72;                  // bf16 per staged row; as floats per parked row: the same 18,432 bytes
constexpr int MVF_COLS = 64;                   // projection columns of a pass
constexpr int MVF_DMAX = 1024, MVF_KSIM_MAX = 6, MVF_REPS_MAX = 32, MVF_FDE_MAX = 4096;
constexpr int MVF_UNIT_MIN = 64, MVF_UNIT_MAX = 1024, MVF_UNITS_TARGET = 2048;
constexpr int MVF_SEQ_MAX = 1 << 24;           // sequences of a call

struct MvfGeom {
  int D, k_sim, B, reps, dp, rpp, npass, fde_dim;           // rpp: repetitions per pass
  bool ok;
  MvfGeom(int32_t D_, int32_t k_sim_, int32_t reps_, int32_t dp_) {
    D = D_; k_sim = k_sim_; reps = reps_; dp = dp_;
    ok = D > 0 && D % 64 == 0 && D <= MVF_DMAX && k_sim >= 0 && k_sim <= MVF_KSIM_MAX && reps >= 1 && reps <= MVF_REPS_MAX &&
         (dp == 16 || dp == 32 || dp == 64);
    B = ok ? 1 << k_sim : 1;
    rpp = ok ? MVF_COLS / dp : 1;
    npass = ok ? (reps + rpp - 1) / rpp : 1;
    fde_dim = ok ? reps * B * dp : 0;
    ok = ok && fde_dim <= MVF_FDE_MAX;
  }
  size_t packed_bytes() const { return (size_t)npass * 3 * (size_t)(D / 16) * 64 * 16; }
  size_t state_bytes() const { return ((size_t)2 * fde_dim + 2 * reps * B + rpp * B) * 4; }
};

// ------------------------------------------------------------------------------------------------ pack
__global__ __launch_bounds__(MVF_THREADS) void mvf_pack_kernel(const uint16_t* __restrict__ planes,
                                                               const uint16_t* __restrict__ proj, MvfGeom g, int64_t npieces,
                                                               u32x4* __restrict__ packed) {
  const int64_t idx = (int64_t)blockIdx.x * MVF_THREADS + threadIdx.x;
  if (idx >= npieces) return;
  const int lane = (int)(idx & 63), c = lane & 31, h = lane >> 5;
  const int64_t rest = idx >> 6;
  const int ks = (int)(rest % (g.D / 16)), tile = (int)(rest / (g.D / 16)), p = tile / 3, j = tile % 3;
  const uint16_t* row = nullptr;
  if (j < 2) {                                                // projection columns 64 p + 32 j + c of [reps d_proj]
    const int col = p * MVF_COLS + 32 * j + c;
    if (col < g.reps * g.dp) row = proj + (long)col * g.D;
  } else if (g.k_sim > 0 && c < g.rpp * g.k_sim) {            // plane c % k_sim of the pass's repetition c / k_sim
    const int r = p * g.rpp + c / g.k_sim;
    if (r < g.reps) row = planes + ((long)r * g.k_sim + c % g.k_sim) * g.D;
  }
  packed[idx] = row ? *(const u32x4*)(row + 16 * ks + 8 * h) : (u32x4){0u, 0u, 0u, 0u};
}

// ------------------------------------------------------------------------------------------------ sequences without rows
__global__ __launch_bounds__(MVF_THREADS) void mvf_empty_kernel(const int64_t* __restrict__ ptr, int32_t nseq, int32_t fde_dim,
                                                                float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long s = (long)blockIdx.x * (MVF_THREADS / 64) + (threadIdx.x >> 6);
  if (s >= nseq || ptr[s + 1] > ptr[s]) return;
  for (int v = lane; v < fde_dim / 4; v += 64) *(f32x4*)(out + s * fde_dim + 4 * v) = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// ------------------------------------------------------------------------------------------------ encode
__global__ __launch_bounds__(MVF_THREADS) void mvf_encode_kernel(
    const bf16_t* __restrict__ rows, const int64_t* __restrict__ ptr, const int32_t* __restrict__ unit,
    const u32x4* __restrict__ packed, MvfGeom g, int32_t is_query, float scale, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint16_t stage[2][MVF_TILE][MVF_PITCH];
  __shared__ uint32_t codes[MVF_TILE][4];
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float (*park)[MVF_PITCH] = (float (*)[MVF_PITCH])&stage[0][0][0];            // the stage, after the K loop
  float* sum = (float*)smem;                                  // [fde_dim]: the FDE's layout
  float* first = sum + g.fde_dim;                             // [fde_dim]: the projected row of a bucket's first row
  int32_t* cnt = (int32_t*)(first + g.fde_dim);               // [reps B]: rows of a bucket
  int32_t* frow = cnt + g.reps * g.B;                         // [reps B]: a bucket's first row, counted from the sequence's
  int32_t* src = frow + g.reps * g.B;                         // [rpp B]: the bucket a block of the pass is written from
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, c = lane & 31, h = lane >> 5;
  const int s0 = unit[blockIdx.x], s1 = unit[blockIdx.x + 1];
  const long r_begin = ptr[s0], r_end = ptr[s1];
  const int nk = g.D / MVF_KT, ksteps = g.D / 16;
  const int rl = lane / g.dp, ci = lane % g.dp;               // the walk: this lane's column of a pass
  const bool sign = wn == 0 && g.k_sim > 0;
  int tile_cur = s0;                                          // the sequence of the tile's first row, or one before it
  for (long row0 = r_begin; row0 < r_end; row0 += MVF_TILE) {
    const int nv = (int)min((long)MVF_TILE, r_end - row0);
    int cur = tile_cur;
    for (int p = 0; p < g.npass; ++p) {
      // ---- the [64, D] x [D, 64 + 32] product: k ascending, the same steps for every row and column
      const u32x4* bp_src = packed + (long)(p * 3 + wn) * ksteps * 64 + lane;
      const u32x4* bs_src = packed + (long)(p * 3 + 2) * ksteps * 64 + lane;
      f32x16 acc, sacc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = sacc[r] = 0.f;
      u32x4 ra[2], bp[4], bs[4], nbp[4], nbs[4];
      auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = (t >> 3) + 32 * i;
          ra[i] = row < nv ? *(const u32x4*)(rows + (row0 + row) * g.D + k0 + (t & 7) * 8) : (u32x4){0u, 0u, 0u, 0u};
        }
      };
      auto put = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *(u32x4*)&stage[buf][(t >> 3) + 32 * i][(t & 7) * 8] = ra[i];
      };
      fetch(0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        bp[u] = bp_src[u * 64];
        bs[u] = sign ? bs_src[u * 64] : (u32x4){0u, 0u, 0u, 0u};
      }
      codes[t >> 2][t & 3] = 0u;
      put(0);
      __syncthreads();
      for (int kt = 0; kt < nk; ++kt) {
        const int cur_buf = kt & 1;
        if (kt + 1 < nk) {
          fetch((kt + 1) * MVF_KT);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            nbp[u] = bp_src[((kt + 1) * 4 + u) * 64];
            if (sign) nbs[u] = bs_src[((kt + 1) * 4 + u) * 64];
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bf16x8 a = *(const bf16x8*)&stage[cur_buf][wm * 32 + c][16 * u + 8 * h];
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, bp[u]), acc, 0, 0, 0);
          if (sign) sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, bs[u]), sacc, 0, 0, 0);
        }
        if (kt + 1 < nk) {
          put(cur_buf ^ 1);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            bp[u] = nbp[u];
            if (sign) bs[u] = nbs[u];
          }
        }
        __syncthreads();
      }
      // ---- park: acc[r] = <row 32 wm + (r & 3) + 8 (r >> 2) + 4 h, column 32 wn + c>
#pragma unroll
      for (int r = 0; r < 16; ++r) park[wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h][wn * 32 + c] = acc[r];
      if (sign && c < g.rpp * g.k_sim) {
        const int srl = c / g.k_sim;
        const uint32_t bit = 1u << (c % g.k_sim);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (sacc[r] > 0.f) atomicOr(&codes[wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h][srl], bit);
      }
      __syncthreads();
      // ---- the tile's segments, one sequence each
      cur = tile_cur;
      const int rep = p * g.rpp + rl;
      const int rb0 = p * g.rpp * g.B;                        // the pass's first (repetition, bucket)
      const int nrb = min(g.rpp, g.reps - p * g.rpp) * g.B;   // at most 256
      long row = row0;
      while (row < row0 + nv) {
        while (ptr[cur + 1] <= row) ++cur;                    // row < ptr[s1]: ends inside the unit
        const long a = ptr[cur], e = ptr[cur + 1];
        const long seg_end = min(e, row0 + nv);
        if (row == a) {                                       // the sequence starts here: its buckets are empty
          if (t < nrb) cnt[rb0 + t] = 0;
          __syncthreads();
        }
        if (rep < g.reps && wave < g.B) {
          const int j1 = (int)(seg_end - row0);
          for (int j = (int)(row - row0); j < j1; ++j) {      // ascending rows: the sum's order
            const int code = (int)codes[j][rl];
            if ((code & 3) == wave) {
              const int rb = rep * g.B + code, idx = rb * g.dp + ci;
              const int n = cnt[rb];                          // the lanes of a repetition read and write the same values
              const float y = park[j][lane];
              sum[idx] = (n ? sum[idx] : 0.f) + y;
              if (!n) {
                first[idx] = y;
                frow[rb] = (int)(row0 + j - a);
              }
              cnt[rb] = n + 1;
            }
          }
        }
        __syncthreads();
        if (seg_end == e) {                                   // the sequence ends here: this pass's part of its FDE
          if (t < nrb) {
            const int b = t & (g.B - 1), base = rb0 + (t - b);
            int best = -1;
            if (cnt[rb0 + t] > 0) {
              best = b;
            } else if (!is_query) {                           // smallest popcount(b xor code), then the lowest row
              int bd = 64, bf = 0;
              for (int cc = 0; cc < g.B; ++cc) {
                if (cnt[base + cc] <= 0) continue;
                const int d = __popc((unsigned)(b ^ cc)), f = frow[base + cc];
                if (d < bd || (d == bd && f < bf)) { bd = d; bf = f; best = cc; }
              }
            }
            src[t] = best;
          }
          __syncthreads();
          float* dst = out + (long)cur * g.fde_dim + (long)rb0 * g.dp;
          for (int v = t; v < nrb * g.dp / 4; v += MVF_THREADS) {
            const int e4 = 4 * v, rbl = e4 / g.dp, i = e4 % g.dp;
            const int n = cnt[rb0 + rbl], sb = src[rbl];
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
            if (n > 0) {
              const f32x4 s = *(const f32x4*)(sum + (rb0 + rbl) * g.dp + i);
              const float fn = (float)n;
#pragma unroll
              for (int u = 0; u < 4; ++u) o[u] = is_query ? s[u] * scale : s[u] / fn * scale;
            } else if (sb >= 0) {
              const f32x4 f = *(const f32x4*)(first + (rb0 + (rbl & ~(g.B - 1)) + sb) * g.dp + i);
#pragma unroll
              for (int u = 0; u < 4; ++u) o[u] = scale * f[u];
            }
            *(f32x4*)(dst + e4) = o;
          }
          __syncthreads();
        }
        row = seg_end;
      }
    }
    tile_cur = cur;
  }
}

// ------------------------------------------------------------------------------------------------ host
// ptr [n + 1] ascends from 0 and ends within `rows`
inline bool mvf_ptr_ok(const int64_t* ptr, int32_t n, int64_t rows) {
  if (!ptr || ptr[0] != 0) return false;
  for (int32_t s = 0; s < n; ++s)
    if (ptr[s + 1] < ptr[s]) return false;
  return ptr[n] <= rows;
}

// the units of a call (first sequence of each, and the end) and the workspace: device copies of ptr and of the units
struct MvfPlan {
  std::vector<int32_t> starts;
  size_t dptr, unit, total;
  bool ok;
  MvfPlan(const int64_t* ptr, int32_t nseq) {
    const int64_t rows = ptr[nseq];
    int64_t target = (rows / MVF_UNITS_TARGET + 63) / 64 * 64;
    target = target < MVF_UNIT_MIN ? MVF_UNIT_MIN : (target > MVF_UNIT_MAX ? MVF_UNIT_MAX : target);
    ok = true;
    starts.push_back(0);
    for (int32_t s = 0; s < nseq; ++s) {
      if (ptr[s + 1] - ptr[s] > 0x7FFFFFFFL) ok = false;      // a bucket's first row is an int32
      if (ptr[s + 1] - ptr[starts.back()] >= target) starts.push_back(s + 1);
    }
    if (starts.back() != nseq) starts.push_back(nseq);
    Arena a;
    dptr = a.take(((size_t)nseq + 1) * 8);
    unit = a.take(starts.size() * 4);
    total = a.off;
  }
};

}  // namespace

extern "C" size_t snx_mv_fde_packed_bytes(int32_t D, int32_t k_sim, int32_t reps, int32_t d_proj) {
  const MvfGeom g(D, k_sim, reps, d_proj);
  return g.ok ? g.packed_bytes() : 0;
}

extern "C" int snx_mv_fde_pack(const void* planes, const void* proj, int32_t D, int32_t k_sim, int32_t reps, int32_t d_proj,
                               void* packed, hipStream_t st) {
  const MvfGeom g(D, k_sim, reps, d_proj);
  if (!g.ok) return SNX_E_SHAPE;
  if (!proj || !packed || (g.k_sim > 0 && !planes) || ((uintptr_t)planes & 15) != 0 || ((uintptr_t)proj & 15) != 0 ||
      ((uintptr_t)packed & 15) != 0)
    return SNX_E_ARG;
  const int64_t npieces = (int64_t)(g.packed_bytes() / 16);
  hipLaunchKernelGGL(mvf_pack_kernel, dim3((unsigned)((npieces + MVF_THREADS - 1) / MVF_THREADS)), dim3(MVF_THREADS), 0, st,
                     (const uint16_t*)planes, (const uint16_t*)proj, g, npieces, (u32x4*)packed);
  SNX_CHECK_LAUNCH();
  return SNX_OK;
}

extern "C" size_t snx_mv_fde_workspace_bytes(const int64_t* mv_ptr, int32_t nseq) {
  if (nseq <= 0 || nseq > MVF_SEQ_MAX || !mvf_ptr_ok(mv_ptr, nseq, 0x7FFFFFFFFFFFFFFFL)) return 0;
  const MvfPlan plan(mv_ptr, nseq);
  return plan.ok ? plan.total : 0;
}

extern "C" int snx_mv_fde_encode(const void* rows, int64_t nrows, const int64_t* mv_ptr, int32_t nseq, const void* packed,
                                 int32_t D, int32_t k_sim, int32_t reps, int32_t d_proj, int32_t is_query, float* out,
                                 void* workspace, size_t ws_bytes, hipStream_t st) {
  const MvfGeom g(D, k_sim, reps, d_proj);
  if (!g.ok || nrows < 0 || nseq < 0 || nseq > MVF_SEQ_MAX) return SNX_E_SHAPE;
  if (nseq == 0) return SNX_OK;
  if (!packed || !out || !workspace || ((uintptr_t)rows & 15) != 0 || ((uintptr_t)packed & 15) != 0 ||
      ((uintptr_t)out & 15) != 0 || ((uintptr_t)workspace & 15) != 0)
    return SNX_E_ARG;
  // mv_ptr is pageable host memory (snx.h): everything the kernel will trust is checked here, before any launch;
  // hipMemcpyAsync below has staged it when it returns
  if (!mvf_ptr_ok(mv_ptr, nseq, nrows)) return SNX_E_ARG;
  const int64_t used = mv_ptr[nseq];
  if (used > 0 && !rows) return SNX_E_ARG;
  const MvfPlan plan(mv_ptr, nseq);
  if (!plan.ok) return SNX_E_SHAPE;
  if (ws_bytes < plan.total) return SNX_E_ARG;
  char* ws = (char*)workspace;
  hipError_t e = hipMemcpyAsync(ws + plan.dptr, mv_ptr, ((size_t)nseq + 1) * 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(ws + plan.unit, plan.starts.data(), plan.starts.size() * 4, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return (int)e;
  const int64_t* dptr = (const int64_t*)(ws + plan.dptr);
  hipLaunchKernelGGL(mvf_empty_kernel, dim3((unsigned)((nseq + MVF_THREADS / 64 - 1) / (MVF_THREADS / 64))), dim3(MVF_THREADS),
                     0, st, dptr, nseq, g.fde_dim, out);
  SNX_CHECK_LAUNCH();
  if (used > 0) {
    const float scale = (float)(1.0 / std::sqrt((double)g.dp));
    hipLaunchKernelGGL(mvf_encode_kernel, dim3((unsigned)(plan.starts.size() - 1)), dim3(MVF_THREADS), g.state_bytes(), st,
                       (const bf16_t*)rows, dptr, (const int32_t*)(ws + plan.unit), (const u32x4*)packed, g, is_query, scale,
                       out);
    SNX_CHECK_LAUNCH();
  }
  return SNX_OK;
}
