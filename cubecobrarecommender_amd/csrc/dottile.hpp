// The fp32 dot-product tile of the inference kernels: one 256-thread workgroup
// computes 16*RM rows x 64 columns of dots over k, the operands staged through LDS 32 k at a time.
// Used by loo.hip (CHUNKED: the forward pass's pinned 64-wide chunks) and simbatch.hip, cubesim.hip
// (one running sum).  out_tile_kernel (recbatch.hip), loss_tile_kernel (evalloss.hip) and
// score_chunk_kernel (audience.hip) keep a copy of the CHUNKED loop that reads the columns before
// the rows: through this function they lost 1 to 3 % of their time (below, and DESIGN.md 4.10).
// The arithmetic per (row, column) is the same; the constants live here alone.  Device only.
#pragma once
#include "common.hpp"
#include "detmath.hpp"

namespace dottile {

constexpr int KS = 32;   // k per LDS stage
constexpr int TC = 64;   // columns per tile
constexpr int KCH = 64;  // dot chunk of the forward pass (pinned)
constexpr int NT = 256;  // workgroup: 16 column groups x 16 row groups

constexpr int F4 = KS / 4;   // float4 per staged row
constexpr int RS = NT / F4;  // rows staged per step: a thread stages local rows tid / F4 + RS * i

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// sum[j][e]: local row (tid >> 4) * RM + j, column 4 * (tid & 15) + e of the tile.
template <int RM>
struct Sums {
  float sum[RM][4];
};

// wcol(k)     : where the k-th value of this thread's column tid & 63 lies, null for a column outside
//               the tile (it is staged as zeros); the value at k + j lies j * wpitch floats behind it.
//               Asked once per stage, for the first of the 8 k that a thread stages 4 apart: one
//               64-bit multiply instead of eight (a callable returning the value cost the distance
//               tile 5 % of its time).
// hrow(lr, k) : the values k .. k + 3 of local row lr (zero for a row that takes no part)
// Both are asked for k below d only; d % KS == 0, and d % KCH == 0 where CHUNKED.  Per (row,
// column): acc = acc + h[k] * w[k] in ascending k from +0, multiply and add separately rounded;
// CHUNKED: acc restarts from +0 at every KCH-th k and the chunk sums are added in order from +0.
// The stages' LDS is the function's own.  The first barrier is at the top of the first stage: what
// the caller wrote to LDS before the call is visible to wcol and hrow, and the previous call's
// readers are done before the stages are overwritten.
template <int RM, bool CHUNKED, class WCol, class HRow>
__device__ __forceinline__ Sums<RM> run(int d, int wpitch, WCol wcol, HRow hrow) {
  using detm::addf;
  using detm::mulf;
  constexpr int TR = 16 * RM;
  __shared__ __attribute__((aligned(16))) float wsm[KS][TC];
  __shared__ __attribute__((aligned(16))) float hsm[TR][KS];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  float tot[RM][4], acc[RM][4];
#pragma unroll
  for (int j = 0; j < RM; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) tot[j][e] = acc[j][e] = 0.f;

  for (int k0 = 0; k0 < d; k0 += KS) {
    __syncthreads();  // the previous stage's readers are done
    {
      const float *wp = wcol(k0 + (tid >> 6));
      float w[KS / 4];
#pragma unroll
      for (int i = 0; i < KS / 4; ++i) w[i] = wp ? wp[(int64_t)(4 * i) * wpitch] : 0.f;
      float4 h[TR / RS];
#pragma unroll
      for (int i = 0; i < TR / RS; ++i) h[i] = hrow(tid / F4 + RS * i, k0 + 4 * (tid % F4));
#pragma unroll
      for (int i = 0; i < KS / 4; ++i) wsm[4 * i + (tid >> 6)][tid & 63] = w[i];
#pragma unroll
      for (int i = 0; i < TR / RS; ++i)
        *reinterpret_cast<float4 *>(&hsm[tid / F4 + RS * i][4 * (tid % F4)]) = h[i];
    }
    __syncthreads();
#pragma unroll 2
    for (int k4 = 0; k4 < KS / 4; ++k4) {
      // The rows' values are read before the columns'.  The order decides which operand of the
      // packed multiply the compiler puts first (this function is optimised before it is inlined, and
      // the kernel's own pass then orders the operands by the position of their LDS reads); with the
      // columns first it parts every multiply from its add by an s_nop.  Holding RM float4 of rows
      // costs the CHUNKED tile a wave per SIMD at RM 4 and 8: those kernels keep their own loop.
      float4 hr[RM], w[4];
#pragma unroll
      for (int j = 0; j < RM; ++j) hr[j] = *reinterpret_cast<const float4 *>(&hsm[ty * RM + j][4 * k4]);
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) w[kk] = *reinterpret_cast<const float4 *>(&wsm[4 * k4 + kk][4 * tx]);
#pragma unroll
      for (int j = 0; j < RM; ++j) {
        const float4 h = hr[j];
        const float hk[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          acc[j][0] = addf(acc[j][0], mulf(hk[kk], w[kk].x));
          acc[j][1] = addf(acc[j][1], mulf(hk[kk], w[kk].y));
          acc[j][2] = addf(acc[j][2], mulf(hk[kk], w[kk].z));
          acc[j][3] = addf(acc[j][3], mulf(hk[kk], w[kk].w));
        }
      }
    }
    if (CHUNKED && (k0 + KS) % KCH == 0) {  // a pinned chunk ends: its partial joins the total
#pragma unroll
      for (int j = 0; j < RM; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          tot[j][e] = addf(tot[j][e], acc[j][e]);
          acc[j][e] = 0.f;
        }
    }
  }

  Sums<RM> s;
#pragma unroll
  for (int j = 0; j < RM; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) s.sum[j][e] = CHUNKED ? tot[j][e] : acc[j][e];
  return s;
}

}  // namespace dottile
