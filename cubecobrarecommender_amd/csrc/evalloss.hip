// cc_recommend_batch_loss_fp32 — the reconstruction loss (Keras binary cross-entropy of output 1)
// and the categorical-accuracy prediction of R rows, on the logits that recommend computes.
//
// The chain: target bitmasks, cc::infer_h3_launch on x (h3 is exactly recommend's), then
//   loss_tile_kernel : out_tile_kernel's tile (recbatch.hip: 64 cards x 16*RM rows, its copy of the
//                      dot-product tile's loop) with another epilogue:
//                      instead of a sort key per card it reduces, per row of the tile, the fp64
//                      loss terms of the tile's 64 cards and the first maximum of p'.  One double,
//                      one float and one int per (tile, row) go to the workspace; nothing of size
//                      R x V is written.
//   loss_rows_kernel : one thread per row adds the tile partials in ascending tile order, divides
//                      by V and keeps the first maximum.
// Pinned arithmetic (tests/eval_loss_ref.py restates it bit for bit):
//   z     fp32 logit as above, + bo
//   t     fp64, no contraction: max(z, 0) - z*y + det_log(1 + det_exp(-|z|)), y from the mask;
//         a card >= V contributes +0.0
//   tile  a lane's 4 cards ((t0 + t1) + t2) + t3, then the 16 lanes of the row group by an xor
//         butterfly (offsets 1, 2, 4, 8: a = a + a[lane ^ off])
//   row   tile partials added from 0.0 in ascending order, / (double)V
//   pred  first index of the maximum of p' = z >= SIG_SAT ? 1 : det_sigmoid32(z) (the rule of
//         cc_sigmoid_cat_accuracy with the deterministic sigmoid); ties go to the lower index
//         within a lane, across the butterfly and across tiles
#include "common.hpp"
#include "detmath.hpp"
#include "dottile.hpp"
#include "infer.hpp"

namespace {

constexpr int KCH = dottile::KCH, KS = dottile::KS;  // the tile's constants (dottile.hpp)
constexpr int TC = dottile::TC;   // cards per output tile
constexpr int ONT = dottile::NT;  // output-tile workgroup
// Eigen scalar_logistic_op<float>: exactly 1 from here on (metrics.hip)
constexpr float SIG_SAT = 15.7243833541870117f;

using detm::addf;
using detm::mulf;
__device__ __forceinline__ double addd(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

// TF's sigmoid_cross_entropy_with_logits of one logit (oracle/model_ref.py's bce)
__device__ __forceinline__ double bce_term(float z, bool y) {
#pragma clang fp contract(off)
  const double z64 = (double)z;
  const double m = z64 > 0.0 ? z64 : 0.0;
  const double zy = z64 * (y ? 1.0 : 0.0);
  const double az = z64 < 0.0 ? -z64 : z64;
  const double l = detm::det_log(1.0 + detm::det_exp(-az));
  const double a = m - zy;
  return a + l;
}

// tile_loss / tile_p / tile_i: [tiles][R], tile-major so that loss_rows_kernel reads coalesced
template <int RM>
__global__ __launch_bounds__(ONT) void loss_tile_kernel(
    const float *__restrict__ h3, const float *__restrict__ Wo, const float *__restrict__ bo, int d,
    int V, int R, const uint32_t *__restrict__ bits, int VW, double *__restrict__ tile_loss,
    float *__restrict__ tile_p, int32_t *__restrict__ tile_i) {
  constexpr int TR = 16 * RM;
  __shared__ __attribute__((aligned(16))) float wsm[KS][TC];
  __shared__ __attribute__((aligned(16))) float hsm[TR][KS];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int nb = blockIdx.x * TC;  // first card of the tile
  const int rb = blockIdx.y * TR;  // first row of the tile
  float tot[RM][4], acc[RM][4];
#pragma unroll
  for (int j = 0; j < RM; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) tot[j][e] = acc[j][e] = 0.f;

  // out_tile_kernel's loop, statement for statement
  for (int k0 = 0; k0 < d; k0 += KS) {
    __syncthreads();  // the previous stage's readers are done
    {
      const int n = tid & 63, gn = nb + n;
      const float *Wp = Wo + ((int64_t)k0 + (tid >> 6)) * V + gn;
      float w[KS / 4];
#pragma unroll
      for (int i = 0; i < KS / 4; ++i) w[i] = gn < V ? Wp[(int64_t)(4 * i) * V] : 0.f;
      constexpr int Q = KS / 4, RS = ONT / Q;  // float4 per row, rows per step
      float4 h[TR / RS];
#pragma unroll
      for (int i = 0; i < TR / RS; ++i) {
        const int gr = rb + tid / Q + RS * i;
        h[i] = gr < R ? *reinterpret_cast<const float4 *>(h3 + (int64_t)gr * d + k0 + 4 * (tid % Q))
                      : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int i = 0; i < KS / 4; ++i) wsm[4 * i + (tid >> 6)][n] = w[i];
#pragma unroll
      for (int i = 0; i < TR / RS; ++i)
        *reinterpret_cast<float4 *>(&hsm[tid / Q + RS * i][4 * (tid % Q)]) = h[i];
    }
    __syncthreads();
#pragma unroll 2
    for (int k4 = 0; k4 < KS / 4; ++k4) {
      float4 w[4];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) w[kk] = *reinterpret_cast<const float4 *>(&wsm[4 * k4 + kk][4 * tx]);
#pragma unroll
      for (int j = 0; j < RM; ++j) {
        const float4 h = *reinterpret_cast<const float4 *>(&hsm[ty * RM + j][4 * k4]);
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
    if ((k0 + KS) % KCH == 0) {  // a pinned chunk ends: its partial joins the total
#pragma unroll
      for (int j = 0; j < RM; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          tot[j][e] = addf(tot[j][e], acc[j][e]);
          acc[j][e] = 0.f;
        }
    }
  }

  // No lane leaves before the butterflies: one with n0 >= V carries +0.0 and no candidate.
  const int n0 = nb + 4 * tx;
  float bias[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) bias[e] = n0 + e < V ? bo[n0 + e] : 0.f;
#pragma unroll
  for (int j = 0; j < RM; ++j) {
    const int gr = rb + ty * RM + j;
    // n0 % 4 == 0: one word for all 4 cards; never read past the row's VW words or past row R
    const uint32_t word = (gr < R && n0 < V) ? bits[(int64_t)gr * VW + (n0 >> 5)] : 0u;
    double s = 0.0;
    float bp = -1.f;  // below every p'
    int bi = 0x7FFFFFFF;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float z = addf(tot[j][e], bias[e]);
      const bool in = n0 + e < V;
      const double t = in ? bce_term(z, (word >> ((n0 + e) & 31)) & 1u) : 0.0;
      s = e == 0 ? t : addd(s, t);
      const float p = z >= SIG_SAT ? 1.0f : detm::det_sigmoid32(z);
      if (in && p > bp) bp = p, bi = n0 + e;  // ascending e: the first maximum
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      s = addd(s, __shfl_xor(s, off));
      const float op = __shfl_xor(bp, off);
      const int oi = __shfl_xor(bi, off);
      if (op > bp || (op == bp && oi < bi)) bp = op, bi = oi;
    }
    if (tx == 0 && gr < R) {
      const int64_t o = (int64_t)blockIdx.x * R + gr;
      tile_loss[o] = s;
      tile_p[o] = bp;
      tile_i[o] = bi;
    }
  }
}

__global__ __launch_bounds__(256) void loss_rows_kernel(const double *__restrict__ tile_loss,
                                                        const float *__restrict__ tile_p,
                                                        const int32_t *__restrict__ tile_i,
                                                        int tiles, int V, int R,
                                                        double *__restrict__ row_loss,
                                                        int32_t *__restrict__ row_pred) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  double s = 0.0;
  float bp = -1.f;
  int bi = 0;
  for (int t = 0; t < tiles; ++t) {
    const int64_t o = (int64_t)t * R + r;
    s = addd(s, tile_loss[o]);
    const float p = tile_p[o];
    if (p > bp) bp = p, bi = tile_i[o];  // ascending tiles: the first maximum
  }
  row_loss[r] = s / (double)V;
  row_pred[r] = bi;
}

// workspace: [E1 partials R*cap*d][zlat R*64][h3 R*d][target bitmasks R*VW]
//            [tile losses tiles*R f64][tile maxima tiles*R f32][their cards tiles*R i32]
struct LossWs {
  size_t part, zlat, h3, bits, tloss, tp, ti, total;
  int VW, tiles;
};
LossWs loss_ws(int V, int d, int R, int max_n) {
  LossWs w;
  const size_t r = (size_t)std::max(R, 1), dd = (size_t)std::max(d, 64);
  w.VW = (std::max(V, 1) + 31) / 32;
  w.tiles = (int)cdiv(std::max(V, 1), TC);
  size_t o = 0;
  w.part = o, o += align256(r * cc::infer_gather_cap(max_n) * dd * sizeof(float));
  w.zlat = o, o += align256(r * 64 * sizeof(float));
  w.h3 = o, o += align256(r * dd * sizeof(float));
  w.bits = o, o += align256(r * w.VW * sizeof(uint32_t));
  w.tloss = o, o += align256(r * w.tiles * sizeof(double));
  w.tp = o, o += align256(r * w.tiles * sizeof(float));
  w.ti = o, o += align256(r * w.tiles * sizeof(int32_t));
  w.total = o;
  return w;
}

template <int RM>
void launch_loss(dim3 grid, hipStream_t s, const float *h3, const float *Wo, const float *bo, int d,
                 int V, int R, const uint32_t *bits, int VW, double *tl, float *tp, int32_t *ti) {
  grid.y = (unsigned)cdiv(R, 16 * RM);
  hipLaunchKernelGGL(loss_tile_kernel<RM>, grid, dim3(ONT), 0, s, h3, Wo, bo, d, V, R, bits, VW, tl,
                     tp, ti);
}

}  // namespace

extern "C" size_t cc_recommend_batch_loss_ws_size(int32_t V, int32_t d, int32_t R, int32_t max_n) {
  return loss_ws(V, d, R, max_n).total + 256;
}

extern "C" int cc_recommend_batch_loss_fp32(const float *params, int32_t V, int32_t d, int32_t R,
                                            const int32_t *row_ptr, const int32_t *idx,
                                            int32_t max_n, const int32_t *tgt_ptr,
                                            const int32_t *tgt, void *ws, double *row_loss,
                                            int32_t *row_pred, void *stream) {
  CC_REQUIRE(params && row_ptr && idx && tgt_ptr && tgt && ws && row_loss && row_pred,
             "cc_recommend_batch_loss_fp32: null pointer");
  CC_REQUIRE(V > 0 && R >= 0 && max_n >= 0 && max_n <= V, "cc_recommend_batch_loss_fp32: V/R/max_n");
  if (int rc = cc::infer_check_d(d, "cc_recommend_batch_loss_fp32")) return rc;
  CC_REQUIRE(((uintptr_t)ws & 255) == 0, "cc_recommend_batch_loss_fp32: ws must be 256-byte aligned");
  if (R == 0) return CC_OK;
  int64_t off[CC_NUM_TENSORS], sz[CC_NUM_TENSORS], tot, mt;
  if (int rc = cc::param_offsets(V, d, off, sz, &tot, &mt)) return rc;
  const LossWs w = loss_ws(V, d, R, max_n);
  hipStream_t s = as_stream(stream);
  char *base = (char *)ws;
  float *h3 = (float *)(base + w.h3);
  uint32_t *bits = (uint32_t *)(base + w.bits);
  double *tl = (double *)(base + w.tloss);
  float *tp = (float *)(base + w.tp);
  int32_t *ti = (int32_t *)(base + w.ti);
  // the targets' masks by the rule of the cube masks: ids outside [0, V) are ignored
  if (int rc = cc::row_bits_launch(tgt_ptr, tgt, R, V, w.VW, bits, s)) return rc;
  if (int rc = cc::infer_h3_launch(params, V, d, R, row_ptr, idx, max_n, (float *)(base + w.part),
                                   (float *)(base + w.zlat), h3, s))
    return rc;
  const float *Wo = params + off[14], *bo = params + off[15];
  const dim3 grid((unsigned)w.tiles, 1);
  // rows per tile: 32 / 64 / 128, as cc_recommend_batch_fp32 chooses them
  if (R <= 32)
    launch_loss<2>(grid, s, h3, Wo, bo, d, V, R, bits, w.VW, tl, tp, ti);
  else if (R <= 64)
    launch_loss<4>(grid, s, h3, Wo, bo, d, V, R, bits, w.VW, tl, tp, ti);
  else
    launch_loss<8>(grid, s, h3, Wo, bo, d, V, R, bits, w.VW, tl, tp, ti);
  CC_LAUNCH_CHECK("loss_tile_kernel");
  hipLaunchKernelGGL(loss_rows_kernel, dim3((unsigned)cdiv(R, 256)), dim3(256), 0, s,
                     (const double *)tl, (const float *)tp, (const int32_t *)ti, w.tiles, V, R,
                     row_loss, row_pred);
  CC_LAUNCH_CHECK("loss_rows_kernel");
  return CC_OK;
}
