// The tower weight-gradient job (tower.hip: dW = H^T G of one 32 x 32 tile from the packed
// transposed images) as device code shared by the launches that host it: tower_dw_packed_kernel
// (tower.hip, one wave per job) and the W1-gradient launch's rider workgroups (embed.hip,
// cc_embed_grad_cs_adam_dw: the W1 kernel is HBM-bound and needs only dPre1 and the xt bits, the
// jobs only the backward chain's hpt / gpt images; their first common consumer is the Adam launch
// after both).  dw_packed_tile is a pure function of (p, job): the result does not depend on the
// launch that runs it.
#pragma once
#include "common.hpp"

namespace cctower {

struct TowerP {
  int d, B, R, maxw;
  const void *w[9];
  void *wt[9];
  const float *b[9];
  void *act[7];
  void *act6t;
  const void *gD3;
  void *gact[5];
  float *gpre1;
  void *gpre1t;  // optional bf16 dPre1^T [d][ceil64(R)]
  float *slab;
  int64_t slab_elems;
  float *gw[9];
  float *gb[9];
  const bf16_t *wpf[9];  // fragment-packed forward / backward weight images (cc_tower_args)
  const bf16_t *wpb[9];
  bf16_t *act6p, *act6tp;  // packed D3 operand images for cc_dec_bce_dw (fast forward only)
  bf16_t *hpt[6], *gpt[6];  // packed transposed H_i / G_i images for the dW kernel (or null)
  bf16_t *gpre1p;           // packed transposed dPre1 for cc_embed_grad_packed (or null)
  const uint32_t *xb;       // x row bitmasks -> xt (fast forward's extra blocks; or null)
  uint32_t *xt;
  int xt_V, xt_rows;
  uint8_t *d3q, *d3qs, *d3tq, *d3tqs;  // D3's MX-FP8 operand images (config 5; wide forward only, or null)
  const uint32_t *yb;       // y row bitmasks [B][y_VW] -> yimg (fast forward's extra blocks; or null)
  uint32_t *yimg;
  int y_VW;
  bool packed, dwpacked;
};

__host__ __device__ inline void chain_dims(int d, int i, int &K, int &N) {
  // K: d, 256, 128, 64, 128, 256;  N: 256, 128, 64, 128, 256, d  (no arrays: no scratch)
  K = i == 0 ? d : i == 1 ? 256 : i == 2 ? 128 : i == 3 ? 64 : i == 4 ? 128 : 256;
  N = i == 0 ? 256 : i == 1 ? 128 : i == 2 ? 64 : i == 3 ? 128 : i == 4 ? 256 : d;
}

// packed-image element offset of fragment (t, j), lane, element e
__device__ __forceinline__ int64_t pack_off(int t, int j, int lane, int red) {
  return (((int64_t)t * (red / 16) + j) * 64 + lane) * 8;
}

// job bid -> (layer l of 6 or 9, chain layer i, tile origin, the layer's rows); false past the last job
__device__ __forceinline__ bool dw_job(const TowerP &p, int bid, int &l, int &i, int &k0, int &n0,
                                       int &row0, int &nrows) {
  const int L = p.R > p.B ? 9 : 6;
  for (l = 0; l < L; ++l) {
    i = l < 6 ? l : l - 3;
    int K, N;
    chain_dims(p.d, i, K, N);
    const int tn = N / 32, nt = (K / 32) * tn;
    if (bid < nt) {
      k0 = 32 * (bid / tn);
      n0 = 32 * (bid % tn);
      row0 = l < 6 ? 0 : p.B;
      nrows = l < 3 ? p.R : (l < 6 ? p.B : p.R - p.B);   // reg branch: rows [B, R)
      return true;
    }
    bid -= nt;
  }
  return false;
}
// the number of jobs (host side: the grid of tower_dw_packed_kernel, the riders' loop bound)
inline int dw_jobs(int d, int B, int R) {
  int jobs = 0;
  for (int l = 0; l < (R > B ? 9 : 6); ++l) {
    int K, N;
    chain_dims(d, l < 6 ? l : l - 3, K, N);
    jobs += (K / 32) * (N / 32);
  }
  return jobs;
}

// dW from the packed transposed images: one wave per 32x32 tile of one layer, dW[k0.., n0..] =
// sum over the layer's rows of H^T G as a chain of v_mfma_f32_32x32x16_bf16 whose A / B fragments
// are whole 1 KB runs of hpt / gpt (no LDS staging, no cross-wave reduce); db from the same B
// fragments on the k0 == 0 tiles.  Rows in order: deterministic.  The calling wave (lane 0..63)
// computes job `job` whole.
constexpr int DWP_U = 8;  // fragment pairs in flight per lane
__device__ __forceinline__ void dw_packed_tile(const TowerP &p, int job, int lane) {
  int l, i, k0, n0, row0, nrows;
  if (!dw_job(p, job, l, i, k0, n0, row0, nrows)) return;
  int K, N;
  chain_dims(p.d, i, K, N);
  const int half = lane >> 5;
  const int R = p.R, j0 = row0 / 16, nj = nrows / 16;
  const bf16_t *ha = p.hpt[i] + pack_off(k0 / 32, j0, lane, R);
  const bf16_t *gb = p.gpt[i] + pack_off(n0 / 32, j0, lane, R);
  f32x16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float cs = 0.f;
  const bool bias = k0 == 0;
  int j = 0;
  for (; j + DWP_U <= nj; j += DWP_U) {
    bf16x8_t a[DWP_U], b[DWP_U];
#pragma unroll
    for (int u = 0; u < DWP_U; ++u) {
      a[u] = *reinterpret_cast<const bf16x8_t *>(ha + (j + u) * 512);
      b[u] = *reinterpret_cast<const bf16x8_t *>(gb + (j + u) * 512);
    }
#pragma unroll
    for (int u = 0; u < DWP_U; ++u) {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[u], b[u], acc, 0, 0, 0);
      if (bias) {
#pragma unroll
        for (int e = 0; e < 8; ++e) cs += (float)b[u][e];
      }
    }
  }
  for (; j < nj; ++j) {
    const bf16x8_t a = *reinterpret_cast<const bf16x8_t *>(ha + j * 512);
    const bf16x8_t b = *reinterpret_cast<const bf16x8_t *>(gb + j * 512);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    if (bias) {
#pragma unroll
      for (int e = 0; e < 8; ++e) cs += (float)b[e];
    }
  }
  float *gw = p.gw[l] + (int64_t)(k0 + 4 * half) * N + n0 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) gw[(int64_t)((r & 3) + 8 * (r >> 2)) * N] = acc[r];
  if (bias) {
    cs += __shfl_xor(cs, 32);
    if (half == 0) p.gb[l][n0 + lane] = cs;
  }
}

// cc_tower_bwd_dw_direct's argument checks for the one-wave-per-tile packed form, for a launch that
// hosts the jobs itself (tower.hip).  Fills p and the job count; fails (cc::fail, with `who` in the
// message) where cc_tower_bwd_dw_direct would fail or would run another kernel: no packed hpt / gpt
// images, or a tall chain that it splits by rows.
int dw_rider_params(const cc_tower_args *t, TowerP &p, int &jobs, const char *who);

}  // namespace cctower
