// cc_leave_one_out_fp32 — p(card | cube without c) for every card c of a cube, every derived row
// bit-identical to the forward pass (infer.hip, oracle/infer_ref.py) on the shorter list.
//
// A launch describes DERIVED ROWS over a CSR batch of cubes: row r is cube row_cube[r] with the
// id at sorted position row_pos[r] left out (-1: nothing left out, the base row).  Two things
// make n + 1 rows of an n-card cube cheap:
//   E1 shares its chunk sums.  The pinned E1 sums the sorted ids in chunks of 32, each from 0 in
//     order, then the chunk sums from 0 in order.  Without the id at position j (chunk cj) the
//     chunks before cj are the cube's own partials, the chunks behind it the cube's partials
//     SHIFTED by one id (ids 32c+1 .. 32c+32), and only chunk cj is summed per row: its other ids
//     in order, then the next chunk's first id.  The same additions in the same order.
//   The output layer is needed at chosen cards only: rows x targets dots against gathered columns
//     of Wo, in the forward pass's pinned 64-wide chunks.
//   loo_partials_kernel: one workgroup per (cube, chunk): 33 rows of W1 loaded once, the chunk's
//                        partial (gather_partials_kernel's additions) and its shifted partial.
//   loo_e1_kernel      : one workgroup per derived row: the own chunk (all loads before the first
//                        add, float4 columns), then the total in chunk order -> e1 [rows][d].
//   tower_kernel       : infer.hip's, unchanged, fed e1 as one-chunk partials (cap = 1): 0 + x is
//                        exact and a total summed from +0 is never -0.
//   loo_tile_kernel    : 32 derived rows x 64 target cards per tile.  A row tile is cut into runs
//                        of rows of one cube; a run meets its cube's targets in the shared
//                        dot-product tile (dottile.hpp) with gathered Wo columns.
//                        Self mode (no targets): only base rows take part, their targets are the
//                        cube's own cards (today's cut values).
//   loo_self_kernel    : self mode's derived rows: one dot per row against the column of its
//                        left-out card, one lane per 64-wide chunk.  Nothing n x n exists.
#include "common.hpp"
#include "detmath.hpp"
#include "dottile.hpp"
#include "infer.hpp"

namespace {

constexpr int GCH = 32;   // gather chunk (pinned)
constexpr int GNT = 128;  // gather workgroup
constexpr int KCH = dottile::KCH;  // dot chunk (pinned)
constexpr int TC = dottile::TC;    // targets per output tile
constexpr int RM = 2;              // rows per thread of the output tile
constexpr int TR = 16 * RM;
constexpr int ONT = dottile::NT;   // output-tile workgroup
constexpr int SR = 16;    // rows per workgroup of loo_self_kernel

using detm::addf;
using detm::mulf;
__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(addf(a.x, b.x), addf(a.y, b.y), addf(a.z, b.z), addf(a.w, b.w));
}
using dottile::zero4;

// What a derived row names.  ok = 0: a cube outside [0, n_cubes), a position outside [-1, n) or a
// cube longer than the partials' pitch; such a row indexes nothing and writes no result.
struct Row {
  int ok, cube, pos, beg, n;
};
__device__ __forceinline__ Row row_of(int r, int n_cubes, const int32_t *__restrict__ row_ptr,
                                      int cap, const int32_t *__restrict__ row_cube,
                                      const int32_t *__restrict__ row_pos) {
  Row w{0, row_cube[r], row_pos[r], 0, 0};
  if ((uint32_t)w.cube >= (uint32_t)n_cubes) return w;
  w.beg = row_ptr[w.cube];
  w.n = row_ptr[w.cube + 1] - w.beg;
  w.ok = w.n >= 0 && w.n <= cap * GCH && w.pos >= -1 && w.pos < w.n;
  return w;
}

// part [cube][c][:]  = sum of W1[id] over sorted positions 32c   .. 32c+31 (below n)
// spart[cube][c][:]  = sum of W1[id] over sorted positions 32c+1 .. 32c+32 (below n)
// both sequential from 0; the second is chunk c of the cube without any one id of an earlier chunk.
__global__ __launch_bounds__(GNT) void loo_partials_kernel(const float *__restrict__ W1, int d, int V,
                                                           const int32_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ idx, int cap,
                                                           float *__restrict__ part,
                                                           float *__restrict__ spart) {
  __shared__ int32_t lst[GCH + 1];
  const int cube = blockIdx.x;
  const int beg = row_ptr[cube];
  const int n = row_ptr[cube + 1] - beg;
  const int nch = min((n + GCH - 1) / GCH, cap);
  for (int c = blockIdx.y; c < nch; c += gridDim.y) {
    const int j0 = c * GCH, cnt = min(GCH + 1, n - j0);  // the 33rd id is the next chunk's first
    __syncthreads();
    if (threadIdx.x <= GCH)
      lst[threadIdx.x] = (int)threadIdx.x < cnt ? card_or_none(idx[beg + j0 + threadIdx.x], V) : -1;
    __syncthreads();
    const int64_t o = ((int64_t)cube * cap + c) * d;
    for (int c4 = threadIdx.x; c4 < d / 4; c4 += GNT) {
      float4 v[GCH + 1];
#pragma unroll
      for (int j = 0; j <= GCH; ++j)
        if (j < cnt)
          v[j] = lst[j] >= 0 ? *reinterpret_cast<const float4 *>(W1 + (int64_t)lst[j] * d + 4 * c4)
                             : zero4();
      float4 a = zero4(), b = zero4();
#pragma unroll
      for (int j = 0; j < GCH; ++j)
        if (j < cnt) a = add4(a, v[j]);
#pragma unroll
      for (int j = 1; j <= GCH; ++j)
        if (j < cnt) b = add4(b, v[j]);
      *reinterpret_cast<float4 *>(part + o + 4 * c4) = a;
      *reinterpret_cast<float4 *>(spart + o + 4 * c4) = b;
    }
  }
}

// e1[r][:] = the E1 total (before bias) of derived row r; one_ptr[r] = r: the CSR of rows of one
// card each, under which tower_kernel reads e1 as one-chunk partials.
__global__ __launch_bounds__(GNT) void loo_e1_kernel(
    const float *__restrict__ W1, int d, int V, int n_cubes, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ idx, int cap, int rows, const int32_t *__restrict__ row_cube,
    const int32_t *__restrict__ row_pos, const float *__restrict__ part,
    const float *__restrict__ spart, float *__restrict__ e1, int32_t *__restrict__ one_ptr) {
  __shared__ int32_t lst[GCH];
  const int r = blockIdx.x;
  if (threadIdx.x == 0) {
    one_ptr[r] = r;
    if (r == rows - 1) one_ptr[rows] = rows;
  }
  const Row w = row_of(r, n_cubes, row_ptr, cap, row_cube, row_pos);  // (block-uniform)
  float *out = e1 + (int64_t)r * d;
  if (!w.ok) {
    for (int c4 = threadIdx.x; c4 < d / 4; c4 += GNT) *reinterpret_cast<float4 *>(out + 4 * c4) = zero4();
    return;
  }
  // the shorter list: n1 ids in nch1 chunks; chunk cj holds the gap (the base row has none)
  const int n1 = w.pos < 0 ? w.n : w.n - 1;
  const int nch1 = (n1 + GCH - 1) / GCH;
  const int cj = w.pos < 0 ? nch1 : w.pos / GCH;
  const int cnt = w.pos < 0 ? 0 : min(GCH, n1 - cj * GCH);  // 0: the chunk lost its only id
  if (threadIdx.x < GCH) {
    int32_t id = -1;
    if ((int)threadIdx.x < cnt) {
      int p = cj * GCH + threadIdx.x;  // position in the shorter list ...
      p += p >= w.pos ? 1 : 0;         // ... and in the cube's: p <= n1 = n - 1
      id = card_or_none(idx[w.beg + p], V);
    }
    lst[threadIdx.x] = id;
  }
  __syncthreads();
  const float *pp = part + (int64_t)w.cube * cap * d;
  const float *sp = spart + (int64_t)w.cube * cap * d;
  for (int c4 = threadIdx.x; c4 < d / 4; c4 += GNT) {
    float4 v[GCH];
#pragma unroll
    for (int j = 0; j < GCH; ++j)
      if (j < cnt)
        v[j] = lst[j] >= 0 ? *reinterpret_cast<const float4 *>(W1 + (int64_t)lst[j] * d + 4 * c4)
                           : zero4();
    float4 own = zero4();
#pragma unroll
    for (int j = 0; j < GCH; ++j)
      if (j < cnt) own = add4(own, v[j]);
    float4 tot = zero4();
    for (int c = 0; c < cj; ++c)
      tot = add4(tot, *reinterpret_cast<const float4 *>(pp + (int64_t)c * d + 4 * c4));
    if (cnt > 0) tot = add4(tot, own);
    for (int c = cj + 1; c < nch1; ++c)
      tot = add4(tot, *reinterpret_cast<const float4 *>(sp + (int64_t)c * d + 4 * c4));
    *reinterpret_cast<float4 *>(out + 4 * c4) = tot;
  }
}

// out[out_ptr[r] + t] = det_sigmoid32(blocked_dot(h3[r], Wo[:, card_t]) + bo[card_t]) for the rows
// that take part and the targets card_t of their cube.  tgt_ptr != nullptr: every valid row, the
// targets tgt[tgt_ptr[cube] .. tgt_ptr[cube + 1]).  tgt_ptr == nullptr (self mode): base rows
// alone, the targets are the cube's own ids.  A target outside [0, V) gives 0.f.  A row writes at
// most out_ptr[r + 1] - out_ptr[r] words.  grid: (row tiles, target-tile stride).
__global__ __launch_bounds__(ONT) void loo_tile_kernel(
    const float *__restrict__ h3, const float *__restrict__ Wo, const float *__restrict__ bo, int d,
    int V, int n_cubes, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ idx, int cap,
    int rows, const int32_t *__restrict__ row_cube, const int32_t *__restrict__ row_pos,
    const int32_t *__restrict__ tgt_ptr, const int32_t *__restrict__ tgt,
    const int32_t *__restrict__ out_ptr, float *__restrict__ out) {
  __shared__ int32_t s_cube[TR], s_act[TR], s_t[TC];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int rb = blockIdx.x * TR;  // first row of the tile
  if (tid < TR) {
    int cube = -1, act = 0;
    if (rb + tid < rows) {
      const Row w = row_of(rb + tid, n_cubes, row_ptr, cap, row_cube, row_pos);
      if (w.ok) {
        cube = w.cube;
        act = tgt_ptr ? 1 : (w.pos < 0 ? 1 : 0);
      }
    }
    s_cube[tid] = cube;
    s_act[tid] = act;
  }
  __syncthreads();
  const int rend = min(TR, rows - rb);
  // runs of rows of one cube (every value below is block-uniform: it comes from LDS)
  for (int s0 = 0; s0 < rend;) {
    const int cube = s_cube[s0];
    int s1 = s0 + 1, any = s_act[s0];
    while (s1 < rend && s_cube[s1] == cube) any |= s_act[s1++];
    const int r0 = s0, r1 = s1;
    s0 = s1;
    if (cube < 0 || !any) continue;
    const int32_t *tl;
    int T;
    if (tgt_ptr) {
      const int tb = tgt_ptr[cube];
      T = tgt_ptr[cube + 1] - tb;
      tl = tgt + tb;
    } else {
      const int beg = row_ptr[cube];
      T = row_ptr[cube + 1] - beg;
      tl = idx + beg;
    }
    for (int ct = blockIdx.y; (int64_t)ct * TC < T; ct += gridDim.y) {
      const int t0 = ct * TC;
      __syncthreads();  // the previous tile's readers of s_t are done
      if (tid < TC) s_t[tid] = t0 + tid < T ? card_or_none(tl[t0 + tid], V) : -1;
      // (the tile's first barrier is behind this write and before its first read of s_t)
      const auto dot = dottile::run<RM, true>(
          d, V,
          [=](int k) {
            const int card = s_t[tid & 63];
            return card >= 0 ? Wo + (int64_t)k * V + card : nullptr;
          },
          [=](int lr, int k) {
            const bool in = lr >= r0 && lr < r1 && s_act[lr];
            return in ? *reinterpret_cast<const float4 *>(h3 + (int64_t)(rb + lr) * d + k) : zero4();
          });

#pragma unroll
      for (int j = 0; j < RM; ++j) {
        const int lr = ty * RM + j;
        if (lr < r0 || lr >= r1 || !s_act[lr]) continue;
        const int ob = out_ptr[rb + lr], span = out_ptr[rb + lr + 1] - ob;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int t = t0 + 4 * tx + e;
          if (t >= T || t >= span) continue;
          const int card = s_t[4 * tx + e];
          out[(int64_t)ob + t] = card >= 0 ? detm::det_sigmoid32(addf(dot.sum[j][e], bo[card])) : 0.f;
        }
      }
    }
  }
}

// Self mode's derived rows: out[out_ptr[r]] = p(left-out card | row r).  16 lanes per row, lane c
// owns the pinned chunk c: its 64 weights and 64 activations are loaded before the first add; the
// chunk partials meet in LDS and lane 0 adds them in order.
__global__ __launch_bounds__(SR * 16) void loo_self_kernel(
    const float *__restrict__ h3, const float *__restrict__ Wo, const float *__restrict__ bo, int d,
    int V, int n_cubes, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ idx, int cap,
    int rows, const int32_t *__restrict__ row_cube, const int32_t *__restrict__ row_pos,
    const int32_t *__restrict__ out_ptr, float *__restrict__ out) {
  __shared__ float ps[SR][17];
  const int ri = threadIdx.x >> 4, c = threadIdx.x & 15;
  const int r = blockIdx.x * SR + ri;
  const int nch = d / KCH;  // <= 16
  int card = -1;
  if (r < rows) {
    const Row w = row_of(r, n_cubes, row_ptr, cap, row_cube, row_pos);
    if (w.ok && w.pos >= 0) card = card_or_none(idx[w.beg + w.pos], V);
  }
  if (card >= 0 && c < nch) {
    const float *Wp = Wo + (int64_t)c * KCH * V + card;
    const float4 *hp = reinterpret_cast<const float4 *>(h3 + (int64_t)r * d + c * KCH);
    float wv[KCH];
    float4 hv[KCH / 4];
#pragma unroll
    for (int k = 0; k < KCH; ++k) wv[k] = Wp[(int64_t)k * V];
#pragma unroll
    for (int k = 0; k < KCH / 4; ++k) hv[k] = hp[k];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < KCH / 4; ++k) {
      acc = addf(acc, mulf(hv[k].x, wv[4 * k]));
      acc = addf(acc, mulf(hv[k].y, wv[4 * k + 1]));
      acc = addf(acc, mulf(hv[k].z, wv[4 * k + 2]));
      acc = addf(acc, mulf(hv[k].w, wv[4 * k + 3]));
    }
    ps[ri][c] = acc;
  }
  __syncthreads();
  if (card >= 0 && c == 0 && out_ptr[r + 1] > out_ptr[r]) {
    float tot = 0.f;
    for (int cc = 0; cc < nch; ++cc) tot = addf(tot, ps[ri][cc]);
    out[out_ptr[r]] = detm::det_sigmoid32(addf(tot, bo[card]));
  }
}

// workspace: [partials n_cubes*cap*d][shifted partials n_cubes*cap*d][e1 rows*d][zlat rows*64]
//            [h3 rows*d][one_ptr rows+1]
struct LooWs {
  size_t part, spart, e1, zlat, h3, one_ptr, total;
  int cap;
};
LooWs loo_ws(int d, int n_cubes, int max_n, int rows) {
  LooWs w;
  const size_t c = (size_t)std::max(n_cubes, 1), r = (size_t)std::max(rows, 1);
  const size_t dd = (size_t)std::max(d, 64);
  w.cap = cc::infer_gather_cap(max_n);
  size_t o = 0;
  w.part = o, o += align256(c * w.cap * dd * sizeof(float));
  w.spart = o, o += align256(c * w.cap * dd * sizeof(float));
  w.e1 = o, o += align256(r * dd * sizeof(float));
  w.zlat = o, o += align256(r * 64 * sizeof(float));
  w.h3 = o, o += align256(r * dd * sizeof(float));
  w.one_ptr = o, o += align256((r + 1) * sizeof(int32_t));
  w.total = o;
  return w;
}

}  // namespace

extern "C" size_t cc_leave_one_out_ws_size(int32_t V, int32_t d, int32_t n_cubes, int32_t max_n,
                                           int32_t rows) {
  (void)V;
  return loo_ws(d, n_cubes, max_n, rows).total;
}

extern "C" int cc_leave_one_out_fp32(const float *params, int32_t V, int32_t d, int32_t n_cubes,
                                     const int32_t *row_ptr, const int32_t *idx, int32_t max_n,
                                     int32_t rows, const int32_t *row_cube, const int32_t *row_pos,
                                     const int32_t *tgt_ptr, const int32_t *tgt,
                                     const int32_t *out_ptr, float *out, void *ws, size_t ws_bytes,
                                     void *stream) {
  CC_REQUIRE(params && row_ptr && idx && row_cube && row_pos && out_ptr && out && ws,
             "cc_leave_one_out_fp32: null pointer");
  CC_REQUIRE(!tgt_ptr || tgt, "cc_leave_one_out_fp32: null pointer (tgt with tgt_ptr)");
  CC_REQUIRE(V > 0 && n_cubes >= 0 && rows >= 0 && max_n >= 0 && max_n <= V,
             "cc_leave_one_out_fp32: V/n_cubes/rows/max_n");
  if (int rc = cc::infer_check_d(d, "cc_leave_one_out_fp32")) return rc;
  CC_REQUIRE(((uintptr_t)ws & 255) == 0, "cc_leave_one_out_fp32: ws must be 256-byte aligned");
  const LooWs w = loo_ws(d, n_cubes, max_n, rows);
  CC_REQUIRE(ws_bytes >= w.total,
             "cc_leave_one_out_fp32: workspace below cc_leave_one_out_ws_size()");
  if (rows == 0) return CC_OK;
  CC_REQUIRE(n_cubes > 0, "cc_leave_one_out_fp32: rows without cubes");
  int64_t off[CC_NUM_TENSORS], sz[CC_NUM_TENSORS], tot, mt;
  if (int rc = cc::param_offsets(V, d, off, sz, &tot, &mt)) return rc;
  const float *W1 = params + off[0], *Wo = params + off[14], *bo = params + off[15];
  char *base = (char *)ws;
  float *part = (float *)(base + w.part), *spart = (float *)(base + w.spart);
  float *e1 = (float *)(base + w.e1), *zlat = (float *)(base + w.zlat), *h3 = (float *)(base + w.h3);
  int32_t *one_ptr = (int32_t *)(base + w.one_ptr);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(loo_partials_kernel, dim3(n_cubes, std::min(w.cap, 64)), dim3(GNT), 0, s, W1, d, V,
                     row_ptr, idx, w.cap, part, spart);
  CC_LAUNCH_CHECK("loo_partials_kernel");
  hipLaunchKernelGGL(loo_e1_kernel, dim3(rows), dim3(GNT), 0, s, W1, d, V, n_cubes, row_ptr, idx, w.cap,
                     rows, row_cube, row_pos, (const float *)part, (const float *)spart, e1, one_ptr);
  CC_LAUNCH_CHECK("loo_e1_kernel");
  if (int rc = cc::infer_towers_launch(params, V, d, rows, one_ptr, e1, zlat, h3, s)) return rc;
  // target tiles a workgroup strides over: a cube's own cards in self mode, unknown here otherwise
  const int gy = tgt_ptr ? 8 : (int)std::min<int64_t>(8, std::max<int64_t>(1, cdiv(max_n, TC)));
  hipLaunchKernelGGL(loo_tile_kernel, dim3((unsigned)cdiv(rows, TR), gy), dim3(ONT), 0, s,
                     (const float *)h3, Wo, bo, d, V, n_cubes, row_ptr, idx, w.cap, rows, row_cube,
                     row_pos, tgt_ptr, tgt, out_ptr, out);
  CC_LAUNCH_CHECK("loo_tile_kernel");
  if (!tgt_ptr) {
    hipLaunchKernelGGL(loo_self_kernel, dim3((unsigned)cdiv(rows, SR)), dim3(SR * 16), 0, s,
                       (const float *)h3, Wo, bo, d, V, n_cubes, row_ptr, idx, w.cap, rows, row_cube,
                       row_pos, out_ptr, out);
    CC_LAUNCH_CHECK("loo_self_kernel");
  }
  return CC_OK;
}
