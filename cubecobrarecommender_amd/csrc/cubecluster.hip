// cc_cube_cluster / cc_cube_assign — cube archetypes: deterministic spherical k-means (cosine
// distance, unit centroids) over the member cubes [0, N) of a cube index (cubesim.hip), and the
// nearest centroid of member or fresh cubes.  DESIGN.md 4.11; tests/cube_cluster_ref.py restates it.
//
// Pinned arithmetic: fp32, multiply and add separately rounded, sums from +0.
//   assign : dist(i, j) = -(sum_t n_i[t] * c_j[t]) in ascending t (dottile::run<RM, false>); the
//            label is the j of the smallest composite orderable(dist) << 32 | j (equal distances:
//            the lower centroid), the distance that one's (a zero is -0.0f).  Centroid rows are
//            taken as they are.
//   update : P[b][j] = sum of n_i over the cubes i of id block [b * CB, (b + 1) * CB) with label j, in
//            ascending i; S[j] = sum of P[b][j] in ascending b; the new centroid is S[j] normalised by
//            the put's arithmetic (ss in index order, inv = 1 / sqrt(max(ss, 1e-12)), S[j][t] * inv);
//            a cluster without members keeps its centroid's bits.
// Kernels, all on one stream and never waited for:
//   centroid_image_kernel : the start centroids (index rows init_ids[j]; cc_cube_assign: the caller's
//                           rows) as the k-major image cT [Kp][kp], kp = k rounded up to 64, the k pad
//                           written as zeros.
//   assign_kernel<RM>     : 16 * RM rows x a run of centroid tiles per workgroup, the distance tile
//                           once per 64 centroids, each thread keeping the best of its 4 columns; a
//                           min over the 16 column lanes by shuffles, then one 64-bit atomic min per
//                           row into best [N] (a small corpus spreads a row tile's centroid tiles
//                           over several workgroups; a min commutes: the same bits on every run).
//   labels_kernel         : best -> label, dist and, one integer atomic per workgroup, the number of
//                           changed labels into changed[t] (integer adds commute as well).
//   block_sums_kernel     : one workgroup per id block.  The block's (label, position) keys sorted in
//                           LDS; a wave takes whole segments, a lane per dimension, the rows added in
//                           ascending id.  Partials are stored compactly, [block][slot][Kp], with a
//                           16-bit slot map [blocks][k] (0: the block has no such label).
//   centroid_kernel       : one wave per cluster.  64 blocks' map entries at a time, a ballot of the
//                           present ones, their partial rows added in ascending block order; then the
//                           normalisation (the sum of squares by one lane in index order), the row
//                           into centroids, the column into cT.  No member: nothing is written.
//   sizes_kernel, finish_kernel : the member counts of the final labels (integer atomics), n_iter
//                           and the -1 tail of changed.
// Gating: changed[t] is zeroed before the first launch and counts iteration t's changed labels.
// N > 0 rows differ from the all -1 start, so changed[t] == 0 behind assign t means "converged at
// t": the update of iteration t reads changed[t], the assign of iteration t + 1 reads changed[t],
// each returns at once on a zero, and every later count then stays zero.  The host queues
// max_iter x (assign, labels, block sums, centroid), the last assign, sizes and finish without a wait.
#include <algorithm>

#include "common.hpp"
#include "cosine.hpp"
#include "cubeindex.hpp"
#include "detmath.hpp"
#include "dottile.hpp"
#include "rowsort.hpp"

namespace {

constexpr int TC = dottile::TC;   // centroids per distance tile
constexpr int DNT = dottile::NT;  // distance-tile workgroup
constexpr int CB = 256;           // cubes per id block of the update (pinned: part of the arithmetic)
constexpr int MAX_CK = 1024;      // clusters per call: the slot map and the size histogram sit in LDS
constexpr int MAX_CLUSTER_K = 8192;  // embedding width: a centroid row is staged in LDS

using cubeindex::index_layout;
using cubeindex::IndexLayout;
using cubeindex::MAX_Q;
using cubeindex::QNT;
using cubeindex::query_rows_kernel;
using detm::addf;
using detm::mulf;
using rowsort::orderable;

int k_pitch(int k) { return (int)cdiv(std::max(k, 1), TC) * TC; }

// Centroid j (one workgroup each) into the image: column j of cT [Kp][kp], zeros behind K.  The row
// is index row ids[j] (clamped into [0, N): the callers have refused any other) when ids is given,
// else src[j][0..K); `out` (optional) receives it as [k][K].
__global__ __launch_bounds__(QNT) void centroid_image_kernel(const float *__restrict__ n, int N, int K, int Kp,
                                                             const int32_t *__restrict__ ids,
                                                             const float *__restrict__ src, int kp,
                                                             float *__restrict__ cT, float *__restrict__ out) {
  const int j = blockIdx.x, tid = threadIdx.x;
  const float *row = ids ? n + (int64_t)min(max(ids[j], 0), N - 1) * Kp : src + (int64_t)j * K;
  for (int t = tid; t < Kp; t += QNT) {
    const float v = t < K ? row[t] : 0.f;
    cT[(int64_t)t * kp + j] = v;
    if (out && t < K) out[(int64_t)j * K + t] = v;
  }
}

// label[i] = -1, best[i] = nothing, changed[0 .. iters] = 0, sizes[0 .. k) = 0
__global__ __launch_bounds__(256) void start_kernel(int N, int32_t *__restrict__ label,
                                                    unsigned long long *__restrict__ best, int iters,
                                                    int32_t *__restrict__ changed, int k,
                                                    int32_t *__restrict__ sizes) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N) label[i] = -1, best[i] = ~0ull;
  if (i <= iters) changed[i] = 0;
  if (i < k) sizes[i] = 0;
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
  return ((uint64_t)hi << 32) | lo;
}

// Rows [0, R) of `rows` [R][Kp] against the centroids of this workgroup's tiles_per tiles of cT
// (blockIdx.y: a corpus too small to fill the device with row tiles alone shares a row tile's
// centroids among several workgroups).  best [R]: the rows' smallest composite so far, joined by a
// 64-bit atomic min: a min commutes, so the result is the same on every run.  ok (optional): rows
// that are no query take no part.  gate (optional): the previous iteration's count, a zero ends the
// kernel.  (4 waves per SIMD, as the neighbours' distance tile: at most 128 VGPRs)
template <int RM>
__global__ __launch_bounds__(DNT, 4) void assign_kernel(const float *__restrict__ rows,
                                                        const int32_t *__restrict__ ok, int R, int Kp,
                                                        const float *__restrict__ cT, int k, int kp,
                                                        int tiles_per, const int32_t *gate,
                                                        unsigned long long *__restrict__ best) {
  if (gate && *gate == 0) return;  // (uniform over the launch)
  const int cb = blockIdx.y * tiles_per * TC, ce = min(k, cb + tiles_per * TC);  // this workgroup's centroids
  constexpr int TR = 16 * RM;
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int rb = blockIdx.x * TR;  // first row of the tile
  // the staging of dist_chunk_kernel (cubesim.hip): one pointer and a bit per staged row
  const int lr0 = tid / dottile::F4, kq = 4 * (tid % dottile::F4);
  const float *qbase = rows + (int64_t)(rb + lr0) * Kp + kq;
  uint32_t qmask = 0u;
#pragma unroll
  for (int i = 0; i < TR / dottile::RS; ++i) {
    const int gr = rb + lr0 + dottile::RS * i;
    if (gr < R && (!ok || ok[gr] != 0)) qmask |= 1u << i;
  }
  // The best of this thread's columns 4 * tx + e of every tile, visited in ascending order: a strictly
  // larger dot alone replaces it, which is the composite's order (the lower centroid of equal
  // distances; a dot is finite and never -0).  It starts at the thread's first column.
  float bdot[RM];
  int bcol[RM];
#pragma unroll
  for (int j = 0; j < RM; ++j) bdot[j] = -INFINITY, bcol[j] = cb + 4 * tx;
  for (int c0 = cb; c0 < ce; c0 += TC) {
    const int gn = c0 + (tid & 63);
    const auto dot = dottile::run<RM, false>(
        Kp, kp, [=](int kk) { return gn < k ? cT + (int64_t)kk * kp + gn : nullptr; },
        [=](int lr, int kk) {
          return (qmask >> ((lr - lr0) / dottile::RS)) & 1u
                     ? *reinterpret_cast<const float4 *>(qbase + (int64_t)(lr - lr0) * Kp + (kk - kq))
                     : dottile::zero4();
        });
#pragma unroll
    for (int j = 0; j < RM; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int col = c0 + 4 * tx + e;
        const bool better = col < k && dot.sum[j][e] > bdot[j];
        bdot[j] = better ? dot.sum[j][e] : bdot[j];
        bcol[j] = better ? col : bcol[j];
      }
  }
#pragma unroll
  for (int j = 0; j < RM; ++j) {
    // (a thread whose first column is no centroid holds nothing)
    uint64_t b = cb + 4 * tx < k ? ((uint64_t)orderable(-bdot[j]) << 32) | (uint32_t)bcol[j] : ~0ull;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
      const uint64_t o = shfl_xor_u64(b, m);
      b = o < b ? o : b;
    }
    const int gr = rb + ty * RM + j;
    if (tx == 0 && gr < R && (!ok || ok[gr] != 0)) atomicMin(best + gr, (unsigned long long)b);
  }
}

// Row i's composite into label and dist (a row that is no query: -1 / 0.f), and best[i] back to
// "nothing" for the next assign.  count (optional): receives the number of rows whose label differs
// from the one `label` held, one integer atomic per workgroup.
__global__ __launch_bounds__(256) void labels_kernel(unsigned long long *__restrict__ best,
                                                     const int32_t *__restrict__ ok, int R, const int32_t *gate,
                                                     int32_t *__restrict__ label, float *__restrict__ dist,
                                                     int32_t *count) {
  if (gate && *gate == 0) return;  // (uniform over the launch)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int diff = 0;
  if (i < R) {
    const uint64_t b = best[i];
    best[i] = ~0ull;
    const bool is_query = !ok || ok[i] != 0;
    const int32_t lab = is_query ? (int32_t)(uint32_t)b : -1;
    if (count) diff = label[i] != lab ? 1 : 0;
    label[i] = lab;
    dist[i] = is_query ? cosine::dist_of_key((uint32_t)(b >> 32)) : 0.f;
  }
  if (count) {  // (uniform)
    __shared__ int wdiff[4];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) diff += __shfl_xor(diff, m, 64);
    if ((threadIdx.x & 63) == 0) wdiff[threadIdx.x >> 6] = diff;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int all = wdiff[0] + wdiff[1] + wdiff[2] + wdiff[3];
      if (all) atomicAdd(count, all);
    }
  }
}

__global__ __launch_bounds__(256) void no_best_kernel(unsigned long long *__restrict__ best, int R) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < R) best[i] = ~0ull;
}

// Ascending compare-exchange of 32-bit keys for rowsort::bitonic_sort
struct CmpSwapU32 {
  uint32_t *a;
  __device__ __forceinline__ void operator()(int i, int pr, bool down) const {
    const uint32_t x = a[i], y = a[pr];
    if ((x > y) == down) {
      a[i] = y;
      a[pr] = x;
    }
  }
};

// Id block b = blockIdx.x: the sums of its cubes' rows per label.  part [blocks][CB][Kp] (the block's
// slots in ascending label), map [blocks][k] (slot + 1, or 0).
__global__ __launch_bounds__(CB) void block_sums_kernel(const float *__restrict__ n, int N, int Kp,
                                                        const int32_t *__restrict__ label, int k,
                                                        const int32_t *__restrict__ gate,
                                                        float *__restrict__ part, uint16_t *__restrict__ map) {
  if (*gate == 0) return;  // converged: the centroids stay
  __shared__ uint32_t key[CB];      // label << 8 | position, ascending; above every key behind N
  __shared__ uint16_t slot_of[MAX_CK];
  __shared__ int seg[CB + 1];       // first sorted position of every slot, and the end
  __shared__ int wtot[CB / 64];
  __shared__ int s_slots;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x;
  const int64_t i0 = (int64_t)b * CB;
  const int cnt = (int)min((int64_t)CB, N - i0);
  // a label outside [0, k) cannot come out of the assign; clamped, it is never used as an index
  key[tid] = tid < cnt ? ((uint32_t)min(max(label[i0 + tid], 0), k - 1) << 8) | (uint32_t)tid : 0xFFFFFFFFu;
  for (int j = tid; j < k; j += CB) slot_of[j] = 0;
  __syncthreads();
  rowsort::bitonic_sort<CB>(CB, CmpSwapU32{key});
  const bool head = tid < cnt && (tid == 0 || (key[tid] >> 8) != (key[tid - 1] >> 8));
  const int slot = rowsort::block_incl_scan<CB>(head ? 1 : 0, wtot) - 1;  // of this position's segment
  if (head) {
    seg[slot] = tid;
    slot_of[key[tid] >> 8] = (uint16_t)(slot + 1);
  }
  if (tid == cnt - 1) {
    seg[slot + 1] = cnt;
    s_slots = slot + 1;
  }
  __syncthreads();
  for (int j = tid; j < k; j += CB) map[(int64_t)b * k + j] = slot_of[j];
  const int slots = s_slots;
  for (int s = w; s < slots; s += CB / 64) {  // (wave-uniform)
    const int p0 = seg[s], p1 = seg[s + 1];
    float *out = part + ((int64_t)b * CB + s) * Kp;
    for (int t = lane; t < Kp; t += 64) {
      float sum = 0.f;
      for (int p = p0; p < p1; ++p) sum = addf(sum, n[(i0 + (key[p] & 255u)) * Kp + t]);
      out[t] = sum;
    }
  }
}

// Cluster j = blockIdx.x, one wave: S = the present partials in ascending block order, normalised.
// Dynamic LDS: Kp floats.
__global__ __launch_bounds__(64) void centroid_kernel(const float *__restrict__ part,
                                                      const uint16_t *__restrict__ map, int blocks, int K,
                                                      int Kp, int k, int kp, const int32_t *__restrict__ gate,
                                                      float *__restrict__ centroids, float *__restrict__ cT) {
  if (*gate == 0) return;
  extern __shared__ __attribute__((aligned(16))) float s_row[];  // [Kp]
  __shared__ float s_inv;
  const int j = blockIdx.x, lane = threadIdx.x;
  bool any = false;
  for (int t0 = 0; t0 < Kp; t0 += 64) {  // (one pass at Kp <= 64)
    const int t = t0 + lane;
    float sum = 0.f;
    for (int b0 = 0; b0 < blocks; b0 += 64) {
      const int bl = b0 + lane;
      const int m = bl < blocks ? (int)map[(int64_t)bl * k + j] : 0;
      uint64_t present = __ballot(m != 0);
      any |= present != 0;
      while (present) {  // (wave-uniform) four partial rows in flight, added in block order
        int bit[4];
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          bit[u] = present ? __ffsll((unsigned long long)present) - 1 : -1;
          present &= present - 1;  // (0 stays 0)
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int slot = __shfl(m, max(bit[u], 0), 64) - 1;
          v[u] = bit[u] >= 0 && t < Kp ? part[((int64_t)(b0 + bit[u]) * CB + slot) * Kp + t] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (bit[u] >= 0) sum = addf(sum, v[u]);
      }
    }
    if (t < Kp) s_row[t] = sum;
  }
  if (!any) return;  // no member: the centroid keeps its bits (wave-uniform)
  __syncthreads();
  if (lane == 0) {
    float ss = 0.f;  // the pinned order is sequential
    for (int t = 0; t < K; ++t) ss = addf(ss, mulf(s_row[t], s_row[t]));
    s_inv = cosine::inv_norm(ss);
  }
  __syncthreads();
  const float inv = s_inv;
  for (int t = lane; t < Kp; t += 64) {
    const float v = t < K ? mulf(s_row[t], inv) : 0.f;
    cT[(int64_t)t * kp + j] = v;
    if (t < K) centroids[(int64_t)j * K + t] = v;
  }
}

// sizes[j] += the cubes of this workgroup's 1,024 ids with label j (sizes zeroed by start_kernel)
__global__ __launch_bounds__(256) void sizes_kernel(const int32_t *__restrict__ label, int N, int k,
                                                    int32_t *__restrict__ sizes) {
  __shared__ int hist[MAX_CK];
  const int tid = threadIdx.x;
  for (int j = tid; j < k; j += 256) hist[j] = 0;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * 1024;
  for (int u = 0; u < 4; ++u) {
    const int64_t i = i0 + u * 256 + tid;
    if (i < N) {
      const int l = label[i];
      if ((uint32_t)l < (uint32_t)k) atomicAdd(&hist[l], 1);
    }
  }
  __syncthreads();
  for (int j = tid; j < k; j += 256)
    if (hist[j]) atomicAdd(&sizes[j], hist[j]);
}

// n_iter = the first t < max_iter with changed[t] == 0 (converged there), else max_iter; the counts
// behind n_iter were never written: -1.
__global__ __launch_bounds__(256) void finish_kernel(int max_iter, int32_t *__restrict__ changed,
                                                     int32_t *__restrict__ n_iter) {
  __shared__ int first;
  const int tid = threadIdx.x;
  if (tid == 0) first = max_iter;
  __syncthreads();
  for (int t = tid; t < max_iter; t += 256)
    if (changed[t] == 0) atomicMin(&first, t);
  __syncthreads();
  const int it = first;
  for (int t = it + 1 + tid; t <= max_iter; t += 256) changed[t] = -1;
  if (tid == 0) *n_iter = it;
}

// workspace: [cT Kp*kp][best max(N, Q)][part blocks*CB*Kp][map blocks*k][qn Q*Kp][qok Q]
struct ClusterWs {
  size_t cT, best, part, map, qn, qok, total;
  int Kp, kp, blocks;
};
ClusterWs cluster_ws(int N, int K, int k, int Q) {
  ClusterWs w;
  w.Kp = cosine::k_pad(K);
  w.kp = k_pitch(k);
  w.blocks = (int)cdiv(std::max(N, 0), CB);
  const size_t kk = (size_t)std::max(k, 1), q = (size_t)std::max(Q, 0);
  size_t o = 0;
  w.cT = o, o += align256((size_t)w.Kp * w.kp * sizeof(float));
  w.best = o, o += align256(std::max((size_t)std::max(N, 0), q) * sizeof(uint64_t));
  w.part = o, o += align256((size_t)w.blocks * CB * w.Kp * sizeof(float));
  w.map = o, o += align256((size_t)w.blocks * kk * sizeof(uint16_t));
  w.qn = o, o += align256(q * w.Kp * sizeof(float));
  w.qok = o, o += align256(q * sizeof(int32_t));
  w.total = o;
  return w;
}

// One assign: the distance tiles, then the rows' labels.  Rows per tile: 32 / 64 / 128 by R; a row
// tile's centroid tiles go to as many workgroups as it takes to reach FILL workgroups in all (the
// arithmetic per (row, centroid) depends on neither).
constexpr int FILL = 2048;
int launch_assign(hipStream_t s, const float *rows, const int32_t *ok, int R, int Kp, const float *cT, int k,
                  int kp, const int32_t *gate, unsigned long long *best, int32_t *label, float *dist,
                  int32_t *count) {
  const int rm = R <= 32 ? 2 : R <= 64 ? 4 : 8, tiles = kp / TC;
  const int row_tiles = (int)cdiv(R, 16 * rm);
  const int tiles_per = (int)cdiv(tiles, std::min<int64_t>(tiles, cdiv(FILL, row_tiles)));
  const dim3 grid((unsigned)row_tiles, (unsigned)cdiv(tiles, tiles_per));
#define CC_ASSIGN(RM) \
  hipLaunchKernelGGL(assign_kernel<RM>, grid, dim3(DNT), 0, s, rows, ok, R, Kp, cT, k, kp, tiles_per, gate, best)
  if (rm == 2)
    CC_ASSIGN(2);
  else if (rm == 4)
    CC_ASSIGN(4);
  else
    CC_ASSIGN(8);
#undef CC_ASSIGN
  CC_LAUNCH_CHECK("assign_kernel");
  hipLaunchKernelGGL(labels_kernel, dim3((unsigned)cdiv(R, 256)), dim3(256), 0, s, best, ok, R, gate, label, dist,
                     count);
  CC_LAUNCH_CHECK("labels_kernel");
  return CC_OK;
}

}  // namespace

extern "C" int32_t cc_cube_cluster_block(void) { return CB; }

extern "C" int32_t cc_cube_cluster_max_k(void) { return MAX_CK; }

extern "C" size_t cc_cube_cluster_ws_size(int32_t N, int32_t K, int32_t k, int32_t Q) {
  return cluster_ws(N, K, k, Q).total + 256;
}

#define CC_CLUSTER_COMMON(name)                                                                           \
  CC_REQUIRE(cap >= 1 && cap <= 0x7FFFFFFF - 64 && K >= 1 && K <= MAX_CLUSTER_K, name ": bad cap/K");     \
  CC_REQUIRE(N >= 0 && N <= cap, name ": N must be 0..cap");                                              \
  CC_REQUIRE(k >= 1 && k <= MAX_CK, name ": k must be 1..cc_cube_cluster_max_k()");                       \
  CC_REQUIRE(((uintptr_t)ws & 255) == 0, name ": ws must be 256-byte aligned");                           \
  CC_REQUIRE(((uintptr_t)index & 255) == 0, name ": index must be 256-byte aligned")

extern "C" int cc_cube_cluster(const void *index, int32_t cap, int32_t N, int32_t K, int32_t k,
                               const int32_t *init_ids, int32_t max_iter, void *ws, int32_t *label,
                               float *dist, float *centroids, int32_t *sizes, int32_t *changed,
                               int32_t *n_iter, void *stream) {
  CC_REQUIRE(index && init_ids && ws && label && dist && centroids && sizes && changed && n_iter,
             "cc_cube_cluster: null pointer");
  CC_CLUSTER_COMMON("cc_cube_cluster");
  CC_REQUIRE(max_iter >= 0 && max_iter <= 0x7FFFFFFF - 1, "cc_cube_cluster: max_iter must not be negative");
  if (N == 0) return CC_OK;
  CC_REQUIRE(k <= N, "cc_cube_cluster: k must be at most N");
  const IndexLayout x = index_layout(cap, K);
  const ClusterWs w = cluster_ws(N, K, k, 0);
  hipStream_t s = as_stream(stream);
  const float *n = (const float *)((const char *)index + x.n);
  char *base = (char *)ws;
  float *cT = (float *)(base + w.cT);
  float *part = (float *)(base + w.part);
  uint16_t *map = (uint16_t *)(base + w.map);
  unsigned long long *best = (unsigned long long *)(base + w.best);
  const int most = std::max(N, std::max(k, max_iter + 1));
  hipLaunchKernelGGL(start_kernel, dim3((unsigned)cdiv(most, 256)), dim3(256), 0, s, N, label, best, max_iter, changed,
                     k, sizes);
  CC_LAUNCH_CHECK("start_kernel");
  hipLaunchKernelGGL(centroid_image_kernel, dim3(k), dim3(QNT), 0, s, n, N, K, x.Kp, init_ids,
                     (const float *)nullptr, w.kp, cT, centroids);
  CC_LAUNCH_CHECK("centroid_image_kernel");
  for (int t = 0; t <= max_iter; ++t) {
    if (launch_assign(s, n, nullptr, N, x.Kp, cT, k, w.kp, t ? changed + (t - 1) : nullptr, best, label, dist,
                      changed + t) != CC_OK)
      return CC_ERR_HIP;
    if (t == max_iter) break;
    hipLaunchKernelGGL(block_sums_kernel, dim3(w.blocks), dim3(CB), 0, s, n, N, x.Kp, label, k, changed + t, part,
                       map);
    CC_LAUNCH_CHECK("block_sums_kernel");
    hipLaunchKernelGGL(centroid_kernel, dim3(k), dim3(64), (size_t)x.Kp * sizeof(float), s, part, map, w.blocks, K,
                       x.Kp, k, w.kp, changed + t, centroids, cT);
    CC_LAUNCH_CHECK("centroid_kernel");
  }
  hipLaunchKernelGGL(sizes_kernel, dim3((unsigned)cdiv(N, 1024)), dim3(256), 0, s, label, N, k, sizes);
  CC_LAUNCH_CHECK("sizes_kernel");
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(256), 0, s, max_iter, changed, n_iter);
  CC_LAUNCH_CHECK("finish_kernel");
  return CC_OK;
}

extern "C" int cc_cube_assign(const void *index, int32_t cap, int32_t N, int32_t K, int32_t k,
                              const float *centroids, int32_t Q, const int32_t *qid, const float *zq, void *ws,
                              int32_t *label, float *dist, void *stream) {
  CC_REQUIRE(index && centroids && ws && label && dist, "cc_cube_assign: null pointer");
  CC_CLUSTER_COMMON("cc_cube_assign");
  CC_REQUIRE(Q >= 0 && Q <= MAX_Q, "cc_cube_assign: Q outside 0..2^22");
  if (Q == 0) return CC_OK;
  const IndexLayout x = index_layout(cap, K);
  const ClusterWs w = cluster_ws(0, K, k, Q);
  hipStream_t s = as_stream(stream);
  const float *n = (const float *)((const char *)index + x.n);
  char *base = (char *)ws;
  float *cT = (float *)(base + w.cT);
  float *qn = (float *)(base + w.qn);
  int32_t *qok = (int32_t *)(base + w.qok);
  unsigned long long *best = (unsigned long long *)(base + w.best);
  hipLaunchKernelGGL(centroid_image_kernel, dim3(k), dim3(QNT), 0, s, n, N, K, x.Kp, (const int32_t *)nullptr,
                     centroids, w.kp, cT, (float *)nullptr);
  CC_LAUNCH_CHECK("centroid_image_kernel");
  hipLaunchKernelGGL(query_rows_kernel, dim3(Q), dim3(QNT), 0, s, n, N, K, x.Kp, qid, zq, qn, qok);
  CC_LAUNCH_CHECK("query_rows_kernel");
  hipLaunchKernelGGL(no_best_kernel, dim3((unsigned)cdiv(Q, 256)), dim3(256), 0, s, best, Q);
  CC_LAUNCH_CHECK("no_best_kernel");
  return launch_assign(s, qn, qok, Q, x.Kp, cT, k, w.kp, nullptr, best, label, dist, nullptr);
}
