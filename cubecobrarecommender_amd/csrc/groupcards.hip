// cc_group_cards_count / cc_group_cards_top — archetype card profiles: a group-by of cubes (CSR of
// sorted distinct card ids) by an integer label into card counts per group, and per group the m
// cards with the largest integer rank key.  DESIGN.md 4.13; tests/group_cards_ref.py restates it.
//
// All integers: count[g][v] = cubes of label g holding card v, size[g] = cubes of label g, total[v]
// = sum over g of count[g][v], N = sum of size.  Integer adds commute, so no output bit depends on
// the path, the slice size, the spans a corpus is streamed in or the order workgroups finish in.
// Kernels, all on one stream and never waited for:
//   label_hist_kernel   : the span's cubes per label, an LDS histogram per 1,024 cubes and one
//                         integer atomic per present label (into the workspace, or straight into size).
//   plan_kernel         : one workgroup.  Scans the label counts into the groups' starts in `order`,
//                         adds them into size, and cuts every group into slices of S cubes: the work
//                         list (group, slice) and its length.
//   scatter_kernel      : the cube ids grouped by label into order [R] (an LDS rank per 1,024 cubes,
//                         one atomic per present label for the workgroup's run; the order inside a
//                         group is whatever it comes to: the counts do not depend on it).
//   count_priv_kernel   : path 1.  A workgroup takes one work item and one card tile of TILE cards:
//                         zeroes TILE 32-bit counters in LDS, walks its cubes one wave per cube (the
//                         lanes read consecutive ids: distinct within a cube, so a wave never collides
//                         with itself; lane q of a wave has fetched the wave's q-th cube's row bounds
//                         up front, so a cube costs one dependent round trip, not three), counts with
//                         LDS atomics and flushes the non-zero counters to count[g]: plain stores
//                         when the group is one slice and nothing is accumulated, else integer
//                         atomics.  With several tiles a row's part of the tile is found by two
//                         binary searches (rows are sorted).
//   total_kernel        : path 1.  total = the column sums of count.
//   count_direct_kernel : path 2.  One wave per cube, an integer atomic into count[g][v] and one
//                         into total[v] per id: no zeroing or flushing of a histogram, which is what
//                         a span with a few cubes per group spends its time on in path 1.
//   top_kernel          : one 1,024-thread workgroup per group: N from size, the candidate count,
//                         rowsel::select_smallest over the V composites (2^45 - key) << 18 | card,
//                         the m results from LDS.
#include <algorithm>

#include "common.hpp"
#include "rowselect.hpp"

namespace {

constexpr int TILE = 22528;         // cards of one LDS histogram: 88 KiB of 32-bit counters
constexpr int CNT = 1024;           // count_priv_kernel's workgroup
constexpr int CWAVES = CNT / 64;
constexpr int MAX_G = 1024;         // groups per call: plan_kernel has a thread per group
constexpr int MAX_ROWS = 1 << 22;   // cubes per call, and the largest N the rank keys admit
constexpr int MAX_V = 1 << 18;      // the composite's card bits
constexpr int MIN_SLICE = 256, MAX_SLICE = 2048;  // cubes per slice (slice_of)
constexpr int FILL = 512;           // workgroups wanted of a span with few groups
// path 0: below this many cubes per group in the span the direct path is taken (measured at
// G = 1,024: direct wins at 1 cube per group, loses two to one at 4)
constexpr int DIRECT_BELOW_ROWS_PER_GROUP = 2;

// The slice size: with enough groups to fill the device alone, twice the mean group (most groups
// are then one slice and flush with plain stores); else what cuts the span into FILL slices.
int slice_of(int R, int G) {
  const int64_t want = G >= 256 ? 2 * cdiv(R, G) : cdiv(R, FILL);
  return (int)std::min<int64_t>(MAX_SLICE, std::max<int64_t>(MIN_SLICE, want));
}

// workspace: [gcount G][gstart G + 1][cursor G][nwork 1][work max_work x 2][order R]
struct GroupWs {
  size_t gcount, gstart, cursor, nwork, work, order, total;
  int max_work;
};
GroupWs group_ws(int R, int G) {
  GroupWs w;
  const size_t r = (size_t)std::max(R, 0), g = (size_t)std::max(G, 1);
  w.max_work = (int)(g + r / MIN_SLICE + 1);  // sum over groups of ceil(n_g / S), S >= MIN_SLICE
  size_t o = 0;
  w.gcount = o, o += align256(g * sizeof(int32_t));
  w.gstart = o, o += align256((g + 1) * sizeof(int32_t));
  w.cursor = o, o += align256(g * sizeof(int32_t));
  w.nwork = o, o += 256;
  w.work = o, o += align256((size_t)w.max_work * 2 * sizeof(int32_t));
  w.order = o, o += align256(r * sizeof(int32_t));
  w.total = o;
  return w;
}

// out[l] += the cubes of this workgroup's 1,024 rows with label l (a label outside [0, G) counts
// nowhere)
__global__ __launch_bounds__(256) void label_hist_kernel(const int32_t *__restrict__ label, int R, int G,
                                                         int32_t *__restrict__ out) {
  __shared__ int hist[MAX_G];
  const int tid = threadIdx.x;
  for (int j = tid; j < G; j += 256) hist[j] = 0;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * 1024;
  for (int u = 0; u < 4; ++u) {
    const int64_t i = i0 + u * 256 + tid;
    if (i < R) {
      const int l = label[i];
      if ((uint32_t)l < (uint32_t)G) atomicAdd(&hist[l], 1);
    }
  }
  __syncthreads();
  for (int j = tid; j < G; j += 256)
    if (hist[j]) atomicAdd(&out[j], hist[j]);
}

__global__ __launch_bounds__(1024) void plan_kernel(const int32_t *__restrict__ gcount, int G, int S,
                                                    int accumulate, int32_t *__restrict__ size,
                                                    int32_t *__restrict__ gstart, int32_t *__restrict__ cursor,
                                                    int32_t *__restrict__ nwork, int32_t *__restrict__ work,
                                                    int max_work) {
  __shared__ int wtot[1024 / 64];
  __shared__ int wb[MAX_G + 1];  // first work item of every group, and the end
  const int tid = threadIdx.x;
  const int n = tid < G ? max(gcount[tid], 0) : 0;
  const int end = rowsort::block_incl_scan<1024>(n, wtot);
  if (tid < G) {
    gstart[tid] = end - n;
    cursor[tid] = end - n;
    size[tid] = accumulate ? size[tid] + n : n;
  }
  if (tid == G - 1) gstart[G] = end;
  const int slices = (n + S - 1) / S;
  const int wend = rowsort::block_incl_scan<1024>(slices, wtot);
  wb[tid] = wend - slices;
  if (tid == 1023) wb[MAX_G] = wend;
  __syncthreads();
  const int nw = min(wb[MAX_G], max_work);  // (never above max_work: S >= MIN_SLICE)
  if (tid == 0) *nwork = nw;
  for (int w = tid; w < nw; w += 1024) {
    int lo = 0, hi = MAX_G + 1;  // the first i with wb[i] > w; its group is i - 1
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (wb[mid] > w)
        hi = mid;
      else
        lo = mid + 1;
    }
    const int g = lo - 1;
    work[2 * w] = g;
    work[2 * w + 1] = w - wb[g];
  }
}

__global__ __launch_bounds__(256) void scatter_kernel(const int32_t *__restrict__ label, int R, int G,
                                                      int32_t *__restrict__ cursor, int32_t *__restrict__ order) {
  __shared__ int hist[MAX_G], base[MAX_G];
  const int tid = threadIdx.x;
  for (int j = tid; j < G; j += 256) hist[j] = 0;
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * 1024;
  int lab[4], rank[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = i0 + u * 256 + tid;
    lab[u] = i < R ? label[i] : -1;
    rank[u] = (uint32_t)lab[u] < (uint32_t)G ? atomicAdd(&hist[lab[u]], 1) : 0;
  }
  __syncthreads();
  for (int j = tid; j < G; j += 256)
    if (hist[j]) base[j] = atomicAdd(&cursor[j], hist[j]);
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if ((uint32_t)lab[u] < (uint32_t)G) {
      const int pos = base[lab[u]] + rank[u];
      if ((uint32_t)pos < (uint32_t)R) order[pos] = (int32_t)(i0 + u * 256 + tid);  // (always: the counts are these labels')
    }
}

// the first p in [a, b) with idx[p] >= v, else b
__device__ __forceinline__ int lower_bound(const int32_t *__restrict__ idx, int a, int b, int v) {
  while (a < b) {
    const int mid = a + ((b - a) >> 1);
    if (idx[mid] < v)
      a = mid + 1;
    else
      b = mid;
  }
  return a;
}

// Dynamic LDS: TILE counters.
__global__ __launch_bounds__(CNT) void count_priv_kernel(const int32_t *__restrict__ row_ptr,
                                                         const int32_t *__restrict__ idx, int V,
                                                         const int32_t *__restrict__ gstart,
                                                         const int32_t *__restrict__ order,
                                                         const int32_t *__restrict__ nwork,
                                                         const int32_t *__restrict__ work, int S, int tiles,
                                                         int accumulate, uint32_t *__restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_hist[];  // [TILE]
  const int w = blockIdx.x;
  if (w >= *nwork) return;  // (block-uniform)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = work[2 * w], slice = work[2 * w + 1];
  const int g0 = gstart[g], g1 = gstart[g + 1];
  const int c0 = g0 + slice * S, c1 = min(g1, c0 + S);
  const int t0 = blockIdx.y * TILE, tn = min(TILE, V - t0);
  for (int v = tid; v < tn; v += CNT) s_hist[v] = 0u;
  __syncthreads();
  for (int cb = c0; cb < c1; cb += CWAVES * 64) {
    // lane q holds the bounds of the wave's q-th cube of this step
    const int c = cb + lane * CWAVES + wv;
    int a = 0, b = 0;
    if (c < c1) {
      const int i = order[c];
      a = row_ptr[i];
      b = row_ptr[i + 1];
    }
    const int left = c1 - cb - wv;  // (wave-uniform)
    const int nc = left > 0 ? min(64, (left + CWAVES - 1) / CWAVES) : 0;
    for (int q = 0; q < nc; ++q) {
      int ra = __shfl(a, q, 64), rb = __shfl(b, q, 64);
      if (tiles > 1) {
        ra = lower_bound(idx, ra, rb, t0);
        rb = lower_bound(idx, ra, rb, t0 + tn);
      }
      for (int p0 = ra; p0 < rb; p0 += 256) {
        int id[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int p = p0 + 64 * u + lane;
          id[u] = p < rb ? idx[p] : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const uint32_t off = (uint32_t)(id[u] - t0);  // an id outside the tile is never an index
          if (off < (uint32_t)tn) atomicAdd(&s_hist[off], 1u);
        }
      }
    }
  }
  __syncthreads();
  uint32_t *out = count + (size_t)g * V + t0;
  const bool plain = !accumulate && g1 - g0 <= S;  // the group's only slice into zeroed counters
  for (int v = tid; v < tn; v += CNT) {
    const uint32_t c = s_hist[v];
    if (c) {
      if (plain)
        out[v] = c;
      else
        atomicAdd(&out[v], c);
    }
  }
}

// total[v] += count[g][v] over this workgroup's groups g = blockIdx.y, + gridDim.y, ... (total zeroed)
__global__ __launch_bounds__(256) void total_kernel(const uint32_t *__restrict__ count, int V, int G,
                                                    uint32_t *__restrict__ total) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  uint32_t sum = 0u;
  for (int g = blockIdx.y; g < G; g += gridDim.y) sum += count[(size_t)g * V + v];
  if (sum) atomicAdd(&total[v], sum);
}

__global__ __launch_bounds__(256) void count_direct_kernel(const int32_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ idx, int R, int V,
                                                           const int32_t *__restrict__ label, int G,
                                                           uint32_t *__restrict__ count,
                                                           uint32_t *__restrict__ total) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= R) return;  // (wave-uniform)
  const int l = label[i];
  if ((uint32_t)l >= (uint32_t)G) return;
  const int a = row_ptr[i], b = row_ptr[i + 1];
  uint32_t *out = count + (size_t)l * V;
  for (int p = a + lane; p < b; p += 64) {
    const int id = idx[p];
    if ((uint32_t)id < (uint32_t)V) {
      atomicAdd(&out[id], 1u);
      atomicAdd(&total[id], 1u);
    }
  }
}

constexpr int64_t KEY_LIMIT = (int64_t)1 << 44;  // |key| <= MAX_ROWS^2
constexpr int CARD_BITS = 18;                    // MAX_V

// Card j of one group as its composite, NONE where it is no candidate.
struct KeyItem {
  const uint32_t *cnt, *tot;
  int64_t s, N;
  int kind;
  uint32_t minc;
  __device__ __forceinline__ uint64_t operator()(int j) const {
    const int64_t a = cnt[j], t = tot[j];
    if ((kind == CC_GROUP_AVOID ? t : a) < (int64_t)minc) return rowsel::NONE;
    int64_t k = kind == CC_GROUP_RATE ? a : kind == CC_GROUP_LIFT ? a * N - t * s : t * s - a * N;
    k = k < -KEY_LIMIT ? -KEY_LIMIT : k > KEY_LIMIT ? KEY_LIMIT : k;  // (no counts of anything: still 64 bits)
    return ((uint64_t)((2 * KEY_LIMIT) - k) << CARD_BITS) | (uint32_t)j;
  }
};

__global__ __launch_bounds__(rowsel::SNT) void top_kernel(const uint32_t *__restrict__ count,
                                                          const int32_t *__restrict__ size,
                                                          const uint32_t *__restrict__ total, int V, int G,
                                                          int kind, uint32_t minc, int m,
                                                          int32_t *__restrict__ cards,
                                                          uint32_t *__restrict__ card_count,
                                                          int32_t *__restrict__ found) {
  __shared__ rowsel::SelectLds s;
  __shared__ unsigned long long s_N;
  __shared__ int s_cand;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_N = 0ull, s_cand = 0;
  __syncthreads();
  if (tid < G) atomicAdd(&s_N, (unsigned long long)min(max(size[tid], 0), MAX_ROWS + 1));
  __syncthreads();
  const int64_t N = (int64_t)s_N, sg = max(size[g], 0);
  const KeyItem item{count + (size_t)g * V, total, sg, N, kind, minc};
  int want = 0;
  if (sg > 0 && N <= MAX_ROWS) {  // (block-uniform)
    int mine = 0;
    for (int j = tid; j < V; j += rowsel::SNT) mine += item(j) != rowsel::NONE ? 1 : 0;
    if (mine) atomicAdd(&s_cand, mine);
    __syncthreads();
    want = min(m, s_cand);
  }
  if (want > 0) rowsel::select_smallest(s, item, V, want, 0xFFFFFFFFu);
  for (int i = tid; i < m; i += rowsel::SNT) {
    const int card = i < want ? (int)(s.sel[i] & ((1u << CARD_BITS) - 1u)) : -1;
    cards[(size_t)g * m + i] = card;
    card_count[(size_t)g * m + i] = card >= 0 ? item.cnt[card] : 0u;
  }
  if (tid == 0) found[g] = want;
}

}  // namespace

extern "C" int32_t cc_group_cards_tile(void) { return TILE; }

extern "C" int32_t cc_group_cards_max_groups(void) { return MAX_G; }

extern "C" size_t cc_group_cards_ws_size(int32_t R, int32_t V, int32_t G, int32_t m) {
  (void)V, (void)m;  // neither a histogram nor a result lives in the workspace
  return group_ws(R, G).total + 256;
}

#define CC_GROUP_COMMON(name)                                                                     \
  CC_REQUIRE(V >= 1 && V <= MAX_V, name ": V must be 1..2^18");                                   \
  CC_REQUIRE(G >= 1 && G <= MAX_G, name ": G must be 1..cc_group_cards_max_groups()");            \
  CC_REQUIRE(((uintptr_t)ws & 255) == 0, name ": ws must be 256-byte aligned")

extern "C" int cc_group_cards_count(const int32_t *row_ptr, const int32_t *idx, int32_t R, int32_t V,
                                    const int32_t *label, int32_t G, int32_t accumulate, int32_t path, void *ws,
                                    uint32_t *count, int32_t *size, uint32_t *total, void *stream) {
  CC_REQUIRE(row_ptr && idx && label && ws && count && size && total, "cc_group_cards_count: null pointer");
  CC_GROUP_COMMON("cc_group_cards_count");
  CC_REQUIRE(R >= 0 && R <= MAX_ROWS, "cc_group_cards_count: R must be 0..2^22");
  CC_REQUIRE(accumulate == 0 || accumulate == 1, "cc_group_cards_count: accumulate must be 0 or 1");
  CC_REQUIRE(path >= 0 && path <= 2, "cc_group_cards_count: path must be 0, 1 or 2");
  hipStream_t s = as_stream(stream);
  if (path == 0) path = (int64_t)R < (int64_t)DIRECT_BELOW_ROWS_PER_GROUP * G ? 2 : 1;
  if (!accumulate) {
    CC_HIP(hipMemsetAsync(count, 0, (size_t)G * V * sizeof(uint32_t), s));
    CC_HIP(hipMemsetAsync(size, 0, (size_t)G * sizeof(int32_t), s));
    CC_HIP(hipMemsetAsync(total, 0, (size_t)V * sizeof(uint32_t), s));
  }
  if (R == 0) return CC_OK;
  const unsigned row_blocks = (unsigned)cdiv(R, 1024);
  if (path == 2) {
    hipLaunchKernelGGL(label_hist_kernel, dim3(row_blocks), dim3(256), 0, s, label, R, G, size);
    CC_LAUNCH_CHECK("label_hist_kernel");
    hipLaunchKernelGGL(count_direct_kernel, dim3((unsigned)cdiv(R, 4)), dim3(256), 0, s, row_ptr, idx, R, V, label, G,
                       count, total);
    CC_LAUNCH_CHECK("count_direct_kernel");
    return CC_OK;
  }
  static const bool attr = hipFuncSetAttribute((const void *)count_priv_kernel,
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(TILE * sizeof(uint32_t))) == hipSuccess;
  CC_REQUIRE(attr, "cc_group_cards_count: dynamic LDS attribute");
  const GroupWs w = group_ws(R, G);
  char *base = (char *)ws;
  int32_t *gcount = (int32_t *)(base + w.gcount), *gstart = (int32_t *)(base + w.gstart);
  int32_t *cursor = (int32_t *)(base + w.cursor), *nwork = (int32_t *)(base + w.nwork);
  int32_t *work = (int32_t *)(base + w.work), *order = (int32_t *)(base + w.order);
  const int S = slice_of(R, G), tiles = (int)cdiv(V, TILE);
  const int grid_work = (int)std::min<int64_t>(w.max_work, std::min(G, R) + R / S);  // >= the work list
  CC_HIP(hipMemsetAsync(gcount, 0, (size_t)G * sizeof(int32_t), s));
  hipLaunchKernelGGL(label_hist_kernel, dim3(row_blocks), dim3(256), 0, s, label, R, G, gcount);
  CC_LAUNCH_CHECK("label_hist_kernel");
  hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(1024), 0, s, gcount, G, S, accumulate, size, gstart, cursor, nwork,
                     work, w.max_work);
  CC_LAUNCH_CHECK("plan_kernel");
  hipLaunchKernelGGL(scatter_kernel, dim3(row_blocks), dim3(256), 0, s, label, R, G, cursor, order);
  CC_LAUNCH_CHECK("scatter_kernel");
  hipLaunchKernelGGL(count_priv_kernel, dim3((unsigned)grid_work, (unsigned)tiles), dim3(CNT),
                     TILE * sizeof(uint32_t), s, row_ptr, idx, V, gstart, order, nwork, work, S, tiles, accumulate,
                     count);
  CC_LAUNCH_CHECK("count_priv_kernel");
  if (accumulate) CC_HIP(hipMemsetAsync(total, 0, (size_t)V * sizeof(uint32_t), s));
  hipLaunchKernelGGL(total_kernel, dim3((unsigned)cdiv(V, 256), (unsigned)std::min(G, 32)), dim3(256), 0, s, count, V,
                     G, total);
  CC_LAUNCH_CHECK("total_kernel");
  return CC_OK;
}

extern "C" int cc_group_cards_top(const uint32_t *count, const int32_t *size, const uint32_t *total, int32_t V,
                                  int32_t G, int32_t kind, int32_t min_count, int32_t m, void *ws, int32_t *cards,
                                  uint32_t *card_count, int32_t *found, void *stream) {
  CC_REQUIRE(count && size && total && ws && cards && card_count && found, "cc_group_cards_top: null pointer");
  CC_GROUP_COMMON("cc_group_cards_top");
  CC_REQUIRE(kind == CC_GROUP_RATE || kind == CC_GROUP_LIFT || kind == CC_GROUP_AVOID,
             "cc_group_cards_top: kind must be CC_GROUP_RATE, CC_GROUP_LIFT or CC_GROUP_AVOID");
  CC_REQUIRE(min_count >= 0, "cc_group_cards_top: min_count must not be negative");
  CC_REQUIRE(m >= 1 && m <= rowsel::MAX_K, "cc_group_cards_top: m must be 1..1024");
  hipLaunchKernelGGL(top_kernel, dim3(G), dim3(rowsel::SNT), 0, as_stream(stream), count, size, total, V, G, kind,
                     (uint32_t)std::max(min_count, 1), m, cards, card_count, found);
  CC_LAUNCH_CHECK("top_kernel");
  return CC_OK;
}
