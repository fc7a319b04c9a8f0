// cc_similar_cards_batch — Q query cards per call, every row bit-identical to cc_similar_cards on
// it (similarity.hip: the pinned arithmetic, fp32, multiply and add separately rounded, sums in
// index order).
//
// The single-request kernel recomputes both norms for every (query, card) and walks rows at a
// stride of K floats.  n_j[i] = e_j[i] * inv_j is the very factor it multiplies (qe[i]*invq is
// n_q[i] of row q), so normalising every card once changes no bit:
//   normalise_kernel : one thread per row over a tile of 128 rows staged through LDS (pitch 33:
//                      coalesced loads, conflict-free row walks).  ss_j in index order,
//                      inv_j = 1/sqrt(max(ss_j, 1e-12)), then n [V][Kp] (row-major, for the
//                      queries) and nT [Kp][Vs] (k-major, for the cards); Kp = K rounded up to the
//                      distance kernel's k stage, the pad written as zeros.  It writes at a row
//                      offset (0 here): cubesim.hip's puts run it through cc::normalise_rows_launch.
//   dist_tile_kernel : one workgroup per tile of 16*RM queries x 64 cards: the shared dot-product
//                      tile (dottile.hpp) with n for both operands and one running
//                      sum, so any K > 0 fits.  The pad adds +0 * +0 to a sum that is never -0: no
//                      bit moves.  Writes the sort key orderable(-dot) of every (query, card) and
//                      the distances only on request.  Query ids come from device memory; one
//                      outside [0, V) is never an index.
//   select_rows_kernel: one workgroup per query.  The composite (key << 32 | card) is unique, so
//                      the N smallest are a radix SELECT of the N-th smallest composite (10-bit
//                      digits from the top, LDS histograms, prefix scan; stops as soon as the
//                      composites at or below the chosen bin are N or a few more) and a bitonic
//                      sort of the survivors in LDS, of which the first N are written: ascending
//                      composite = ascending distance, equal distances lower card first = numpy
//                      argsort(kind='stable').
//   sort_rows_kernel : N above the select's cap: one workgroup per query sorts all V
//                      (key, card) pairs (stable LSD radix sort from ascending card order, four
//                      8-bit passes — a distance key differs in all 32 bits — through two
//                      ping-pong buffers in the workspace) and writes the first N.
// The returned distance is rebuilt from the key: orderable() is a bijection except that it folds
// -0 onto +0, and a distance is -dot with dot never -0, so a zero distance is always -0.0f.
#include <algorithm>

#include "common.hpp"
#include "cosine.hpp"
#include "detmath.hpp"
#include "dottile.hpp"
#include "rowsort.hpp"

namespace {

constexpr int KS = dottile::KS;   // k per stage of the normalise tile: the distance tile's
constexpr int TC = dottile::TC;   // cards per distance tile
constexpr int DNT = dottile::NT;  // distance-tile workgroup
constexpr int NR = 128;       // normalise: rows per workgroup, one thread each
constexpr int SNT = 1024;     // select / sort workgroup
constexpr int MAX_N = 2048;   // survivors sorted in LDS
constexpr int MAX_Q = 1 << 22;
constexpr int SBITS = 8;      // sort digit
constexpr int SPASSES = 4;

using detm::addf;
using detm::mulf;
using rowsort::orderable;  // similarity.hip's sort key
using cosine::dist_of_key;

// A 128 x 32 tile of z into LDS, zeros outside [0, rows) x [0, K): a thread's 32 loads are issued
// together (an address that is always valid, the value dropped afterwards), then stored.
__device__ __forceinline__ void stage_tile(float (*tile)[KS + 1], const float *__restrict__ z, int rows,
                                           int K, int r0, int k0) {
  static_assert(NR % KS == 0, "a thread keeps its column: step u holds rows u * NR / KS + tid / KS");
  const int c = threadIdx.x % KS, rq = threadIdx.x / KS;
  const bool col_ok = k0 + c < K;
  float x[KS];
#pragma unroll
  for (int u = 0; u < KS; ++u) {
    const int r = u * (NR / KS) + rq;
    const bool ok = col_ok && r0 + r < rows;
    const float v = z[ok ? (int64_t)(r0 + r) * K + k0 + c : 0];
    x[u] = ok ? v : 0.f;
  }
#pragma unroll
  for (int u = 0; u < KS; ++u) tile[u * (NR / KS) + rq][c] = x[u];
}

// rows of z -> rows [0, rows) of n [.][Kp] and columns [0, rows) of nT [Kp][pitch] (a row offset is
// in the pointers).  One thread per row, so a row's bits do not depend on where a launch starts or ends.
__global__ __launch_bounds__(NR) void normalise_kernel(const float *__restrict__ z, int rows, int K, int Kp,
                                                       int pitch, float *__restrict__ n,
                                                       float *__restrict__ nT) {
  __shared__ float tile[NR][KS + 1];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * NR, row = r0 + tid;
  float ss = 0.f;
  for (int k0 = 0; k0 < Kp; k0 += KS) {
    __syncthreads();  // the previous stage's readers are done
    stage_tile(tile, z, rows, K, r0, k0);
    __syncthreads();
    const int kc = min(KS, K - k0);
    for (int c = 0; c < kc; ++c) {
      const float x = tile[tid][c];
      ss = addf(ss, mulf(x, x));
    }
  }
  const float inv = cosine::inv_norm(ss);
  for (int k0 = 0; k0 < Kp; k0 += KS) {
    __syncthreads();
    stage_tile(tile, z, rows, K, r0, k0);
    __syncthreads();
#pragma unroll 8
    for (int c = 0; c < KS; ++c) {
      const float v = mulf(tile[tid][c], inv);
      tile[tid][c] = v;
      if (row < rows) nT[(int64_t)(k0 + c) * pitch + row] = v;
    }
    __syncthreads();
    for (int t = tid; t < NR * KS; t += NR) {
      const int r = t / KS, c = t % KS;
      if (r0 + r < rows) n[(int64_t)(r0 + r) * Kp + k0 + c] = tile[r][c];
    }
  }
}

template <int RM>
__global__ __launch_bounds__(DNT) void dist_tile_kernel(const float *__restrict__ n,
                                                        const float *__restrict__ nT, int V,
                                                        int Kp, int Vs, int Q,
                                                        const int32_t *__restrict__ queries,
                                                        uint32_t *__restrict__ keys,
                                                        float *__restrict__ dist_all) {
  constexpr int TR = 16 * RM;
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int nb = blockIdx.x * TC;  // first card of the tile
  const int rb = blockIdx.y * TR;  // first query of the tile
  // A thread stages local rows lr0 + RS * i at k offset kq: their pointers, null for a row past Q
  // or a query id outside [0, V)
  const int lr0 = tid / dottile::F4, kq = 4 * (tid % dottile::F4);
  const float *qrow[TR / dottile::RS];
#pragma unroll
  for (int i = 0; i < TR / dottile::RS; ++i) {
    const int gr = rb + lr0 + dottile::RS * i;
    const int q = gr < Q ? queries[gr] : -1;
    qrow[i] = (uint32_t)q < (uint32_t)V ? n + (int64_t)q * Kp + kq : nullptr;
  }
  const int gn = nb + (tid & 63);
  const auto dot = dottile::run<RM, false>(
      Kp, Vs, [=](int k) { return gn < V ? nT + (int64_t)k * Vs + gn : nullptr; },
      [=](int lr, int k) {
        const float *row = qrow[(lr - lr0) / dottile::RS];
        return row ? *reinterpret_cast<const float4 *>(row + (k - kq)) : dottile::zero4();
      });

  const int n0 = nb + 4 * tx;
  if (n0 >= V) return;
#pragma unroll
  for (int j = 0; j < RM; ++j) {
    const int gr = rb + ty * RM + j;
    if (gr >= Q) continue;
    const bool ok = (uint32_t)queries[gr] < (uint32_t)V;
    float dd[4];
    uint32_t key[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dd[e] = ok ? -dot.sum[j][e] : 0.f;
      key[e] = orderable(dd[e]);
    }
    uint32_t *kr = keys + (int64_t)gr * Vs + n0;  // Vs % 4 == 0: 16-B aligned, the pad is ours
    *reinterpret_cast<uint4 *>(kr) = make_uint4(key[0], key[1], key[2], key[3]);
    if (dist_all) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n0 + e < V) dist_all[(int64_t)gr * V + n0 + e] = dd[e];
    }
  }
}

// A row whose query id is outside [0, V): -1 / 0.f, nothing read.
__device__ __forceinline__ void fill_invalid_row(int32_t *oi, float *od, int N) {
  for (int i = threadIdx.x; i < N; i += SNT) {
    oi[i] = -1;
    od[i] = 0.f;
  }
}

__global__ __launch_bounds__(SNT) void select_rows_kernel(const uint32_t *__restrict__ keys, int Vs,
                                                          int V, const int32_t *__restrict__ queries,
                                                          int N, int32_t *__restrict__ out_idx,
                                                          float *__restrict__ out_dist) {
  __shared__ uint32_t hist[1024];
  __shared__ int wtot[SNT / 64];
  __shared__ uint64_t s_prefix, s_mask;
  __shared__ int s_rem, s_done, s_cnt;
  __shared__ uint64_t sel[MAX_N];
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  int32_t *oi = out_idx + (int64_t)r * N;
  float *od = out_dist + (int64_t)r * N;
  if ((uint32_t)queries[r] >= (uint32_t)V) {  // (block-uniform)
    fill_invalid_row(oi, od, N);
    return;
  }
  const uint32_t *k = keys + (int64_t)r * Vs;
  // The select stops as soon as the composites at or below the chosen bin fit `limit`: the sort
  // then orders a few more than N and the first N are written.  One size step of the bitonic
  // network is cheaper than one more pass over the row, and distances are dense in the key's top
  // bits only, so two passes usually do.
  int PN = 1;
  while (PN < N) PN <<= 1;
  const int limit = min(MAX_N, 2 * PN);
  if (tid == 0) {
    s_prefix = 0;
    s_mask = 0;
    s_rem = N;
    s_done = 0;
    s_cnt = 0;
  }
  __syncthreads();
  // composite bits: key in 32..63, card in 0..31; digits from the top, the windows split at bit 32
  // so that a window holding no bit of any card is skipped
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = pass < 3 ? 54 - 10 * pass : pass == 3 ? 32 : pass < 7 ? 22 - 10 * (pass - 4) : 0;
    const uint32_t dmask = (pass == 3 || pass == 7) ? 3u : 1023u;
    if (shift < 32 && ((uint32_t)(V - 1) >> shift) == 0u) continue;  // no card has a bit up here
    if (s_done) break;
    const uint64_t prefix = s_prefix, mask = s_mask;
    const int rem = s_rem;
    hist[tid] = 0u;
    __syncthreads();
    for (int j = tid; j < V; j += SNT) {
      const uint64_t cmp = ((uint64_t)k[j] << 32) | (uint32_t)j;
      if ((cmp & mask) == prefix) atomicAdd(&hist[(uint32_t)(cmp >> shift) & dmask], 1u);
    }
    __syncthreads();
    // thread t owns bin t: its inclusive scan is the count of matching items in bins <= it
    const int v = (int)hist[tid];
    const int le = rowsort::block_incl_scan<SNT>(v, wtot), lt = le - v;
    if (le >= rem && lt < rem) {  // exactly one bin: the one holding the rem-th smallest
      s_prefix = prefix | ((uint64_t)tid << shift);
      s_mask = mask | ((uint64_t)dmask << shift);
      s_rem = rem - lt;
      s_done = (N - (rem - lt)) + v <= limit;  // everything at or below this bin: N or a few more
    }
    __syncthreads();
  }
  // the bits outside the mask are below every decided digit or zero in every composite: on the
  // decided bits, a candidate <=> at or below the prefix; all passes done, exactly N of them
  const uint64_t T = s_prefix, M = s_mask;
  for (int j = tid; j < V; j += SNT) {
    const uint64_t cmp = ((uint64_t)k[j] << 32) | (uint32_t)j;
    if ((cmp & M) <= T) {
      const int pos = atomicAdd(&s_cnt, 1);
      if (pos < limit) sel[pos] = cmp;
    }
  }
  __syncthreads();
  const int cnt = min(s_cnt, limit);  // (N <= cnt <= limit by the counts; never past sel)
  int P = PN;
  while (P < cnt) P <<= 1;
  for (int i = cnt + tid; i < P; i += SNT) sel[i] = ~0ull;  // above every candidate
  __syncthreads();
  rowsort::bitonic_sort<SNT>(P, rowsort::CmpSwapU64<false>{sel});
  for (int i = tid; i < N; i += SNT) {
    const uint64_t cmp = sel[i];
    oi[i] = (int32_t)(uint32_t)cmp;
    od[i] = dist_of_key((uint32_t)(cmp >> 32));
  }
}

// Full ranking of one row: rowsort::radix_rank_row with a digit plan for 32-bit keys (a distance key
// differs in all 32 bits) and the ascending order kept.  (key, card) pairs ping-pong through
// pa / pb as one 64-bit word; the last pass stores nothing but the row's first N.
constexpr int RU = 8;  // items a lane loads ahead of ranking them

struct SortRow {
  using Item = uint64_t;  // key << 32 | card
  static constexpr int PASSES = SPASSES, RADIX_BITS = SBITS;
  static_assert(SPASSES % 2 == 0 && SBITS * SPASSES == 32, "pass 0 reads the keys, the last writes the results");
  static __device__ constexpr int bits(int) { return SBITS; }
  const uint32_t *k;
  uint64_t *bufa, *bufb;
  int32_t *oi;
  float *od;
  int N;
  __device__ __forceinline__ Item load(int pass, int i) const {  // pass 0 reads the keys
    return pass == 0 ? ((uint64_t)k[i] << 32) | (uint32_t)i : ((pass & 1) ? bufa : bufb)[i];
  }
  __device__ __forceinline__ uint32_t digit(Item x, int pass) const {
    return ((uint32_t)(x >> 32) >> (SBITS * pass)) & (uint32_t)((1 << SBITS) - 1);
  }
  __device__ __forceinline__ void store(int pass, uint32_t pos, Item x) const {
    ((pass & 1) ? bufb : bufa)[pos] = x;
  }
  __device__ __forceinline__ void emit(uint32_t pos, Item x) const {
    if (pos < (uint32_t)N) {
      oi[pos] = (int32_t)(uint32_t)x;
      od[pos] = dist_of_key((uint32_t)(x >> 32));
    }
  }
};

__global__ __launch_bounds__(SNT) void sort_rows_kernel(const uint32_t *__restrict__ keys, int Vs,
                                                        int V, const int32_t *__restrict__ queries,
                                                        int N, uint64_t *pa, uint64_t *pb, int Vp,
                                                        int32_t *__restrict__ out_idx,
                                                        float *__restrict__ out_dist) {
  __shared__ uint32_t hist[SNT / 64 << SBITS];
  __shared__ int wtot[SNT / 64];
  const int r = blockIdx.x;
  int32_t *oi = out_idx + (int64_t)r * N;
  float *od = out_dist + (int64_t)r * N;
  if ((uint32_t)queries[r] >= (uint32_t)V) {  // (block-uniform)
    fill_invalid_row(oi, od, N);
    return;
  }
  const SortRow t{keys + (int64_t)r * Vs, pa + (int64_t)r * Vp, pb + (int64_t)r * Vp, oi, od, N};
  rowsort::radix_rank_row<SNT, RU>(t, V, hist, wtot);
}

// workspace: [n V*Kp][nT Kp*Vs][keys Q*Vs] and, for N above the select's cap, the two
// (key, card) ping-pong buffers [Q][Vp] of 64-bit words (Vp a multiple of 16: no two rows share a
// 128-byte line)
struct SimWs {
  size_t n, nT, keys, pa, pb, total;
  int Kp, Vs, Vp;
};
SimWs sim_ws(int V, int K, int Q, int N) {
  SimWs w;
  const size_t v = (size_t)std::max(V, 1), q = (size_t)std::max(Q, 1);
  w.Kp = cosine::k_pad(K);
  w.Vs = (int)((v + 3) & ~(size_t)3);
  w.Vp = (int)((v + 15) & ~(size_t)15);
  size_t o = 0;
  w.n = o, o += align256(v * w.Kp * sizeof(float));
  w.nT = o, o += align256((size_t)w.Kp * w.Vs * sizeof(float));
  w.keys = o, o += align256(q * w.Vs * sizeof(uint32_t));
  w.pa = w.pb = o;
  if (N > MAX_N) {
    w.pa = o, o += align256(q * w.Vp * sizeof(uint64_t));
    w.pb = o, o += align256(q * w.Vp * sizeof(uint64_t));
  }
  w.total = o;
  return w;
}

template <int RM>
void launch_dist(hipStream_t s, const float *n, const float *nT, int V, int Kp, int Vs, int Q,
                 const int32_t *queries, uint32_t *keys, float *dist_all) {
  const dim3 grid((unsigned)cdiv(V, TC), (unsigned)cdiv(Q, 16 * RM));
  hipLaunchKernelGGL(dist_tile_kernel<RM>, grid, dim3(DNT), 0, s, n, nT, V, Kp, Vs, Q, queries, keys,
                     dist_all);
}

}  // namespace

int cc::normalise_rows_launch(const float *z, int rows, int K, int Kp, int pitch, int n0, float *n,
                              float *nT, hipStream_t s) {
  hipLaunchKernelGGL(normalise_kernel, dim3((unsigned)cdiv(rows, NR)), dim3(NR), 0, s, z, rows, K, Kp,
                     pitch, n + (int64_t)n0 * Kp, nT + n0);
  CC_LAUNCH_CHECK("normalise_kernel");
  return CC_OK;
}

extern "C" int32_t cc_similar_batch_max_n(void) { return MAX_N; }

extern "C" size_t cc_similar_batch_ws_size(int32_t V, int32_t K, int32_t Q, int32_t N) {
  return sim_ws(V, K, Q, N).total + 256;
}

// Every argument check of both entries, before anything is created or launched.
static int similar_batch_check(const char *who, const float *emb, int V, int K, int Q,
                               const int32_t *queries, int N, void *ws, int32_t *out_idx,
                               float *out_dist) {
  const std::string name(who);
  CC_REQUIRE(emb && queries && ws && out_idx && out_dist, name + ": null pointer");
  CC_REQUIRE(V > 0 && K > 0 && V <= 0x7FFFFFFF - 64 && K <= 0x7FFFFFFF - KS, name + ": bad V/K");
  CC_REQUIRE(Q >= 0 && Q <= MAX_Q, name + ": Q outside 0..2^22");
  CC_REQUIRE(N >= 1 && N <= V, name + ": N must be 1..V");
  CC_REQUIRE(((uintptr_t)ws & 255) == 0, name + ": ws must be 256-byte aligned");
  return CC_OK;
}

// The launches of both entries (arguments checked).  ev (the timed entry): four events recorded
// before the first kernel and behind each of the three.
static int similar_batch_launch(const float *emb, int V, int K, int Q, const int32_t *queries, int N,
                                void *ws, int32_t *out_idx, float *out_dist, float *dist_all,
                                hipStream_t s, hipEvent_t *ev) {
  if (Q == 0) return CC_OK;
  const SimWs w = sim_ws(V, K, Q, N);
  char *base = (char *)ws;
  float *n = (float *)(base + w.n), *nT = (float *)(base + w.nT);
  uint32_t *keys = (uint32_t *)(base + w.keys);
  if (ev) CC_HIP(hipEventRecord(ev[0], s));
  if (int rc = cc::normalise_rows_launch(emb, V, K, w.Kp, w.Vs, 0, n, nT, s)) return rc;
  if (ev) CC_HIP(hipEventRecord(ev[1], s));
  // queries per tile: 32 / 64 / 128 (the arithmetic per (query, card) does not depend on it)
  if (Q <= 32)
    launch_dist<2>(s, n, nT, V, w.Kp, w.Vs, Q, queries, keys, dist_all);
  else if (Q <= 64)
    launch_dist<4>(s, n, nT, V, w.Kp, w.Vs, Q, queries, keys, dist_all);
  else
    launch_dist<8>(s, n, nT, V, w.Kp, w.Vs, Q, queries, keys, dist_all);
  CC_LAUNCH_CHECK("dist_tile_kernel");
  if (ev) CC_HIP(hipEventRecord(ev[2], s));
  if (N <= MAX_N) {
    hipLaunchKernelGGL(select_rows_kernel, dim3(Q), dim3(SNT), 0, s, keys, w.Vs, V, queries, N,
                       out_idx, out_dist);
    CC_LAUNCH_CHECK("select_rows_kernel");
  } else {
    hipLaunchKernelGGL(sort_rows_kernel, dim3(Q), dim3(SNT), 0, s, keys, w.Vs, V, queries, N,
                       (uint64_t *)(base + w.pa), (uint64_t *)(base + w.pb), w.Vp, out_idx, out_dist);
    CC_LAUNCH_CHECK("sort_rows_kernel");
  }
  if (ev) CC_HIP(hipEventRecord(ev[3], s));
  return CC_OK;
}

extern "C" int cc_similar_cards_batch(const float *emb, int32_t V, int32_t K, int32_t Q,
                                      const int32_t *queries, int32_t N, void *ws, int32_t *out_idx,
                                      float *out_dist, float *dist_all, void *stream) {
  if (int rc = similar_batch_check("cc_similar_cards_batch", emb, V, K, Q, queries, N, ws, out_idx, out_dist))
    return rc;
  return similar_batch_launch(emb, V, K, Q, queries, N, ws, out_idx, out_dist, dist_all,
                              as_stream(stream), nullptr);
}

// The same call for measurements (tools/similarity_batch_bench.py): HIP events around each kernel,
// then a wait for the last one.  kernel_ms: host [3] = normalise, distance tile, select or sort.
extern "C" int cc_similar_cards_batch_timed(const float *emb, int32_t V, int32_t K, int32_t Q,
                                            const int32_t *queries, int32_t N, void *ws,
                                            int32_t *out_idx, float *out_dist, float *dist_all,
                                            float *kernel_ms, void *stream) {
  CC_REQUIRE(kernel_ms, "cc_similar_cards_batch_timed: null pointer");
  int rc = similar_batch_check("cc_similar_cards_batch_timed", emb, V, K, Q, queries, N, ws, out_idx, out_dist);
  if (rc != CC_OK) return rc;
  kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0.f;
  if (Q == 0) return CC_OK;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < 4 && rc == CC_OK; ++i)
    if (hipEventCreate(&ev[i]) != hipSuccess) rc = cc::fail(CC_ERR_HIP, "cc_similar_cards_batch_timed: hipEventCreate");
  if (rc == CC_OK)
    rc = similar_batch_launch(emb, V, K, Q, queries, N, ws, out_idx, out_dist, dist_all,
                              as_stream(stream), ev);
  if (rc == CC_OK) {
    if (hipEventSynchronize(ev[3]) != hipSuccess)
      rc = cc::fail(CC_ERR_HIP, "cc_similar_cards_batch_timed: hipEventSynchronize");
    for (int i = 0; i < 3 && rc == CC_OK; ++i)
      if (hipEventElapsedTime(&kernel_ms[i], ev[i], ev[i + 1]) != hipSuccess)
        rc = cc::fail(CC_ERR_HIP, "cc_similar_cards_batch_timed: hipEventElapsedTime");
  }
  for (int i = 0; i < 4; ++i)
    if (ev[i]) (void)hipEventDestroy(ev[i]);
  return rc;
}
