// cc_cube_index_put / cc_cube_neighbours — a resident index of cube embeddings and the exact k
// nearest cubes of Q queries over it.  The arithmetic is card similarity's (similarity.hip,
// simbatch.hip, oracle/similarity_ref.py): fp32, multiply and add separately rounded,
// ss = sum e[i]^2 in index order, inv = 1/sqrt(max(ss, 1e-12)), n[i] = e[i] * inv,
// dist = -sum n_q[i] * n_j[i] in index order from +0; ranking by ascending composite
// (orderable(dist) << 32 | cube), which is unique: numpy argsort(kind='stable').
//
// The index is n [cap][Kp] (row-major, for member queries) and nT [Kp][caps] (k-major, for the
// corpus side of the distance tile), Kp = K rounded up to the tile's k stage, caps = cap rounded
// up to 64.  It is written by puts alone and normalised once:
//   normalise_kernel  : simbatch.hip's, at the put's row offset (cc::normalise_rows_launch).  One
//                       thread per row, so a row's bits do not depend on where a put starts or
//                       ends; the k pad of the rows it writes is written as zeros.
// A search runs, once per call,
//   query_rows_kernel : one 64-thread workgroup per query.  A member's row is copied from n, a
//                       fresh embedding is normalised by put's arithmetic (staged through LDS, the
//                       sum by one thread in index order), into qn [Q][Kp]; qok [Q] says whether the
//                       row is a query at all (an id outside [0, N) never is).
// then per chunk of the corpus (cubes [c0, c0 + cl)), so that the keys are [Q][chunk], never [Q][N],
//   dist_chunk_kernel : simbatch.hip's distance tile (dottile.hpp), 16*RM queries
//                       x 64 cubes per workgroup, the query rows from qn, the cubes from nT at c0.
//                       Writes orderable(-dot).
//   select_chunk_kernel: one workgroup per query.  The chunk's min(k, population) smallest
//                       composites, the row's skip left out, by the radix select and bitonic sort
//                       of select_rows_kernel, stored with global cube ids as candidates
//                       [Q][chunks][k]; unused slots hold a sentinel above every composite.
// and at the end
//   merge_rows_kernel : one workgroup per query.  The same select over the row's k * chunks
//                       candidates; writes the first min(k, candidates) ids and distances and the
//                       -1 / 0.f tail.  A corpus of one chunk needs no merge: its select writes
//                       the rows itself.
// Every cube is a candidate of exactly one chunk and a chunk keeps its k smallest, so the k
// smallest of the row are among the candidates whatever the chunk size; the composite order is
// total, so no output bit depends on the chunk, the batch or the launch.
#include <algorithm>

#include "common.hpp"
#include "cosine.hpp"
#include "cubeindex.hpp"
#include "detmath.hpp"
#include "dottile.hpp"
#include "rowselect.hpp"
#include "rowsort.hpp"

namespace {

constexpr int TC = dottile::TC;   // cubes per distance tile
constexpr int DNT = dottile::NT;  // distance-tile workgroup
using cubeindex::index_layout;
using cubeindex::IndexLayout;
using cubeindex::MAX_Q;
using cubeindex::QNT;
using cubeindex::query_rows_kernel;  // (cubeindex.hpp, shared with cubecluster.hip)

using detm::addf;
using detm::mulf;
using rowsort::orderable;
using rowsel::CandItem;
using rowsel::MAX_K;  // neighbours per query
using rowsel::NONE;   // above every composite of a finite distance
using rowsel::select_smallest;
using rowsel::SelectLds;
using rowsel::SNT;
using rowsel::write_row;

using cosine::dist_of_key;
using cosine::inv_norm;
using cosine::k_pad;

// keys [Q][pitch] of the chunk's cubes [c0, c0 + cl): key (r, j) = orderable(-dot(qn[r], n[c0 + j]))
// (4 waves per SIMD, as simbatch.hip's tile has at RM = 8: at most 128 VGPRs)
template <int RM>
__global__ __launch_bounds__(DNT, 4) void dist_chunk_kernel(const float *__restrict__ qn,
                                                            const int32_t *__restrict__ qok,
                                                            const float *__restrict__ nT, int caps, int c0,
                                                            int cl, int Kp, int Q, int pitch,
                                                            uint32_t *__restrict__ keys) {
  constexpr int TR = 16 * RM;
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int nb = blockIdx.x * TC;  // first cube of the tile, inside the chunk
  const int rb = blockIdx.y * TR;  // first query of the tile
  // A thread stages local rows lr0 + RS * i at k offset kq: one pointer, the distance to it uniform
  // (a multiple of RS rows and the stage's first k), and a bit per row that is inside Q and a query
  const int lr0 = tid / dottile::F4, kq = 4 * (tid % dottile::F4);
  const float *qbase = qn + (int64_t)(rb + lr0) * Kp + kq;
  uint32_t qmask = 0u;
#pragma unroll
  for (int i = 0; i < TR / dottile::RS; ++i) {
    const int gr = rb + lr0 + dottile::RS * i;
    if (gr < Q && qok[gr] != 0) qmask |= 1u << i;
  }
  const int gn = nb + (tid & 63);
  const auto dot = dottile::run<RM, false>(
      Kp, caps, [=](int k) { return gn < cl ? nT + (int64_t)k * caps + c0 + gn : nullptr; },
      [=](int lr, int k) {
        return (qmask >> ((lr - lr0) / dottile::RS)) & 1u
                   ? *reinterpret_cast<const float4 *>(qbase + (int64_t)(lr - lr0) * Kp + (k - kq))
                   : dottile::zero4();
      });

  const int n0 = nb + 4 * tx;
  if (n0 >= cl) return;
#pragma unroll
  for (int j = 0; j < RM; ++j) {
    const int gr = rb + ty * RM + j;
    if (gr >= Q) continue;
    uint32_t key[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) key[e] = orderable(-dot.sum[j][e]);
    // pitch % 64 == 0 and cl <= pitch: 16-B aligned, and the pad behind cl is this row's own
    *reinterpret_cast<uint4 *>(keys + (int64_t)gr * pitch + n0) = make_uint4(key[0], key[1], key[2], key[3]);
  }
}

struct ChunkItem {  // key << 32 | cube position inside the chunk; the skipped cube is no candidate
  const uint32_t *k;
  int skip;
  __device__ __forceinline__ uint64_t operator()(int j) const {
    const uint64_t cmp = ((uint64_t)k[j] << 32) | (uint32_t)j;  // loaded whatever j: no branch
    return j == skip ? NONE : cmp;
  }
};

// The select kernels are held to 80 allocated SGPRs (72 and the 6 the hardware adds, in steps of
// 16): at 96 a CU takes one 1,024-thread workgroup instead of two, and these loops, one load in
// flight per lane, then run 1.4 times as long (measured: 184 against 129 us).
#define CUBESIM_SELECT_KERNEL __attribute__((amdgpu_num_sgpr(72))) __global__ __launch_bounds__(SNT)

// Candidates of (query r, this chunk): cand[r][chunk][0..k), global cube ids, NONE behind the last.
// FINAL (the corpus is one chunk): the chunk's candidates are the row's result, written as such.
template <bool FINAL>
CUBESIM_SELECT_KERNEL void select_chunk_kernel(const uint32_t *__restrict__ keys, int pitch, int c0, int cl,
                                               const int32_t *__restrict__ qok,
                                               const int32_t *__restrict__ skip, int k, int chunk_no,
                                               int chunks, uint64_t *__restrict__ cand,
                                               int32_t *__restrict__ out_idx, float *__restrict__ out_dist) {
  __shared__ SelectLds s;
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  int want = 0;
  if (qok[r]) {  // (block-uniform)
    const int sk = skip ? skip[r] : -1;
    const int skl = (sk >= c0 && sk < c0 + cl) ? sk - c0 : -1;  // inside this chunk: its position
    want = min(k, cl - (skl >= 0 ? 1 : 0));
    if (want > 0) select_smallest(s, ChunkItem{keys + (int64_t)r * pitch, skl}, cl, want, (uint32_t)(cl - 1));
  } else if (!FINAL) {
    return;  // the merge reads nothing of a row that is no query
  }
  if (FINAL) {
    write_row(s, want, k, out_idx + (int64_t)r * k, out_dist + (int64_t)r * k, dist_of_key);  // c0 == 0
  } else {
    uint64_t *out = cand + ((int64_t)r * chunks + chunk_no) * k;
    // c0 + position < 2^31: the sum stays inside the low word
    for (int i = tid; i < want; i += SNT) out[i] = s.sel[i] + (uint32_t)c0;
    for (int i = max(want, 0) + tid; i < k; i += SNT) out[i] = NONE;
  }
}

CUBESIM_SELECT_KERNEL void merge_rows_kernel(const uint64_t *__restrict__ cand, int chunks,
                                                         int N, const int32_t *__restrict__ qok,
                                                         const int32_t *__restrict__ skip, int k,
                                                         int32_t *__restrict__ out_idx,
                                                         float *__restrict__ out_dist) {
  __shared__ SelectLds s;
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  int32_t *oi = out_idx + (int64_t)r * k;
  float *od = out_dist + (int64_t)r * k;
  int want = 0;
  if (qok[r]) {  // (block-uniform)
    const int sk = skip ? skip[r] : -1;
    want = min(k, N - ((uint32_t)sk < (uint32_t)N ? 1 : 0));
  }
  // chunks * k stays below 2^31: larger counts are refused by the entry
  if (want > 0) select_smallest(s, CandItem{cand + (int64_t)r * chunks * k}, chunks * k, want, (uint32_t)(N - 1));
  write_row(s, want, k, oi, od, dist_of_key);
}

// workspace: [keys Q*pitch][cand Q*chunks*k][qn Q*Kp][qok Q], pitch = the chunk, or N rounded up to
// 64 where that is less: it grows with Q * chunk and Q * k * chunks, never with Q * N
struct SearchWs : rowsel::ChunkPlan {
  size_t qn, qok, keys, cand, total;
  int Kp;
};
SearchWs search_ws(int N, int K, int Q, int k, int chunk) {
  SearchWs w{rowsel::chunk_plan(N, chunk)};
  const size_t q = (size_t)std::max(Q, 1);
  w.Kp = k_pad(K);
  size_t o = 0;
  w.keys = o, o += align256(q * w.pitch * sizeof(uint32_t));
  w.cand = o, o += align256(q * (size_t)w.chunks * (size_t)std::max(k, 1) * sizeof(uint64_t));
  w.qn = o, o += align256(q * w.Kp * sizeof(float));
  w.qok = o, o += align256(q * sizeof(int32_t));
  w.total = o;
  return w;
}

template <int RM>
void launch_dist(hipStream_t s, const float *qn, const int32_t *qok, const float *nT, int caps, int c0,
                 int cl, int Kp, int Q, int pitch, uint32_t *keys) {
  const dim3 grid((unsigned)cdiv(cl, TC), (unsigned)cdiv(Q, 16 * RM));
  hipLaunchKernelGGL(dist_chunk_kernel<RM>, grid, dim3(DNT), 0, s, qn, qok, nT, caps, c0, cl, Kp, Q, pitch,
                     keys);
}

}  // namespace

extern "C" size_t cc_cube_index_size(int32_t cap, int32_t K) { return index_layout(cap, K).total; }

extern "C" int cc_cube_index_put(void *index, int32_t cap, int32_t K, int32_t n0, int32_t rows,
                                 const float *z, void *stream) {
  CC_REQUIRE(index && z, "cc_cube_index_put: null pointer");
  CC_REQUIRE(((uintptr_t)index & 255) == 0, "cc_cube_index_put: index must be 256-byte aligned");
  CC_REQUIRE(cap >= 1 && cap <= 0x7FFFFFFF - 64 && K >= 1 && K <= 0x7FFFFFFF - dottile::KS,
             "cc_cube_index_put: bad cap/K");
  CC_REQUIRE(n0 >= 0 && rows >= 0 && (int64_t)n0 + rows <= cap,
             "cc_cube_index_put: rows [n0, n0 + rows) must lie inside [0, cap)");
  if (rows == 0) return CC_OK;
  const IndexLayout x = index_layout(cap, K);
  char *base = (char *)index;
  return cc::normalise_rows_launch(z, rows, K, x.Kp, x.caps, n0, (float *)(base + x.n),
                                   (float *)(base + x.nT), as_stream(stream));
}

extern "C" int32_t cc_cube_neighbours_max_k(void) { return MAX_K; }

extern "C" size_t cc_cube_neighbours_ws_size(int32_t N, int32_t K, int32_t Q, int32_t k, int32_t chunk) {
  return search_ws(N, K, Q, k, chunk).total + 256;
}

extern "C" int cc_cube_neighbours(const void *index, int32_t cap, int32_t N, int32_t K, int32_t Q,
                                  const int32_t *qid, const float *zq, const int32_t *skip, int32_t k,
                                  int32_t chunk, void *ws, int32_t *out_idx, float *out_dist,
                                  void *stream) {
  CC_REQUIRE(index && ws && out_idx && out_dist, "cc_cube_neighbours: null pointer");
  CC_REQUIRE(cap >= 1 && cap <= 0x7FFFFFFF - 64 && K >= 1 && K <= 0x7FFFFFFF - dottile::KS,
             "cc_cube_neighbours: bad cap/K");
  CC_REQUIRE(N >= 1 && N <= cap, "cc_cube_neighbours: N must be 1..cap");
  CC_REQUIRE(Q >= 0 && Q <= MAX_Q, "cc_cube_neighbours: Q outside 0..2^22");
  CC_REQUIRE(k >= 1 && k <= MAX_K, "cc_cube_neighbours: k must be 1..cc_cube_neighbours_max_k()");
  CC_REQUIRE(chunk == 0 || (chunk > 0 && chunk % 64 == 0),
             "cc_cube_neighbours: chunk must be 0 or a positive multiple of 64");
  CC_REQUIRE(((uintptr_t)ws & 255) == 0, "cc_cube_neighbours: ws must be 256-byte aligned");
  CC_REQUIRE(((uintptr_t)index & 255) == 0, "cc_cube_neighbours: index must be 256-byte aligned");
  const SearchWs w = search_ws(N, K, Q, k, chunk);
  CC_REQUIRE((int64_t)w.chunks * k <= 0x7FFFFFFF, "cc_cube_neighbours: k * chunks above 2^31 - 1, use a larger chunk");
  if (Q == 0) return CC_OK;
  const IndexLayout x = index_layout(cap, K);
  hipStream_t s = as_stream(stream);
  const float *n = (const float *)((const char *)index + x.n);
  const float *nT = (const float *)((const char *)index + x.nT);
  char *base = (char *)ws;
  float *qn = (float *)(base + w.qn);
  int32_t *qok = (int32_t *)(base + w.qok);
  uint32_t *keys = (uint32_t *)(base + w.keys);
  uint64_t *cand = (uint64_t *)(base + w.cand);
  hipLaunchKernelGGL(query_rows_kernel, dim3(Q), dim3(QNT), 0, s, n, N, K, x.Kp, qid, zq, qn, qok);
  CC_LAUNCH_CHECK("query_rows_kernel");
  const bool one_chunk = w.chunks == 1;  // its select writes the rows: no merge
  for (int c = 0; c < w.chunks; ++c) {
    const int c0 = (int)((int64_t)c * w.chunk), cl = std::min(w.chunk, N - c0);
    // queries per tile: 32 / 64 / 128 (the arithmetic per (query, cube) does not depend on it)
    if (Q <= 32)
      launch_dist<2>(s, qn, qok, nT, x.caps, c0, cl, x.Kp, Q, w.pitch, keys);
    else if (Q <= 64)
      launch_dist<4>(s, qn, qok, nT, x.caps, c0, cl, x.Kp, Q, w.pitch, keys);
    else
      launch_dist<8>(s, qn, qok, nT, x.caps, c0, cl, x.Kp, Q, w.pitch, keys);
    CC_LAUNCH_CHECK("dist_chunk_kernel");
    if (one_chunk)
      hipLaunchKernelGGL(select_chunk_kernel<true>, dim3(Q), dim3(SNT), 0, s, keys, w.pitch, c0, cl, qok, skip,
                         k, c, w.chunks, cand, out_idx, out_dist);
    else
      hipLaunchKernelGGL(select_chunk_kernel<false>, dim3(Q), dim3(SNT), 0, s, keys, w.pitch, c0, cl, qok, skip,
                         k, c, w.chunks, cand, out_idx, out_dist);
    CC_LAUNCH_CHECK("select_chunk_kernel");
  }
  if (!one_chunk) {
    hipLaunchKernelGGL(merge_rows_kernel, dim3(Q), dim3(SNT), 0, s, cand, w.chunks, N, qok, skip, k, out_idx,
                       out_dist);
    CC_LAUNCH_CHECK("merge_rows_kernel");
  }
  return CC_OK;
}
