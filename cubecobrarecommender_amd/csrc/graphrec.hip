// cc_graph_rec_f64 / cc_graph_rank_f64 / cc_graph_rec_target_ranks_f64 — the co-occurrence baseline (N5): the
// reference's simple_recs / simple_cuts (src/scripts/recommend.py, cut_cards.py) for R cubes per
// call on the f64 graph M that cc_adjacency leaves on the device.
//
// Pinned arithmetic, per cube S (sorted distinct ids) and card j:
//   score[j] = fold over i in S ascending of acc = acc + (i == j ? +0.0 : M[i][j]), acc from +0.0
// in f64, every add rounded, nothing reassociated.  For j outside S that is simple_recs' column
// sum, for j in S simple_cuts' (diagonal zeroed); M's own diagonal is never used as a value.
//
//   graph_score_kernel : a gather-sum of the cube's rows of M, memory-bound (n * V * 8 bytes per
//                     cube against a 3.9 GB M at V = 22,000).  One workgroup per (column tile,
//                     cube); a lane owns CPL adjacent columns and walks the cube's ids (staged in
//                     LDS, IDCH at a time) in ascending order with U rows in flight: the U loads
//                     are issued first, then added strictly in order.  The row id is wave-uniform
//                     (readfirstlane), so a row's base is scalar arithmetic.  CPL = 2 with one
//                     16-byte load per row where adj and ld allow it, two 8-byte loads otherwise;
//                     below WIDE_ROWS cubes CPL = 1 and U = 16: a single request has only V lanes
//                     of parallelism and the sum over i cannot be split, so it is latency-bound
//                     and takes the most lanes and the most loads in flight.  Workgroups are
//                     numbered through cc_xcd_run with the cube as the fast index: an XCD runs
//                     one column tile for a run of neighbouring cubes, which all walk ascending
//                     ids, so the row segments of the cards they share are hits in that XCD's L2.
//                     The walk meets i == j exactly when j is a cube card: that is the diagonal
//                     rule, the in-cube flag and the card's cut-value slot at once (no bitmask, no
//                     search).  Writes the sort key of every card, the cut values, and the scores
//                     on request.
//   key            : the f64 bits made monotone (negative: all bits flipped, else the sign bit
//                     set), -0.0 first folded onto +0.0; 0 for a cube card (no finite score maps
//                     to 0).  The ranking is descending (key, card): equal scores higher card
//                     index first, cube cards last.
//   graph_topn_kernel : recbatch.hip's topn_rows_kernel on the 96-bit (key, card): radix select of
//                     the want-th largest (10-bit digits from the top of the key, then of the
//                     card; stops once the chosen bin holds exactly the remaining count), then a
//                     bitonic sort of the at most MAX_AMOUNT survivors in LDS as (key, card) pairs.
//   graph_rank_kernel : cc_graph_rank_f64's ranking of every card: rowsort.hpp's radix_rank_row
//                     on the 64-bit key, a stable LSD radix sort of (key, card) in 7 passes
//                     (see the kernel).
//   graph_target_ranks_kernel : one workgroup per row, one wave per target at a time: the rank is
//                     a plain count of the cards whose (key, card) is above the target's over the
//                     row's keys (V * 8 bytes from L2 against the n * V * 8 the scoring pass read).
#include <limits.h>

#include <algorithm>

#include "common.hpp"
#include "rowsort.hpp"
#include "topn_tiles.hpp"

namespace {

constexpr int GNT = 256;          // scoring workgroup: a tile of GNT * CPL columns
constexpr int WIDE_U = 8;           // rows a lane keeps in flight when it owns two columns (A/B: DESIGN §4)
constexpr int IDCH = 1024;        // cube ids staged in LDS at a time
constexpr int WIDE_ROWS = 16;     // from this many cubes per call a lane owns two columns
constexpr int SNT = 1024;         // ranking / counting workgroup
constexpr int MAX_AMOUNT = 2048;  // survivors sorted in LDS
constexpr int MAX_CUTOFFS = 8;

__device__ __forceinline__ uint64_t key_of(double s, bool in_cube) {
  if (in_cube) return 0ull;
  uint64_t b = (uint64_t)__double_as_longlong(s);
  if ((b << 1) == 0ull) b = 0ull;  // -0.0 ranks as +0.0
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
__device__ __forceinline__ double score_of(uint64_t key) {
  const uint64_t b = (key >> 63) ? (key ^ (1ull << 63)) : ~key;
  return __longlong_as_double((long long)b);
}
__device__ __forceinline__ bool pair_gt(uint64_t ka, uint32_t ca, uint64_t kb, uint32_t cb) {
  return ka > kb || (ka == kb && ca > cb);
}

// U rows of the cube, ids[0 .. U) at cube position pos: all loads first, then the adds in order.
template <int CPL, bool VEC, int U>
__device__ __forceinline__ void score_rows(const double *__restrict__ col, int64_t ld,
                                           const int32_t *ids, int pos, int j0, int V,
                                           bool has1, double (&acc)[CPL], int (&cut)[CPL]) {
  int i[U];
  double v[U][CPL];
#pragma unroll
  for (int u = 0; u < U; ++u) i[u] = __builtin_amdgcn_readfirstlane(ids[u]);
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int c = 0; c < CPL; ++c) v[u][c] = 0.0;
    if ((uint32_t)i[u] >= (uint32_t)V) continue;  // (wave-uniform) never index with such an id
    const double *p = col + (int64_t)i[u] * ld;
    if (VEC && has1) {
      const double2 t = *reinterpret_cast<const double2 *>(p);
      v[u][0] = t.x;
      v[u][CPL - 1] = t.y;
    } else {
      v[u][0] = p[0];
      if (CPL > 1 && has1) v[u][CPL - 1] = p[CPL - 1];
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if ((uint32_t)i[u] >= (uint32_t)V) continue;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const bool diag = i[u] == j0 + c;
      acc[c] = acc[c] + (diag ? 0.0 : v[u][c]);
      if (diag) cut[c] = pos + u;
    }
  }
}

template <int CPL, bool VEC, int U>
__global__ __launch_bounds__(GNT) void graph_score_kernel(
    const double *__restrict__ adj, int64_t ld, int V, int R, const int32_t *__restrict__ row_ptr,
    const int32_t *__restrict__ idx, uint64_t *__restrict__ keys, int Vs,
    double *__restrict__ cut_vals, double *__restrict__ scores) {
  static_assert(CPL == 1 || CPL == 2, "a lane owns one column or two");
  static_assert(!VEC || CPL == 2, "the 16-byte load is two columns");
  __shared__ int32_t s_ids[IDCH];
  const int tid = threadIdx.x;
  // cube fastest: see the header
  const int l = cc_xcd_run((int)blockIdx.x, (int)gridDim.x);  // (A/B against blockIdx.x: DESIGN §4)
  const int tile = l / R, r = l - tile * R;
  const int beg = row_ptr[r], n = row_ptr[r + 1] - beg;
  const int j0 = (tile * GNT + tid) * CPL;
  const bool live = j0 < V, has1 = j0 + CPL - 1 < V;
  const double *col = adj + j0;  // dereferenced by live lanes only
  double acc[CPL];
  int cut[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) acc[c] = 0.0, cut[c] = -1;

  for (int c0 = 0; c0 < n; c0 += IDCH) {
    const int m = min(IDCH, n - c0);
    __syncthreads();  // the previous chunk's readers are done
    for (int k = tid; k < m; k += GNT) s_ids[k] = idx[beg + c0 + k];
    __syncthreads();
    if (!live) continue;
    int k = 0;
    for (; k + U <= m; k += U)
      score_rows<CPL, VEC, U>(col, ld, s_ids + k, c0 + k, j0, V, has1, acc, cut);
    for (; k < m; ++k) score_rows<CPL, VEC, 1>(col, ld, s_ids + k, c0 + k, j0, V, has1, acc, cut);
  }
  if (!live) return;
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const int j = j0 + c;
    if (j >= V) continue;
    const bool in_cube = cut[c] >= 0;
    keys[(int64_t)r * Vs + j] = key_of(acc[c], in_cube);
    if (scores) scores[(int64_t)r * V + j] = acc[c];
    if (in_cube) cut_vals[beg + cut[c]] = acc[c];
  }
}

// Compare-exchange of the pairs (k[i], c[i]) for rowsort::bitonic_sort: descending.
struct CmpSwapPairs {
  uint64_t *k;
  uint32_t *c;
  __device__ __forceinline__ void operator()(int i, int pr, bool down) const {
    const uint64_t kx = k[i], ky = k[pr];
    const uint32_t cx = c[i], cy = c[pr];
    if (pair_gt(ky, cy, kx, cx) == down) {
      k[i] = ky, c[i] = cy;
      k[pr] = kx, c[pr] = cx;
    }
  }
};

__global__ __launch_bounds__(SNT) void graph_topn_kernel(const uint64_t *__restrict__ keys, int Vs,
                                                         int V, const int32_t *__restrict__ row_ptr,
                                                         int amount, int A,
                                                         int32_t *__restrict__ n_add,
                                                         int32_t *__restrict__ additions,
                                                         double *__restrict__ add_vals) {
  __shared__ uint32_t hist[1024];
  __shared__ int wtot[SNT / 64];
  __shared__ uint64_t s_kpre, s_kmask;
  __shared__ uint32_t s_cpre, s_cmask;
  __shared__ int s_rem, s_done, s_cnt;
  __shared__ uint64_t selk[MAX_AMOUNT];
  __shared__ uint32_t selc[MAX_AMOUNT];
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  const int n = row_ptr[r + 1] - row_ptr[r];
  const int want = max(0, min(min(amount > 0 ? amount : 1, V - n), MAX_AMOUNT));
  int32_t *adds = additions + (int64_t)r * A;
  double *addv = add_vals + (int64_t)r * A;
  for (int i = want + tid; i < A; i += SNT) {  // the unused tail
    adds[i] = -1;
    addv[i] = 0.0;
  }
  if (tid == 0) n_add[r] = want;
  if (want == 0) return;
  const uint64_t *k = keys + (int64_t)r * Vs;
  if (tid == 0) {
    s_kpre = 0, s_kmask = 0;
    s_cpre = 0, s_cmask = 0;
    s_rem = want;
    s_done = 0;
    s_cnt = 0;
  }
  __syncthreads();
  // digits from the top: the key's 64 bits in passes 0..6 (6 x 10 + 4), the card's in 7..10
  for (int pass = 0; pass < 11; ++pass) {
    const bool on_key = pass < 7;
    int shift;
    uint32_t dmask;
    if (on_key) {
      shift = pass < 6 ? 54 - 10 * pass : 0;
      dmask = pass < 6 ? 1023u : 15u;
    } else {
      shift = 30 - 10 * (pass - 7);
      dmask = pass == 7 ? 3u : 1023u;
      if (((uint32_t)(V - 1) >> shift) == 0u) continue;  // no card has a bit up here
    }
    if (s_done) break;
    const uint64_t kpre = s_kpre, kmask = s_kmask;
    const uint32_t cpre = s_cpre, cmask = s_cmask;
    const int rem = s_rem;
    hist[tid] = 0u;
    __syncthreads();
    for (int j = tid; j < V; j += SNT) {
      const uint64_t key = k[j];
      if ((key & kmask) == kpre && ((uint32_t)j & cmask) == cpre)
        atomicAdd(&hist[on_key ? (uint32_t)(key >> shift) & dmask : ((uint32_t)j >> shift) & dmask], 1u);
    }
    __syncthreads();
    // thread t owns bin 1023 - t: its inclusive scan is the count of matching items in bins >= it
    const int v = (int)hist[1023 - tid];
    const int ge = rowsort::block_incl_scan<SNT>(v, wtot), gt = ge - v;
    if (ge >= rem && gt < rem) {  // exactly one bin: the one holding the rem-th largest
      if (on_key) {
        s_kpre = kpre | ((uint64_t)(1023 - tid) << shift);
        s_kmask = kmask | ((uint64_t)dmask << shift);
      } else {
        s_cpre = cpre | ((uint32_t)(1023 - tid) << shift);
        s_cmask = cmask | (dmask << shift);
      }
      s_rem = rem - gt;
      s_done = v == rem - gt;  // the whole bin is wanted: every pair >= the prefix is in
    }
    __syncthreads();
  }
  const uint64_t Tk = s_kpre;
  const uint32_t Tc = s_cpre;
  for (int j = tid; j < V; j += SNT) {
    const uint64_t key = k[j];
    if (key > Tk || (key == Tk && (uint32_t)j >= Tc)) {
      const int pos = atomicAdd(&s_cnt, 1);
      if (pos < MAX_AMOUNT) selk[pos] = key, selc[pos] = (uint32_t)j;
    }
  }
  __syncthreads();
  int P = 1;
  while (P < want) P <<= 1;
  for (int i = min(s_cnt, want) + tid; i < P; i += SNT) selk[i] = 0ull, selc[i] = 0u;  // below every candidate
  __syncthreads();
  rowsort::bitonic_sort<SNT>(P, CmpSwapPairs{selk, selc});
  for (int i = tid; i < want; i += SNT) {
    adds[i] = (int32_t)selc[i];
    addv[i] = score_of(selk[i]);
  }
}

__global__ __launch_bounds__(SNT) void graph_target_ranks_kernel(
    const uint64_t *__restrict__ keys, int Vs, int V, const int32_t *__restrict__ tgt_ptr,
    const int32_t *__restrict__ tgt, const int32_t *__restrict__ cutoffs, int n_cut,
    int32_t *__restrict__ ranks, double *__restrict__ tgt_vals,
    unsigned long long *__restrict__ hits) {
  __shared__ uint32_t s_hit[MAX_CUTOFFS + 1];
  __shared__ int s_best;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = blockIdx.x;
  const int tbeg = tgt_ptr[r], T = tgt_ptr[r + 1] - tbeg;
  if (T <= 0) return;  // (block-uniform) nothing to rank, nothing to count
  if (tid <= MAX_CUTOFFS) s_hit[tid] = 0u;
  if (tid == 0) s_best = INT_MAX;
  __syncthreads();
  const uint64_t *k = keys + (int64_t)r * Vs;
  for (int ti = w; ti < T; ti += SNT / 64) {  // (wave-uniform) one target per wave at a time
    const int t = tgt[tbeg + ti];
    uint64_t kt = 0ull;
    if ((uint32_t)t < (uint32_t)V) kt = k[t];  // never index with an id outside the row
    int rank = -1;
    double val = 0.0;
    if (kt) {  // a candidate: inside [0, V) and outside the cube
      int cnt = 0;
      for (int j = 2 * lane; j < V; j += 128) {  // Vs is even: the pair is inside the row's pitch
        const ulonglong2 kk = *reinterpret_cast<const ulonglong2 *>(k + j);
        cnt += pair_gt(kk.x, (uint32_t)j, kt, (uint32_t)t) ? 1 : 0;
        cnt += (j + 1 < V && pair_gt(kk.y, (uint32_t)j + 1u, kt, (uint32_t)t)) ? 1 : 0;
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
      rank = cnt;
      val = score_of(kt);
      if (hits && lane == 0) {
        for (int c = 0; c < n_cut; ++c)
          if (rank < cutoffs[c]) atomicAdd(&s_hit[c], 1u);
        atomicAdd(&s_hit[MAX_CUTOFFS], 1u);
        atomicMin(&s_best, rank);
      }
    }
    if (lane == 0) {
      ranks[tbeg + ti] = rank;
      tgt_vals[tbeg + ti] = val;
    }
  }
  if (!hits) return;
  __syncthreads();
  if (tid < n_cut && s_hit[tid]) atomicAdd(hits + tid, (unsigned long long)s_hit[tid]);
  if (tid == n_cut && s_hit[MAX_CUTOFFS]) {
    atomicAdd(hits + n_cut, (unsigned long long)s_hit[MAX_CUTOFFS]);  // targets counted
    if (n_cut > 0 && s_best < cutoffs[0]) atomicAdd(hits + n_cut + 1, 1ull);  // the row's best is a hit
  }
}

// Full ranking of one row: rowsort::radix_rank_row on the graph's 64-bit key.  A stable LSD radix
// sort of ascending (key, card) from ascending card order, RANK_PASSES passes of tiles::BITS bits
// (6 x 10, then the top 4), one workgroup per row.  Pass 0 reads the row's keys (the card is the
// index); later passes ping-pong the key and the card through two parallel arrays each (ka / ca,
// kb / cb).  The last pass stores nothing but the row's results: ascending position pos is
// descending position V - 1 - pos, and the cube cards (key 0, below every finite score's key) hold
// the first n ascending positions, i.e. the last n descending ones, which want <= V - n never
// reaches.
constexpr int RANK_PASSES = 7;
constexpr int RANK_U = 8;  // items a lane loads ahead of ranking them

struct GraphRankRow {
  struct Item {
    uint64_t key;
    uint32_t card;
  };
  static constexpr int PASSES = RANK_PASSES, RADIX_BITS = tiles::BITS;
  static __device__ constexpr int bits(int pass) {
    return pass == RANK_PASSES - 1 ? 64 - tiles::BITS * (RANK_PASSES - 1) : tiles::BITS;
  }
  const uint64_t *k;
  uint64_t *ka, *kb;
  uint32_t *ca, *cb;
  int32_t *adds;
  double *addv;  // may be null
  int V, want;
  __device__ __forceinline__ Item load(int pass, int i) const {
    if (pass == 0) return {k[i], (uint32_t)i};  // the card is the index
    return {((pass & 1) ? ka : kb)[i], ((pass & 1) ? ca : cb)[i]};
  }
  __device__ __forceinline__ uint32_t digit(const Item &x, int pass) const {
    return (uint32_t)(x.key >> (tiles::BITS * pass)) & (uint32_t)(tiles::R - 1);
  }
  __device__ __forceinline__ void store(int pass, uint32_t pos, const Item &x) const {
    ((pass & 1) ? kb : ka)[pos] = x.key;
    ((pass & 1) ? cb : ca)[pos] = x.card;
  }
  __device__ __forceinline__ void emit(uint32_t pos, const Item &x) const {
    const int q = V - 1 - (int)pos;  // descending position
    if (q < want) {
      adds[q] = (int32_t)x.card;
      if (addv) addv[q] = score_of(x.key);
    }
  }
};

__global__ __launch_bounds__(SNT) void graph_rank_kernel(
    const uint64_t *__restrict__ keys, int Vs, int V, const int32_t *__restrict__ row_ptr,
    int amount, int A, uint64_t *ka, uint64_t *kb, uint32_t *ca, uint32_t *cb, int Vp,
    int32_t *__restrict__ n_add, int32_t *__restrict__ additions, double *__restrict__ add_vals) {
  __shared__ uint32_t hist[SNT / 64 * tiles::R];
  __shared__ int wtot[SNT / 64];
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  const int n = row_ptr[r + 1] - row_ptr[r];
  const int want = max(0, min(amount > 0 ? amount : 1, V - n));
  int32_t *adds = additions + (int64_t)r * A;
  double *addv = add_vals ? add_vals + (int64_t)r * A : nullptr;
  for (int i = want + tid; i < A; i += SNT) {  // the unused tail
    adds[i] = -1;
    if (addv) addv[i] = 0.0;
  }
  if (tid == 0) n_add[r] = want;
  if (want == 0) return;
  const int64_t o = (int64_t)r * Vp;
  const GraphRankRow t{keys + (int64_t)r * Vs, ka + o, kb + o, ca + o, cb + o, adds, addv, V, want};
  rowsort::radix_rank_row<SNT, RANK_U>(t, V, hist, wtot);
}

// workspace: the rows' sort keys [R][Vs]; Vs a multiple of 16, so rows start on a 128-byte line
int key_pitch(int V) { return (std::max(V, 1) + 15) & ~15; }

// the ranking entry's workspace: the keys as above, then the sort's ping-pong arrays, keys
// [R][Vp] x 2 and cards [R][Vp] x 2; Vp a multiple of 32, so no two rows share a 128-byte line
// of either
int rank_pitch(int V) { return (std::max(V, 1) + 31) & ~31; }
struct RankWs {
  uint64_t *keys, *ka, *kb;
  uint32_t *ca, *cb;
  size_t bytes;
};
RankWs rank_ws_of(void *base, int V, int R) {
  const size_t rows = (size_t)std::max(R, 1);
  const size_t nk = align256(rows * key_pitch(V) * sizeof(uint64_t));
  const size_t np8 = align256(rows * rank_pitch(V) * sizeof(uint64_t));
  const size_t np4 = align256(rows * rank_pitch(V) * sizeof(uint32_t));
  char *p = (char *)base;
  RankWs w;
  w.keys = (uint64_t *)p;
  w.ka = (uint64_t *)(p + nk);
  w.kb = (uint64_t *)(p + nk + np8);
  w.ca = (uint32_t *)(p + nk + 2 * np8);
  w.cb = (uint32_t *)(p + nk + 2 * np8 + np4);
  w.bytes = nk + 2 * np8 + 2 * np4 + 256;
  return w;
}

template <int CPL, bool VEC, int U>
void launch_score(int64_t blocks, hipStream_t s, const double *adj, int64_t ld, int V, int R,
                  const int32_t *row_ptr, const int32_t *idx, uint64_t *keys, int Vs,
                  double *cut_vals, double *scores) {
  hipLaunchKernelGGL((graph_score_kernel<CPL, VEC, U>), dim3((unsigned)blocks), dim3(GNT), 0, s, adj,
                     ld, V, R, row_ptr, idx, keys, Vs, cut_vals, scores);
}

// The checks both entries share, then the scoring launch: every row's keys in the workspace, its
// cut values and (on request) its scores.
int graph_keys_launch(const char *who, const double *adj, int64_t ld, int V, int R,
                      const int32_t *row_ptr, const int32_t *idx, int max_n, void *ws,
                      double *cut_vals, double *scores, hipStream_t s) {
  const std::string w(who);
  CC_REQUIRE(V > 0 && R >= 0 && max_n >= 0 && max_n <= V, w + ": V/R/max_n");
  CC_REQUIRE(ld >= V, w + ": ld below V");
  CC_REQUIRE(((uintptr_t)adj & 7) == 0, w + ": adj must be 8-byte aligned");
  CC_REQUIRE(((uintptr_t)ws & 255) == 0, w + ": ws must be 256-byte aligned");
  const bool wide = R >= WIDE_ROWS;
  const int64_t blocks = cdiv(V, GNT * (wide ? 2 : 1)) * (int64_t)R;
  CC_REQUIRE(blocks <= INT_MAX, w + ": R too large for one launch");
  if (R == 0) return CC_OK;
  uint64_t *keys = (uint64_t *)ws;
  const int Vs = key_pitch(V);
  if (!wide)
    launch_score<1, false, 16>(blocks, s, adj, ld, V, R, row_ptr, idx, keys, Vs, cut_vals, scores);
  else if (((uintptr_t)adj & 15) == 0 && (ld & 1) == 0)
    launch_score<2, true, WIDE_U>(blocks, s, adj, ld, V, R, row_ptr, idx, keys, Vs, cut_vals, scores);
  else
    launch_score<2, false, WIDE_U>(blocks, s, adj, ld, V, R, row_ptr, idx, keys, Vs, cut_vals, scores);
  CC_LAUNCH_CHECK("graph_score_kernel");
  return CC_OK;
}

}  // namespace

extern "C" int32_t cc_graph_rec_max_amount(void) { return MAX_AMOUNT; }

extern "C" size_t cc_graph_rec_ws_size(int32_t V, int32_t R, int32_t max_n) {
  (void)max_n;  // the cubes' ids are staged in LDS: nothing in the workspace scales with them
  return align256((size_t)std::max(R, 1) * key_pitch(V) * sizeof(uint64_t)) + 256;
}

extern "C" int cc_graph_rec_f64(const double *adj, int64_t ld, int32_t V, int32_t R,
                                const int32_t *row_ptr, const int32_t *idx, int32_t max_n,
                                int32_t amount, void *ws, int32_t *n_add, int32_t *additions,
                                double *add_vals, double *cut_vals, double *scores, void *stream) {
  CC_REQUIRE(adj && row_ptr && idx && ws && n_add && additions && add_vals && cut_vals,
             "cc_graph_rec_f64: null pointer");
  CC_REQUIRE(amount <= MAX_AMOUNT, "cc_graph_rec_f64: amount above cc_graph_rec_max_amount()");
  hipStream_t s = as_stream(stream);
  if (int rc = graph_keys_launch("cc_graph_rec_f64", adj, ld, V, R, row_ptr, idx, max_n, ws,
                                 cut_vals, scores, s))
    return rc;
  if (R == 0) return CC_OK;
  const int A = amount > 0 ? amount : 1;
  hipLaunchKernelGGL(graph_topn_kernel, dim3(R), dim3(SNT), 0, s, (const uint64_t *)ws,
                     key_pitch(V), V, row_ptr, amount, A, n_add, additions, add_vals);
  CC_LAUNCH_CHECK("graph_topn_kernel");
  return CC_OK;
}

extern "C" size_t cc_graph_rank_ws_size(int32_t V, int32_t R, int32_t max_n) {
  (void)max_n;
  return rank_ws_of(nullptr, V, R).bytes;
}

extern "C" int cc_graph_rank_f64(const double *adj, int64_t ld, int32_t V, int32_t R,
                                 const int32_t *row_ptr, const int32_t *idx, int32_t max_n,
                                 int32_t amount, void *ws, int32_t *n_add, int32_t *additions,
                                 double *add_vals, double *cut_vals, double *scores, void *stream) {
  CC_REQUIRE(adj && row_ptr && idx && ws && n_add && additions && cut_vals,
             "cc_graph_rank_f64: null pointer");
  hipStream_t s = as_stream(stream);
  if (int rc = graph_keys_launch("cc_graph_rank_f64", adj, ld, V, R, row_ptr, idx, max_n, ws,
                                 cut_vals, scores, s))
    return rc;
  if (R == 0) return CC_OK;
  const int A = std::min(amount > 0 ? amount : 1, V);
  const RankWs w = rank_ws_of(ws, V, R);
  hipLaunchKernelGGL(graph_rank_kernel, dim3(R), dim3(SNT), 0, s, (const uint64_t *)w.keys,
                     key_pitch(V), V, row_ptr, amount, A, w.ka, w.kb, w.ca, w.cb, rank_pitch(V),
                     n_add, additions, add_vals);
  CC_LAUNCH_CHECK("graph_rank_kernel");
  return CC_OK;
}

extern "C" int cc_graph_rec_target_ranks_f64(
    const double *adj, int64_t ld, int32_t V, int32_t R, const int32_t *row_ptr, const int32_t *idx,
    int32_t max_n, const int32_t *tgt_ptr, const int32_t *tgt, const int32_t *cutoffs,
    int32_t n_cutoffs, void *ws, int32_t *ranks, double *tgt_vals, unsigned long long *hits,
    double *cut_vals, double *scores, void *stream) {
  CC_REQUIRE(adj && row_ptr && idx && tgt_ptr && tgt && ws && ranks && tgt_vals && cut_vals,
             "cc_graph_rec_target_ranks_f64: null pointer");
  CC_REQUIRE(n_cutoffs >= 0 && n_cutoffs <= MAX_CUTOFFS && (n_cutoffs == 0 || cutoffs),
             "cc_graph_rec_target_ranks_f64: n_cutoffs outside 0..8, or cutoffs null");
  hipStream_t s = as_stream(stream);
  if (int rc = graph_keys_launch("cc_graph_rec_target_ranks_f64", adj, ld, V, R, row_ptr, idx,
                                 max_n, ws, cut_vals, scores, s))
    return rc;
  if (R == 0) return CC_OK;
  hipLaunchKernelGGL(graph_target_ranks_kernel, dim3(R), dim3(SNT), 0, s, (const uint64_t *)ws,
                     key_pitch(V), V, tgt_ptr, tgt, cutoffs, n_cutoffs, ranks, tgt_vals, hits);
  CC_LAUNCH_CHECK("graph_target_ranks_kernel");
  return CC_OK;
}
