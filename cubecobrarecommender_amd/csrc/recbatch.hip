// cc_recommend_batch_fp32 — R cubes per call, every row bit-identical to cc_recommend_fp32 on it.
//
// The single-cube output layer (infer.hip: out_kernel) streams the whole of Wo once per row; a
// batch shares it.  E1 and the towers reuse gather_partials_kernel + tower_kernel (mode 2, one
// workgroup per row) for h3 [R, d]; the rest is here:
//   row_bits_kernel : one workgroup per row clears the row's cube bitmask and sets it from the
//                     row's ids (nothing in the workspace survives from an earlier call).
//   out_tile_kernel : one workgroup per tile of 16*RM rows x 64 cards: the dot-product tile of
//                     DESIGN.md 4.10 in out_kernel's pinned 64-wide chunks (its own copy of
//                     dottile.hpp's loop: see there), so any d fits, then + bo[n], det_sigmoid32.  Writes the sort key of every card,
//                     the probability of every cube card into its cut-value slot (binary search
//                     of the row's sorted ids), and the probabilities only on request.
//   topn_rows_kernel: one workgroup per row.  The composite (key' << 32 | card) is unique, so
//                     the want largest are a radix SELECT of the want-th largest composite (10-bit
//                     digits from the top, LDS histograms, suffix scan; stops as soon as the
//                     chosen bin holds exactly the remaining count) and a bitonic sort of the
//                     survivors in LDS — descending composite = descending probability, equal
//                     probabilities higher card index first; cube cards (key' = 0) never make it
//                     because want <= V - n.
// cc_recommend_batch_rank_fp32 runs the same chain for any amount, with the select replaced by
//   rank_rows_kernel: one workgroup per row sorts all V (key', card) pairs (rowsort.hpp's stable
//                     LSD radix sort, three 10-bit passes through two ping-pong buffers in the
//                     workspace)
//                     and writes the first want entries of the descending order.
// cc_recommend_batch_target_ranks_fp32 runs the same chain and then, instead of ranking the row,
//   target_ranks_kernel: one workgroup per row counts, for each of the row's chosen target cards,
//                     the candidates ranked before it (held-out evaluation; see the kernel).
// The *_pool_* entries run the same three chains with a second reason for key' = 0: a row may name
// a card pool (a bit row of allowed cards), and its candidates are the pool's cards outside the cube.
//   row_mask_kernel : replaces row_bits_kernel: the row's cube bit row, its exclusion bit row
//                     (cube | ~pool) and n_cand[r], the cards with the exclusion bit clear.
//   out_tile_kernel<RM, true> takes the key from the exclusion word and the cut-value search from
//                     the cube word; topn_rows_kernel<true> / rank_rows_kernel<true> take want from
//                     n_cand[r] instead of V - n; target_ranks_kernel is fed the pooled keys.
// cc::batch_select_launch is the select chain (keys + topn_rows_kernel, pooled or not) as
// complete.hip runs it pass after pass; the two select entries run its pieces behind their checks.
// Host half: six entries = a null-pointer check + batch_front (every other check, the keys) + one
// of three back halves (select_launch, rank_launch, the target_ranks_kernel launch).
#include "common.hpp"
#include "detmath.hpp"
#include "dottile.hpp"
#include "infer.hpp"
#include "rowsort.hpp"
#include "topn_tiles.hpp"

namespace {

constexpr int KCH = dottile::KCH, KS = dottile::KS;  // the tile's constants (dottile.hpp)
constexpr int TC = dottile::TC;   // cards per output tile
constexpr int ONT = dottile::NT;  // output-tile workgroup
constexpr int SNT = 1024;    // top-N workgroup
constexpr int MAX_AMOUNT = 2048;  // survivors sorted in LDS

using detm::addf;
using detm::mulf;

// (also evalloss.hip's target masks, through cc::row_bits_launch: ids outside [0, V) are ignored)
__global__ __launch_bounds__(256) void row_bits_kernel(const int32_t *__restrict__ row_ptr,
                                                       const int32_t *__restrict__ idx, int V,
                                                       int VW, uint32_t *__restrict__ bits) {
  const int r = blockIdx.x;
  uint32_t *b = bits + (int64_t)r * VW;
  for (int i = threadIdx.x; i < VW; i += 256) b[i] = 0u;
  __syncthreads();
  const int beg = row_ptr[r], end = row_ptr[r + 1];
  for (int i = beg + (int)threadIdx.x; i < end; i += 256) {
    const int j = idx[i];
    if ((uint32_t)j < (uint32_t)V) atomicOr(&b[j >> 5], 1u << (j & 31));
  }
}

// The pooled chain's row masks.  pools: [n_pools][VW] bit rows of allowed cards; pool_of_row[r] = -1:
// the row has no pool (every card allowed); any other value outside [0, n_pools) is never used as
// an index and allows nothing.  Bits at or above V of a pool row are ignored: the last word's count
// is masked to its V & 31 valid bits (the exclusion bits up there are never read as a card's).
// n_cand[r] = allowed cards - the cube cards among them: a cube card's atomicOr on the exclusion
// row returns the word as it was, so exactly one thread sees its bit go from clear to set.
// Integer sums: any reduction order gives the same count.  0 <= n_cand[r] <= V - n.
__global__ __launch_bounds__(256) void row_mask_kernel(const int32_t *__restrict__ row_ptr,
                                                       const int32_t *__restrict__ idx, int V,
                                                       int VW, const uint32_t *__restrict__ pools,
                                                       int n_pools,
                                                       const int32_t *__restrict__ pool_of_row,
                                                       uint32_t *__restrict__ bits,
                                                       uint32_t *__restrict__ excl,
                                                       int32_t *__restrict__ n_cand) {
  __shared__ int wsum[256 / 64];
  const int r = blockIdx.x;
  uint32_t *b = bits + (int64_t)r * VW;
  uint32_t *x = excl + (int64_t)r * VW;
  const int p = pool_of_row[r];
  const bool has_pool = (uint32_t)p < (uint32_t)n_pools;  // (block-uniform)
  const uint32_t *pw = has_pool ? pools + (int64_t)p * VW : nullptr;
  int cnt = 0;
  for (int i = threadIdx.x; i < VW; i += 256) {
    uint32_t allowed = has_pool ? pw[i] : (p == -1 ? ~0u : 0u);
    if (i == VW - 1 && (V & 31)) allowed &= (1u << (V & 31)) - 1u;
    b[i] = 0u;
    x[i] = ~allowed;
    cnt += __popc(allowed);
  }
  __syncthreads();
  const int beg = row_ptr[r], end = row_ptr[r + 1];
  for (int i = beg + (int)threadIdx.x; i < end; i += 256) {
    const int j = idx[i];
    if ((uint32_t)j < (uint32_t)V) {
      const uint32_t bit = 1u << (j & 31);
      atomicOr(&b[j >> 5], bit);
      if (!(atomicOr(&x[j >> 5], bit) & bit)) --cnt;  // an allowed card that the cube takes
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) n_cand[r] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// POOL: the key comes from the row's exclusion word (excl: cube | ~pool), the cut-value slot search
// stays driven by the cube word, so a card that is merely outside the pool never enters the binary
// search.  Without POOL excl is not read.
template <int RM, bool POOL>
__global__ __launch_bounds__(ONT) void out_tile_kernel(
    const float *__restrict__ h3, const float *__restrict__ Wo, const float *__restrict__ bo, int d,
    int V, int R, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ idx,
    const uint32_t *__restrict__ bits, int VW, uint32_t *__restrict__ keys, int Vs,
    float *__restrict__ cut_vals, float *__restrict__ probs, const uint32_t *__restrict__ excl) {
  constexpr int TR = 16 * RM;
  // dottile::run<RM, true>'s loop, statement for statement but for the order of the two LDS reads
  // (DESIGN.md 4.10).  LDS stage: KS of a chunk's 64 k at a time (the chunk accumulator runs across its stages), so
  // that four workgroups fit a CU
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

  const int n0 = nb + 4 * tx;
  if (n0 >= V) return;
  float bias[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) bias[e] = n0 + e < V ? bo[n0 + e] : 0.f;
#pragma unroll
  for (int j = 0; j < RM; ++j) {
    const int gr = rb + ty * RM + j;
    if (gr >= R) continue;
    const uint32_t word = bits[(int64_t)gr * VW + (n0 >> 5)];  // n0 % 4 == 0: one word for all 4
    const uint32_t xword = POOL ? excl[(int64_t)gr * VW + (n0 >> 5)] : word;
    uint32_t key[4];
    float p[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      p[e] = detm::det_sigmoid32(addf(tot[j][e], bias[e]));
      key[e] = tiles::key_of(p[e], (xword >> ((n0 + e) & 31)) & 1u);
    }
    uint32_t *kr = keys + (int64_t)gr * Vs + n0;  // Vs % 4 == 0: 16-B aligned, the pad is ours
    *reinterpret_cast<uint4 *>(kr) = make_uint4(key[0], key[1], key[2], key[3]);
    if (probs) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n0 + e < V) probs[(int64_t)gr * V + n0 + e] = p[e];
    }
    if ((word >> (n0 & 31)) & 0xFu) {  // a cube card among the 4: its cut-value slot
      const int beg = row_ptr[gr], end = row_ptr[gr + 1];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (!((word >> ((n0 + e) & 31)) & 1u) || n0 + e >= V) continue;
        int lo = beg, hi = end;  // first position with idx >= card
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (idx[mid] < n0 + e) lo = mid + 1; else hi = mid;
        }
        if (lo < end && idx[lo] == n0 + e) cut_vals[lo] = p[e];
      }
    }
  }
}

// POOL: the row's candidates are the n_cand[r] cards whose exclusion bit is clear (row_mask_kernel),
// and every other card has key' = 0: want <= n_cand[r], so the want-th largest composite is a
// candidate's, the select's threshold has key' != 0 and no excluded card passes it.
template <bool POOL>
__global__ __launch_bounds__(SNT) void topn_rows_kernel(const uint32_t *__restrict__ keys, int Vs,
                                                        int V, const int32_t *__restrict__ row_ptr,
                                                        int amount, int A,
                                                        int32_t *__restrict__ n_add,
                                                        int32_t *__restrict__ additions,
                                                        float *__restrict__ add_vals,
                                                        const int32_t *__restrict__ n_cand) {
  __shared__ uint32_t hist[1024];
  __shared__ int wtot[SNT / 64];
  __shared__ uint64_t s_prefix, s_mask;
  __shared__ int s_rem, s_done, s_cnt;
  __shared__ uint64_t sel[MAX_AMOUNT];
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  const int cand = POOL ? n_cand[r] : V - (row_ptr[r + 1] - row_ptr[r]);
  const int want = max(0, min(min(amount > 0 ? amount : 1, cand), MAX_AMOUNT));
  int32_t *adds = additions + (int64_t)r * A;
  float *addv = add_vals + (int64_t)r * A;
  for (int i = want + tid; i < A; i += SNT) {  // the unused tail
    adds[i] = -1;
    addv[i] = 0.f;
  }
  if (tid == 0) n_add[r] = want;
  if (want == 0) return;
  const uint32_t *k = keys + (int64_t)r * Vs;
  if (tid == 0) {
    s_prefix = 0;
    s_mask = 0;
    s_rem = want;
    s_done = 0;
    s_cnt = 0;
  }
  __syncthreads();
  // composite bits: key' in 32..61 (key' < 2^30), card in 0..31; digits from the top
  for (int pass = 0; pass < 7; ++pass) {
    const int shift = pass < 6 ? 52 - 10 * pass : 0;
    const uint32_t dmask = pass < 6 ? 1023u : 3u;
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
    // thread t owns bin 1023 - t: its inclusive scan is the count of matching items in bins >= it
    const int v = (int)hist[1023 - tid];
    const int ge = rowsort::block_incl_scan<SNT>(v, wtot), gt = ge - v;
    if (ge >= rem && gt < rem) {  // exactly one bin: the one holding the rem-th largest
      s_prefix = prefix | ((uint64_t)(1023 - tid) << shift);
      s_mask = mask | ((uint64_t)dmask << shift);
      s_rem = rem - gt;
      s_done = v == rem - gt;  // the whole bin is wanted: every composite >= the prefix is in
    }
    __syncthreads();
  }
  const uint64_t T = s_prefix;
  for (int j = tid; j < V; j += SNT) {
    const uint64_t cmp = ((uint64_t)k[j] << 32) | (uint32_t)j;
    if (cmp >= T) {
      const int pos = atomicAdd(&s_cnt, 1);
      if (pos < MAX_AMOUNT) sel[pos] = cmp;
    }
  }
  __syncthreads();
  int P = 1;
  while (P < want) P <<= 1;
  for (int i = min(s_cnt, want) + tid; i < P; i += SNT) sel[i] = 0ull;  // below every candidate
  __syncthreads();
  rowsort::bitonic_sort<SNT>(P, rowsort::CmpSwapU64<true>{sel});
  for (int i = tid; i < want; i += SNT) {
    const uint64_t cmp = sel[i];
    adds[i] = (int32_t)(uint32_t)cmp;
    addv[i] = __uint_as_float((uint32_t)(cmp >> 32) - 1u);
  }
}

// Full ranking of one row: rowsort::radix_rank_row over ascending key' from ascending card order,
// tiles::PASSES passes of tiles::BITS bits, one workgroup per row.  (key', card) pairs ping-pong
// through pa / pb as one 64-bit word; the last pass stores nothing but the row's results:
// ascending position pos is descending position V - 1 - pos, and the cube cards (key' = 0) hold
// the first n ascending positions, i.e. the last n descending ones, which want <= V - n never
// reaches.  POOL: the excluded cards (cube or outside the pool, key' = 0) hold the first
// V - n_cand[r] ascending positions, the last V - n_cand[r] descending ones, which
// want <= n_cand[r] never reaches.
constexpr int RU = 8;  // items a lane loads ahead of ranking them: the loads' latency is paid once

struct RankRow {
  using Item = uint64_t;  // key' << 32 | card
  static constexpr int PASSES = tiles::PASSES, RADIX_BITS = tiles::BITS;
  static __device__ constexpr int bits(int) { return tiles::BITS; }
  const uint32_t *k;
  uint64_t *bufa, *bufb;
  int32_t *adds;
  float *addv;
  int V, want;
  __device__ __forceinline__ Item load(int pass, int i) const {  // pass 0 reads the keys
    return pass == 0 ? ((uint64_t)k[i] << 32) | (uint32_t)i : ((pass & 1) ? bufa : bufb)[i];
  }
  __device__ __forceinline__ uint32_t digit(Item x, int pass) const {
    return tiles::digit((uint32_t)(x >> 32), pass);
  }
  __device__ __forceinline__ void store(int pass, uint32_t pos, Item x) const {
    ((pass & 1) ? bufb : bufa)[pos] = x;
  }
  __device__ __forceinline__ void emit(uint32_t pos, Item x) const {
    const int q = V - 1 - (int)pos;  // descending position
    if (q < want) {
      adds[q] = (int32_t)(uint32_t)x;
      addv[q] = __uint_as_float((uint32_t)(x >> 32) - 1u);
    }
  }
};

template <bool POOL>
__global__ __launch_bounds__(SNT) void rank_rows_kernel(const uint32_t *__restrict__ keys, int Vs,
                                                        int V, const int32_t *__restrict__ row_ptr,
                                                        int amount, int A, uint64_t *pa,
                                                        uint64_t *pb, int Vp,
                                                        int32_t *__restrict__ n_add,
                                                        int32_t *__restrict__ additions,
                                                        float *__restrict__ add_vals,
                                                        const int32_t *__restrict__ n_cand) {
  __shared__ uint32_t hist[SNT / 64 * tiles::R];
  __shared__ int wtot[SNT / 64];
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  const int cand = POOL ? n_cand[r] : V - (row_ptr[r + 1] - row_ptr[r]);
  const int want = max(0, min(amount > 0 ? amount : 1, cand));
  int32_t *adds = additions + (int64_t)r * A;
  float *addv = add_vals + (int64_t)r * A;
  for (int i = want + tid; i < A; i += SNT) {  // the unused tail
    adds[i] = -1;
    addv[i] = 0.f;
  }
  if (tid == 0) n_add[r] = want;
  if (want == 0) return;
  const RankRow t{keys + (int64_t)r * Vs, pa + (int64_t)r * Vp, pb + (int64_t)r * Vp, adds, addv, V, want};
  rowsort::radix_rank_row<SNT, RU>(t, V, hist, wtot);
}

// Position of chosen cards in a row's ranking without sorting the row: the rank of target t is the
// number of candidates (key' != 0) whose composite (key' << 32 | card) is above t's.  One workgroup
// per row; up to TCH of the row's targets at a time:
//   stage : the targets' composites into LDS (0 for a target outside [0, V) or inside the cube:
//           below every candidate, so it sorts behind the Tv valid ones), bitonic sort, descending.
//   count : the row's keys are streamed once with 16-byte loads.  A candidate x at or below the
//           smallest target composite beats no target and is dropped after one comparison (with a
//           useful model that is nearly every card).  Otherwise g = #{targets >= x} (binary
//           search) and x is above exactly the sorted targets p >= g: cnt[g] += 1, the lanes of a
//           wave that share g adding once between them (ballot match on the bits of g) — with few
//           targets most of a wave lands on one counter.
//   scan  : the rank of sorted target p is the inclusive prefix sum of cnt over g <= p.
//   write : every target looks its composite up in the sorted chunk (duplicates find the same
//           first position) and takes that rank; results go to the target's own slot.
// More targets than TCH: further chunks over the same keys (L2-resident).  The hit counters are
// summed per thread, reduced in LDS and added with one atomic per workgroup and counter.
constexpr int TCH = 2048;     // targets per chunk: 16 KB of composites + 8 KB of counts
constexpr int MAX_CUTOFFS = 8;

// (8 waves per SIMD = two workgroups per CU: without the attribute the cut-offs and pointers
// take 101 SGPRs, one too many)
__global__ __launch_bounds__(SNT) __attribute__((amdgpu_waves_per_eu(8, 8))) void target_ranks_kernel(
    const uint32_t *__restrict__ keys, int Vs, int V, const int32_t *__restrict__ tgt_ptr,
    const int32_t *__restrict__ tgt, const int32_t *__restrict__ cutoffs, int n_cut,
    int32_t *__restrict__ ranks, float *__restrict__ tgt_vals, unsigned long long *__restrict__ hits) {
  static_assert(TCH == 2 * SNT, "the scan gives every thread two counters");
  __shared__ uint64_t srt[TCH];
  __shared__ uint32_t cnt[TCH];
  __shared__ int wtot[SNT / 64];
  __shared__ uint32_t s_hit[MAX_CUTOFFS + 1];
  __shared__ int s_best;
  const int tid = threadIdx.x, lane = tid & 63;
  const uint64_t lt = (1ull << lane) - 1ull;
  const int r = blockIdx.x;
  const int tbeg = tgt_ptr[r], T = tgt_ptr[r + 1] - tbeg;
  if (T <= 0) return;  // (block-uniform) nothing to rank, nothing to count
  const uint32_t *k = keys + (int64_t)r * Vs;
  int cut[MAX_CUTOFFS];
#pragma unroll
  for (int c = 0; c < MAX_CUTOFFS; ++c) cut[c] = (hits && c < n_cut) ? cutoffs[c] : 0;
  uint32_t hit[MAX_CUTOFFS], nvalid = 0;
#pragma unroll
  for (int c = 0; c < MAX_CUTOFFS; ++c) hit[c] = 0u;
  int best = 0x7FFFFFFF;
  const int steps = (int)cdiv(V, 4 * SNT);  // the same trip count for every lane: ballots inside

  for (int cb = 0; cb < T; cb += TCH) {
    const int Tc = min(TCH, T - cb);
    int P = 1, nbits = 0;
    while (P < Tc) P <<= 1, ++nbits;
    const int32_t *tg = tgt + tbeg + cb;
    for (int i = tid; i < P; i += SNT) {
      uint64_t x = 0ull;
      if (i < Tc) {
        const int t = tg[i];
        if ((uint32_t)t < (uint32_t)V) {  // never index with an id outside the row
          const uint32_t key = k[t];
          if (key) x = ((uint64_t)key << 32) | (uint32_t)t;
        }
      }
      srt[i] = x;
      cnt[i] = 0u;
    }
    __syncthreads();
    rowsort::bitonic_sort<SNT>(P, rowsort::CmpSwapU64<true>{srt});
    int Tv = 0;  // valid targets: the first position holding 0
    for (int hi = P; Tv < hi;) {
      const int mid = (Tv + hi) >> 1;
      if (srt[mid] != 0ull) Tv = mid + 1; else hi = mid;
    }
    if (Tv > 0) {
      const uint64_t low = srt[Tv - 1];
      for (int st = 0; st < steps; ++st) {
        const int base = 4 * (st * SNT + tid);
        uint4 kk = make_uint4(0u, 0u, 0u, 0u);
        if (base < V) kk = *reinterpret_cast<const uint4 *>(k + base);  // base + 3 < Vs
        const uint32_t ke[4] = {kk.x, kk.y, kk.z, kk.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint64_t x = ((uint64_t)ke[e] << 32) | (uint32_t)(base + e);
          const bool above = base + e < V && ke[e] != 0u && x > low;
          if (__ballot(above) == 0ull) continue;  // (wave-uniform)
          int g = 0;  // first position with srt[g] < x; above: g < Tv
          if (above)
            for (int hi = Tv - 1; g < hi;) {
              const int mid = (g + hi) >> 1;
              if (srt[mid] >= x) g = mid + 1; else hi = mid;
            }
          const uint64_t m = rowsort::wave_match((uint32_t)g, above, nbits);
          if (above && (m & lt) == 0ull) atomicAdd(&cnt[g], (uint32_t)__popcll(m));
        }
      }
    }
    __syncthreads();
    {  // inclusive prefix sums in place; thread tid owns counters 2 tid and 2 tid + 1
      const int c0 = 2 * tid < P ? (int)cnt[2 * tid] : 0;
      const int c1 = 2 * tid + 1 < P ? (int)cnt[2 * tid + 1] : 0;
      const int incl = rowsort::block_incl_scan<SNT>(c0 + c1, wtot);
      if (2 * tid < P) cnt[2 * tid] = (uint32_t)(incl - c1);
      if (2 * tid + 1 < P) cnt[2 * tid + 1] = (uint32_t)incl;
    }
    __syncthreads();
    for (int i = tid; i < Tc; i += SNT) {
      const int t = tg[i];
      uint32_t key = 0u;
      if ((uint32_t)t < (uint32_t)V) key = k[t];
      int rank = -1;
      float val = 0.f;
      if (key) {
        const uint64_t x = ((uint64_t)key << 32) | (uint32_t)t;
        int p = 0;  // first position with srt[p] <= x: x itself
        for (int hi = Tv - 1; p < hi;) {
          const int mid = (p + hi) >> 1;
          if (srt[mid] > x) p = mid + 1; else hi = mid;
        }
        rank = (int)cnt[p];
        val = __uint_as_float(key - 1u);
        ++nvalid;
        best = min(best, rank);
#pragma unroll
        for (int c = 0; c < MAX_CUTOFFS; ++c) hit[c] += rank < cut[c] ? 1u : 0u;
      }
      ranks[tbeg + cb + i] = rank;
      tgt_vals[tbeg + cb + i] = val;
    }
    __syncthreads();  // srt and cnt are free for the next chunk
  }

  if (!hits) return;
  if (tid <= MAX_CUTOFFS) s_hit[tid] = 0u;
  if (tid == 0) s_best = 0x7FFFFFFF;
  __syncthreads();
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < MAX_CUTOFFS; ++c) hit[c] += __shfl_xor(hit[c], off);
    nvalid += __shfl_xor(nvalid, off);
    best = min(best, __shfl_xor(best, off));
  }
  if (lane == 0 && nvalid) {
#pragma unroll
    for (int c = 0; c < MAX_CUTOFFS; ++c)
      if (hit[c]) atomicAdd(&s_hit[c], hit[c]);
    atomicAdd(&s_hit[MAX_CUTOFFS], nvalid);
    atomicMin(&s_best, best);
  }
  __syncthreads();
  if (tid < n_cut && s_hit[tid]) atomicAdd(hits + tid, (unsigned long long)s_hit[tid]);
  if (tid == n_cut && s_hit[MAX_CUTOFFS]) {
    atomicAdd(hits + n_cut, (unsigned long long)s_hit[MAX_CUTOFFS]);  // targets counted
    if (n_cut > 0 && s_best < cut[0]) atomicAdd(hits + n_cut + 1, 1ull);  // the row's best is a hit
  }
}

// workspace: [E1 partials R*cap*d][zlat R*64][h3 R*d][keys R*Vs][cube bitmasks R*VW]
struct BatchWs {
  size_t part, zlat, h3, keys, bits, total;
  int Vs, VW;
};
BatchWs batch_ws(int V, int d, int R, int max_n) {
  BatchWs w;
  const size_t r = (size_t)std::max(R, 1), dd = (size_t)std::max(d, 64);
  w.Vs = (std::max(V, 1) + 3) & ~3;
  w.VW = (std::max(V, 1) + 31) / 32;
  size_t o = 0;
  w.part = o, o += align256(r * cc::infer_gather_cap(max_n) * dd * sizeof(float));
  w.zlat = o, o += align256(r * 64 * sizeof(float));
  w.h3 = o, o += align256(r * dd * sizeof(float));
  w.keys = o, o += align256(r * w.Vs * sizeof(uint32_t));
  w.bits = o, o += align256(r * w.VW * sizeof(uint32_t));
  w.total = o;
  return w;
}

// the pooled entries' share of the workspace, behind the batch workspace:
// [exclusion bitmasks R*VW][n_cand R]
struct PoolWs {
  size_t excl, ncand, total;
};
PoolWs pool_ws(const BatchWs &w, int R) {
  PoolWs p;
  const size_t r = (size_t)std::max(R, 1);
  size_t o = w.total;
  p.excl = o, o += align256(r * w.VW * sizeof(uint32_t));
  p.ncand = o, o += align256(r * sizeof(int32_t));
  p.total = o;
  return p;
}

// A pooled call's extra arguments (device pointers); the unpooled entries pass none.
struct Pools {
  const uint32_t *pools;
  int n_pools;
  const int32_t *pool_of_row;
};

template <int RM>
void launch_out(dim3 grid, hipStream_t s, const float *h3, const float *Wo, const float *bo, int d,
                int V, int R, const int32_t *row_ptr, const int32_t *idx, const uint32_t *bits,
                int VW, uint32_t *keys, int Vs, float *cut_vals, float *probs,
                const uint32_t *excl) {
  grid.y = (unsigned)cdiv(R, 16 * RM);
  if (excl)
    hipLaunchKernelGGL((out_tile_kernel<RM, true>), grid, dim3(ONT), 0, s, h3, Wo, bo, d, V, R,
                       row_ptr, idx, bits, VW, keys, Vs, cut_vals, probs, excl);
  else
    hipLaunchKernelGGL((out_tile_kernel<RM, false>), grid, dim3(ONT), 0, s, h3, Wo, bo, d, V, R,
                       row_ptr, idx, bits, VW, keys, Vs, cut_vals, probs, excl);
}

}  // namespace

extern "C" int32_t cc_recommend_batch_max_amount(void) { return MAX_AMOUNT; }

int cc::row_bits_launch(const int32_t *row_ptr, const int32_t *idx, int R, int V, int VW,
                        uint32_t *bits, hipStream_t s) {
  hipLaunchKernelGGL(row_bits_kernel, dim3(R), dim3(256), 0, s, row_ptr, idx, V, VW, bits);
  CC_LAUNCH_CHECK("row_bits_kernel");
  return CC_OK;
}

// A pooled call's argument checks (who: the entry's name).  optional: the entry takes pools or none
// (complete.hip, diverse.hip), so the rules hold once any of the three is given.
int cc::pools_check(const char *who, const uint32_t *pools, int n_pools, const int32_t *pool_of_row,
                    bool optional) {
  if (optional && !(pools || n_pools || pool_of_row)) return CC_OK;
  const std::string w(who);
  CC_REQUIRE(pool_of_row, w + (optional ? ": null pointer (pool_of_row with pools)" : ": null pointer"));
  CC_REQUIRE(n_pools >= 0, w + ": n_pools is negative");
  CC_REQUIRE(pools || n_pools == 0, w + ": pools is null with n_pools > 0");
  return CC_OK;
}

namespace {
// The arguments all six entries share.
struct BatchArgs {
  const float *params;
  int V, d, R;
  const int32_t *row_ptr, *idx;
  int max_n;
  void *ws;
  float *cut_vals, *probs;
  hipStream_t s;
};

// What the front leaves for a back half: the layout, the rows' keys, a pooled call's candidate
// counts (null without pools) and the bytes of workspace the chain (with the pools' share) holds.
struct BatchKeys {
  BatchWs w;
  const uint32_t *keys;
  const int32_t *n_cand;
  size_t after;
};
}  // namespace

// The launches all entries share: row masks, h3, then the output layer, which leaves every row's
// sort keys in the workspace, its cut values and (on request) its probabilities.  pl: a pooled
// call's arguments, or null.  The arguments are checked; R > 0.
static int batch_keys_launch(const BatchArgs &a, const Pools *pl, BatchKeys *k) {
  int64_t off[CC_NUM_TENSORS], sz[CC_NUM_TENSORS], tot, mt;
  if (int rc = cc::param_offsets(a.V, a.d, off, sz, &tot, &mt)) return rc;
  const BatchWs w = batch_ws(a.V, a.d, a.R, a.max_n);
  char *base = (char *)a.ws;
  float *h3 = (float *)(base + w.h3);
  uint32_t *keys = (uint32_t *)(base + w.keys), *bits = (uint32_t *)(base + w.bits);
  const uint32_t *excl = nullptr;
  *k = BatchKeys{w, keys, nullptr, w.total};
  if (pl) {
    const PoolWs p = pool_ws(w, a.R);
    excl = (const uint32_t *)(base + p.excl);
    k->n_cand = (const int32_t *)(base + p.ncand);
    k->after = p.total;
    hipLaunchKernelGGL(row_mask_kernel, dim3(a.R), dim3(256), 0, a.s, a.row_ptr, a.idx, a.V, w.VW,
                       pl->pools, pl->n_pools, pl->pool_of_row, bits, (uint32_t *)(base + p.excl),
                       (int32_t *)(base + p.ncand));
    CC_LAUNCH_CHECK("row_mask_kernel");
  } else if (int rc = cc::row_bits_launch(a.row_ptr, a.idx, a.R, a.V, w.VW, bits, a.s)) {
    return rc;
  }
  if (int rc = cc::infer_h3_launch(a.params, a.V, a.d, a.R, a.row_ptr, a.idx, a.max_n,
                                   (float *)(base + w.part), (float *)(base + w.zlat), h3, a.s))
    return rc;
  const float *Wo = a.params + off[14], *bo = a.params + off[15];
  const dim3 grid((unsigned)cdiv(a.V, TC), 1);
  // rows per tile: 32 / 64 / 128 (the arithmetic per (row, card) does not depend on it)
  const auto out = a.R <= 32 ? &launch_out<2> : a.R <= 64 ? &launch_out<4> : &launch_out<8>;
  out(grid, a.s, h3, Wo, bo, a.d, a.V, a.R, a.row_ptr, a.idx, bits, w.VW, keys, w.Vs, a.cut_vals,
      a.probs, excl);
  CC_LAUNCH_CHECK("out_tile_kernel");
  return CC_OK;
}

// The checked front of all six entries, behind the entry's own null-pointer check (who: the
// entry's name): the pools' rules for a pooled call, the common rules with the entry's own one
// (own_ok, own_msg behind the name) where it has always stood, between d and the workspace's
// alignment, then the keys.  R == 0 is no error and launches nothing (*k is then not written):
// the entry returns in place of its back half.
static int batch_front(const char *who, const BatchArgs &a, const Pools *pl, bool own_ok,
                       const char *own_msg, BatchKeys *k) {
  const std::string w(who);
  if (pl)
    if (int rc = cc::pools_check(who, pl->pools, pl->n_pools, pl->pool_of_row, false)) return rc;
  CC_REQUIRE(a.V > 0 && a.R >= 0 && a.max_n >= 0 && a.max_n <= a.V, w + ": V/R/max_n");
  if (int rc = cc::infer_check_d(a.d, who)) return rc;
  CC_REQUIRE(own_ok, w + own_msg);
  CC_REQUIRE(((uintptr_t)a.ws & 255) == 0, w + ": ws must be 256-byte aligned");
  if (a.R == 0) return CC_OK;
  return batch_keys_launch(a, pl, k);
}

// The back halves, on the keys of a launched front (the third, target_ranks_kernel, stands in its
// entry).  The select: every row's first
// max(amount, 1) candidates; the row pitch of additions / add_vals is max(amount, 1).
static int select_launch(const BatchArgs &a, const BatchKeys &k, int amount, int32_t *n_add,
                         int32_t *additions, float *add_vals) {
  const int A = amount > 0 ? amount : 1;
  const auto kernel = k.n_cand ? &topn_rows_kernel<true> : &topn_rows_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(a.R), dim3(SNT), 0, a.s, k.keys, k.w.Vs, a.V, a.row_ptr, amount,
                     A, n_add, additions, add_vals, k.n_cand);
  CC_LAUNCH_CHECK("topn_rows_kernel");
  return CC_OK;
}

// rank workspace: the chain's, then the two (key', card) ping-pong buffers [R][Vp] of 64-bit
// words; Vp is a multiple of 16, so no two rows share a 128-byte line
static size_t rank_pitch(int V) { return ((size_t)std::max(V, 1) + 15) & ~(size_t)15; }
static size_t rank_buf_bytes(int V, int R) {
  return align256((size_t)std::max(R, 1) * rank_pitch(V) * sizeof(uint64_t));
}

// The full ranking: any amount, result rows of min(max(amount, 1), V) entries.
static int rank_launch(const BatchArgs &a, const BatchKeys &k, int amount, int32_t *n_add,
                       int32_t *additions, float *add_vals) {
  char *bufs = (char *)a.ws + k.after;
  uint64_t *pa = (uint64_t *)bufs, *pb = (uint64_t *)(bufs + rank_buf_bytes(a.V, a.R));
  const int A = std::min(amount > 0 ? amount : 1, a.V);
  const auto kernel = k.n_cand ? &rank_rows_kernel<true> : &rank_rows_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(a.R), dim3(SNT), 0, a.s, k.keys, k.w.Vs, a.V, a.row_ptr, amount,
                     A, pa, pb, (int)rank_pitch(a.V), n_add, additions, add_vals, k.n_cand);
  CC_LAUNCH_CHECK("rank_rows_kernel");
  return CC_OK;
}

// ---------------------------------------------------------------------- pieces for complete.hip
namespace cc {
int batch_max_amount() { return MAX_AMOUNT; }

// bytes of workspace batch_select_launch uses (pooled: with the pools' share)
size_t batch_select_ws_bytes(int V, int d, int R, int max_n, bool pooled) {
  const BatchWs w = batch_ws(V, d, R, max_n);
  return pooled ? pool_ws(w, R).total : w.total;
}

// The chain behind cc_recommend_batch_fp32 (pool_of_row null) and cc_recommend_batch_pool_fp32:
// keys, then the select.  The arguments are the entries', already checked; R > 0.
int batch_select_launch(const float *params, int V, int d, int R, const int32_t *row_ptr,
                        const int32_t *idx, int max_n, int amount, void *ws, int32_t *n_add,
                        int32_t *additions, float *add_vals, float *cut_vals, float *probs,
                        const uint32_t *pools, int n_pools, const int32_t *pool_of_row,
                        hipStream_t s) {
  const BatchArgs a{params, V, d, R, row_ptr, idx, max_n, ws, cut_vals, probs, s};
  const Pools pl{pools, n_pools, pool_of_row};
  BatchKeys k;
  if (int rc = batch_keys_launch(a, pool_of_row ? &pl : nullptr, &k)) return rc;
  return select_launch(a, k, amount, n_add, additions, add_vals);
}
}  // namespace cc

// ------------------------------------------------------------------------------------ the entries
// Workspace of an entry: the chain's (pooled: with the pools' share), the ranking's two buffers,
// and 256 bytes for the caller to align in.
static size_t entry_ws_size(int V, int d, int R, int max_n, bool pooled, bool ranked) {
  return cc::batch_select_ws_bytes(V, d, R, max_n, pooled) + (ranked ? 2 * rank_buf_bytes(V, R) : 0) +
         256;
}
#define CC_BATCH_WS_SIZE(name, pooled, ranked)                             \
  extern "C" size_t name(int32_t V, int32_t d, int32_t R, int32_t max_n) { \
    return entry_ws_size(V, d, R, max_n, pooled, ranked);                  \
  }
CC_BATCH_WS_SIZE(cc_recommend_batch_ws_size, false, false)
CC_BATCH_WS_SIZE(cc_recommend_batch_pool_ws_size, true, false)
CC_BATCH_WS_SIZE(cc_recommend_batch_rank_ws_size, false, true)
CC_BATCH_WS_SIZE(cc_recommend_batch_rank_pool_ws_size, true, true)
CC_BATCH_WS_SIZE(cc_recommend_batch_target_ranks_ws_size, false, false)
CC_BATCH_WS_SIZE(cc_recommend_batch_target_ranks_pool_ws_size, true, false)
#undef CC_BATCH_WS_SIZE

// cc_recommend_batch[_rank][_pool]_fp32 (who); rank: the full ranking, which has no amount cap.
static int recommend_entry(const char *who, bool rank, const BatchArgs &a, int amount,
                           int32_t *n_add, int32_t *additions, float *add_vals, const Pools *pl) {
  CC_REQUIRE(a.params && a.row_ptr && a.idx && a.ws && n_add && additions && add_vals && a.cut_vals,
             std::string(who) + ": null pointer");
  BatchKeys k;
  if (int rc = batch_front(who, a, pl, rank || amount <= MAX_AMOUNT,
                           ": amount above cc_recommend_batch_max_amount()", &k))
    return rc;
  if (a.R == 0) return CC_OK;
  return (rank ? rank_launch : select_launch)(a, k, amount, n_add, additions, add_vals);
}

extern "C" int cc_recommend_batch_fp32(const float *params, int32_t V, int32_t d, int32_t R,
                                       const int32_t *row_ptr, const int32_t *idx, int32_t max_n,
                                       int32_t amount, void *ws, int32_t *n_add,
                                       int32_t *additions, float *add_vals, float *cut_vals,
                                       float *probs, void *stream) {
  return recommend_entry(
      "cc_recommend_batch_fp32", false,
      {params, V, d, R, row_ptr, idx, max_n, ws, cut_vals, probs, as_stream(stream)}, amount, n_add,
      additions, add_vals, nullptr);
}

extern "C" int cc_recommend_batch_pool_fp32(const float *params, int32_t V, int32_t d, int32_t R,
                                            const int32_t *row_ptr, const int32_t *idx,
                                            int32_t max_n, int32_t amount, void *ws,
                                            int32_t *n_add, int32_t *additions, float *add_vals,
                                            float *cut_vals, float *probs, const uint32_t *pools,
                                            int32_t n_pools, const int32_t *pool_of_row,
                                            void *stream) {
  const Pools pl{pools, n_pools, pool_of_row};
  return recommend_entry(
      "cc_recommend_batch_pool_fp32", false,
      {params, V, d, R, row_ptr, idx, max_n, ws, cut_vals, probs, as_stream(stream)}, amount, n_add,
      additions, add_vals, &pl);
}

extern "C" int cc_recommend_batch_rank_fp32(const float *params, int32_t V, int32_t d, int32_t R,
                                            const int32_t *row_ptr, const int32_t *idx,
                                            int32_t max_n, int32_t amount, void *ws,
                                            int32_t *n_add, int32_t *additions, float *add_vals,
                                            float *cut_vals, float *probs, void *stream) {
  return recommend_entry(
      "cc_recommend_batch_rank_fp32", true,
      {params, V, d, R, row_ptr, idx, max_n, ws, cut_vals, probs, as_stream(stream)}, amount, n_add,
      additions, add_vals, nullptr);
}

extern "C" int cc_recommend_batch_rank_pool_fp32(
    const float *params, int32_t V, int32_t d, int32_t R, const int32_t *row_ptr,
    const int32_t *idx, int32_t max_n, int32_t amount, void *ws, int32_t *n_add,
    int32_t *additions, float *add_vals, float *cut_vals, float *probs, const uint32_t *pools,
    int32_t n_pools, const int32_t *pool_of_row, void *stream) {
  const Pools pl{pools, n_pools, pool_of_row};
  return recommend_entry(
      "cc_recommend_batch_rank_pool_fp32", true,
      {params, V, d, R, row_ptr, idx, max_n, ws, cut_vals, probs, as_stream(stream)}, amount, n_add,
      additions, add_vals, &pl);
}

// cc_recommend_batch_target_ranks[_pool]_fp32 (who).  Ranks of chosen cards: one counting workgroup
// per row on the keys (no ping-pong buffers, no R x V result).  The pooled keys give a card outside
// its row's pool key' = 0, as a cube card has: the kernel ranks such a target -1 with value 0 and
// counts the pool's candidates alone.
static int target_ranks_entry(const char *who, const BatchArgs &a, const int32_t *tgt_ptr,
                              const int32_t *tgt, const int32_t *cutoffs, int n_cutoffs,
                              int32_t *ranks, float *tgt_vals, unsigned long long *hits,
                              const Pools *pl) {
  CC_REQUIRE(a.params && a.row_ptr && a.idx && tgt_ptr && tgt && a.ws && ranks && tgt_vals &&
                 a.cut_vals,
             std::string(who) + ": null pointer");
  BatchKeys k;
  if (int rc = batch_front(who, a, pl,
                           n_cutoffs >= 0 && n_cutoffs <= MAX_CUTOFFS && (n_cutoffs == 0 || cutoffs),
                           ": n_cutoffs outside 0..8, or cutoffs null", &k))
    return rc;
  if (a.R == 0) return CC_OK;
  hipLaunchKernelGGL(target_ranks_kernel, dim3(a.R), dim3(SNT), 0, a.s, k.keys, k.w.Vs, a.V,
                     tgt_ptr, tgt, cutoffs, n_cutoffs, ranks, tgt_vals, hits);
  CC_LAUNCH_CHECK("target_ranks_kernel");
  return CC_OK;
}

extern "C" int cc_recommend_batch_target_ranks_fp32(
    const float *params, int32_t V, int32_t d, int32_t R, const int32_t *row_ptr,
    const int32_t *idx, int32_t max_n, const int32_t *tgt_ptr, const int32_t *tgt,
    const int32_t *cutoffs, int32_t n_cutoffs, void *ws, int32_t *ranks, float *tgt_vals,
    unsigned long long *hits, float *cut_vals, float *probs, void *stream) {
  return target_ranks_entry(
      "cc_recommend_batch_target_ranks_fp32",
      {params, V, d, R, row_ptr, idx, max_n, ws, cut_vals, probs, as_stream(stream)}, tgt_ptr, tgt,
      cutoffs, n_cutoffs, ranks, tgt_vals, hits, nullptr);
}

extern "C" int cc_recommend_batch_target_ranks_pool_fp32(
    const float *params, int32_t V, int32_t d, int32_t R, const int32_t *row_ptr,
    const int32_t *idx, int32_t max_n, const int32_t *tgt_ptr, const int32_t *tgt,
    const int32_t *cutoffs, int32_t n_cutoffs, void *ws, int32_t *ranks, float *tgt_vals,
    unsigned long long *hits, float *cut_vals, float *probs, const uint32_t *pools,
    int32_t n_pools, const int32_t *pool_of_row, void *stream) {
  const Pools pl{pools, n_pools, pool_of_row};
  return target_ranks_entry(
      "cc_recommend_batch_target_ranks_pool_fp32",
      {params, V, d, R, row_ptr, idx, max_n, ws, cut_vals, probs, as_stream(stream)}, tgt_ptr, tgt,
      cutoffs, n_cutoffs, ranks, tgt_vals, hits, &pl);
}
