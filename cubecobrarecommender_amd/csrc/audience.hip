// cc_audience_put / cc_audience_fp32 — card audience: a resident corpus of cubes, kept as the
// decoder's last hidden rows h3 with the cubes' card lists beside them, and for T query cards the
// k cubes of the corpus that want each card most, p[t][c] = p(card t | cube c).
//
// Every p is the forward pass's own bits (infer.hip, oracle/infer_ref.py): h3[c] is
// cc::infer_h3_launch's row of cube c, and the output layer is out_kernel's dot at the asked
// columns only: k in pinned chunks of 64 from 0, chunk partials added in order from 0, multiply
// and add separately rounded, + bias, det_sigmoid32.  The ranking per card is ascending composite
// (orderable(-p) << 32 | cube): descending p, equal p lower cube id first, which is unique.
//
// The corpus is h3 [cap][d], ptr [cap + 1] and ids [card_cap] (a CSR of sorted distinct card ids
// with absolute offsets).  A put runs the towers of its R rows straight into h3 rows
// [n0, n0 + R) (one workgroup per row: a row's bits do not depend on the put) and
//   put_lists_kernel   : copies the rows' ids behind nnz0 and writes ptr [n0, n0 + R].
// A query runs, once per call,
//   gather_cards_kernel: the T columns of Wo into wT [d][Tp] (Tp = T rounded up to 64, zero
//                        columns for the pad and for cards outside [0, V)), their biases, the
//                        checked cards, and zeroes the counts.  The only V-strided loads.
// then per chunk of the corpus (cubes [c0, c0 + cl)), so that the keys are [T][chunk], never [T][N],
//   score_chunk_kernel : 64 cubes x 64 cards per workgroup, the dot-product tile of DESIGN.md
//                        4.10 in the pinned chunks (out_tile_kernel's loop, restated).  The card tiles of one
//                        cube tile are neighbouring workgroups: h3 comes from HBM once per chunk.
//                        Membership: the tile's 64 cards sorted in LDS (equal runs kept); the
//                        tile's cubes are one segment of ids, read coalesced by all threads with
//                        four loads in flight, each id tried against a 2,048-bit filter of the
//                        cards and only then binary-searched among them; a hit finds its cube in
//                        the tile's row offsets and sets the bits of the whole equal run (a false
//                        positive of the filter only costs the search).  Writes orderable(-p), or a
//                        sentinel above every real key for a cube that plays the card (unless
//                        members are included), and adds the three counts as integers.
//   select_chunk_kernel: one workgroup per card: the chunk's min(k, candidates) smallest
//                        composites (rowselect.hpp) with global cube ids as cand [T][chunks][k].
// and at the end
//   merge_rows_kernel  : one workgroup per card, the same select over its k * chunks candidates.
//                        A corpus of one chunk needs no merge: its select writes the rows.
// Counts are integer atomics (order-free); everything else is a pure function of (card, cube).
#include <algorithm>

#include "common.hpp"
#include "detmath.hpp"
#include "dottile.hpp"
#include "infer.hpp"
#include "rowselect.hpp"
#include "rowsort.hpp"

namespace {

constexpr int KCH = dottile::KCH, KS = dottile::KS;  // the tile's constants (dottile.hpp)
constexpr int TC = dottile::TC;   // cards per score tile
constexpr int RM = 4;             // cubes per thread of the score tile
constexpr int TR = 16 * RM;
constexpr int ONT = dottile::NT;  // score-tile workgroup
constexpr int GNT = 256;  // gather / put workgroup
constexpr int BLOOM = 2048;  // bits of a tile's card filter, by the id's low bits
constexpr int MAX_T = 4096;
constexpr int MAX_PUT_ROWS = 65535;  // the gather's grid.y
constexpr int MAX_CHUNK = 1 << 20;
constexpr uint32_t MEMBER = 0xFFFFFFFFu;  // no candidate: real keys end at orderable(-0.f) = 0x80000000

using detm::addf;
using detm::mulf;
using rowsel::CandItem;
using rowsel::MAX_K;
using rowsel::NONE;
using rowsel::select_smallest;
using rowsel::SelectLds;
using rowsel::SNT;
using rowsel::write_row;
using rowsort::orderable;

// orderable's inverse on keys of -p, p >= 0: the zero comes back as +0.f
__device__ __forceinline__ float prob_of_key(uint32_t key) {
  return (key & 0x80000000u) ? 0.f : __uint_as_float(~key & 0x7FFFFFFFu);
}

// ids [nnz0, nnz0 + nnz) and ptr [n0, n0 + R] of the corpus from a put's CSR (row_ptr[0] == 0,
// row_ptr[R] == nnz); an offset outside [0, nnz] is clamped, so ptr never leaves the put's ids.
__global__ __launch_bounds__(GNT) void put_lists_kernel(const int32_t *__restrict__ row_ptr,
                                                        const int32_t *__restrict__ idx, int R, int nnz,
                                                        int n0, int nnz0, int32_t *__restrict__ ptr,
                                                        int32_t *__restrict__ ids) {
  const int count = max(R + 1, nnz);
  for (int64_t i = (int64_t)blockIdx.x * GNT + threadIdx.x; i < count; i += (int64_t)gridDim.x * GNT) {
    if (i <= R) ptr[n0 + i] = nnz0 + min(max(row_ptr[i], 0), nnz);
    if (i < nnz) ids[nnz0 + i] = idx[i];
  }
}

// wT[k][t] = Wo[k][card_t], bo_g[t] = bo[card_t], card_g[t] = the checked card (-1 for none and for
// the pad), cnt[t] = 0, out_counts[t][0..3) = 0.  One thread per word of wT.
__global__ __launch_bounds__(GNT) void gather_cards_kernel(const float *__restrict__ Wo,
                                                           const float *__restrict__ bo, int d, int V, int T,
                                                           int Tp, const int32_t *__restrict__ cards,
                                                           float *__restrict__ wT, float *__restrict__ bo_g,
                                                           int32_t *__restrict__ card_g,
                                                           int32_t *__restrict__ cnt,
                                                           int32_t *__restrict__ out_counts) {
  const int64_t i = (int64_t)blockIdx.x * GNT + threadIdx.x;
  if (i >= (int64_t)d * Tp) return;
  const int kk = (int)(i / Tp), t = (int)(i % Tp);
  const int card = t < T ? card_or_none(cards[t], V) : -1;
  wT[i] = card >= 0 ? Wo[(int64_t)kk * V + card] : 0.f;
  if (kk == 0) {
    bo_g[t] = card >= 0 ? bo[card] : 0.f;
    card_g[t] = card;
    cnt[t] = 0;
    if (t < T) out_counts[3 * t] = out_counts[3 * t + 1] = out_counts[3 * t + 2] = 0;
  }
}

// keys [T][pitch] of the chunk's cubes [c0, c0 + cl): key (t, j) = orderable(-p[t][c0 + j]), MEMBER
// where cube c0 + j is no candidate of card t.  Block b: cube tile b / ntt, card tile b % ntt.
// (4 waves per SIMD: at most 128 VGPRs)
__global__ __launch_bounds__(ONT, 4) void score_chunk_kernel(
    const float *__restrict__ h3, const int32_t *__restrict__ ptr, const int32_t *__restrict__ ids, int d,
    int c0, int cl, const float *__restrict__ wT, const float *__restrict__ bo_g,
    const int32_t *__restrict__ card_g, int T, int Tp, int ntt, int include_members, float threshold,
    int pitch, uint32_t *__restrict__ keys, int32_t *__restrict__ cnt, int32_t *__restrict__ out_counts) {
  constexpr int F4 = KS / 4, RS = ONT / F4;  // float4 per cube row, cube rows per step
  static_assert(KS * TC + TR * KS <= TC * (TR + 1), "the key tile reuses the stages' LDS");
  static_assert(3 * TC <= ONT && 2 * TR <= ONT && TR + 1 <= ONT && BLOOM / 32 <= ONT,
                "one thread per counter, mask word, row offset and filter word");
  __shared__ __attribute__((aligned(16))) float smem[TC * (TR + 1)];
  float(*wsm)[TC] = reinterpret_cast<float(*)[TC]>(smem);            // [KS][TC]
  float(*hsm)[KS] = reinterpret_cast<float(*)[KS]>(smem + KS * TC);  // [TR][KS]
  uint32_t(*ksm)[TR + 1] = reinterpret_cast<uint32_t(*)[TR + 1]>(smem);  // [TC][TR + 1], behind the loop
  __shared__ int32_t s_card[TC], s_sorted[TC], s_perm[TC];
  __shared__ uint32_t s_mask[TR][2];  // bit t of row r: cube r plays the tile's card t
  __shared__ int32_t s_cnt[3][TC];
  __shared__ int32_t s_ptr[TR + 1];       // the tile's rows in ids
  __shared__ uint32_t s_bloom[BLOOM / 32];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int nb = (blockIdx.x / ntt) * TR;  // first cube of the tile, inside the chunk
  const int t0 = (blockIdx.x % ntt) * TC;  // first card of the tile

  // ---- membership
  if (tid < TC) s_card[tid] = card_g[t0 + tid];  // t0 + tid < Tp
  if (tid < 2 * TR) (&s_mask[0][0])[tid] = 0u;
  if (tid < 3 * TC) (&s_cnt[0][0])[tid] = 0;
  if (tid < BLOOM / 32) s_bloom[tid] = 0u;
  // the tile's cubes are neighbours in the CSR: their ids are one segment; a row behind cl is empty
  if (tid <= TR) s_ptr[tid] = ptr[c0 + nb + min(tid, cl - nb)];
  __syncthreads();
  if (tid < TC) {  // rank sort: no card sorts behind every id, equal cards keep their order
    const int32_t mine = s_card[tid] < 0 ? 0x7FFFFFFF : s_card[tid];
    int rank = 0;
    for (int j = 0; j < TC; ++j) {
      const int32_t other = s_card[j] < 0 ? 0x7FFFFFFF : s_card[j];
      rank += (other < mine || (other == mine && j < tid)) ? 1 : 0;
    }
    s_sorted[rank] = mine;
    s_perm[rank] = tid;
    if (s_card[tid] >= 0) atomicOr(&s_bloom[(mine & (BLOOM - 1)) >> 5], 1u << (mine & 31));
  }
  __syncthreads();
  {
    // every thread strides over the segment, four loads in flight; an id whose bit of the cards'
    // 2,048-bit filter is clear (all but a few per cent) is done after one LDS read
    const int beg = s_ptr[0], end = s_ptr[TR];
    for (int j0 = beg + tid; j0 < end; j0 += 4 * ONT) {
      int32_t id[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) id[u] = j0 + u * ONT < end ? ids[j0 + u * ONT] : -1;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int32_t x = id[u];
        if (x < 0 || !((s_bloom[(x & (BLOOM - 1)) >> 5] >> (x & 31)) & 1u)) continue;
        int pos = 0;  // the number of sorted cards below x, or 63
#pragma unroll
        for (int step = TC / 2; step > 0; step >>= 1)
          if (s_sorted[pos + step - 1] < x) pos += step;
        if (s_sorted[pos] != x) continue;
        const int j = j0 + u * ONT;
        int r = 0;  // the cube of position j: the last row that starts at or before it
#pragma unroll
        for (int step = TR / 2; step > 0; step >>= 1)
          if (s_ptr[r + step] <= j) r += step;
        for (; pos < TC && s_sorted[pos] == x; ++pos) {
          const int t = s_perm[pos];
          atomicOr(&s_mask[r][t >> 5], 1u << (t & 31));
        }
      }
    }
  }

  // ---- scores: out_tile_kernel's loop (recbatch.hip), statement for statement
  float tot[RM][4], acc[RM][4];
#pragma unroll
  for (int j = 0; j < RM; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) tot[j][e] = acc[j][e] = 0.f;
  // the rows this thread stages are RS rows of h3 apart: one pointer, and a bit per row inside cl
  const float *hbase = h3 + (int64_t)(c0 + nb + tid / F4) * d + 4 * (tid % F4);
  uint32_t hmask = 0u;
#pragma unroll
  for (int i = 0; i < TR / RS; ++i)
    if (nb + tid / F4 + RS * i < cl) hmask |= 1u << i;

  for (int k0 = 0; k0 < d; k0 += KS) {
    __syncthreads();  // the previous stage's readers are done
    {
      const int c = tid & 63;
      const float *Wp = wT + ((int64_t)k0 + (tid >> 6)) * Tp + t0 + c;  // inside [d][Tp]: the pad is there
      float w[KS / 4];
#pragma unroll
      for (int i = 0; i < KS / 4; ++i) w[i] = Wp[(int64_t)(4 * i) * Tp];
      float4 h[TR / RS];
#pragma unroll
      for (int i = 0; i < TR / RS; ++i)
        h[i] = (hmask >> i) & 1u ? *reinterpret_cast<const float4 *>(hbase + (int64_t)(RS * i) * d + k0)
                                 : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int i = 0; i < KS / 4; ++i) wsm[4 * i + (tid >> 6)][c] = w[i];
#pragma unroll
      for (int i = 0; i < TR / RS; ++i)
        *reinterpret_cast<float4 *>(&hsm[tid / F4 + RS * i][4 * (tid % F4)]) = h[i];
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
  __syncthreads();  // the last stage's readers are done (and the mask is complete): smem is ksm now

  // ---- keys and counts
  const float4 b4 = *reinterpret_cast<const float4 *>(bo_g + t0 + 4 * tx);
  const float bias[4] = {b4.x, b4.y, b4.z, b4.w};
  int n_mem[4] = {0, 0, 0, 0}, n_cand[4] = {0, 0, 0, 0}, n_above[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < RM; ++j) {
    const int lr = ty * RM + j;
    const bool cube_ok = nb + lr < cl;
    const uint64_t mrow = ((uint64_t)s_mask[lr][1] << 32) | s_mask[lr][0];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int tl = 4 * tx + e;
      const bool ok = cube_ok && s_card[tl] >= 0;
      const bool member = (mrow >> tl) & 1ull;
      const bool cand = ok && (include_members || !member);
      const float p = detm::det_sigmoid32(addf(tot[j][e], bias[e]));
      ksm[tl][lr] = cand ? min(orderable(-p), MEMBER - 1u) : MEMBER;
      n_mem[e] += (ok && member) ? 1 : 0;
      n_cand[e] += cand ? 1 : 0;
      n_above[e] += (cand && p >= threshold) ? 1 : 0;
    }
  }
  // a wave holds four cube groups of every card group: lanes 16 and 32 apart share their cards
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    int v[3] = {n_mem[e], n_cand[e], n_above[e]};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      v[q] += __shfl_xor(v[q], 16, 64);
      v[q] += __shfl_xor(v[q], 32, 64);
      if ((tid & 63) < 16 && v[q]) atomicAdd(&s_cnt[q][4 * tx + e], v[q]);
    }
  }
  __syncthreads();
  for (int i = 0; i < TC / (ONT / 64); ++i) {  // a wave writes 64 cubes of one card: 256 contiguous bytes
    const int row = (ONT / 64) * i + (tid >> 6), col = tid & 63;
    if (t0 + row < T && nb + col < cl) keys[(int64_t)(t0 + row) * pitch + nb + col] = ksm[row][col];
  }
  if (tid < 3 * TC) {
    const int q = tid / TC, t = t0 + tid % TC;
    const int v = s_cnt[q][tid % TC];
    if (v && t < T) {
      atomicAdd(out_counts + 3 * t + q, v);
      if (q == 1) atomicAdd(cnt + t, v);  // the chunk's candidates, for its select
    }
  }
}

struct KeyItem {  // key << 32 | cube position inside the chunk; a member is no candidate
  const uint32_t *k;
  __device__ __forceinline__ uint64_t operator()(int j) const {
    const uint32_t key = k[j];
    return key == MEMBER ? NONE : ((uint64_t)key << 32) | (uint32_t)j;
  }
};

// Candidates of (card t, this chunk): cand[t][chunk][0..k), global cube ids, NONE behind the last.
// cnt[t] is the chunk's candidate count, taken and cleared for the next chunk's score launch.
// FINAL (the corpus is one chunk): the chunk's candidates are the row's result, written as such.
template <bool FINAL>
__global__ __launch_bounds__(SNT) void select_chunk_kernel(const uint32_t *__restrict__ keys, int pitch, int c0,
                                                           int cl, int32_t *__restrict__ cnt, int k,
                                                           int chunk_no, int chunks, uint64_t *__restrict__ cand,
                                                           int32_t *__restrict__ out_idx,
                                                           float *__restrict__ out_p) {
  __shared__ SelectLds s;
  __shared__ int s_n;
  const int tid = threadIdx.x;
  const int t = blockIdx.x;
  if (tid == 0) {
    s_n = cnt[t];
    cnt[t] = 0;
  }
  __syncthreads();
  const int want = min(k, min(max(s_n, 0), cl));  // (block-uniform)
  if (want > 0) select_smallest(s, KeyItem{keys + (int64_t)t * pitch}, cl, want, (uint32_t)(cl - 1));
  if (FINAL) {
    write_row(s, want, k, out_idx + (int64_t)t * k, out_p + (int64_t)t * k, prob_of_key);  // c0 == 0
  } else {
    uint64_t *out = cand + ((int64_t)t * chunks + chunk_no) * k;
    // c0 + position < 2^31: the sum stays inside the low word
    for (int i = tid; i < want; i += SNT) out[i] = s.sel[i] + (uint32_t)c0;
    for (int i = want + tid; i < k; i += SNT) out[i] = NONE;
  }
}

__global__ __launch_bounds__(SNT) void merge_rows_kernel(const uint64_t *__restrict__ cand, int chunks, int N,
                                                         const int32_t *__restrict__ out_counts, int k,
                                                         int32_t *__restrict__ out_idx,
                                                         float *__restrict__ out_p) {
  __shared__ SelectLds s;
  const int t = blockIdx.x;
  const int want = min(k, min(max(out_counts[3 * t + 1], 0), N));  // (block-uniform)
  // chunks * k stays below 2^31: larger counts are refused by the entry
  if (want > 0) select_smallest(s, CandItem{cand + (int64_t)t * chunks * k}, chunks * k, want, (uint32_t)(N - 1));
  write_row(s, want, k, out_idx + (int64_t)t * k, out_p + (int64_t)t * k, prob_of_key);
}

// corpus: [h3 cap*d][ptr cap+1][ids card_cap]; the offsets do not depend on card_cap
struct CorpusLayout {
  size_t h3, ptr, ids;
};
CorpusLayout corpus_layout(int cap, int d) {
  CorpusLayout x;
  const size_t c = (size_t)std::max(cap, 1);
  size_t o = 0;
  x.h3 = o, o += align256(c * std::max(d, 64) * sizeof(float));
  x.ptr = o, o += align256((c + 1) * sizeof(int32_t));
  x.ids = o;
  return x;
}

// put workspace: [partials R*gather_cap(max_n)*d][zlat R*64]
struct PutWs {
  size_t part, zlat, total;
};
PutWs put_ws(int R, int d, int max_n) {
  PutWs w;
  const size_t r = (size_t)std::max(R, 1), dd = (size_t)std::max(d, 64);
  size_t o = 0;
  w.part = o, o += align256(r * cc::infer_gather_cap(max_n) * dd * sizeof(float));
  w.zlat = o, o += align256(r * 64 * sizeof(float));
  w.total = o;
  return w;
}

// query workspace: [wT d*Tp][bo Tp][card Tp][cnt Tp][keys T*pitch][cand T*chunks*k], pitch = the
// chunk, or N rounded up to 64 where that is less: it grows with T * chunk and T * k * chunks,
// never with T * N
struct QueryWs : rowsel::ChunkPlan {
  size_t wT, bo, card, cnt, keys, cand, total;
  int Tp;
};
QueryWs query_ws(int N, int d, int T, int k, int chunk) {
  QueryWs w{rowsel::chunk_plan(N, chunk)};
  const size_t t = (size_t)std::max(T, 1), dd = (size_t)std::max(d, 64);
  w.Tp = (int)cdiv((int64_t)t, TC) * TC;
  size_t o = 0;
  w.wT = o, o += align256(dd * w.Tp * sizeof(float));
  w.bo = o, o += align256((size_t)w.Tp * sizeof(float));
  w.card = o, o += align256((size_t)w.Tp * sizeof(int32_t));
  w.cnt = o, o += align256((size_t)w.Tp * sizeof(int32_t));
  w.keys = o, o += align256(t * w.pitch * sizeof(uint32_t));
  w.cand = o, o += align256(t * (size_t)w.chunks * (size_t)std::max(k, 1) * sizeof(uint64_t));
  w.total = o;
  return w;
}

}  // namespace

extern "C" size_t cc_audience_corpus_size(int32_t cap, int32_t card_cap, int32_t d) {
  return corpus_layout(cap, d).ids + align256((size_t)std::max(card_cap, 1) * sizeof(int32_t));
}

extern "C" size_t cc_audience_corpus_ptr_offset(int32_t cap, int32_t d) { return corpus_layout(cap, d).ptr; }

extern "C" size_t cc_audience_corpus_ids_offset(int32_t cap, int32_t d) { return corpus_layout(cap, d).ids; }

extern "C" size_t cc_audience_put_ws_size(int32_t R, int32_t d, int32_t max_n) {
  return put_ws(R, d, max_n).total;
}

extern "C" int cc_audience_put(const float *params, int32_t V, int32_t d, void *corpus, int32_t cap,
                               int32_t card_cap, int32_t n0, int32_t nnz0, int32_t R,
                               const int32_t *row_ptr, const int32_t *idx, int32_t nnz, int32_t max_n,
                               void *ws, void *stream) {
  CC_REQUIRE(params && corpus && row_ptr && idx && ws, "cc_audience_put: null pointer");
  CC_REQUIRE(((uintptr_t)corpus & 255) == 0, "cc_audience_put: corpus must be 256-byte aligned");
  CC_REQUIRE(((uintptr_t)ws & 255) == 0, "cc_audience_put: ws must be 256-byte aligned");
  CC_REQUIRE(V > 0 && cap >= 1 && card_cap >= 1 && card_cap <= 0x7FFFFFFF - 4 * ONT,
             "cc_audience_put: bad V/cap/card_cap");
  if (int rc = cc::infer_check_d(d, "cc_audience_put")) return rc;
  CC_REQUIRE(n0 >= 0 && R >= 0 && (int64_t)n0 + R <= cap,
             "cc_audience_put: rows [n0, n0 + R) must lie inside [0, cap)");
  CC_REQUIRE(nnz0 >= 0 && nnz >= 0 && (int64_t)nnz0 + nnz <= card_cap,
             "cc_audience_put: ids [nnz0, nnz0 + nnz) must lie inside [0, card_cap)");
  CC_REQUIRE(max_n >= 0 && max_n <= V && (int64_t)nnz <= (int64_t)R * max_n,
             "cc_audience_put: max_n outside [0, V] or nnz above R * max_n");
  CC_REQUIRE(R <= MAX_PUT_ROWS, "cc_audience_put: more than 65535 rows in one put");
  if (R == 0) return CC_OK;
  const CorpusLayout x = corpus_layout(cap, d);
  const PutWs w = put_ws(R, d, max_n);
  char *cb = (char *)corpus, *wb = (char *)ws;
  hipStream_t s = as_stream(stream);
  if (int rc = cc::infer_h3_launch(params, V, d, R, row_ptr, idx, max_n, (float *)(wb + w.part),
                                   (float *)(wb + w.zlat), (float *)(cb + x.h3) + (int64_t)n0 * d, s))
    return rc;
  const unsigned blocks = (unsigned)std::min<int64_t>(2048, cdiv(std::max(R + 1, nnz), GNT));
  hipLaunchKernelGGL(put_lists_kernel, dim3(blocks), dim3(GNT), 0, s, row_ptr, idx, R, nnz, n0, nnz0,
                     (int32_t *)(cb + x.ptr), (int32_t *)(cb + x.ids));
  CC_LAUNCH_CHECK("put_lists_kernel");
  return CC_OK;
}

extern "C" int32_t cc_audience_max_k(void) { return MAX_K; }

extern "C" size_t cc_audience_ws_size(int32_t N, int32_t d, int32_t T, int32_t k, int32_t chunk) {
  return query_ws(N, d, T, k, chunk).total;
}

extern "C" int cc_audience_fp32(const float *params, int32_t V, int32_t d, const void *corpus,
                                int32_t cap, int32_t N, int32_t T, const int32_t *cards, int32_t k,
                                int32_t chunk, int32_t include_members, float threshold, void *ws,
                                int32_t *out_idx, float *out_p, int32_t *out_counts, void *stream) {
  CC_REQUIRE(params && corpus && cards && ws && out_idx && out_p && out_counts,
             "cc_audience_fp32: null pointer");
  CC_REQUIRE(V > 0 && cap >= 1, "cc_audience_fp32: bad V/cap");
  if (int rc = cc::infer_check_d(d, "cc_audience_fp32")) return rc;
  CC_REQUIRE(N >= 1 && N <= cap, "cc_audience_fp32: N must be 1..cap");
  CC_REQUIRE(T >= 0 && T <= MAX_T, "cc_audience_fp32: T outside 0..4096");
  CC_REQUIRE(k >= 1 && k <= MAX_K, "cc_audience_fp32: k must be 1..cc_audience_max_k()");
  CC_REQUIRE(chunk == 0 || (chunk > 0 && chunk % 64 == 0 && chunk <= MAX_CHUNK),
             "cc_audience_fp32: chunk must be 0 or a positive multiple of 64 up to 2^20");
  CC_REQUIRE(threshold >= 0.f && threshold <= 1.f, "cc_audience_fp32: threshold outside [0, 1]");
  CC_REQUIRE(((uintptr_t)ws & 255) == 0, "cc_audience_fp32: ws must be 256-byte aligned");
  CC_REQUIRE(((uintptr_t)corpus & 255) == 0, "cc_audience_fp32: corpus must be 256-byte aligned");
  const QueryWs w = query_ws(N, d, T, k, chunk);
  CC_REQUIRE((int64_t)w.chunks * k <= 0x7FFFFFFF, "cc_audience_fp32: k * chunks above 2^31 - 1, use a larger chunk");
  if (T == 0) return CC_OK;
  int64_t off[CC_NUM_TENSORS], sz[CC_NUM_TENSORS], tot, mt;
  if (int rc = cc::param_offsets(V, d, off, sz, &tot, &mt)) return rc;
  const float *Wo = params + off[14], *bo = params + off[15];
  const CorpusLayout x = corpus_layout(cap, d);
  const char *cb = (const char *)corpus;
  const float *h3 = (const float *)(cb + x.h3);
  const int32_t *ptr = (const int32_t *)(cb + x.ptr), *ids = (const int32_t *)(cb + x.ids);
  char *base = (char *)ws;
  float *wT = (float *)(base + w.wT), *bo_g = (float *)(base + w.bo);
  int32_t *card_g = (int32_t *)(base + w.card), *cnt = (int32_t *)(base + w.cnt);
  uint32_t *keys = (uint32_t *)(base + w.keys);
  uint64_t *cand = (uint64_t *)(base + w.cand);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(gather_cards_kernel, dim3((unsigned)cdiv((int64_t)d * w.Tp, GNT)), dim3(GNT), 0, s, Wo, bo,
                     d, V, T, w.Tp, cards, wT, bo_g, card_g, cnt, out_counts);
  CC_LAUNCH_CHECK("gather_cards_kernel");
  const int ntt = w.Tp / TC;
  const bool one_chunk = w.chunks == 1;  // its select writes the rows: no merge
  for (int c = 0; c < w.chunks; ++c) {
    const int c0 = (int)((int64_t)c * w.chunk), cl = std::min(w.chunk, N - c0);
    // at most 2^14 cube tiles x 64 card tiles
    hipLaunchKernelGGL(score_chunk_kernel, dim3((unsigned)(cdiv(cl, TR) * ntt)), dim3(ONT), 0, s, h3, ptr, ids, d,
                       c0, cl, (const float *)wT, (const float *)bo_g, (const int32_t *)card_g, T, w.Tp, ntt,
                       include_members ? 1 : 0, threshold, w.pitch, keys, cnt, out_counts);
    CC_LAUNCH_CHECK("score_chunk_kernel");
    if (one_chunk)
      hipLaunchKernelGGL(select_chunk_kernel<true>, dim3(T), dim3(SNT), 0, s, (const uint32_t *)keys, w.pitch, c0, cl,
                         cnt, k, c, w.chunks, cand, out_idx, out_p);
    else
      hipLaunchKernelGGL(select_chunk_kernel<false>, dim3(T), dim3(SNT), 0, s, (const uint32_t *)keys, w.pitch, c0,
                         cl, cnt, k, c, w.chunks, cand, out_idx, out_p);
    CC_LAUNCH_CHECK("select_chunk_kernel");
  }
  if (!one_chunk) {
    hipLaunchKernelGGL(merge_rows_kernel, dim3(T), dim3(SNT), 0, s, (const uint64_t *)cand, w.chunks, N,
                       (const int32_t *)out_counts, k, out_idx, out_p);
    CC_LAUNCH_CHECK("merge_rows_kernel");
  }
  return CC_OK;
}
