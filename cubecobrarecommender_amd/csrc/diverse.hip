// cc_recommend_diverse_fp32 — greedy maximal marginal relevance over every row's first M candidates
// (the definition is pinned in include/ccrec.h).
//
// The candidates are the batched select chain's (cc::batch_select_launch at amount = M, into the
// workspace: the same cards, order and bits as cc_recommend_batch_fp32), then
//   rerank_kernel : one workgroup per row, one thread per candidate position j.
//     stage   wave w copies the rows emb[c[j]] of candidates j = w, w + waves, ... into LDS k-major,
//             nT[k][j] with an odd pitch (M | 1): the global reads are one row of K floats per
//             instruction, the LDS writes (stride pitch) fall on distinct banks.  Then thread j
//             runs the index-order sum of squares down its column and scales it in place; the
//             k pad [K, Kp) is staged as zeros.
//     pick t  score = (lambda p) - (mu red) in thread j's registers; the argmax runs on one 64-bit
//             key per thread, (orderable(score) << 32) | (NONE - j): the greatest key is the
//             greatest score and, among equal scores (-0 == +0), the smallest j.  Four DPP steps
//             reduce a row of 16 lanes, four readlanes the wave; the waves' winners go through
//             LDS (two sets of slots, alternating by t: one barrier per pick) and every thread
//             reduces them from four 16-byte reads.
//     update  32 k at a time, lane l of every wave reads nT[k0 + (l & 31)][pick] once and the k loop
//             takes its value from that register by readlane (an SGPR operand); thread j reads its
//             own column (consecutive lanes, consecutive banks).  Kp separately rounded
//             multiply-adds in index order; red = dot if greater.
//   p, c, red and taken never leave the registers; nothing goes to global memory between picks
//   but the pick's four output words.
#include "common.hpp"
#include "cosine.hpp"
#include "detmath.hpp"
#include "infer.hpp"
#include "rowsort.hpp"

namespace {

constexpr int DNT = 512;         // the largest re-rank workgroup: one thread per candidate
constexpr int DNW = DNT / 64;
constexpr int MAX_CAND = DNT;
constexpr uint32_t NONE = 0x7FFFFFFFu;  // key 0: no candidate left (its j is never an index)

__host__ __device__ inline int pitch_of(int M) { return M | 1; }
// dynamic LDS: nT [Kp][pitch], then the waves' winning keys (64 bits) x 2 sets of DNW slots
__host__ __device__ inline size_t lds_words(int M, int Kp) {
  return (size_t)Kp * pitch_of(M) + 4 * DNW;
}
constexpr size_t LDS_MAX_WORDS = (size_t)64 * (MAX_CAND | 1) + 4 * DNW;  // 131,456 B of the CU's 160 KiB

__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }
// max with the lane a DPP control names (a permutation within a row of 16 lanes: every lane has a source)
template <int CTRL>
__device__ __forceinline__ uint64_t dpp_max(uint64_t k) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)k, CTRL, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(k >> 32), CTRL, 0xF, 0xF, false);
  return umax64(k, ((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ uint64_t lane_key(uint64_t k, int l) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(k >> 32), l) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)k, l);
}
// the wave's greatest key, in every lane (all 64 lanes take part)
__device__ __forceinline__ uint64_t wave_max(uint64_t k) {
  k = dpp_max<0xB1>(k);   // quad_perm [1,0,3,2]
  k = dpp_max<0x4E>(k);   // quad_perm [2,3,0,1]
  k = dpp_max<0x141>(k);  // row_half_mirror
  k = dpp_max<0x140>(k);  // row_mirror
  return umax64(umax64(lane_key(k, 0), lane_key(k, 16)), umax64(lane_key(k, 32), lane_key(k, 48)));
}

__global__ __launch_bounds__(DNT) void rerank_kernel(
    const float *__restrict__ emb, int V, int K, int Kp, int M, int amount, float lambda, float mu,
    const int32_t *__restrict__ cand_n, const int32_t *__restrict__ cand,
    const float *__restrict__ cand_p, int A, int32_t *__restrict__ n_add,
    int32_t *__restrict__ additions, float *__restrict__ add_vals, float *__restrict__ redundancy,
    int32_t *__restrict__ base_rank) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float dsm[];
  const int P = pitch_of(M);
  float *nT = dsm;
  uint64_t *slots = reinterpret_cast<uint64_t *>(dsm + (size_t)Kp * P);  // [2][DNW] (Kp * P is a multiple of 32 words)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
  const int r = blockIdx.x;
  const int cnt = min(min(max(cand_n[r], 0), M), (int)blockDim.x);  // (block-uniform)
  const int picks = min(min(max(amount, 1), cnt), A);
  if (tid == 0) n_add[r] = picks;
  if (cnt == 0) return;
  const int32_t *c_row = cand + (int64_t)r * M;
  const float *p_row = cand_p + (int64_t)r * M;

  if (tid < 2 * DNW) slots[tid] = 0;  // the slots of waves the launch does not have stay empty
  for (int j = w; j < cnt; j += nw) {
    const int32_t id = c_row[j];
    const bool ok = (uint32_t)id < (uint32_t)V;
    const float *e = emb + (int64_t)(ok ? id : 0) * K;
    for (int k = lane; k < Kp; k += 64) nT[k * P + j] = (ok && k < K) ? e[k] : 0.f;
  }
  __syncthreads();
  bool live = tid < cnt;  // this thread's candidate exists and is not taken
  int32_t cj = -1;
  float pj = 0.f, lp = 0.f, red = 0.f;
  if (live) {
    float *col = nT + tid;
    float ss = 0.f;
    for (int k = 0; k < K; ++k) ss = detm::addf(ss, detm::mulf(col[k * P], col[k * P]));
    const float inv = cosine::inv_norm(ss);
    for (int k = 0; k < K; ++k) col[k * P] = detm::mulf(col[k * P], inv);
    cj = c_row[tid];
    pj = p_row[tid];
    lp = detm::mulf(lambda, pj);
  }
  __syncthreads();

  for (int t = 0; t < picks; ++t) {
    const float score = detm::addf(lp, -detm::mulf(mu, red));
    uint64_t key = live ? ((uint64_t)rowsort::orderable(score) << 32) | (NONE - (uint32_t)tid) : 0;
    key = wave_max(key);
    uint64_t *slot = slots + (t & 1) * DNW;
    if (lane == 0) slot[w] = key;
    __syncthreads();
    const ulonglong2 *s2 = reinterpret_cast<const ulonglong2 *>(slot);
    const ulonglong2 a = s2[0], b = s2[1], c = s2[2], d = s2[3];
    key = umax64(umax64(umax64(a.x, a.y), umax64(b.x, b.y)), umax64(umax64(c.x, c.y), umax64(d.x, d.y)));
    const int pick = (int)(NONE - (uint32_t)key);  // (block-uniform)
    if (key == 0 || (uint32_t)pick >= (uint32_t)cnt) break;  // nothing left: cannot happen with picks <= cnt
    if (tid == pick) {
      const int64_t o = (int64_t)r * A + t;
      additions[o] = cj;
      add_vals[o] = pj;
      redundancy[o] = red;
      base_rank[o] = pick;
      live = false;
    }
    // a wave with a candidate left runs the update with all 64 lanes (readlane reads any lane's
    // register, so no lane may skip the load of pv); a lane without one works on column 0
    if (t + 1 < picks && __ballot(live) != 0) {
      const float *col = nT + (live ? tid : 0), *pc = nT + pick;
      float dot = 0.f;
      for (int k0 = 0; k0 < Kp; k0 += 32) {
        const float pv = pc[(k0 + (lane & 31)) * P];
#pragma unroll
        for (int kk = 0; kk < 32; ++kk)
          dot = detm::addf(dot, detm::mulf(col[(k0 + kk) * P],
                                           __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pv), kk))));
      }
      if (live && dot > red) red = dot;
    }
  }
}

// workspace: [the select chain's, with the pools' share][candidate counts R][candidates R*M]
//            [their probabilities R*M]
struct DiverseWs {
  size_t ncand, cand, vals, total;
};
DiverseWs diverse_ws(int V, int d, int R, int max_n, int M) {
  DiverseWs w;
  const size_t r = (size_t)std::max(R, 1), m = (size_t)std::max(M, 1);
  size_t o = align256(cc::batch_select_ws_bytes(V, d, R, max_n, true));
  w.ncand = o, o += align256(r * sizeof(int32_t));
  w.cand = o, o += align256(r * m * sizeof(int32_t));
  w.vals = o, o += align256(r * m * sizeof(float));
  w.total = o;
  return w;
}

}  // namespace

extern "C" int32_t cc_recommend_diverse_max_candidates(void) {
  return std::min(MAX_CAND, cc::batch_max_amount());
}

extern "C" size_t cc_recommend_diverse_ws_size(int32_t V, int32_t d, int32_t R, int32_t max_n,
                                               int32_t M, int32_t K) {
  (void)K;  // the embeddings are staged in LDS: no workspace depends on their width
  return diverse_ws(V, d, R, max_n, M).total;
}

extern "C" int cc_recommend_diverse_fp32(const float *params, int32_t V, int32_t d, int32_t R,
                                         const int32_t *row_ptr, const int32_t *idx, int32_t max_n,
                                         int32_t amount, int32_t M, float lambda, const float *emb,
                                         int32_t K, const uint32_t *pools, int32_t n_pools,
                                         const int32_t *pool_of_row, int32_t A, int32_t *n_add,
                                         int32_t *additions, float *add_vals, float *redundancy,
                                         int32_t *base_rank, float *cut_vals, void *ws,
                                         size_t ws_bytes, void *stream) {
  CC_REQUIRE(params && row_ptr && idx && emb && n_add && additions && add_vals && redundancy &&
                 base_rank && cut_vals && ws,
             "cc_recommend_diverse_fp32: null pointer");
  if (int rc = cc::pools_check("cc_recommend_diverse_fp32", pools, n_pools, pool_of_row, true)) return rc;
  CC_REQUIRE(V > 0 && R >= 0 && max_n >= 0 && max_n <= V && K >= 1,
             "cc_recommend_diverse_fp32: V/R/max_n/K");
  if (int rc = cc::infer_check_d(d, "cc_recommend_diverse_fp32")) return rc;
  CC_REQUIRE(lambda >= 0.f && lambda <= 1.f, "cc_recommend_diverse_fp32: lambda outside [0, 1]");
  CC_REQUIRE(M >= 1 && M <= cc_recommend_diverse_max_candidates(),
             "cc_recommend_diverse_fp32: M outside [1, cc_recommend_diverse_max_candidates()]");
  const int Kp = cosine::k_pad(K);
  CC_REQUIRE(lds_words(M, Kp) <= LDS_MAX_WORDS,
             "cc_recommend_diverse_fp32: M candidates of K floats do not fit the LDS tile");
  CC_REQUIRE(A >= std::min(std::max(amount, 1), M),
             "cc_recommend_diverse_fp32: A below min(max(amount, 1), M)");
  CC_REQUIRE(((uintptr_t)ws & 255) == 0, "cc_recommend_diverse_fp32: ws must be 256-byte aligned");
  const DiverseWs w = diverse_ws(V, d, R, max_n, M);
  CC_REQUIRE(ws_bytes >= w.total,
             "cc_recommend_diverse_fp32: workspace below cc_recommend_diverse_ws_size()");
  if (R == 0) return CC_OK;
  static const bool attr =
      hipFuncSetAttribute((const void *)rerank_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(LDS_MAX_WORDS * 4)) == hipSuccess;
  CC_REQUIRE(attr, "cc_recommend_diverse_fp32: dynamic LDS attribute");
  char *base = (char *)ws;
  int32_t *ncand = (int32_t *)(base + w.ncand), *cand = (int32_t *)(base + w.cand);
  float *vals = (float *)(base + w.vals);
  hipStream_t s = as_stream(stream);
  if (int rc = cc::batch_select_launch(params, V, d, R, row_ptr, idx, max_n, M, ws, ncand, cand,
                                       vals, cut_vals, nullptr, pools, n_pools, pool_of_row, s))
    return rc;
  const int nt = (int)cdiv(M, 64) * 64;
  hipLaunchKernelGGL(rerank_kernel, dim3(R), dim3(nt), lds_words(M, Kp) * 4, s, emb, V, K, Kp, M,
                     amount, lambda, 1.f - lambda, (const int32_t *)ncand, (const int32_t *)cand,
                     (const float *)vals, A, n_add, additions, add_vals, redundancy, base_rank);
  CC_LAUNCH_CHECK("rerank_kernel");
  return CC_OK;
}
