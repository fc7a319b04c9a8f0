// cc_complete_fp32 — greedy completion of R cubes to a target size, every pass bit-identical to
// cc_recommend_batch_fp32 / cc_recommend_batch_pool_fp32 on the cube as it stands.
//
// A pass is the batched select chain of recbatch.hip (row masks, gather, towers, output tile,
// topn_rows_kernel with amount = per_step) on the current CSR, then
//   grow_kernel : one workgroup per row folds the row's first take_r picks into its sorted ids and
//                 appends them to the row's results.  take_r = min(picks, target_r - n_r), 0 for a
//                 finished row (copied unchanged).  The new row_ptr is the old one plus the takes
//                 of the rows before (an integer sum every workgroup makes for itself: R is a few
//                 thousand at most).  An old id moves up by the picks below it (binary search of
//                 the picks, sorted in LDS); a pick lands at (old ids below it) + (picks below it).
// The CSR stays contiguous, as the chain's kernels read it: two CSR buffers in the workspace, pass
// t reads one (pass 0 the caller's) and grow_kernel writes the other.  All grids come from host
// sizes; nothing is read back between passes and no workgroup waits for another.
#include "common.hpp"
#include "infer.hpp"

namespace {

constexpr int GNT = 256;       // grow workgroup
constexpr int MAX_STEP = 256;  // picks per row and pass: one thread each, sorted in LDS

// n_added = 0 and the whole of added / added_vals -1 / 0.f: the unused tail of every row
__global__ __launch_bounds__(GNT) void complete_init_kernel(int A, int32_t *__restrict__ n_added,
                                                            int32_t *__restrict__ added,
                                                            float *__restrict__ added_vals) {
  const int r = blockIdx.x;
  if (threadIdx.x == 0) n_added[r] = 0;
  for (int i = threadIdx.x; i < A; i += GNT) {
    added[(int64_t)r * A + i] = -1;
    added_vals[(int64_t)r * A + i] = 0.f;
  }
}

// picks of row q that join it: never more than the pass selected, than per_step, or than the row
// has room for below min(target, max_n) (max_n: the pitch the CSR buffers were sized for)
__device__ __forceinline__ int take_of(int q, const int32_t *__restrict__ rp,
                                       const int32_t *__restrict__ n_add,
                                       const int32_t *__restrict__ target_n, int max_n,
                                       int per_step) {
  const int n = rp[q + 1] - rp[q];
  return max(0, min(min(n_add[q], per_step), min(target_n[q], max_n) - n));
}

__global__ __launch_bounds__(GNT) void grow_kernel(
    int R, int max_n, int per_step, const int32_t *__restrict__ rp_in,
    const int32_t *__restrict__ idx_in, const int32_t *__restrict__ target_n,
    const int32_t *__restrict__ n_add, const int32_t *__restrict__ picks,
    const float *__restrict__ pick_vals, int32_t *__restrict__ rp_out,
    int32_t *__restrict__ idx_out, int64_t idx_cap, int A, int32_t *__restrict__ n_added,
    int32_t *__restrict__ added, float *__restrict__ added_vals) {
  __shared__ int32_t s_pick[MAX_STEP], s_sorted[MAX_STEP];
  __shared__ int wsum[GNT / 64];
  const int tid = threadIdx.x;
  const int r = blockIdx.x;
  int before = 0;  // picks joining the rows before this one
  for (int q = tid; q < r; q += GNT) before += take_of(q, rp_in, n_add, target_n, max_n, per_step);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
  if ((tid & 63) == 0) wsum[tid >> 6] = before;
  const int beg = rp_in[r], n = rp_in[r + 1] - beg;
  const int take = take_of(r, rp_in, n_add, target_n, max_n, per_step);  // (block-uniform)
  const int had = n_added[r];
  if (tid < take) s_pick[tid] = picks[(int64_t)r * per_step + tid];
  __syncthreads();
  before = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  const int64_t nbeg = (int64_t)(beg - rp_in[0]) + before;
  if (tid == 0) {
    rp_out[r] = (int32_t)nbeg;
    if (r == R - 1) rp_out[R] = (int32_t)(nbeg + n + take);
    n_added[r] = had + take;
  }
  int mine = 0, below = 0;  // this thread's pick and the picks below it (ids are distinct)
  if (tid < take) {
    mine = s_pick[tid];
    for (int i = 0; i < take; ++i) below += s_pick[i] < mine ? 1 : 0;
    s_sorted[below] = mine;
  }
  __syncthreads();
  if (tid < take) {
    int lo = 0;  // old ids below the pick
    for (int hi = n; lo < hi;) {
      const int mid = (lo + hi) >> 1;
      if (idx_in[beg + mid] < mine) lo = mid + 1; else hi = mid;
    }
    const int64_t pos = nbeg + lo + below;
    if (pos < idx_cap) idx_out[pos] = mine;
    if (had + tid < A) {
      added[(int64_t)r * A + had + tid] = mine;
      added_vals[(int64_t)r * A + had + tid] = pick_vals[(int64_t)r * per_step + tid];
    }
  }
  for (int i = tid; i < n; i += GNT) {
    const int id = idx_in[beg + i];
    int lo = 0;  // picks below the old id
    for (int hi = take; lo < hi;) {
      const int mid = (lo + hi) >> 1;
      if (s_sorted[mid] < id) lo = mid + 1; else hi = mid;
    }
    const int64_t pos = nbeg + i + lo;
    if (pos < idx_cap) idx_out[pos] = id;
  }
}

// workspace: [the select chain's, with the pools' share][row_ptr R+1] x 2 [idx R*max_n] x 2
//            [cut values R*max_n (scratch)][n_add R][picks R*per_step][pick values R*per_step]
struct CompleteWs {
  size_t rp[2], ix[2], cuts, nadd, picks, pvals, total;
  size_t idx_cap;
};
CompleteWs complete_ws(int V, int d, int R, int max_n, int per_step) {
  CompleteWs w;
  const size_t r = (size_t)std::max(R, 1), ps = (size_t)std::max(per_step, 1);
  w.idx_cap = r * (size_t)std::max(max_n, 1);
  size_t o = align256(cc::batch_select_ws_bytes(V, d, R, max_n, true));
  for (int b = 0; b < 2; ++b) w.rp[b] = o, o += align256((r + 1) * sizeof(int32_t));
  for (int b = 0; b < 2; ++b) w.ix[b] = o, o += align256(w.idx_cap * sizeof(int32_t));
  w.cuts = o, o += align256(w.idx_cap * sizeof(float));
  w.nadd = o, o += align256(r * sizeof(int32_t));
  w.picks = o, o += align256(r * ps * sizeof(int32_t));
  w.pvals = o, o += align256(r * ps * sizeof(float));
  w.total = o;
  return w;
}

}  // namespace

extern "C" int32_t cc_complete_max_per_step(void) {
  return std::min(MAX_STEP, cc::batch_max_amount());
}

extern "C" size_t cc_complete_ws_size(int32_t V, int32_t d, int32_t R, int32_t max_n,
                                      int32_t per_step) {
  return complete_ws(V, d, R, max_n, per_step).total;
}

extern "C" int cc_complete_fp32(const float *params, int32_t V, int32_t d, int32_t R,
                                const int32_t *row_ptr, const int32_t *idx, int32_t max_n,
                                const int32_t *target_n, int32_t per_step, int32_t passes,
                                const uint32_t *pools, int32_t n_pools, const int32_t *pool_of_row,
                                int32_t A, int32_t *n_added, int32_t *added, float *added_vals,
                                void *ws, size_t ws_bytes, void *stream) {
  CC_REQUIRE(params && row_ptr && idx && target_n && n_added && added && added_vals && ws,
             "cc_complete_fp32: null pointer");
  if (int rc = cc::pools_check("cc_complete_fp32", pools, n_pools, pool_of_row, true)) return rc;
  CC_REQUIRE(V > 0 && R >= 0 && max_n >= 0 && max_n <= V && A >= 1,
             "cc_complete_fp32: V/R/max_n/A");
  if (int rc = cc::infer_check_d(d, "cc_complete_fp32")) return rc;
  CC_REQUIRE(per_step >= 1 && per_step <= cc_complete_max_per_step(),
             "cc_complete_fp32: per_step outside [1, cc_complete_max_per_step()]");
  CC_REQUIRE(passes >= 0, "cc_complete_fp32: passes is negative");
  CC_REQUIRE(((uintptr_t)ws & 255) == 0, "cc_complete_fp32: ws must be 256-byte aligned");
  const CompleteWs w = complete_ws(V, d, R, max_n, per_step);
  CC_REQUIRE(ws_bytes >= w.total, "cc_complete_fp32: workspace below cc_complete_ws_size()");
  if (R == 0 || passes == 0) return CC_OK;
  char *base = (char *)ws;
  int32_t *rp_buf[2] = {(int32_t *)(base + w.rp[0]), (int32_t *)(base + w.rp[1])};
  int32_t *ix_buf[2] = {(int32_t *)(base + w.ix[0]), (int32_t *)(base + w.ix[1])};
  float *cuts = (float *)(base + w.cuts), *pvals = (float *)(base + w.pvals);
  int32_t *nadd = (int32_t *)(base + w.nadd), *picks = (int32_t *)(base + w.picks);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(complete_init_kernel, dim3(R), dim3(GNT), 0, s, A, n_added, added, added_vals);
  CC_LAUNCH_CHECK("complete_init_kernel");
  const int32_t *rp = row_ptr, *ix = idx;
  for (int t = 0; t < passes; ++t) {
    if (int rc = cc::batch_select_launch(params, V, d, R, rp, ix, max_n, per_step, ws, nadd, picks,
                                         pvals, cuts, nullptr, pools, n_pools, pool_of_row, s))
      return rc;
    hipLaunchKernelGGL(grow_kernel, dim3(R), dim3(GNT), 0, s, R, max_n, per_step, rp, ix, target_n,
                       (const int32_t *)nadd, (const int32_t *)picks, (const float *)pvals,
                       rp_buf[t & 1], ix_buf[t & 1], (int64_t)w.idx_cap, A, n_added, added,
                       added_vals);
    CC_LAUNCH_CHECK("grow_kernel");
    rp = rp_buf[t & 1], ix = ix_buf[t & 1];
  }
  return CC_OK;
}
