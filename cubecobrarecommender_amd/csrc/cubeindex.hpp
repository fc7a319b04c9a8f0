// What the kernels over a cube index share (cubesim.hip: neighbours, cubecluster.hip: archetypes):
// the index's layout and the kernel that turns a call's queries into normalised rows.
#pragma once
#include <algorithm>

#include "common.hpp"
#include "cosine.hpp"
#include "detmath.hpp"

namespace cubeindex {

constexpr int QNT = 64;  // query rows: one thread each
constexpr int MAX_Q = 1 << 22;

inline int cap_pitch(int cap) { return (int)cdiv(std::max(cap, 1), 64) * 64; }

// index: [n cap*Kp][nT Kp*caps]
struct IndexLayout {
  size_t n, nT, total;
  int Kp, caps;
};
inline IndexLayout index_layout(int cap, int K) {
  IndexLayout x;
  x.Kp = cosine::k_pad(K);
  x.caps = cap_pitch(cap);
  size_t o = 0;
  x.n = o, o += align256((size_t)std::max(cap, 1) * x.Kp * sizeof(float));
  x.nT = o, o += align256((size_t)x.Kp * x.caps * sizeof(float));
  x.total = o;
  return x;
}

// Query r (one workgroup each): the index row qid[r] (0 <= qid[r] < N), else the raw embedding
// zq[r] (a negative or absent id, zq given), else none.
static __global__ __launch_bounds__(QNT) void query_rows_kernel(const float *__restrict__ n, int N, int K, int Kp,
                                                                const int32_t *__restrict__ qid,
                                                                const float *__restrict__ zq,
                                                                float *__restrict__ qn, int32_t *__restrict__ qok) {
  using detm::addf;
  using detm::mulf;
  __shared__ float stage[QNT];
  __shared__ float s_inv;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int id = qid ? qid[r] : -1;  // (block-uniform, as is every branch below)
  float *out = qn + (int64_t)r * Kp;
  if ((uint32_t)id < (uint32_t)N) {
    const float *src = n + (int64_t)id * Kp;
    for (int i = tid; i < Kp; i += QNT) out[i] = src[i];
  } else if (id < 0 && zq) {
    const float *e = zq + (int64_t)r * K;
    float ss = 0.f;  // thread 0's: the pinned order is sequential
    for (int k0 = 0; k0 < K; k0 += QNT) {
      __syncthreads();  // the previous stage is summed
      if (k0 + tid < K) stage[tid] = e[k0 + tid];
      __syncthreads();
      if (tid == 0)
        for (int c = 0; c < min(QNT, K - k0); ++c) ss = addf(ss, mulf(stage[c], stage[c]));
    }
    if (tid == 0) s_inv = cosine::inv_norm(ss);
    __syncthreads();
    const float inv = s_inv;
    for (int i = tid; i < Kp; i += QNT) out[i] = i < K ? mulf(e[i], inv) : 0.f;
  }
  if (tid == 0) qok[r] = ((uint32_t)id < (uint32_t)N || (id < 0 && zq)) ? 1 : 0;
}

}  // namespace cubeindex
