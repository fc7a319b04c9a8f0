// What the two cosine-distance searches share (simbatch.hip: cards, cubesim.hip: cubes): the pinned
// normalisation and the key's way back to a distance.  The arithmetic is similarity.hip's: fp32,
// multiply and add separately rounded (detm::mulf / detm::addf), sums in index order.
#pragma once
#include "common.hpp"
#include "dottile.hpp"

namespace cosine {

__device__ __forceinline__ float inv_norm(float ss) { return 1.f / sqrtf(fmaxf(ss, 1e-12f)); }

// rowsort::orderable's inverse on distances: the only zero a distance takes is -0.0f (a distance
// is -dot with dot never -0)
__device__ __forceinline__ float dist_of_key(uint32_t key) {
  if (key == 0x80000000u) return __uint_as_float(0x80000000u);
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// K rounded up to the distance tile's k stage
inline int k_pad(int K) { return (int)cdiv(K > 1 ? K : 1, dottile::KS) * dottile::KS; }

}  // namespace cosine

namespace cc {
// simbatch.hip's normalise_kernel: rows of z [rows][K] -> n [n0 + r][Kp] (row-major) and
// nT [Kp][pitch] at column n0 + r (k-major), the k pad of the rows it writes as zeros
int normalise_rows_launch(const float *z, int rows, int K, int Kp, int pitch, int n0, float *n,
                          float *nT, hipStream_t s);
}  // namespace cc
