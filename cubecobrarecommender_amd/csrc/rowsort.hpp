// Workgroup primitives of the ranking kernels (recbatch.hip, simbatch.hip, graphrec.hip, topn.hip,
// similarity.hip): one row, one NT-thread workgroup of 64-lane waves.  Device only.
//
// Contract of everything below that takes NT: called by all NT threads of the block from uniform
// control flow (a barrier is inside); the LDS is the caller's (wtot: [NT / 64] ints, hist:
// [NT / 64][radix] words) and must not be in use by a thread that has not reached the call; on
// return every thread has passed a barrier behind the last LDS access, so the LDS is free again
// and the caller's own LDS / global writes from before the call are visible block-wide.
// wave_match needs the whole wave (ballots): lanes diverge only through `valid`.
//
// The three select kernels (topn_rows_kernel, select_rows_kernel, graph_topn_kernel) share the scan
// and the bitonic sort but stay separate kernels: they differ in direction, in the stop rule (exact
// want against "N or a few more, up to limit") and in width (64-bit composite against 64-bit key +
// card), and a common form needs more policy than it removes.
#pragma once
#include "common.hpp"

namespace rowsort {

// The one float-to-ascending-key map: ascending key == ascending float, -0 folded into +0.
__device__ __forceinline__ uint32_t orderable(float f) {
  uint32_t u = __float_as_uint(f == 0.f ? 0.f : f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Inclusive scan of one int per thread over the NT-thread block; wtot: [NT / 64] LDS scratch.
// Two barriers: wtot may be reused as soon as the call returns.
template <int NT>
__device__ __forceinline__ int block_incl_scan(int v, int *wtot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) wtot[w] = x;
  __syncthreads();
  int before = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; ++i) before += i < w ? wtot[i] : 0;
  __syncthreads();
  return before + x;
}

// The ballot multisplit: the valid lanes of the wave that hold digit dg (a value below 2^nbits).
// The bit count is wave-uniform: wave_match<8>(dg, valid) where the caller's own code fixes it (the
// loop then has a literal bound, as the per-file copies had), wave_match(dg, valid, nbits) where it
// is a value, constant-folded or not (no unroll pragma: a run-time count cannot honour it).
template <int BITS = 0>
__device__ __forceinline__ uint64_t wave_match(uint32_t dg, bool valid, int nbits = BITS) {
  uint64_t m = __ballot(valid);
  for (int bit = 0; bit < (BITS > 0 ? BITS : nbits); ++bit) {
    const bool b = (dg >> bit) & 1u;
    const uint64_t bb = __ballot(b);
    m &= b ? bb : ~bb;
  }
  return m;
}

// Bitonic network over positions [0, P) in LDS by the whole block; P a power of two, the entries
// written and a barrier passed before the call.  f(i, pr, down) compare-exchanges positions
// i < pr: the larger entry ends at i when down, at pr otherwise (so the result is descending; an
// f that does the opposite sorts ascending).  Every step ends with a barrier.
template <int NT, class CmpSwap>
__device__ __forceinline__ void bitonic_sort(int P, CmpSwap f) {
  const int tid = threadIdx.x;
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < P; i += NT) {
        const int pr = i ^ stride;
        if (pr > i) f(i, pr, (i & size) == 0);
      }
      __syncthreads();
    }
}
// 64-bit words: descending, or ascending.
template <bool DESC>
struct CmpSwapU64 {
  uint64_t *a;
  __device__ __forceinline__ void operator()(int i, int pr, bool down) const {
    const uint64_t x = a[i], y = a[pr];
    if ((DESC ? x < y : x > y) == down) {
      a[i] = y;
      a[pr] = x;
    }
  }
};

// Full ranking of one row of V items: a stable LSD radix sort, ascending, from the order pass 0
// loads them in.  Wave w owns a contiguous slice of the current arrangement; inside a wave the rank
// is the ballot multisplit, across waves the exclusive scan of the (digit, wave) counts in
// digit-major order: no atomics, one order on every run.  A lane loads RU items ahead of ranking
// them, so the loads' latency is paid once.  T supplies what differs between the rankings:
//   Item                      what moves (trivially copyable; Item{} stands in outside the slice)
//   PASSES, RADIX_BITS        passes; hist is [NT / 64][1 << RADIX_BITS], 1 << RADIX_BITS <= NT
//   bits(pass)                digit bits of the pass, <= RADIX_BITS
//   load(pass, i)             item i of the arrangement the pass reads (pass 0: the row's input)
//   digit(item, pass)         below 2^bits(pass)
//   store(pass, pos, item)    every pass but the last: item to position pos of the next arrangement
//   emit(pos, item)           the last pass: the item's final ascending position, nothing stored
// store and emit are called with pos < V only (pos >= V needs inconsistent counts: never written).
// Arrangements live in global memory: the fence and barrier behind each pass order a pass's stores
// before the next pass's loads.
template <int NT, int RU, class T>
__device__ __forceinline__ void radix_rank_row(const T &t, int V, uint32_t *hist, int *wtot) {
  constexpr int NW = NT / 64, R = 1 << T::RADIX_BITS;
  static_assert(R <= NT && R % 64 == 0, "a thread scans its digit's column");
  using Item = typename T::Item;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  const bool owner = R == NT || tid < R;  // of digit tid's column
  const int S = (int)cdiv(cdiv(V, NW), 64) * 64;  // per-wave slice
  const int lo = min(V, w * S), hi = min(V, lo + S);
  uint32_t *hw = hist + w * R;  // [wave][digit]
  for (int pass = 0; pass < T::PASSES; ++pass) {
    const bool last = pass == T::PASSES - 1;
    const int nbits = T::bits(pass);
#pragma unroll
    for (int i = 0; i < R / 64; ++i) hist[i * NT + tid] = 0u;  // NW * R words
    __syncthreads();
    for (int base0 = lo; base0 < hi; base0 += 64 * RU) {
      Item item[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        const int i = base0 + 64 * u + lane;
        item[u] = i < hi ? t.load(pass, i) : Item{};
      }
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        if (base0 + 64 * u >= hi) break;
        const bool valid = base0 + 64 * u + lane < hi;
        const uint32_t dg = t.digit(item[u], pass);
        const uint64_t m = wave_match(dg, valid, nbits);
        if (valid && (m & lt) == 0) hw[dg] += (uint32_t)__popcll(m);
      }
    }
    __syncthreads();
    {  // exclusive scan in (digit, wave) order
      uint32_t c[NW];
      int s = 0;
      if (owner) {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
          c[i] = hist[i * R + tid];
          s += (int)c[i];
        }
      }
      int off = block_incl_scan<NT>(s, wtot) - s;
      if (owner) {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
          hist[i * R + tid] = (uint32_t)off;
          off += (int)c[i];
        }
      }
    }
    __syncthreads();
    for (int base0 = lo; base0 < hi; base0 += 64 * RU) {
      Item item[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        const int i = base0 + 64 * u + lane;
        item[u] = i < hi ? t.load(pass, i) : Item{};
      }
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        if (base0 + 64 * u >= hi) break;
        const bool valid = base0 + 64 * u + lane < hi;
        const uint32_t dg = t.digit(item[u], pass);
        const uint64_t m = wave_match(dg, valid, nbits);
        const uint32_t basepos = hw[dg];
        const uint32_t pos = basepos + (uint32_t)__popcll(m & lt);
        if (valid && pos < (uint32_t)V) {
          if (last)
            t.emit(pos, item[u]);
          else
            t.store(pass, pos, item[u]);
        }
        if (valid && (m & lt) == 0) hw[dg] = basepos + (uint32_t)__popcll(m);
      }
    }
    __threadfence_block();
    __syncthreads();
  }
}

}  // namespace rowsort
