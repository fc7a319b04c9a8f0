// The exact k-smallest select of the chunked searches (cubesim.hip, audience.hip): one 1,024-thread
// workgroup per row picks the `want` smallest 64-bit composites (key << 32 | id, unique per row) of
// a row of items and leaves them ascending in LDS.  Built on rowsort.hpp; device code but for
// chunk_plan, the host's split of the corpus.
//
// The scheme both searches share: the corpus is walked in chunks, a chunk's min(k, population)
// smallest composites are kept as the row's candidates with global ids, and the same select over
// the k * chunks candidates gives the row.  Every item is a candidate of exactly one chunk and a
// chunk keeps its k smallest, so the k smallest of the row are among the candidates whatever the
// chunk size; the composite order is total, so no output bit depends on the chunk.
#pragma once
#include "rowsort.hpp"

namespace rowsel {

constexpr int SNT = 1024;     // select workgroup
constexpr int MAX_K = 1024;   // results per row
constexpr int MAX_SEL = 2048; // survivors sorted in LDS
constexpr uint64_t NONE = ~0ull;  // no candidate: above every composite of a real key
constexpr int DEFAULT_CHUNK = 1 << 16;

// A search's walk over a corpus of N items: chunks of `chunk` items (0: the default), and the key
// rows' pitch: the chunk, or N rounded up to 64 where that is less.
struct ChunkPlan {
  int chunk, pitch, chunks;
};
inline ChunkPlan chunk_plan(int N, int chunk) {
  const int64_t n = N > 1 ? N : 1;
  ChunkPlan p;
  p.chunk = chunk > 0 ? chunk : DEFAULT_CHUNK;
  p.pitch = (int)(p.chunk < cdiv(n, 64) * 64 ? p.chunk : cdiv(n, 64) * 64);
  p.chunks = (int)cdiv(n, p.chunk);
  return p;
}

// The LDS of one select (select_rows_kernel's).
struct SelectLds {
  uint32_t hist[1024];
  int wtot[SNT / 64];
  uint64_t prefix, mask;
  int rem, done, cnt;
  uint64_t sel[MAX_SEL];
};

// The `want` smallest of the composites item(0..count) that are not NONE, ascending in s.sel[0..want);
// 1 <= want <= MAX_K and at most the number of such items.  id_max: no composite has a bit of its low
// word above id_max's.  select_rows_kernel's radix select (10-bit digits from the top, windows split
// at bit 32, stopping once the composites at or below the chosen bin fit the sort) and bitonic sort.
template <class Item>
__device__ __forceinline__ void select_smallest(SelectLds &s, const Item &item, int count, int want,
                                                uint32_t id_max) {
  const int tid = threadIdx.x;
  int PN = 1;
  while (PN < want) PN <<= 1;
  const int limit = min(MAX_SEL, 2 * PN);
  if (tid == 0) {
    s.prefix = 0;
    s.mask = 0;
    s.rem = want;
    s.done = 0;
    s.cnt = 0;
  }
  __syncthreads();
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = pass < 3 ? 54 - 10 * pass : pass == 3 ? 32 : pass < 7 ? 22 - 10 * (pass - 4) : 0;
    const uint32_t dmask = (pass == 3 || pass == 7) ? 3u : 1023u;
    if (shift < 32 && (id_max >> shift) == 0u) continue;  // no id has a bit up here
    if (s.done) break;
    const uint64_t prefix = s.prefix, mask = s.mask;
    const int rem = s.rem;
    s.hist[tid] = 0u;
    __syncthreads();
    for (int j = tid; j < count; j += SNT) {
      const uint64_t cmp = item(j);
      if (cmp != NONE && (cmp & mask) == prefix) atomicAdd(&s.hist[(uint32_t)(cmp >> shift) & dmask], 1u);
    }
    __syncthreads();
    // thread t owns bin t: its inclusive scan is the count of matching items in bins <= it
    const int v = (int)s.hist[tid];
    const int le = rowsort::block_incl_scan<SNT>(v, s.wtot), lt = le - v;
    if (le >= rem && lt < rem) {  // exactly one bin: the one holding the rem-th smallest
      s.prefix = prefix | ((uint64_t)tid << shift);
      s.mask = mask | ((uint64_t)dmask << shift);
      s.rem = rem - lt;
      s.done = (want - (rem - lt)) + v <= limit;  // everything at or below this bin: want or a few more
    }
    __syncthreads();
  }
  // the bits outside the mask are below every decided digit or zero in every composite: on the
  // decided bits, a candidate <=> at or below the prefix; all passes done, exactly `want` of them
  const uint64_t T = s.prefix, M = s.mask;
  for (int j = tid; j < count; j += SNT) {
    const uint64_t cmp = item(j);
    if (cmp != NONE && (cmp & M) <= T) {
      const int pos = atomicAdd(&s.cnt, 1);
      if (pos < limit) s.sel[pos] = cmp;
    }
  }
  __syncthreads();
  const int cnt = min(s.cnt, limit);  // (want <= cnt <= limit by the counts; never past sel)
  int P = PN;
  while (P < cnt) P <<= 1;
  for (int i = cnt + tid; i < P; i += SNT) s.sel[i] = NONE;
  __syncthreads();
  rowsort::bitonic_sort<SNT>(P, rowsort::CmpSwapU64<false>{s.sel});
}

// The first `want` entries of s.sel as a result row (the composite's id, value_of_key of its key),
// then the -1 / 0.f tail up to k.
template <class ValueOfKey>
__device__ __forceinline__ void write_row(const SelectLds &s, int want, int k, int32_t *oi, float *ov,
                                          ValueOfKey value_of_key) {
  for (int i = threadIdx.x; i < want; i += SNT) {
    const uint64_t cmp = s.sel[i];
    oi[i] = (int32_t)(uint32_t)cmp;
    ov[i] = value_of_key((uint32_t)(cmp >> 32));
  }
  for (int i = max(want, 0) + threadIdx.x; i < k; i += SNT) {
    oi[i] = -1;
    ov[i] = 0.f;
  }
}

// A row's candidates of all chunks, as the chunk selects stored them.
struct CandItem {
  const uint64_t *c;
  __device__ __forceinline__ uint64_t operator()(int j) const { return c[j]; }
};

}  // namespace rowsel
