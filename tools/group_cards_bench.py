"""Archetype card profiles: cc_group_cards_count under its two paths beside two torch group-bys on
the same resident data, and cc_group_cards_top.

Workload: V = 22,000, cubes from synthetic.py's popularity-skewed generator (sizes 180..720, about
436 cards on average) as a CSR resident on the device, labels from a fixed seed; (N, G) =
(65,536, 256) and (2^20, 1,024).  The large corpus is the 65,536 generated cubes repeated 16 times
under fresh labels: generating is not what is measured, and the count's work per cube is the same.

1. Times (the default run).  Device time between two events on the stream, all rows alternating
   inside one run after two warm-up rounds, every repeat kept, with median and min..max:
     cc_group_cards_count at path 1 (privatised), 2 (direct) and 0 (chosen), accumulate = 0;
     cc_group_cards_top at m = 100 (lift);
     torch.bincount(label_of_entry * V + idx, minlength = G V), the key construction inside;
     torch.zeros(G V).scatter_add_(0, key, ones), the key construction inside.
   Both torch rows use the entries' labels prepared outside the timing (a repeat_interleave the
   library does not need), and their extra memory is reported beside the library's workspace.
   The bar: path 0 is no slower than the faster torch row at both shapes, their min..max ranges
   deciding where the medians do not.
   Reported beside it: bytes per second (nnz 4 + N 8 + G V 4 over the time) against 8 TB/s.
2. The crossing (same run): spans of 1,024 .. 65,536 cubes at G = 1,024, accumulate = 1, path 1
   against path 2: what the path 0 rule is taken from.
3. End to end at the small shape: groupcards.group_cards from host lists (packing, upload, count,
   top, copy back) beside np.add.at on the host, one run each.
4. `--trace-workload`: five count calls of each path and five top calls at the small shape, to be
   run under `rocprofv3 --kernel-trace --stats` (no counters).

    python tools/group_cards_bench.py [--repeats 7] [--out profiles/group_cards_bench.json]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/group_cards_bench.py --trace-workload
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V, M_TOP = 22000, 100
SHAPES = ((1 << 16, 256), (1 << 20, 1024))
SPANS = (1024, 4096, 16384, 65536)
HBM_BYTES_PER_S = 8e12


def spread(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'repeats': list(v)}


def event_ms(fns, repeats):
    """Device ms of each named call between two events, alternating; two warm-up rounds first."""
    import torch
    times = {name: [] for name in fns}
    for i in range(repeats + 2):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= 2:
                times[name].append(a.elapsed_time(b))
    return {name: spread(v) for name, v in times.items()}


class Corpus:
    """N cubes as a device CSR (the generated 65,536 repeated as often as it takes) and labels."""

    def __init__(self, base, N, G):
        import torch
        indptr, indices = base
        reps = N // (len(indptr) - 1)
        lens = torch.from_numpy(np.diff(indptr)).cuda().repeat(reps)
        self.N, self.G = N, G
        self.row_ptr = torch.zeros(N + 1, device='cuda', dtype=torch.int32)
        self.row_ptr[1:] = torch.cumsum(lens, 0)
        self.idx = torch.from_numpy(indices).cuda().repeat(reps)
        self.nnz = int(self.idx.numel())
        self.label = torch.from_numpy(np.random.default_rng(20250601 + G).integers(0, G, N).astype(np.int32)).cuda()
        self.lens = lens


class Native:
    """cc_group_cards_count / _top by direct calls on kept buffers."""

    def __init__(self, c):
        import torch
        from cubecobrarecommender_amd import _lib as L
        self.L, self.c = L, c
        self.ws_bytes = int(L.lib().cc_group_cards_ws_size(c.N, V, c.G, M_TOP))
        self.ws = torch.empty(self.ws_bytes // 4 + 64, device='cuda', dtype=torch.int32)
        self.count = torch.empty(c.G * V, device='cuda', dtype=torch.int32)
        self.size = torch.empty(c.G, device='cuda', dtype=torch.int32)
        self.total = torch.empty(V, device='cuda', dtype=torch.int32)
        self.cards = torch.empty(c.G * M_TOP, device='cuda', dtype=torch.int32)
        self.ccnt = torch.empty(c.G * M_TOP, device='cuda', dtype=torch.int32)
        self.found = torch.empty(c.G, device='cuda', dtype=torch.int32)

    def run(self, path, r0=0, r1=None, accumulate=0):
        import ctypes as C
        L, c = self.L, self.c
        r1 = c.N if r1 is None else r1
        L.call('cc_group_cards_count', C.c_void_p(c.row_ptr.data_ptr() + 4 * r0), L.ptr(c.idx), r1 - r0, V,
               C.c_void_p(c.label.data_ptr() + 4 * r0), c.G, accumulate, path, L.ptr(self.ws), L.ptr(self.count),
               L.ptr(self.size), L.ptr(self.total), L.stream_ptr())

    def top(self):
        L = self.L
        L.call('cc_group_cards_top', L.ptr(self.count), L.ptr(self.size), L.ptr(self.total), V, self.c.G, 1, 1, M_TOP,
               L.ptr(self.ws), L.ptr(self.cards), L.ptr(self.ccnt), L.ptr(self.found), L.stream_ptr())


def measure(base, N, G, repeats):
    import torch
    c = Corpus(base, N, G)
    nat = Native(c)
    entry_label = torch.repeat_interleave(c.label.long(), c.lens)          # outside the timing
    idx64_free = c.idx                                                       # int32: widened inside the key
    ones = torch.ones(c.nnz, device='cuda', dtype=torch.int32)
    keep = {}

    def bincount():
        keep['b'] = torch.bincount(entry_label * V + idx64_free, minlength=G * V)

    def scatter():
        keep['s'] = torch.zeros(G * V, device='cuda', dtype=torch.int32).scatter_add_(0, entry_label * V + idx64_free, ones)

    ms = event_ms({'count_path1': lambda: nat.run(1), 'count_path2': lambda: nat.run(2), 'count_path0': lambda: nat.run(0),
                   'top_m100': nat.top, 'torch_bincount': bincount, 'torch_scatter_add': scatter}, repeats)
    torch.cuda.synchronize()
    nat.run(0)
    torch.cuda.synchronize()
    assert bool((nat.count.long() == keep['b']).all()) and bool((nat.count == keep['s']).all())
    torch_rows = ('torch_bincount', 'torch_scatter_add')
    best = min(torch_rows, key=lambda r: ms[r]['median'])
    p0 = ms['count_path0']
    met = p0['median'] <= ms[best]['median'] or p0['min'] <= ms[best]['max']
    moved = c.nnz * 4 + N * 8 + G * V * 4
    out = {'N': N, 'G': G, 'V': V, 'nnz': c.nnz, 'ms': ms, 'faster_torch_row': best, 'bar_met': bool(met),
           'path0_bytes_per_s': moved / (p0['median'] * 1e-3),
           'path0_share_of_hbm': moved / (p0['median'] * 1e-3) / HBM_BYTES_PER_S,
           'extra_bytes': {'cc_group_cards_ws': nat.ws_bytes, 'torch_bincount': c.nnz * 8 * 2 + G * V * 8,
                           'torch_scatter_add': c.nnz * 8 * 2 + c.nnz * 4}}
    if G == SHAPES[-1][1]:
        spans = {}
        for rows in SPANS:
            t = event_ms({'path1': lambda: nat.run(1, 0, rows, 1), 'path2': lambda: nat.run(2, 0, rows, 1)}, repeats)
            spans[rows] = {k: {f: v[f] for f in ('median', 'min', 'max')} for k, v in t.items()}
        out['span_crossing_ms'] = spans
    line = ', '.join(f"{k} {v['median']:.3f} ({v['min']:.3f}..{v['max']:.3f})" for k, v in ms.items())
    print(f'N={N} G={G} nnz={c.nnz}: {line} ms; path 0 at {out["path0_share_of_hbm"]:.2%} of 8 TB/s; bar '
          f'{"met" if met else "MISSED"}', file=sys.stderr, flush=True)
    return out


def end_to_end(base, N, G):
    """group_cards from host lists beside np.add.at, host seconds, one run each."""
    from cubecobrarecommender_amd.groupcards import group_cards
    indptr, indices = base
    cubes = [indices[indptr[i]:indptr[i + 1]] for i in range(N)]
    label = np.random.default_rng(20250601 + G).integers(0, G, N).astype(np.int32)
    group_cards(cubes[:256], label[:256], V, M_TOP, G=G)                     # the library is loaded and warm
    t0 = time.perf_counter()
    res = group_cards(cubes, label, V, M_TOP, G=G, counts=True)
    t1 = time.perf_counter()
    table = np.zeros((G, V), np.int64)
    np.add.at(table, (np.repeat(label, np.diff(indptr)), indices), 1)
    t2 = time.perf_counter()
    assert np.array_equal(table, res.counts)
    return {'N': N, 'G': G, 'group_cards_s': t1 - t0, 'numpy_add_at_s': t2 - t1}


def trace_workload(base):
    import torch
    c = Corpus(base, *SHAPES[0])
    nat = Native(c)
    for _ in range(5):
        for path in (1, 2):
            nat.run(path)
        nat.top()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default='')
    ap.add_argument('--trace-workload', action='store_true')
    ap.add_argument('--shapes', type=int, default=len(SHAPES), help='the first so many shapes')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('group_cards_bench needs a GPU: nothing is measured without one')
    from cubecobrarecommender_amd.synthetic import synthetic_cubes
    base = synthetic_cubes(SHAPES[0][0], V, seed=20250601)
    if a.trace_workload:
        return trace_workload(base)
    if a.repeats < 7:
        raise SystemExit('at least 7 repeats')
    result = {'repeats': a.repeats, 'shapes': [measure(base, N, G, a.repeats) for N, G in SHAPES[:a.shapes]],
              'end_to_end': end_to_end(base, *SHAPES[0])}
    doc = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    print(doc)
    if not all(s['bar_met'] for s in result['shapes']):
        raise SystemExit('cc_group_cards_count at path 0 is slower than the faster torch group-by')


if __name__ == '__main__':
    main()
