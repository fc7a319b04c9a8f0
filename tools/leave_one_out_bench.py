"""Leave-one-out scores: Recommender.leave_one_out against the only other way to the same numbers.

Workload: V = 22,000, d = 512, 64 cubes of 360 distinct cards from a fixed seed, random weights.
End to end on the host clock, both paths ending with the results in host memory, alternating inside
one run after a warm-up of each; every repeat is kept, with median and min..max.
  (a) leave_one_out    : `rec.leave_one_out(cubes)` in self mode (cc_leave_one_out_fp32).
  (b) derived_cubes    : the n cubes-without-one-card built on the host,
                         `rec.recommend_many(derived, 0, want_probs=True)` over them, and the
                         diagonal read off the n x V probabilities.
The first results are compared bit for bit.  The bar: (a)'s median is below (b)'s.
`launch_ms`: device time of one cc_leave_one_out_fp32 call over --launch-cubes cubes between two
events on the stream (no host packing, no copies back).
--only-a N runs path (a) N times and nothing else: the run to put under a kernel profiler for the
share of tower_kernel.
One JSON document on stdout (and in --out).

    python tools/leave_one_out_bench.py [--repeats 7] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cubecobrarecommender_amd import _lib as L                                   # noqa: E402
from cubecobrarecommender_amd.launches import upload, ws_elems                   # noqa: E402
from cubecobrarecommender_amd.leaveoneout import Plan                            # noqa: E402

V, D, CUBES, CARDS = 22000, 512, 64, 360


def spread(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'repeats': list(v)}


def derived_cubes(cube):
    u = np.unique(cube)
    return u, [np.delete(u, j) for j in range(len(u))]


def path_b(rec, cubes):
    """Per cube, p(c | cube without c) in sorted card order through the batched recommend path."""
    out = []
    for cube in cubes:
        u, derived = derived_cubes(cube)
        rows = rec.recommend_many(derived, 0, want_probs=True)
        out.append(np.array([rows[j]['probs'][u[j]] for j in range(len(u))], np.float32))
    return out


def timed(fns, repeats):
    """Seconds per call of each named function, alternating; one warm-up call of each first, whose
    results are returned."""
    first = {name: fn() for name, fn in fns.items()}
    times = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    return first, times


def launch_ms(rec, cubes, repeats):
    """Device ms of one cc_leave_one_out_fp32 call over `cubes` (self mode): two warm-up calls, then
    the repeats."""
    plan = Plan(cubes, None, V, 10 ** 9)
    a = plan.arrays(0)
    dev = rec.dev
    t = {k: upload(a[k], dev) for k in ('row_ptr', 'idx', 'row_cube', 'row_pos', 'out_ptr')}
    ws = torch.empty(ws_elems(L.lib().cc_leave_one_out_ws_size(V, D, a['n_cubes'], a['max_n'], a['rows'])),
                     device=dev, dtype=torch.int32)
    out = torch.empty(int(a['out_ptr'][-1]), device=dev, dtype=torch.float32)
    times = []
    for i in range(repeats + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.call('cc_leave_one_out_fp32', L.ptr(rec.params), V, D, a['n_cubes'], L.ptr(t['row_ptr']), L.ptr(t['idx']),
               a['max_n'], a['rows'], L.ptr(t['row_cube']), L.ptr(t['row_pos']), None, None, L.ptr(t['out_ptr']),
               L.ptr(out), L.ptr(ws), ws.numel() * 4, L.stream_ptr())
        e1.record()
        e1.synchronize()
        if i >= 2:
            times.append(e0.elapsed_time(e1))
    return {'cubes': len(cubes), 'rows': a['rows'], 'ms': spread(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--launch-cubes', type=int, default=11, help='cubes of the device-timed launch (3971 rows)')
    ap.add_argument('--only-a', type=int, default=0, metavar='N', help='run path (a) N times and nothing else')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('leave_one_out_bench needs a GPU: nothing is measured without one')
    if a.repeats < 7 and not a.only_a:
        raise SystemExit('at least 7 repeats')
    from cubecobrarecommender_amd.model import CC_Recommender
    rec = CC_Recommender(V, d=D, seed=1).recommender()
    rng = np.random.default_rng(20250301)
    cubes = [rng.choice(V, CARDS, replace=False) for _ in range(CUBES)]
    if a.only_a:
        for _ in range(a.only_a):
            rec.leave_one_out(cubes)
        return
    rows = CUBES * (CARDS + 1)
    first, times = timed({'leave_one_out': lambda: rec.leave_one_out(cubes),
                          'derived_cubes': lambda: path_b(rec, cubes)}, a.repeats)
    for cube, got, want in zip(cubes, first['leave_one_out'], first['derived_cubes']):
        assert np.array_equal(got['loo_vals'], want[np.searchsorted(np.unique(cube), cube)]), 'the paths differ'
    result = {'V': V, 'd': D, 'cubes': CUBES, 'cards': CARDS, 'derived_rows': rows, 'repeats': a.repeats,
              'values_equal_bit_for_bit': True,
              'us_per_cube': {k: spread([t * 1e6 / CUBES for t in v]) for k, v in times.items()},
              'us_per_derived_row': {k: spread([t * 1e6 / rows for t in v]) for k, v in times.items()},
              'launch_ms': launch_ms(rec, cubes[:a.launch_cubes], a.repeats)}
    med = {k: v['median'] for k, v in result['us_per_cube'].items()}
    result['bar_met'] = med['leave_one_out'] < med['derived_cubes']
    print(f"us/cube: leave_one_out {med['leave_one_out']:.1f}  derived cubes {med['derived_cubes']:.1f}  "
          f"(x{med['derived_cubes'] / med['leave_one_out']:.1f})", file=sys.stderr, flush=True)
    doc = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    print(doc)
    if not result['bar_met']:
        raise SystemExit('leave_one_out is not faster than recommend_many over the derived cubes')


if __name__ == '__main__':
    main()
