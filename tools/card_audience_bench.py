"""Card audience: CubeCorpus.audience against what the code base offered before it.

Workload: V = 22,000; d = 512 and 256; N = 65,536 synthetic cubes of 360 distinct cards (one card
from each of 360 strata of 61 ids, fixed seed), random weights; T = 64 cards; k = 100.
End to end on the host clock, every path ending with its results in host memory, alternating
inside one run after a warm-up of each; every repeat is kept, with median and min..max.
  (a) audience        : `corpus.audience(cards, k)` over the resident corpus of all N cubes.
  (b) recommend_many  : `rec.recommend_many(slice, 1, want_probs=True)`, the asked columns picked on
                        the host, the cubes that hold the card left out, np.lexsort per card.  Measured
                        on a --slice cube slice and SCALED linearly to N (the full run would copy
                        N x V floats, 5.8 GB): `scaled_s` is labelled as such.
  (c) leave_one_out   : `rec.leave_one_out(slice, targets=cards)`, whose 'base' rows are the same
                        numbers; measured on --loo-slice cubes, scaled the same way.
On the slices the three paths' values are compared bit for bit (a corpus of the slice alone).
The bar: (a)'s median is at most one tenth of (b)'s scaled median: (b) computes all V output columns
(344 times the dots at T = 64) and copies R x V floats, so a factor of 10 leaves room for host
overhead that does not depend on the kernels.
Reported without a bar: `launch_ms`, the device time of one cc_audience_fp32 call between two events
on the stream, with the h3 bytes/s and multiply + add lane-ops/s it amounts to beside the two derived
floors (134 MB of h3 at 5 TB/s; 2 N d T separately rounded VALU lane-ops at 78.6 T/s); the build
time of the corpus; and one N = 2^20 run at d = 256 (the 65,536 cubes put 16 times) with its
workspace bytes beside T x N x 4.
One JSON document on stdout (and in --out).

    python tools/card_audience_bench.py [--repeats 7] [--out FILE]
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
from cubecobrarecommender_amd.audience import CubeCorpus                         # noqa: E402
from cubecobrarecommender_amd.launches import upload, ws_elems                   # noqa: E402
from cubecobrarecommender_amd.recommender import pack_cubes                      # noqa: E402

V, N, CARDS, T, K = 22000, 65536, 360, 64, 100
HBM_BYTES_PER_S, VALU_LANE_OPS_PER_S = 5.0e12, 256 * 4 * 32 * 2.4e9


def spread(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'repeats': list(v)}


def synthetic(n, seed):
    """[n, 360] sorted distinct card ids: one from each stratum of V // 360 ids."""
    width = V // CARDS
    rng = np.random.default_rng(seed)
    return (np.arange(CARDS, dtype=np.int64) * width)[None, :] + rng.integers(0, width, (n, CARDS))


def by_recommend_many(rec, cubes, cards, k):
    """(cubes [T, k], probs [T, k]) of the slice through the batched recommend path."""
    rows = rec.recommend_many(cubes, 1, want_probs=True)
    p = np.stack([r['probs'][cards] for r in rows])                # [S, T]
    member = np.stack([np.isin(cards, c) for c in cubes])
    ids = np.arange(len(cubes))
    out_i, out_p = np.full((len(cards), k), -1, np.int32), np.zeros((len(cards), k), np.float32)
    for t in range(len(cards)):
        ci, cp = ids[~member[:, t]], p[~member[:, t], t]
        order = np.lexsort((ci, -cp))[:k]
        out_i[t, :len(order)], out_p[t, :len(order)] = ci[order], cp[order]
    return out_i, out_p


def by_leave_one_out(rec, cubes, cards):
    """p [S, T]: the base rows."""
    return np.stack([o['base'] for o in rec.leave_one_out(cubes, targets=cards)])


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


def launch_ms(corpus, cards, k, repeats):
    """Device ms of one cc_audience_fp32 call: two warm-up calls, then the repeats."""
    rec, dev, n = corpus.rec, corpus.dev, len(corpus)
    ws_bytes = int(L.lib().cc_audience_ws_size(n, rec.d, len(cards), k, 0))
    ws = torch.empty(ws_elems(ws_bytes), device=dev, dtype=torch.int32)
    c_d = upload(np.asarray(cards, np.int32), dev)
    idx = torch.empty(len(cards), k, device=dev, dtype=torch.int32)
    p = torch.empty(len(cards), k, device=dev, dtype=torch.float32)
    cnt = torch.empty(len(cards), 3, device=dev, dtype=torch.int32)
    times = []
    for i in range(repeats + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.call('cc_audience_fp32', L.ptr(rec.params), rec.V, rec.d, L.ptr(corpus._buf), corpus.capacity, n, len(cards),
               L.ptr(c_d), k, 0, 0, 0.5, L.ptr(ws), L.ptr(idx), L.ptr(p), L.ptr(cnt), L.stream_ptr())
        e1.record()
        e1.synchronize()
        if i >= 2:
            times.append(e0.elapsed_time(e1))
    s = statistics.median(times) * 1e-3
    return {'ms': spread(times), 'workspace_bytes': ws_bytes, 'keys_if_T_x_N_bytes': len(cards) * n * 4,
            'h3_bytes_per_s': n * rec.d * 4 / s, 'h3_floor_us': n * rec.d * 4 / HBM_BYTES_PER_S * 1e6,
            'lane_ops_per_s': 2 * n * rec.d * len(cards) / s,
            'valu_floor_us': 2 * n * rec.d * len(cards) / VALU_LANE_OPS_PER_S * 1e6}


def run(d, a, cubes, cards):
    from cubecobrarecommender_amd.model import CC_Recommender
    rec = CC_Recommender(V, d=d, seed=1).recommender()
    t0 = time.perf_counter()
    corpus = CubeCorpus(rec, cubes)
    build_s = time.perf_counter() - t0
    part, loo_part = list(cubes[:a.slice]), list(cubes[:a.loo_slice])
    first, times = timed({'audience': lambda: corpus.audience(cards, K),
                          'recommend_many': lambda: by_recommend_many(rec, part, cards, K)}, a.repeats)
    loo_first, loo_times = timed({'leave_one_out': lambda: by_leave_one_out(rec, loo_part, cards)}, a.loo_repeats)
    # the slices' values, bit for bit: a corpus of the slice alone
    small = CubeCorpus(rec, part).audience(cards, K)
    want_i, want_p = first['recommend_many']
    assert np.array_equal(small['cubes'], want_i) and np.array_equal(small['probs'].view(np.uint32),
                                                                    want_p.view(np.uint32)), 'the paths differ'
    every = CubeCorpus(rec, loo_part).audience(cards, min(a.loo_slice, 1024), include_members=True)
    base = loo_first['leave_one_out']
    for t in range(len(cards)):
        assert np.array_equal(every['probs'][t].view(np.uint32),
                              base[every['cubes'][t], t].view(np.uint32)), 'leave_one_out differs'
    med = statistics.median
    result = {'d': d, 'build_s_per_65536_cubes': build_s * 65536 / len(cubes),
              'audience_s': spread(times['audience']),
              'recommend_many_slice_s': spread(times['recommend_many']), 'slice': a.slice,
              'recommend_many_scaled_s': med(times['recommend_many']) * len(cubes) / a.slice,
              'leave_one_out_slice_s': spread(loo_times['leave_one_out']), 'loo_slice': a.loo_slice,
              'leave_one_out_scaled_s': med(loo_times['leave_one_out']) * len(cubes) / a.loo_slice,
              'scaled': 'the two baselines are measured on their slices and scaled linearly to N',
              'values_equal_bit_for_bit': True,
              'launch': launch_ms(corpus, cards, K, a.repeats)}
    result['speedup_over_recommend_many_scaled'] = result['recommend_many_scaled_s'] / med(times['audience'])
    result['bar_met'] = med(times['audience']) * 10 <= result['recommend_many_scaled_s']
    print(f"d = {d}: audience {med(times['audience']) * 1e3:.2f} ms, recommend_many (scaled) "
          f"{result['recommend_many_scaled_s']:.2f} s, leave_one_out (scaled) {result['leave_one_out_scaled_s']:.2f} s, "
          f"launch {result['launch']['ms']['median']:.3f} ms", file=sys.stderr, flush=True)
    return result, rec


def run_large(rec, cubes, cards, repeats):
    """N = 2^20: the 65,536 cubes put 16 times (one packing)."""
    row_ptr, idx, _, _, _ = pack_cubes(cubes, V)
    times = 16
    corpus = CubeCorpus(rec, capacity=times * len(cubes), card_capacity=times * len(idx))
    t0 = time.perf_counter()
    for _ in range(times):
        corpus._append(row_ptr, idx, 4096)
    build_s = time.perf_counter() - t0
    secs = []
    for i in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = corpus.audience(cards, K)
        if i:
            secs.append(time.perf_counter() - t0)
    assert np.all(out['found'] == K)
    return {'d': rec.d, 'N': len(corpus), 'put_s': build_s, 'audience_s': spread(secs),
            'launch': launch_ms(corpus, cards, K, repeats)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--loo-repeats', type=int, default=3)
    ap.add_argument('--slice', type=int, default=4096, help='cubes of the recommend_many baseline')
    ap.add_argument('--loo-slice', type=int, default=256, help='cubes of the leave_one_out baseline')
    ap.add_argument('--cubes', type=int, default=N)
    ap.add_argument('--no-large', action='store_true', help='skip the N = 2^20 run')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('card_audience_bench needs a GPU: nothing is measured without one')
    if a.repeats < 7:
        raise SystemExit('at least 7 repeats')
    cubes = synthetic(a.cubes, 20250401)
    cards = np.random.default_rng(7).choice(V, T, replace=False)
    result = {'V': V, 'N': a.cubes, 'cards_per_cube': CARDS, 'T': T, 'k': K, 'repeats': a.repeats, 'runs': []}
    rec = None
    for d in (512, 256):
        r, rec = run(d, a, cubes, cards)
        result['runs'].append(r)
    if not a.no_large:
        result['large'] = run_large(rec, cubes, cards, 3)
    result['bar_met'] = all(r['bar_met'] for r in result['runs'])
    doc = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    print(doc)
    if not result['bar_met']:
        raise SystemExit('audience is not ten times faster than recommend_many scaled to N')


if __name__ == '__main__':
    main()
