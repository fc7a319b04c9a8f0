"""Diverse recommendations: Recommender.recommend_diverse_many against what a caller had to write
before it, and against the plain ranking it starts from.

Workload: V = 22,000, d = 256, R = 64 and 512 cubes of 180 distinct cards from a fixed seed, random
weights, the model's own card embeddings (K = 64); candidates M = 256 and the maximum; amount = 30
and 100; trade 0.7.
End to end on the host clock, every path ending with its results in host memory, alternating inside
one run after a warm-up of each; every repeat is kept, with median and min..max, in µs per row.
  (a) diverse    : `rec.recommend_diverse_many(cubes, amount, candidates=M)` (cc_recommend_diverse_fp32).
  (b) host_loop  : `rec.recommend_many(cubes, M)`, then the numpy loop of tests/diverse_ref.py per cube
                   on the embeddings in host memory.  The loop is host work only and slow, so it is
                   timed --host-repeats times (default 1); its recommend_many share is (c)'s.
  (c) plain      : `rec.recommend_many(cubes, M)` alone: what the re-rank is added to.
(a) and (b) are compared bit for bit.  No bar is set: the numbers are the result.
`device`: device ms between two events on the stream around one cc_recommend_diverse_fp32 call and
around one cc_recommend_batch_fp32 call at amount = M on the same rows (no host packing, no copies
back); their difference is the re-rank's share, and over `amount` the time per pick of a launch.
--only-a N runs path (a) N times at --rows / --candidates / --amount and nothing else: the run to
put under a kernel profiler.
One JSON document on stdout (and in --out).

    python tools/recommend_diverse_bench.py [--repeats 5] [--host-repeats 1] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cubecobrarecommender_amd import _lib as L                                   # noqa: E402
from cubecobrarecommender_amd.launches import upload, ws_elems                   # noqa: E402
from cubecobrarecommender_amd.recommender import pack_cubes                      # noqa: E402
from cubecobrarecommender_amd.similarity import card_embeddings                  # noqa: E402
from tests import diverse_ref                                                    # noqa: E402

V, D, CARDS, TRADE = 22000, 256, 180, 0.7
ROWS = (64, 512)
AMOUNTS = (30, 100)


def spread(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'repeats': list(v)}


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


def device_ms(rec, cubes, emb, amount, M, repeats):
    """Device ms of one cc_recommend_diverse_fp32 call and of one cc_recommend_batch_fp32 call at
    amount = M over `cubes`: two warm-up calls of each, then the repeats, alternating."""
    dev, lib = rec.dev, L.lib()
    row_ptr, idx, max_n, _, _ = pack_cubes(cubes, V)
    R, K = len(cubes), emb.shape[1]
    A = min(max(amount, 1), M)
    rp, ix = upload(row_ptr, dev), upload(idx, dev)
    ws = torch.empty(ws_elems(max(lib.cc_recommend_diverse_ws_size(V, D, R, max_n, M, K),
                                  lib.cc_recommend_batch_ws_size(V, D, R, max_n))), device=dev, dtype=torch.int32)
    nadd = torch.empty(R, device=dev, dtype=torch.int32)
    adds, rank = (torch.empty(R, M, device=dev, dtype=torch.int32) for _ in range(2))
    addv, red = (torch.empty(R, M, device=dev, dtype=torch.float32) for _ in range(2))
    cuts = torch.empty(len(idx), device=dev, dtype=torch.float32)

    def diverse():
        L.call('cc_recommend_diverse_fp32', L.ptr(rec.params), V, D, R, L.ptr(rp), L.ptr(ix), max_n, amount, M,
               TRADE, L.ptr(emb), K, None, 0, None, A, L.ptr(nadd), L.ptr(adds), L.ptr(addv), L.ptr(red),
               L.ptr(rank), L.ptr(cuts), L.ptr(ws), ws.numel() * 4, L.stream_ptr())

    def select():
        L.call('cc_recommend_batch_fp32', L.ptr(rec.params), V, D, R, L.ptr(rp), L.ptr(ix), max_n, M, L.ptr(ws),
               L.ptr(nadd), L.ptr(adds), L.ptr(addv), L.ptr(cuts), None, L.stream_ptr())
    times = {'diverse': [], 'select': []}
    for i in range(repeats + 2):
        for name, fn in (('diverse', diverse), ('select', select)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= 2:
                times[name].append(e0.elapsed_time(e1))
    rerank = [a - b for a, b in zip(times['diverse'], times['select'])]
    return {'diverse_ms': spread(times['diverse']), 'select_ms': spread(times['select']),
            'rerank_ms': spread(rerank), 'rerank_us_per_pick': spread([t * 1e3 / A for t in rerank])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-repeats', type=int, default=1)
    ap.add_argument('--only-a', type=int, default=0, metavar='N', help='run path (a) N times and nothing else')
    ap.add_argument('--rows', type=int, default=512, help='rows of the --only-a run')
    ap.add_argument('--candidates', type=int, default=0, help='candidates of the --only-a run (0: the maximum)')
    ap.add_argument('--amount', type=int, default=100, help='amount of the --only-a run')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('recommend_diverse_bench needs a GPU: nothing is measured without one')
    if (a.repeats < 3 or a.host_repeats < 1) and not a.only_a:
        raise SystemExit('at least 3 repeats and 1 host repeat')
    from cubecobrarecommender_amd.model import CC_Recommender
    rec = CC_Recommender(V, d=D, seed=1).recommender()
    top = int(L.lib().cc_recommend_diverse_max_candidates())
    rng = np.random.default_rng(20250601)
    cubes = [rng.choice(V, CARDS, replace=False) for _ in range(max(ROWS + (a.rows,)))]
    emb = card_embeddings(rec)
    emb_host = emb.cpu().numpy()
    if a.only_a:
        for _ in range(a.only_a):
            rec.recommend_diverse_many(cubes[:a.rows], a.amount, trade=TRADE, candidates=a.candidates or top)
        return
    result = {'V': V, 'd': D, 'K': int(emb.shape[1]), 'cards': CARDS, 'trade': TRADE, 'repeats': a.repeats,
              'host_repeats': a.host_repeats, 'max_candidates': top, 'unit': 'us per row', 'cases': []}
    for R in ROWS:
        for M in (256, top):
            for amount in AMOUNTS:
                rows = cubes[:R]
                first, times = timed({'diverse': lambda: rec.recommend_diverse_many(rows, amount, trade=TRADE,
                                                                                   candidates=M),
                                      'plain': lambda: rec.recommend_many(rows, M)}, a.repeats)
                loop = []
                for _ in range(a.host_repeats):
                    t0 = time.perf_counter()
                    want = diverse_ref.host_loop(first['plain'], emb_host, amount, TRADE)
                    loop.append(time.perf_counter() - t0)
                for got, (ids, vals, red, rank) in zip(first['diverse'], want):
                    assert np.array_equal(got['additions'], ids) and np.array_equal(got['base_rank'], rank), 'differ'
                    assert np.array_equal(got['add_vals'].view(np.uint32), vals.view(np.uint32)), 'the paths differ'
                    assert np.array_equal(got['redundancy'].view(np.uint32), red.view(np.uint32)), 'the paths differ'
                plain = statistics.median(times['plain'])
                per_row = lambda v: spread([t * 1e6 / R for t in v])             # noqa: E731
                case = {'rows': R, 'candidates': M, 'amount': amount, 'results_equal_bit_for_bit': True,
                        'diverse': per_row(times['diverse']), 'plain': per_row(times['plain']),
                        'host_loop_alone': per_row(loop), 'host_loop': per_row([plain + t for t in loop]),
                        'device': device_ms(rec, rows, emb, amount, M, a.repeats)}
                case['ratio_host_loop_over_diverse'] = case['host_loop']['median'] / case['diverse']['median']
                case['ratio_diverse_over_plain'] = case['diverse']['median'] / case['plain']['median']
                result['cases'].append(case)
                print(f"R {R} M {M} amount {amount}: us/row diverse {case['diverse']['median']:.1f}  plain "
                      f"{case['plain']['median']:.1f}  host loop {case['host_loop']['median']:.1f}; device ms diverse "
                      f"{case['device']['diverse_ms']['median']:.3f} select {case['device']['select_ms']['median']:.3f} "
                      f"({case['device']['rerank_us_per_pick']['median']:.2f} us per pick)", file=sys.stderr, flush=True)
    doc = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    print(doc)


if __name__ == '__main__':
    main()
