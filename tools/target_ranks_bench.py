"""Held-out evaluation throughput: positions of hidden cards by sorting every row vs by counting.

Workload: V = 20,884, d = 512, cubes of 360-540 cards from a fixed seed, 20 % of each cube hidden,
R in {64, 512, 4096}.  Modes (cubes/s, wall clock including the host-side packing and look-ups):
  sort  : Recommender.recommend_many(visible, 30000) (every card of every row sorted on the device,
          R x V additions and values copied back) + a host look-up of the hidden cards' positions
  count : Recommender.target_ranks(visible, hidden)
`sort` uses only API older than target_ranks, so the same file run with ``--modes sort`` on an older
tree gives the baseline.  Each repeat visits the modes in turn (alternating), after a warm-up of
every mode; the table reports the median and the min..max spread of the repeats.  The two modes'
ranks are compared once per R (they must be equal).  One JSON document on stdout (and in --out).

--kernels adds HIP-event times (ms per call, median of the repeats) of direct ABI calls on the same
batch, one launch of R rows: `rank` = cc_recommend_batch_rank_fp32, `count` =
cc_recommend_batch_target_ranks_fp32, `chain` = the latter with empty target lists (its kernel
returns at once: the shared launches up to the keys alone).  rank_rows_kernel and
target_ranks_kernel alone are the differences rank - chain and count - chain.

    python tools/target_ranks_bench.py [--modes sort,count] [--rows 64,512,4096] [--kernels]
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

from cubecobrarecommender_amd import _lib as L                      # noqa: E402
from cubecobrarecommender_amd.layout import Layout                  # noqa: E402
from cubecobrarecommender_amd.recommender import Recommender, pack_cubes   # noqa: E402
from oracle import model_ref                                        # noqa: E402

V, D, ALL, HIDE = 20884, 512, 30000, 0.2


def make_split(R, seed=20251019):
    """R cubes of 360-540 distinct cards, 20 % of each (rounded down) hidden: (visible, hidden)."""
    rng = np.random.default_rng(seed)
    visible, hidden = [], []
    for _ in range(R):
        cube = rng.choice(V, int(rng.integers(360, 541)), replace=False)
        k = int(HIDE * len(cube))
        hidden.append(cube[:k].copy())
        visible.append(cube[k:].copy())
    return visible, hidden


def run_sort(rec, visible, hidden):
    outs = rec.recommend_many(visible, ALL)
    ranks = []
    pos = np.empty(V, np.int32)
    for o, h in zip(outs, hidden):
        adds = o['additions']
        pos[adds] = np.arange(len(adds), dtype=np.int32)
        ranks.append(pos[h].copy())
    return ranks


def run_count(rec, visible, hidden):
    return rec.target_ranks(visible, hidden)[0]


MODES = {'sort': run_sort, 'count': run_count}


def kernel_times(rec, visible, hidden, repeats):
    """HIP-event ms per direct call (one launch of all rows): rank, count, chain."""
    dev, R, lib = rec.dev, len(visible), L.lib()
    row_ptr, idx, max_n, _, _ = pack_cubes(visible, V)
    tgt_ptr = np.zeros(R + 1, np.int32)
    tgt_ptr[1:] = np.cumsum([len(h) for h in hidden])
    tgt = np.concatenate(hidden).astype(np.int32)
    rp, ix = torch.from_numpy(row_ptr).to(dev), torch.from_numpy(idx).to(dev)
    tp, tg = torch.from_numpy(tgt_ptr).to(dev), torch.from_numpy(tgt).to(dev)
    tp0 = torch.zeros_like(tp)
    ws = torch.empty(int(lib.cc_recommend_batch_rank_ws_size(V, D, R, max_n)) // 4 + 64, device=dev,
                     dtype=torch.int32)
    nadd = torch.empty(R, device=dev, dtype=torch.int32)
    adds = torch.empty(R, V, device=dev, dtype=torch.int32)
    addv = torch.empty(R, V, device=dev)
    cutv = torch.empty(len(idx), device=dev)
    ranks = torch.empty(len(tgt), device=dev, dtype=torch.int32)
    vals = torch.empty(len(tgt), device=dev)
    s = L.stream_ptr()

    def rank():
        L.call('cc_recommend_batch_rank_fp32', L.ptr(rec.params), V, D, R, L.ptr(rp), L.ptr(ix), max_n, ALL,
               L.ptr(ws), L.ptr(nadd), L.ptr(adds), L.ptr(addv), L.ptr(cutv), None, s)

    def count(t_ptr=tp):
        L.call('cc_recommend_batch_target_ranks_fp32', L.ptr(rec.params), V, D, R, L.ptr(rp), L.ptr(ix), max_n,
               L.ptr(t_ptr), L.ptr(tg), None, 0, L.ptr(ws), L.ptr(ranks), L.ptr(vals), None, L.ptr(cutv), None, s)

    calls = {'rank': rank, 'count': count, 'chain': lambda: count(tp0)}
    times = {m: [] for m in calls}
    for m in calls:
        calls[m]()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for m, fn in calls.items():                  # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[m].append(a.elapsed_time(b))
    out = {m: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for m, v in times.items()}
    out['rank_rows_kernel'] = out['rank']['median'] - out['chain']['median']
    out['target_ranks_kernel'] = out['count']['median'] - out['chain']['median']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--modes', default='sort,count')
    ap.add_argument('--rows', default='64,512,4096')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    modes = [m for m in a.modes.split(',') if m]
    rows = [int(r) for r in a.rows.split(',')]
    P = model_ref.init_params(V, D, seed=20250301, bias_std=0.01)
    rec = Recommender(Layout(V, D).pack(P), V, D)
    result = {'V': V, 'd': D, 'hide': HIDE, 'repeats': a.repeats, 'rows': {}}
    for R in rows:
        visible, hidden = make_split(R)
        calls = max(1, 64 // R)
        first = {}
        for m in modes:                              # warm-up: allocations, pinned staging, caches
            first[m] = MODES[m](rec, visible, hidden)
            MODES[m](rec, visible, hidden)
        if len(first) == 2:
            assert all(np.array_equal(x, y) for x, y in zip(first['sort'], first['count'])), 'ranks differ'
        del first
        samples = {m: [] for m in modes}
        for _ in range(a.repeats):
            for m in modes:                          # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _c in range(calls):
                    MODES[m](rec, visible, hidden)
                torch.cuda.synchronize()
                samples[m].append(R * calls / (time.perf_counter() - t0))
        row = {m: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for m, v in samples.items()}
        row['targets'] = int(sum(len(h) for h in hidden))
        line = f'R={R:5d} ' + '  '.join(
            f'{m}: {statistics.median(v):10.0f} ({min(v):.0f}..{max(v):.0f}) cubes/s' for m, v in samples.items())
        if a.kernels:                                # one launch of all rows; the results stay on the device
            row['kernels_ms'] = kernel_times(rec, visible, hidden, a.repeats)
            k = row['kernels_ms']
            line += (f"  | ms: rank {k['rank']['median']:.3f} count {k['count']['median']:.3f} chain "
                     f"{k['chain']['median']:.3f} -> rank_rows_kernel {k['rank_rows_kernel']:.3f} "
                     f"target_ranks_kernel {k['target_ranks_kernel']:.3f}")
        result['rows'][str(R)] = row
        print(line, file=sys.stderr, flush=True)
    doc = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    print(doc)


if __name__ == '__main__':
    main()
