"""Card pools: "the best AMOUNT cards among these" by the pooled call vs the spelling older trees have.

Workload and protocol of tools/recommend_batch_bench.py: V = 20,884, d = 512, R = 512 cubes of
360-540 cards from a fixed seed, amount 100.  Modes (milliseconds per call of R cubes, wall clock
including the host-side packing and unpacking):
  unpooled : Recommender.recommend_many(cubes, amount): the call the pools must not slow down
  filter   : recommend_many(cubes, 30000), every card ranked and copied back, then per cube the first
             `amount` pool members of its additions picked on the host (one numpy mask and slice per
             cube, no dictionaries: the cheapest host filter there is)
  pool     : recommend_many(cubes, amount, pool=pool)
`unpooled` and `filter` use only API older than the pools, so the same file run with
``--modes unpooled,filter`` in an older tree gives the baseline; run the two trees' processes in
turn to compare `unpooled`.  Pools: the first int(V * share) cards of a fixed permutation, for each
share of --shares (default 1/6 and 2 %).  Each repeat visits the modes in turn (alternating), after a
warm-up of every mode; the table reports the median and the min..max spread of the repeats.  One JSON
document on stdout (and in --out).

    python tools/recommend_pool_bench.py [--modes unpooled,filter,pool] [--rows 512] [--amount 100]
                                         [--shares 0.16667,0.02] [--repeats 7]
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

from cubecobrarecommender_amd.layout import Layout                  # noqa: E402
from cubecobrarecommender_amd.recommender import Recommender        # noqa: E402
from oracle import model_ref                                        # noqa: E402

V, D = 20884, 512
ALL = 30000


def make_cubes(R, seed=20251019):
    rng = np.random.default_rng(seed)
    return [rng.choice(V, int(rng.integers(360, 541)), replace=False) for _ in range(R)]


def pool_cards(share, seed=20260101):
    return np.sort(np.random.default_rng(seed).permutation(V)[:max(1, int(V * share))])


def run_unpooled(rec, cubes, amount, ids):
    return rec.recommend_many(cubes, amount)


def run_filter(rec, cubes, amount, ids):
    member = np.zeros(V, bool)
    member[ids] = True
    out = []
    for o in rec.recommend_many(cubes, ALL):
        keep = np.flatnonzero(member[o['additions']])[:max(amount, 1)]
        out.append({'additions': o['additions'][keep], 'add_vals': o['add_vals'][keep], 'cut_vals': o['cut_vals']})
    return out


_pools = {}


def run_pool(rec, cubes, amount, ids):
    if id(ids) not in _pools:
        _pools[id(ids)] = rec.card_pool(ids)       # uploaded once, as a server would keep it
    return rec.recommend_many(cubes, amount, pool=_pools[id(ids)])


MODES = {'unpooled': run_unpooled, 'filter': run_filter, 'pool': run_pool}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--modes', default='unpooled,filter,pool')
    ap.add_argument('--rows', default='512')
    ap.add_argument('--amount', type=int, default=100)
    ap.add_argument('--shares', default='0.16667,0.02')
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--check', action='store_true', help='assert that filter and pool agree, bit for bit')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    modes = [m for m in a.modes.split(',') if m]
    P = model_ref.init_params(V, D, seed=20250301, bias_std=0.01)
    rec = Recommender(Layout(V, D).pack(P), V, D)
    pools = {s: pool_cards(float(s)) for s in a.shares.split(',') if s}
    result = {'V': V, 'd': D, 'amount': a.amount, 'repeats': a.repeats, 'unit': 'ms per call', 'rows': {}}
    for R in [int(r) for r in a.rows.split(',')]:
        cubes = make_cubes(R)
        # unpooled does not depend on the pool: one line; the others one line per share
        lines = [(m, s) for m in modes for s in (pools if m != 'unpooled' else [next(iter(pools))])]
        for m, s in lines:                           # warm-up: allocations, staging buffers, caches
            MODES[m](rec, cubes, a.amount, pools[s])
            MODES[m](rec, cubes, a.amount, pools[s])
        if a.check and 'filter' in modes and 'pool' in modes:
            for s in pools:
                x, y = run_filter(rec, cubes, a.amount, pools[s]), run_pool(rec, cubes, a.amount, pools[s])
                for ox, oy in zip(x, y):
                    assert all(np.array_equal(ox[k], oy[k]) for k in ('additions', 'add_vals', 'cut_vals'))
        samples = {line: [] for line in lines}
        for _ in range(a.repeats):
            for m, s in lines:                       # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                MODES[m](rec, cubes, a.amount, pools[s])
                torch.cuda.synchronize()
                samples[(m, s)].append(1e3 * (time.perf_counter() - t0))
        table = {}
        for (m, s), v in samples.items():
            name = m if m == 'unpooled' else f'{m}@{s}'
            table[name] = {'median': statistics.median(v), 'min': min(v), 'max': max(v)}
            if m != 'unpooled':
                table[name]['pool_size'] = int(len(pools[s]))
        result['rows'][str(R)] = table
        print(f'R={R:5d} ' + '  '.join(f'{k}: {t["median"]:.2f} ({t["min"]:.2f}..{t["max"]:.2f}) ms'
                                       for k, t in table.items()), file=sys.stderr, flush=True)
    doc = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    print(doc)


if __name__ == '__main__':
    main()
