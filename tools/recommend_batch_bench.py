"""Recommend throughput: many cubes per call vs the single-cube paths.

Workload: V = 20,884, d = 512, amount 100, cubes of 360-540 cards from a fixed seed,
R in {1, 8, 64, 512, 4096}.  Modes (cubes/s, wall clock including the host-side packing):
  loop    : R calls of Recommender.recommend
  compose : encode_lists + decode ([R, V] probabilities) + one cc_topn per row
  batch   : Recommender.recommend_many
`loop` and `compose` use only API older than the batched call, so the same file run with
``--modes loop,compose`` on an older tree gives the baseline.  Each repeat visits the modes in turn
(alternating), after a warm-up of every mode; the table reports the median and the min..max spread
of the repeats.  One JSON document on stdout (and in --out).

    python tools/recommend_batch_bench.py [--modes loop,compose,batch] [--rows 1,8,64,512,4096]
                                          [--amount 100]
--amount above every |V| (the web endpoint's default is 30000) ranks every card of every cube.
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
from cubecobrarecommender_amd.recommender import Recommender        # noqa: E402
from oracle import model_ref                                        # noqa: E402

V, D, AMOUNT = 20884, 512, 100


def make_cubes(R, seed=20251019):
    rng = np.random.default_rng(seed)
    return [rng.choice(V, int(rng.integers(360, 541)), replace=False) for _ in range(R)]


def run_loop(rec, cubes):
    return [rec.recommend(c, AMOUNT) for c in cubes]


def run_compose(rec, cubes):
    """The pieces by hand: batched encoder + decoder, then the single-row ranking per cube."""
    R = len(cubes)
    dev = rec.dev
    probs = rec.decode(rec.encode_lists(cubes))
    uniq = [np.unique(np.asarray(c, np.int64)).astype(np.int32) for c in cubes]
    ptr = np.zeros(R + 1, np.int64)
    ptr[1:] = np.cumsum([len(u) for u in uniq])
    idx = torch.from_numpy(np.concatenate(uniq)).to(dev)
    adds = torch.zeros(R, min(AMOUNT, V), device=dev, dtype=torch.int32)
    addv = torch.zeros(R, min(AMOUNT, V), device=dev)
    cutv = torch.zeros(int(ptr[-1]), device=dev)
    nadd = torch.zeros(R, device=dev, dtype=torch.int32)
    ws = torch.zeros(int(L.lib().cc_topn_workspace_size(V)) // 4 + 64, device=dev, dtype=torch.int32)
    s = L.stream_ptr()
    for r in range(R):
        lo, n = int(ptr[r]), len(uniq[r])
        L.call('cc_topn', L.ptr(probs[r]), V, L.ptr(idx[lo:]), n, AMOUNT, L.ptr(adds[r]), L.ptr(nadd[r:]),
               L.ptr(addv[r]), L.ptr(cutv[lo:]), None, L.ptr(ws), s)
    return adds.cpu().numpy(), addv.cpu().numpy(), cutv.cpu().numpy()


def run_batch(rec, cubes):
    return rec.recommend_many(cubes, AMOUNT)


MODES = {'loop': run_loop, 'compose': run_compose, 'batch': run_batch}


def main():
    global AMOUNT
    ap = argparse.ArgumentParser()
    ap.add_argument('--modes', default='loop,compose,batch')
    ap.add_argument('--rows', default='1,8,64,512,4096')
    ap.add_argument('--amount', type=int, default=AMOUNT)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    AMOUNT = a.amount
    modes = [m for m in a.modes.split(',') if m]
    rows = [int(r) for r in a.rows.split(',')]
    P = model_ref.init_params(V, D, seed=20250301, bias_std=0.01)
    rec = Recommender(Layout(V, D).pack(P), V, D)
    result = {'V': V, 'd': D, 'amount': AMOUNT, 'repeats': a.repeats, 'rows': {}}
    for R in rows:
        cubes = make_cubes(R)
        calls = max(1, 64 // R)                  # several calls per sample at small R
        for m in modes:                          # warm-up: allocations, the request graph, caches
            MODES[m](rec, cubes)
            MODES[m](rec, cubes)
        samples = {m: [] for m in modes}
        for _ in range(a.repeats):
            for m in modes:                      # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _c in range(calls):
                    MODES[m](rec, cubes)
                torch.cuda.synchronize()
                samples[m].append(R * calls / (time.perf_counter() - t0))
        result['rows'][str(R)] = {
            m: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for m, v in samples.items()}
        print(f'R={R:5d} ' + '  '.join(
            f'{m}: {statistics.median(v):10.0f} ({min(v):.0f}..{max(v):.0f}) cubes/s' for m, v in samples.items()),
            file=sys.stderr, flush=True)
    doc = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    print(doc)


if __name__ == '__main__':
    main()
