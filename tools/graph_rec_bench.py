"""Co-occurrence baseline throughput: cc_graph_rec_f64 on the device-built graph.

Workload: V = 22,000, the graph M of 65,536 synthetic cubes (the benchmark's corpus and seed) built
on the device by cc_adjacency (3.9 GB of f64, far past the 256 MiB Infinity Cache); requests are
the corpus' first R cubes, R in {1, 64, 512}, amount 100.  Per R, HIP-event times of direct ABI
calls, one launch of all rows, results left on the device (median and min..max of the repeats,
the calls visited in turn after a warm-up of each):
  full  : cc_graph_rec_f64 (scoring + the select-and-sort ranking)
  score : cc_graph_rec_target_ranks_f64 with empty target lists: its counting kernel returns at
          once, so this is graph_score_kernel alone (plus one empty launch)
  ranks : the same call with 20 % of each cube hidden and ranked (the graph here is the whole
          corpus': a timing, not an evaluation)
  rank  : cc_graph_rank_f64 with amount = V (scoring + the full sort of every row); the sort's own
          time is rank - score
and from them: us per cube, and the scoring kernel's gathered bytes, sum_r n_r * V * 8, over its
time, in TB/s.  The yardstick is the guide's rate for whole rows gathered from HBM into registers,
5.5-5.8 TB/s; rows that neighbouring cubes share can come from L2 instead, and R = 1 is
latency-bound (the pinned order forbids splitting a cube's sum).
`wall` is GraphRecommender.recommend_many end to end (packing, launch, D2H, host cut order);
`rank_wall` is GraphRecommender.rank_many(cubes) end to end, every card of every cube ranked, and
`argsort_wall` the same complete lists the way they were made before the device sort:
recommend_many(cubes, 1, want_scores=True) and a host argsort(kind='stable') per cube, as
api.simple_recs' fallback does it; the two are timed in turn in the same process and their lists
compared.  `numpy` is the pinned definition on the host: an explicit ascending loop of row adds per
cube over the same M in host memory, min(R, --host-rows) cubes on 16 threads.  The device scores of those
cubes are compared with the host's, bit for bit.  One JSON document on stdout (and in --out).

    python tools/graph_rec_bench.py [--rows 1,64,512] [--repeats 9] [--wall-repeats 5] [--cubes 65536] [--no-host]
"""
import argparse
import concurrent.futures as cf
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cubecobrarecommender_amd import _lib as L                      # noqa: E402
from cubecobrarecommender_amd.graphrec import GraphRecommender      # noqa: E402
from cubecobrarecommender_amd.recommender import pack_cubes         # noqa: E402
from cubecobrarecommender_amd.synthetic import synthetic_cubes      # noqa: E402

V, AMOUNT, HIDE, GUIDE_TBS = 22000, 100, 0.2, (5.5, 5.8)


def host_scores(M, cube):
    """The pinned definition: rows added in ascending order, the cube's own diagonal entries as 0."""
    acc = np.zeros(M.shape[0], np.float64)
    for i in np.unique(cube):
        row = M[i].copy()
        row[i] = 0.0
        acc = acc + row
    return acc


def kernel_times(rec, cubes, repeats):
    """HIP-event ms per direct call (one launch of all rows): full, score, ranks, rank."""
    dev, R, lib = rec.dev, len(cubes), L.lib()
    rng = np.random.default_rng(1)
    visible, hidden = [], []
    for c in cubes:
        c = rng.permutation(np.unique(c))
        k = int(HIDE * len(c))
        hidden.append(c[:k])
        visible.append(c[k:])
    row_ptr, idx, max_n, _, _ = pack_cubes(cubes, V)
    vrow_ptr, vidx, vmax_n, _, _ = pack_cubes(visible, V)
    tgt_ptr = np.zeros(R + 1, np.int32)
    tgt_ptr[1:] = np.cumsum([len(h) for h in hidden])
    tgt = np.concatenate(hidden).astype(np.int32)
    rp, ix = torch.from_numpy(row_ptr).to(dev), torch.from_numpy(idx).to(dev)
    vrp, vix = torch.from_numpy(vrow_ptr).to(dev), torch.from_numpy(vidx).to(dev)
    tp, tg = torch.from_numpy(tgt_ptr).to(dev), torch.from_numpy(tgt if len(tgt) else np.zeros(1, np.int32)).to(dev)
    tp0 = torch.zeros_like(tp)
    ws = torch.empty(int(lib.cc_graph_rec_ws_size(V, R, max_n)) // 4 + 64, device=dev, dtype=torch.int32)
    nadd = torch.empty(R, device=dev, dtype=torch.int32)
    adds = torch.empty(R, AMOUNT, device=dev, dtype=torch.int32)
    addv = torch.empty(R, AMOUNT, device=dev, dtype=torch.float64)
    cutv = torch.empty(len(idx), device=dev, dtype=torch.float64)
    ranks = torch.empty(max(len(tgt), 1), device=dev, dtype=torch.int32)
    vals = torch.empty(max(len(tgt), 1), device=dev, dtype=torch.float64)
    rws = torch.empty(int(lib.cc_graph_rank_ws_size(V, R, max_n)) // 4 + 64, device=dev, dtype=torch.int32)
    radds = torch.empty(R, V, device=dev, dtype=torch.int32)
    raddv = torch.empty(R, V, device=dev, dtype=torch.float64)
    s = L.stream_ptr()

    def rank():
        L.call('cc_graph_rank_f64', L.ptr(rec.adj), rec.ld, V, R, L.ptr(rp), L.ptr(ix), max_n, V, L.ptr(rws),
               L.ptr(nadd), L.ptr(radds), L.ptr(raddv), L.ptr(cutv), None, s)

    def full():
        L.call('cc_graph_rec_f64', L.ptr(rec.adj), rec.ld, V, R, L.ptr(rp), L.ptr(ix), max_n, AMOUNT, L.ptr(ws),
               L.ptr(nadd), L.ptr(adds), L.ptr(addv), L.ptr(cutv), None, s)

    def count(rp_, ix_, n_, t_ptr):
        L.call('cc_graph_rec_target_ranks_f64', L.ptr(rec.adj), rec.ld, V, R, L.ptr(rp_), L.ptr(ix_), n_,
               L.ptr(t_ptr), L.ptr(tg), None, 0, L.ptr(ws), L.ptr(ranks), L.ptr(vals), None, L.ptr(cutv), None, s)

    calls = {'full': full, 'score': lambda: count(rp, ix, max_n, tp0), 'ranks': lambda: count(vrp, vix, vmax_n, tp),
             'rank': rank}
    times = {m: [] for m in calls}
    for fn in calls.values():
        fn()
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
    gathered = float(len(idx)) * V * 8
    out['gathered_bytes'] = gathered
    out['score_tb_per_s'] = gathered / (out['score']['median'] * 1e-3) / 1e12
    out['score_tb_per_s_best'] = gathered / (out['score']['min'] * 1e-3) / 1e12
    out['us_per_cube'] = out['full']['median'] * 1e3 / R
    out['sort_ms'] = out['rank']['median'] - out['score']['median']
    return out


def argsort_lists(rec, cubes):
    """Every cube's complete list from the device's scores and a host argsort per cube
    (api.simple_recs without rank_many)."""
    outs = rec.recommend_many(cubes, 1, want_scores=True)
    lists = []
    for c, o in zip(cubes, outs):
        vec = np.zeros(V)
        vec[c] = 1
        missing = np.where(vec == 0)[0]
        lists.append(missing[np.argsort(o['scores'][missing], kind='stable')[::-1]])
    return lists


def complete_list_walls(rec, cubes, repeats):
    """Wall-clock us per cube of rank_many(cubes) and of argsort_lists, in turn, after a warm-up
    of each; their lists are compared."""
    R = len(cubes)
    ways = {'rank_wall': lambda: [o['additions'] for o in rec.rank_many(cubes)],
            'argsort_wall': lambda: argsort_lists(rec, cubes)}
    lists = {m: fn() for m, fn in ways.items()}
    assert all(np.array_equal(a, b) for a, b in zip(lists['rank_wall'], lists['argsort_wall'])), \
        'rank_many and the host argsort give different lists'
    walls = {m: [] for m in ways}
    for _ in range(repeats):
        for m, fn in ways.items():                   # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            walls[m].append((time.perf_counter() - t0) * 1e6 / R)
    out = {m: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for m, v in walls.items()}
    out['lists_equal'] = True
    out['argsort_over_rank'] = out['argsort_wall']['median'] / out['rank_wall']['median']
    out['rank_max_below_argsort_min'] = out['rank_wall']['max'] < out['argsort_wall']['min']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', default='1,64,512')
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--wall-repeats', type=int, default=5)
    ap.add_argument('--cubes', type=int, default=65536)
    ap.add_argument('--host-rows', type=int, default=64)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    rows = [int(r) for r in a.rows.split(',')]
    indptr, indices = synthetic_cubes(a.cubes, V, seed=20250301)
    rec = GraphRecommender.from_cubes(indptr, indices, V)
    M = None if a.no_host else rec.adj.cpu().numpy()
    result = {'V': V, 'cubes': a.cubes, 'amount': AMOUNT, 'repeats': a.repeats, 'guide_tb_per_s': GUIDE_TBS,
              'adj_gb': V * V * 8 / 1e9, 'rows': {}}
    for R in rows:
        cubes = [indices[indptr[c]:indptr[c + 1]] for c in range(R)]
        row = {'cards_per_cube': float(np.mean([len(c) for c in cubes])), 'kernels_ms': kernel_times(rec, cubes, a.repeats)}
        k = row['kernels_ms']
        rec.recommend_many(cubes, AMOUNT)            # warm-up: workspace, pinned staging
        wall = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _c in range(max(1, 64 // R)):
                outs = rec.recommend_many(cubes, AMOUNT)
            wall.append((time.perf_counter() - t0) * 1e6 / (R * max(1, 64 // R)))
        row['wall_us_per_cube'] = {'median': statistics.median(wall), 'min': min(wall), 'max': max(wall)}
        row['complete_lists_us_per_cube'] = cl = complete_list_walls(rec, cubes, a.wall_repeats)
        line = (f"R={R:4d} n={row['cards_per_cube']:.0f}  ms: full {k['full']['median']:.3f} score "
                f"{k['score']['median']:.3f} ({k['score']['min']:.3f}..{k['score']['max']:.3f}) ranks "
                f"{k['ranks']['median']:.3f} -> {k['us_per_cube']:.1f} us/cube, scoring {k['score_tb_per_s']:.2f} TB/s"
                f" | wall {row['wall_us_per_cube']['median']:.1f} us/cube"
                f" | rank {k['rank']['median']:.3f} ({k['rank']['min']:.3f}..{k['rank']['max']:.3f}) ms, sort "
                f"{k['sort_ms']:.3f} ms | every card: rank_many {cl['rank_wall']['median']:.1f} "
                f"({cl['rank_wall']['min']:.1f}..{cl['rank_wall']['max']:.1f}) us/cube, host argsort "
                f"{cl['argsort_wall']['median']:.1f} ({cl['argsort_wall']['min']:.1f}..{cl['argsort_wall']['max']:.1f})"
                f" us/cube, x{cl['argsort_over_rank']:.1f}")
        if M is not None:
            Rh = min(R, a.host_rows)
            host_scores(M, cubes[0])                 # warm-up: the pages of M
            t0 = time.perf_counter()
            with cf.ThreadPoolExecutor(16) as ex:
                want = list(ex.map(lambda c: host_scores(M, c), cubes[:Rh]))
            row['numpy_us_per_cube'] = (time.perf_counter() - t0) * 1e6 / Rh
            row['numpy_rows'] = Rh
            got = rec.recommend_many(cubes[:Rh], AMOUNT, want_scores=True)
            row['bits_equal'] = all(np.array_equal(g['scores'].view(np.uint64), w.view(np.uint64))
                                    for g, w in zip(got, want))
            assert row['bits_equal'], 'device scores differ from the pinned definition'
            assert all(np.array_equal(o['additions'], g['additions']) for o, g in zip(outs, got))
            line += f" | numpy {row['numpy_us_per_cube']:.0f} us/cube ({Rh} cubes, 16 threads), bits equal"
        result['rows'][str(R)] = row
        print(line, file=sys.stderr, flush=True)
        # the gate of the device sort: from 512 cubes its slowest repeat beats the host argsort's fastest
        assert R < 512 or cl['rank_max_below_argsort_min'], 'rank_many is not faster than the host argsort'
    doc = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    print(doc)


if __name__ == '__main__':
    main()
