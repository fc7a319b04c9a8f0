"""Validation-loss throughput: the held-out BCE from R x V probabilities on the host vs reduced per
row on the device.

Workload: V = 20,884, d = 512, cubes of 360-540 cards from a fixed seed (the targets are the cubes
themselves), R in {64, 512, 4096}.  Modes (cubes/s, wall clock including the host-side packing):
  probs  : Recommender.recommend_many(cubes, 1, want_probs=True) (R x V fp32 probabilities copied
           back) + the BCE of them in numpy (float64 logs of the fp32 probabilities)
  device : Recommender.reconstruction_loss(cubes)
`probs` uses only API older than reconstruction_loss, so the same file run with ``--modes probs`` on
an older tree gives the baseline.  Each repeat visits the modes in turn (alternating), after a
warm-up of every mode; the table reports the median and the min..max spread of the repeats.  The two
modes' mean losses are compared once per R (they agree to the fp32 probabilities' precision; the
figure is reported, not gated).  One JSON document on stdout (and in --out).

--kernels adds HIP-event times (ms per call, median of the repeats) of direct ABI calls on the same
batch, one launch of R rows: `loss` = cc_recommend_batch_loss_fp32, `chain` =
cc_recommend_batch_target_ranks_fp32 with empty target lists (its kernel returns at once: the
forward and the output tile with the sort-key epilogue alone).  Both run the same forward and the
same accumulate loop, so loss - chain is what the loss epilogue and the row reduce cost beyond the
key epilogue.

    python tools/eval_loss_bench.py [--modes probs,device] [--rows 64,512,4096] [--kernels]
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

V, D = 20884, 512


def make_cubes(R, seed=20251020):
    """R cubes of 360-540 distinct cards."""
    rng = np.random.default_rng(seed)
    return [rng.choice(V, int(rng.integers(360, 541)), replace=False) for _ in range(R)]


def run_probs(rec, cubes):
    """Mean BCE from the probabilities: -[y log p + (1 - y) log(1 - p)], mean over V then rows."""
    outs = rec.recommend_many(cubes, 1, want_probs=True)
    total = 0.0
    with np.errstate(divide='ignore'):
        for o, c in zip(outs, cubes):
            p = o['probs'].astype(np.float64)
            l = -np.log1p(-p)
            l[c] = -np.log(p[c])
            total += float(l.mean())
    return total / len(cubes)


def run_device(rec, cubes):
    row_loss, _ = rec.reconstruction_loss(cubes)
    return float(np.sum(row_loss)) / len(cubes)


MODES = {'probs': run_probs, 'device': run_device}


def kernel_times(rec, cubes, repeats):
    """HIP-event ms per direct call (one launch of all rows): loss, chain."""
    dev, R, lib = rec.dev, len(cubes), L.lib()
    row_ptr, idx, max_n, _, _ = pack_cubes(cubes, V)
    rp, ix = torch.from_numpy(row_ptr).to(dev), torch.from_numpy(idx).to(dev)
    tp0 = torch.zeros_like(rp)
    ws = torch.empty(max(int(lib.cc_recommend_batch_loss_ws_size(V, D, R, max_n)),
                         int(lib.cc_recommend_batch_target_ranks_ws_size(V, D, R, max_n))) // 4 + 64,
                     device=dev, dtype=torch.int32)
    loss = torch.empty(R, device=dev, dtype=torch.float64)
    pred = torch.empty(R, device=dev, dtype=torch.int32)
    cutv = torch.empty(len(idx), device=dev)
    ranks = torch.empty(1, device=dev, dtype=torch.int32)
    vals = torch.empty(1, device=dev)
    s = L.stream_ptr()

    def run_loss():
        L.call('cc_recommend_batch_loss_fp32', L.ptr(rec.params), V, D, R, L.ptr(rp), L.ptr(ix), max_n,
               L.ptr(rp), L.ptr(ix), L.ptr(ws), L.ptr(loss), L.ptr(pred), s)

    def run_chain():
        L.call('cc_recommend_batch_target_ranks_fp32', L.ptr(rec.params), V, D, R, L.ptr(rp), L.ptr(ix), max_n,
               L.ptr(tp0), L.ptr(ix), None, 0, L.ptr(ws), L.ptr(ranks), L.ptr(vals), None, L.ptr(cutv), None, s)

    calls = {'loss': run_loss, 'chain': run_chain}
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
    out['loss_minus_chain'] = out['loss']['median'] - out['chain']['median']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--modes', default='probs,device')
    ap.add_argument('--rows', default='64,512,4096')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--kernels', action='store_true')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    modes = [m for m in a.modes.split(',') if m]
    rows = [int(r) for r in a.rows.split(',')]
    P = model_ref.init_params(V, D, seed=20250301, bias_std=0.01)
    rec = Recommender(Layout(V, D).pack(P), V, D)
    result = {'V': V, 'd': D, 'repeats': a.repeats, 'rows': {}}
    for R in rows:
        cubes = make_cubes(R)
        calls = max(1, 64 // R)
        first = {}
        for m in modes:                              # warm-up: allocations, pinned staging, caches
            first[m] = MODES[m](rec, cubes)
            MODES[m](rec, cubes)
        samples = {m: [] for m in modes}
        for _ in range(a.repeats):
            for m in modes:                          # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _c in range(calls):
                    MODES[m](rec, cubes)
                torch.cuda.synchronize()
                samples[m].append(R * calls / (time.perf_counter() - t0))
        row = {m: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for m, v in samples.items()}
        row['bce'] = first
        line = f'R={R:5d} ' + '  '.join(
            f'{m}: {statistics.median(v):10.0f} ({min(v):.0f}..{max(v):.0f}) cubes/s' for m, v in samples.items())
        if len(first) == 2:
            row['bce_rel_diff'] = abs(first['probs'] - first['device']) / first['device']
            line += f"  bce {first['device']:.9f} (probs differs by {row['bce_rel_diff']:.1e} rel)"
        if a.kernels and 'device' in modes:          # one launch of all rows; the results stay on the device
            row['kernels_ms'] = kernel_times(rec, cubes, a.repeats)
            k = row['kernels_ms']
            line += (f"  | ms: loss {k['loss']['median']:.3f} ({k['loss']['min']:.3f}..{k['loss']['max']:.3f}) chain "
                     f"{k['chain']['median']:.3f} ({k['chain']['min']:.3f}..{k['chain']['max']:.3f})"
                     f" -> loss - chain {k['loss_minus_chain']:.3f}")
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
