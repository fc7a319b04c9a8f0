"""Card similarity, one request per call against many per call.

Workload: V = 22,000 cards, K = 64, `relu` embeddings max(normal, 0) from a fixed seed, N = 40
neighbours; Q in {1, 16, 512, 4096, V} query cards (the first Q ids), and N = cap + 1 (the sort
path) at Q = 512.  Per (Q, N), end to end on the host clock, both ending with the results in host
memory:
  single : a loop of similar(emb, q, N) (cc_similar_cards: two launches, a synchronise and two
           copies per query).  Its cost per query does not depend on Q, so above --single-cap
           queries the loop runs the first --single-cap of them (`single_queries` says how many).
  batch  : similar_many(emb, queries, N) (cc_similar_cards_batch in launches of 512 rows)
The two alternate inside one run after a warm-up of each; every repeat is kept, with the median.
The bar: at Q = 512 and Q = V every repeat of `batch` is below every repeat of `single`, per query.
The rows both paths return are compared bit for bit.

`kernels_ms`: HIP-event times of the three kernels of one 512-row launch
(cc_similar_cards_batch_timed), medians of the repeats, for N = 40 (select) and N = cap + 1 (sort),
and the distance kernel's achieved rate two ways: 2 Q V K separately rounded operations against
half the 157.3 TF fp32 vector peak (a multiply and an add where the peak counts one FMA), and the
Q V 4 bytes of sort keys it writes against 8 TB/s.  One JSON document on stdout (and in --out).

    python tools/similarity_batch_bench.py [--repeats 7] [--single-cap 2048] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cubecobrarecommender_amd import _lib as L                                   # noqa: E402
from cubecobrarecommender_amd.similarity import similar, similar_many            # noqa: E402

V, K, N_SMALL, LAUNCH_ROWS = 22000, 64, 40, 512
PEAK_UNFUSED_FLOPS, PEAK_BYTES = 157.3e12 / 2, 8e12


def spread(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'repeats': list(v)}


def wall_per_query(emb, queries, N, repeats, single_cap):
    """us per query of the single loop and of similar_many, alternating."""
    sq = queries[:single_cap]

    def single():
        return [similar(emb, int(q), N) for q in sq]

    def batch():
        return similar_many(emb, queries, N)
    ref, got = single(), batch()                     # warm-up of both, and the comparison
    for r, (si, sd) in enumerate(ref):
        assert np.array_equal(got[0][r], si) and np.array_equal(got[1][r].view(np.uint32), sd.view(np.uint32)), r
    times = {'single': [], 'batch': []}
    for _ in range(repeats):
        for name, fn, count in (('single', single, len(sq)), ('batch', batch, len(queries))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e6 / count)
    return {'single_queries': len(sq), 'single_us_per_query': spread(times['single']),
            'batch_us_per_query': spread(times['batch']),
            'every_batch_repeat_below_every_single_repeat': max(times['batch']) < min(times['single'])}


def kernel_times(emb, N, repeats):
    """HIP-event ms of each kernel of one LAUNCH_ROWS-row launch, and the distance kernel's rates."""
    lib, dev, Q = L.lib(), emb.device, LAUNCH_ROWS
    q_d = torch.arange(Q, device=dev, dtype=torch.int32)
    ws = torch.empty(int(lib.cc_similar_batch_ws_size(V, K, Q, N)) // 4 + 64, device=dev, dtype=torch.int32)
    idx = torch.empty(Q, N, device=dev, dtype=torch.int32)
    dist = torch.empty(Q, N, device=dev, dtype=torch.float32)
    ms = (C.c_float * 3)()
    rows = []
    for i in range(repeats + 2):                     # two warm-up calls
        L.call('cc_similar_cards_batch_timed', L.ptr(emb), V, K, Q, L.ptr(q_d), N, L.ptr(ws), L.ptr(idx), L.ptr(dist),
               None, C.cast(ms, C.c_void_p), L.stream_ptr())
        if i >= 2:
            rows.append(list(ms))
    names = ('normalise', 'distance_tile', 'select' if N <= int(lib.cc_similar_batch_max_n()) else 'sort')
    out = {n: spread([r[i] for r in rows]) for i, n in enumerate(names)}
    t = out['distance_tile']['median'] * 1e-3
    ops, key_bytes = 2.0 * Q * V * K, 4.0 * Q * V
    out['distance_ops'] = ops
    out['distance_tflops_unfused'] = ops / t / 1e12
    out['distance_share_of_unfused_fp32_peak'] = ops / t / PEAK_UNFUSED_FLOPS
    out['distance_key_bytes'] = key_bytes
    out['distance_key_tb_per_s'] = key_bytes / t / 1e12
    out['distance_share_of_8_tb_per_s'] = key_bytes / t / PEAK_BYTES
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--single-cap', type=int, default=2048)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('similarity_batch_bench needs a GPU: nothing is measured without one')
    rng = np.random.default_rng(20250301)
    emb = torch.from_numpy(np.maximum(rng.standard_normal((V, K)).astype(np.float32), 0)).cuda()
    cap = int(L.lib().cc_similar_batch_max_n())
    result = {'V': V, 'K': K, 'cap': cap, 'repeats': a.repeats, 'rows_per_launch': LAUNCH_ROWS, 'wall': [], 'kernels_ms': {}}
    for Q, N in ((1, N_SMALL), (16, N_SMALL), (512, N_SMALL), (4096, N_SMALL), (V, N_SMALL), (512, cap + 1)):
        row = {'Q': Q, 'N': N, **wall_per_query(emb, np.arange(Q, dtype=np.int64), N, a.repeats, a.single_cap)}
        result['wall'].append(row)
        s, b = row['single_us_per_query'], row['batch_us_per_query']
        print(f"Q={Q:6d} N={N:5d}  us/query: single {s['median']:.1f} ({s['min']:.1f}..{s['max']:.1f})  batch "
              f"{b['median']:.2f} ({b['min']:.2f}..{b['max']:.2f})  x{s['median'] / b['median']:.1f}",
              file=sys.stderr, flush=True)
    for N in (N_SMALL, cap + 1):
        k = result['kernels_ms'][str(N)] = kernel_times(emb, N, a.repeats)
        rank = 'select' if 'select' in k else 'sort'
        print(f"Q={LAUNCH_ROWS} N={N:5d}  ms: normalise {k['normalise']['median']:.3f} distance "
              f"{k['distance_tile']['median']:.3f} {rank} {k[rank]['median']:.3f} | distance "
              f"{k['distance_tflops_unfused']:.1f} TF of separately rounded ops "
              f"({100 * k['distance_share_of_unfused_fp32_peak']:.0f} % of 78.65), keys "
              f"{k['distance_key_tb_per_s']:.2f} TB/s", file=sys.stderr, flush=True)
    result['bar_met'] = all(r['every_batch_repeat_below_every_single_repeat'] for r in result['wall']
                            if r['N'] == N_SMALL and r['Q'] in (512, V))
    doc = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    print(doc)
    if not result['bar_met']:
        raise SystemExit('the batched path is not below the single loop in every repeat')


if __name__ == '__main__':
    main()
