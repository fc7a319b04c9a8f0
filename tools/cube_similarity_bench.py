"""Similar cubes: the resident cube index against the batched card path on the same matrix.

Workload: K = 64, `relu` embeddings max(normal, 0) from a fixed seed, Q = 512 member queries (evenly
spread ids), k = 40 neighbours, the query itself kept (the answer `similar_many` gives).  End to end
on the host clock, both paths ending with the results in host memory, alternating inside one run
after a warm-up of each; every repeat is kept, with median and min..max.
  N = 65,536 : `similar_many(emb, ids, k)` (cc_similar_cards_batch: normalises all N rows per launch,
               [Q][N] keys) against `CubeIndex.neighbours(ids, k, exclude_self=False)` (the index
               normalised once, outside the timing, as it is in use).  The rows are compared bit for
               bit.  The bar: the index path's median is not above the card path's.
  N = 2^20   : the index path alone (the card path would need 2 GiB of keys per launch): us per
               query and the workspace bytes, beside the bytes of a [Q][N] key matrix.
`launch_ms`: device time of one 512-row call of each entry between two events on the stream.
  build      : CubeIndex(model, cubes) (pack + encode + put, the index resident afterwards) for
               --build-cubes synthetic cubes at V = 22,000, d = 256, per 65,536 cubes.
One JSON document on stdout (and in --out).

    python tools/cube_similarity_bench.py [--repeats 7] [--build-cubes 65536] [--out FILE]
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
from cubecobrarecommender_amd.cubesim import LATENT, CubeIndex                   # noqa: E402
from cubecobrarecommender_amd.similarity import similar_many                     # noqa: E402

K, Q, NEIGHBOURS = LATENT, 512, 40
N_BOTH, N_LARGE = 1 << 16, 1 << 20
BUILD_V, BUILD_D = 22000, 256


def spread(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'repeats': list(v)}


def relu_embeddings(N, seed=20250301):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.maximum(rng.standard_normal((N, K), dtype=np.float32), 0)).cuda()


def timed(fns, repeats, count):
    """us per query of each named function, alternating; one warm-up call of each first, whose
    results are returned."""
    first = {name: fn() for name, fn in fns.items()}
    times = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e6 / count)
    return first, {name: spread(v) for name, v in times.items()}


def event_ms(call, repeats):
    """Device ms of call() between two events on the current stream: two warm-up calls, then the
    repeats."""
    out = []
    for i in range(repeats + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        if i >= 2:
            out.append(a.elapsed_time(b))
    return spread(out)


def launch_times(emb, index, ids, repeats):
    """One 512-row call of each entry on the device clock (no host packing, no copies back)."""
    lib, dev, N = L.lib(), emb.device, emb.shape[0]
    q_d = torch.from_numpy(ids.astype(np.int32)).to(dev)
    idx = torch.empty(Q, NEIGHBOURS, device=dev, dtype=torch.int32)
    dist = torch.empty(Q, NEIGHBOURS, device=dev, dtype=torch.float32)
    ws_c = torch.empty(int(lib.cc_similar_batch_ws_size(N, K, Q, NEIGHBOURS)) // 4 + 64, device=dev, dtype=torch.int32)
    ws_i = torch.empty(int(lib.cc_cube_neighbours_ws_size(N, K, Q, NEIGHBOURS, 0)) // 4 + 64, device=dev,
                       dtype=torch.int32)
    torch.cuda.synchronize()
    return {
        'cc_similar_cards_batch': event_ms(lambda: L.call(
            'cc_similar_cards_batch', L.ptr(emb), N, K, Q, L.ptr(q_d), NEIGHBOURS, L.ptr(ws_c), L.ptr(idx),
            L.ptr(dist), None, L.stream_ptr()), repeats),
        'cc_cube_neighbours': event_ms(lambda: L.call(
            'cc_cube_neighbours', L.ptr(index._buf), index.capacity, N, K, Q, L.ptr(q_d), None, None, NEIGHBOURS, 0,
            L.ptr(ws_i), L.ptr(idx), L.ptr(dist), L.stream_ptr()), repeats),
    }


def build_times(n_cubes, repeats):
    from cubecobrarecommender_amd.model import CC_Recommender
    from cubecobrarecommender_amd.synthetic import synthetic_cubes
    indptr, idx = synthetic_cubes(n_cubes, BUILD_V)
    cubes = [idx[indptr[c]:indptr[c + 1]] for c in range(n_cubes)]
    rec = CC_Recommender(BUILD_V, d=BUILD_D, seed=1).recommender()
    times = []
    for i in range(repeats + 1):                     # one warm-up build
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = CubeIndex(rec, cubes)
        torch.cuda.synchronize()
        if i:
            times.append((time.perf_counter() - t0) * 1e3 * 65536 / n_cubes)
        assert len(index) == n_cubes
        del index
    return {'V': BUILD_V, 'd': BUILD_D, 'cubes': n_cubes, 'card_ids': int(indptr[-1]),
            'ms_per_65536_cubes': spread(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--build-cubes', type=int, default=65536, help='0 skips the index build')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cube_similarity_bench needs a GPU: nothing is measured without one')
    if a.repeats < 7:
        raise SystemExit('at least 7 repeats')
    lib = L.lib()
    result = {'K': K, 'Q': Q, 'k': NEIGHBOURS, 'repeats': a.repeats, 'rows_per_launch': 512}

    emb = relu_embeddings(N_BOTH)
    index = CubeIndex.from_latents(emb)
    ids = np.arange(Q, dtype=np.int64) * (N_BOTH // Q)
    first, wall = timed({'similar_many': lambda: similar_many(emb, ids, NEIGHBOURS),
                         'cube_index': lambda: index.neighbours(ids, NEIGHBOURS, exclude_self=False)}, a.repeats, Q)
    (ci, cd), (xi, xd) = first['similar_many'], first['cube_index']
    assert np.array_equal(ci, xi) and np.array_equal(cd.view(np.uint32), xd.view(np.uint32)), 'the paths differ'
    both = {'N': N_BOTH, 'us_per_query': wall, 'rows_equal_bit_for_bit': True,
            'launch_ms': launch_times(emb, index, ids, a.repeats),
            'ws_bytes': {'cc_similar_cards_batch': int(lib.cc_similar_batch_ws_size(N_BOTH, K, Q, NEIGHBOURS)),
                         'cc_cube_neighbours': int(lib.cc_cube_neighbours_ws_size(N_BOTH, K, Q, NEIGHBOURS, 0))},
            'index_bytes': int(lib.cc_cube_index_size(N_BOTH, K))}
    both['bar_met'] = wall['cube_index']['median'] <= wall['similar_many']['median']
    result['both_paths'] = both
    s, c = wall['similar_many'], wall['cube_index']
    print(f"N={N_BOTH} us/query: similar_many {s['median']:.3f} ({s['min']:.3f}..{s['max']:.3f})  cube index "
          f"{c['median']:.3f} ({c['min']:.3f}..{c['max']:.3f})", file=sys.stderr, flush=True)
    del emb, index

    emb = relu_embeddings(N_LARGE, seed=20250302)
    index = CubeIndex.from_latents(emb)
    del emb
    ids = np.arange(Q, dtype=np.int64) * (N_LARGE // Q)
    _, wall = timed({'cube_index': lambda: index.neighbours(ids, NEIGHBOURS, exclude_self=False)}, a.repeats, Q)
    result['large'] = {'N': N_LARGE, 'us_per_query': wall,
                       'ws_bytes': int(lib.cc_cube_neighbours_ws_size(N_LARGE, K, Q, NEIGHBOURS, 0)),
                       'key_matrix_bytes_avoided': Q * N_LARGE * 4,
                       'index_bytes': int(lib.cc_cube_index_size(N_LARGE, K))}
    c = wall['cube_index']
    print(f"N={N_LARGE} us/query: cube index {c['median']:.3f} ({c['min']:.3f}..{c['max']:.3f})  workspace "
          f"{result['large']['ws_bytes'] / 2**20:.1f} MiB", file=sys.stderr, flush=True)
    del index

    if a.build_cubes:
        result['build'] = build_times(a.build_cubes, a.repeats)
        b = result['build']['ms_per_65536_cubes']
        print(f"build: {b['median']:.1f} ms per 65,536 cubes ({b['min']:.1f}..{b['max']:.1f})", file=sys.stderr, flush=True)
    doc = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    print(doc)
    if not both['bar_met']:
        raise SystemExit('the cube index path is above the card path at N = 65,536')


if __name__ == '__main__':
    main()
