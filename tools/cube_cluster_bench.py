"""Cube archetypes: cc_cube_cluster beside a torch loop on the same normalised latents, and the
assign kernel's rate beside the neighbours' distance tile.

Workload: K = 64, `relu` latents max(normal, 0) from a fixed seed, start ids from a fixed seed;
N = 65,536 with k = 256 and N = 2^20 with k = 1,024.

1. Times (the default run).  Device time between two events on the stream, both paths alternating
   inside one run after a warm-up of each, every repeat kept, with median and min..max:
     cc_cube_cluster at max_iter = 0 (one assign) and at max_iter = ITERS (ITERS updates, ITERS + 1
     assigns; none of the shapes converges that early), per iteration their difference over ITERS;
     the torch loop (`n @ c.T`, argmax, index_add_, normalise: what the library offered before)
     over the same start and the same number of assigns and updates.
   The torch path may fuse multiply-adds and use matrix cores, and its index_add_ adds atomically:
   it is neither the pinned arithmetic nor reproducible, so labels are compared by count only.
   Both workspaces are reported: cc_cube_cluster_ws_size against the [N][k] fp32 scores, the int64
   labels and the [k][K] sums of the torch loop.
2. Kernel rate (`--trace-workload`, run under `rocprofv3 --kernel-trace --stats`, no counters; then
   `--trace-stats DIR` reads the kernel statistics it wrote).  At N = 65,536: assign_kernel<8>'s
   time per separately rounded operation (2 N k K per launch) over dist_chunk_kernel<8>'s (2 Q N K
   per launch of a CubeIndex.neighbours call of Q = 512 over the same index).  The bar: the ratio is
   not above 1.10.

    python tools/cube_cluster_bench.py [--repeats 7] [--out FILE]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/cube_cluster_bench.py --trace-workload
    python tools/cube_cluster_bench.py --trace-stats DIR [--out FILE]      (no GPU needed)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, ITERS, Q_NEIGH, K_NEIGH = 64, 8, 512, 40
SHAPES = ((1 << 16, 256), (1 << 20, 1024))
BAR = 1.10


def spread(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'repeats': list(v)}


def relu_index(N, seed=20250401):
    import torch
    from cubecobrarecommender_amd.cubesim import CubeIndex
    rng = np.random.default_rng(seed)
    emb = torch.from_numpy(np.maximum(rng.standard_normal((N, K), dtype=np.float32), 0)).cuda()
    return CubeIndex.from_latents(emb), torch.nn.functional.normalize(emb, dim=1)


class Native:
    """cc_cube_cluster by direct calls on kept buffers (no host packing, no copies back)."""

    def __init__(self, index, N, k, init, max_iter):
        import torch
        from cubecobrarecommender_amd import _lib as L
        dev = index.dev
        self.L, self.index, self.N, self.k, self.max_iter = L, index, N, k, max_iter
        self.ws_bytes = int(L.lib().cc_cube_cluster_ws_size(N, K, k, 0))
        self.ws = torch.empty(self.ws_bytes // 4 + 64, device=dev, dtype=torch.int32)
        self.ids = torch.from_numpy(init).to(dev)
        self.lab = torch.empty(N, device=dev, dtype=torch.int32)
        self.dist = torch.empty(N, device=dev, dtype=torch.float32)
        self.cent = torch.empty(k, K, device=dev, dtype=torch.float32)
        self.tail = torch.empty(k + max_iter + 2, device=dev, dtype=torch.int32)

    def __call__(self):
        L, k = self.L, self.k
        L.call('cc_cube_cluster', L.ptr(self.index._buf), self.index.capacity, self.N, K, k, L.ptr(self.ids),
               self.max_iter, L.ptr(self.ws), L.ptr(self.lab), L.ptr(self.dist), L.ptr(self.cent), L.ptr(self.tail),
               L.ptr(self.tail[k:]), L.ptr(self.tail[-1:]), L.stream_ptr())

    def n_iter(self):
        return int(self.tail[-1].item())


def torch_loop(n, init, max_iter):
    """max_iter updates and max_iter + 1 assigns from the rows `init`; the labels."""
    import torch
    c = n[init.long()].clone()
    for t in range(max_iter + 1):
        lab = (n @ c.T).argmax(1)
        if t == max_iter:
            break
        S = torch.zeros_like(c).index_add_(0, lab, n)
        live = torch.zeros(len(c), device=n.device, dtype=torch.bool).index_fill_(0, lab, True)
        c = torch.where(live[:, None], torch.nn.functional.normalize(S, dim=1), c)
    return lab


def event_ms(fns, repeats):
    """Device ms of each named call between two events, alternating; two warm-up rounds first."""
    import torch
    times = {name: [] for name in fns}
    for i in range(repeats + 2):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= 2:
                times[name].append(a.elapsed_time(b))
    return {name: spread(v) for name, v in times.items()}


def measure(N, k, repeats):
    import torch
    index, n = relu_index(N)
    init = np.random.default_rng(7).choice(N, k, replace=False).astype(np.int32)
    init_d = torch.from_numpy(init).cuda()
    one, run = Native(index, N, k, init, 0), Native(index, N, k, init, ITERS)
    ms = event_ms({'native_one_assign': one, 'native_run': run, 'torch_one_assign': lambda: torch_loop(n, init_d, 0),
                   'torch_run': lambda: torch_loop(n, init_d, ITERS)}, repeats)
    torch.cuda.synchronize()
    assert run.n_iter() == ITERS, f'converged after {run.n_iter()} iterations: the run is shorter than it is timed as'
    labels = torch_loop(n, init_d, ITERS)
    per_iter = {p: (ms[p + '_run']['median'] - ms[p + '_one_assign']['median']) / ITERS for p in ('native', 'torch')}
    out = {'N': N, 'k': k, 'K': K, 'iterations': ITERS, 'ms': ms, 'ms_per_iteration': per_iter,
           'labels_equal_to_torch': int((labels.int() == run.lab).sum().item()),
           'ws_bytes': {'cc_cube_cluster': run.ws_bytes, 'torch_loop': N * k * 4 + N * 8 + k * K * 4},
           'ws_bound_bytes': 2 * N * K * 4 + N * k // 64 + 64 * k * K + (1 << 20)}
    assert out['ws_bytes']['cc_cube_cluster'] <= out['ws_bound_bytes']
    print(f"N={N} k={k}: run of {ITERS} iterations native {ms['native_run']['median']:.3f} ms "
          f"({ms['native_run']['min']:.3f}..{ms['native_run']['max']:.3f}), torch {ms['torch_run']['median']:.3f} ms "
          f"({ms['torch_run']['min']:.3f}..{ms['torch_run']['max']:.3f}); per iteration {per_iter['native']:.3f} / "
          f"{per_iter['torch']:.3f} ms; workspace {run.ws_bytes / 2**20:.1f} / "
          f"{out['ws_bytes']['torch_loop'] / 2**20:.1f} MiB", file=sys.stderr, flush=True)
    return out


def trace_workload():
    """What the kernel trace is taken of: at N = 65,536, five cluster runs of 2 iterations (15
    assign launches) and five neighbours calls of Q = 512 (one distance-tile launch each)."""
    import torch
    N, k = SHAPES[0]
    index, _ = relu_index(N)
    init = np.random.default_rng(7).choice(N, k, replace=False).astype(np.int32)
    run = Native(index, N, k, init, 2)
    ids = np.arange(Q_NEIGH, dtype=np.int64) * (N // Q_NEIGH)
    for _ in range(5):
        run()
        torch.cuda.synchronize()
        index.neighbours(ids, K_NEIGH, exclude_self=False, rows_per_launch=Q_NEIGH)
    assert run.n_iter() == 2


def trace_stats(root):
    """The two kernels' average times out of rocprofv3's kernel statistics under `root`."""
    files = sorted(glob.glob(os.path.join(root, '**', '*kernel_stats.csv'), recursive=True))
    if not files:
        raise SystemExit(f'no *kernel_stats.csv under {root}')
    N, k = SHAPES[0]
    found = {}
    for row in csv.DictReader(open(files[-1])):
        for name in ('assign_kernel', 'dist_chunk_kernel'):
            if name in row['Name']:
                found[name] = {'name': row['Name'], 'calls': int(row['Calls']), 'average_ns': float(row['AverageNs']),
                               'min_ns': float(row['MinNs']), 'max_ns': float(row['MaxNs'])}
    if len(found) != 2:
        raise SystemExit(f'{files[-1]}: assign_kernel and dist_chunk_kernel are not both in it')
    ops = {'assign_kernel': 2 * N * k * K, 'dist_chunk_kernel': 2 * Q_NEIGH * N * K}
    for name, f in found.items():
        f['ops_per_launch'] = ops[name]
        f['ps_per_op'] = f['average_ns'] * 1e3 / ops[name]
    ratio = found['assign_kernel']['ps_per_op'] / found['dist_chunk_kernel']['ps_per_op']
    return {'file': os.path.basename(files[-1]), 'N': N, 'k': k, 'Q': Q_NEIGH, 'kernels': found,
            'assign_over_dist_chunk': ratio, 'bar': BAR, 'bar_met': ratio <= BAR}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default='')
    ap.add_argument('--trace-workload', action='store_true')
    ap.add_argument('--trace-stats', default='', metavar='DIR')
    a = ap.parse_args()
    if a.trace_stats:
        result = {'kernel_rate': trace_stats(a.trace_stats)}
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit('cube_cluster_bench needs a GPU: nothing is measured without one')
        if a.trace_workload:
            return trace_workload()
        if a.repeats < 7:
            raise SystemExit('at least 7 repeats')
        result = {'repeats': a.repeats, 'shapes': [measure(N, k, a.repeats) for N, k in SHAPES]}
    doc = json.dumps(result)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        if os.path.exists(a.out):                    # the other half of the document is kept
            doc = json.dumps({**json.load(open(a.out)), **result})
        with open(a.out, 'w') as fh:
            fh.write(doc + '\n')
    print(doc)
    if a.trace_stats and not result['kernel_rate']['bar_met']:
        raise SystemExit(f"assign_kernel is {result['kernel_rate']['assign_over_dist_chunk']:.3f} x dist_chunk_kernel "
                         f"per operation, above {BAR}")


if __name__ == '__main__':
    main()
