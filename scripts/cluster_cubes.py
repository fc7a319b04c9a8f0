#!/usr/bin/env python3
"""`cluster_cubes.py name k [--out FILE.npz] [--seed S] [--max-iter T] [--n-init R]`: the cubes in k
archetypes.

Loads ml_files/<name> and the cubes the way scripts/similar_cubes.py does (data/maps/nameToId.json +
data/cube/*.json, or --synthetic C V with the same seed argument), encodes every cube on the GPU
into a resident index (CubeIndex) and groups them by deterministic spherical k-means on the
encoder's latents (CubeIndex.cluster): the same bits on every run.
One line per cluster is printed: cluster, size, then the cubes nearest its centroid with their
cosine similarity.  With --out, `labels` int32 [C], `dists` float32 [C], `centroids` float32
[k, 64] and `sizes` int32 [k] are written."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('name')
    ap.add_argument('k', type=int)
    ap.add_argument('--out', default=None, help='FILE.npz for labels, dists, centroids and sizes')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--max-iter', type=int, default=50)
    ap.add_argument('--n-init', type=int, default=1)
    ap.add_argument('--synthetic', nargs=2, type=int, metavar=('C', 'V'))
    ap.add_argument('--data-dir', default='./data')
    ap.add_argument('--out-dir', default='./ml_files')
    return ap.parse_args(argv)


def main(argv=None, print_fn=print):
    a = parse_args(argv)
    from cubecobrarecommender_amd import api
    from cubecobrarecommender_amd import data as D
    from cubecobrarecommender_amd.model import load_model
    from cubecobrarecommender_amd.synthetic import synthetic_cubes
    model = load_model(os.path.join(a.out_dir, a.name))
    if a.synthetic:
        C, V = a.synthetic
        indptr, idx = synthetic_cubes(C, V, seed=a.seed)
    else:
        V, name_lookup, card_to_int, _ = D.get_card_maps(os.path.join(a.data_dir, 'maps', 'nameToId.json'))
        indptr, idx = D.lists_to_csr(D.build_cube_lists(os.path.join(a.data_dir, 'cube'), name_lookup, card_to_int))
    if V != model.N:
        raise SystemExit(f'the model has {model.N} cards, the data {V}')
    cubes = [idx[indptr[c]:indptr[c + 1]] for c in range(len(indptr) - 1)]
    res = model.cube_index(cubes).cluster(a.k, seed=a.seed, max_iter=a.max_iter, n_init=a.n_init)
    for row in api.cube_clusters_report(res, representatives=5):
        print_fn(row['id'], row['size'], ' '.join(f'{j}:{s:.4f}' for j, s in row['representatives']))
    if a.out:
        np.savez(a.out, labels=res.labels, dists=res.dists, centroids=res.centroids, sizes=res.sizes)
        print_fn(f'{a.out}: {res.N} cubes in {res.k} clusters, {res.n_iter} iterations'
                 f'{"" if res.converged else " (not converged)"}, objective {res.objective:.6f}')
    return res


if __name__ == '__main__':
    main()
