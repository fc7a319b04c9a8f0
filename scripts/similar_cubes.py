#!/usr/bin/env python3
"""`similar_cubes.py name k [--query I ...] [--out FILE.npz]`: the k cubes most like a cube.

Loads ml_files/<name> and the cubes the way scripts/evaluate.py does (data/maps/nameToId.json +
data/cube/*.json, or --synthetic C V with the same seed argument), encodes every cube on the GPU
into a resident index (CubeIndex) and ranks by the cosine distance of the encoder's latents, as
scripts/similarity.py does for cards.
With --query the k nearest cubes of those cube ids are printed, one line per neighbour: query,
rank, cube id, distance (the cube itself is left out).
Without it the neighbours of every cube are written to --out: `indices` int32 [C, n] and `dists`
float32 [C, n], n = min(k, C - 1); one summary line is printed."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('name')
    ap.add_argument('k', type=int)
    ap.add_argument('--query', nargs='+', type=int, default=None, metavar='I', help='cube ids to ask about')
    ap.add_argument('--out', default=None, help='FILE.npz for the table of every cube')
    ap.add_argument('--synthetic', nargs=2, type=int, metavar=('C', 'V'))
    ap.add_argument('--data-dir', default='./data')
    ap.add_argument('--out-dir', default='./ml_files')
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args(argv)
    if a.query is None and not a.out:
        ap.error('give --query I ... or --out FILE.npz')
    return a


def main(argv=None, print_fn=print):
    a = parse_args(argv)
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
    index = model.cube_index(cubes)
    if a.query is not None:
        indices, dists = index.neighbours(a.query, a.k)
        for q, row, drow in zip(a.query, indices, dists):
            for rank, (j, dv) in enumerate(zip(row.tolist(), drow.tolist())):
                print_fn(q, rank + 1, j, dv)
    else:
        indices, dists = index.table(a.k)
    if a.out:
        np.savez(a.out, indices=indices, dists=dists)
        print_fn(f'{a.out}: {indices.shape[0]} cubes x {indices.shape[1]} neighbours')
    return indices, dists


if __name__ == '__main__':
    main()
