#!/usr/bin/env python3
"""`similarity_table.py N --out FILE.npz`: the N most similar cards of every card, in one pass.

What scripts/similarity.py prints for one card, for all V of them (cc_similar_cards_batch):
FILE.npz holds `indices` int32 [V, n] and `dists` float32 [V, n] (row j = similarity.py on card j,
the card itself first unless another ties at -1) and `names`, the card names in id order.
Model ml_files/high_req unless --model-dir; --id-map as ml_recommend.py."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cubecobrarecommender_amd import api  # noqa: E402
from cubecobrarecommender_amd.similarity import similarity_table  # noqa: E402


def main(argv=None, print_fn=print):
    ap = argparse.ArgumentParser()
    ap.add_argument('N', type=int)
    ap.add_argument('--out', required=True)
    ap.add_argument('--model-dir', default='ml_files/high_req')
    ap.add_argument('--id-map', default='ml_files/recommender_id_map.json')
    ap.add_argument('--rows-per-launch', type=int, default=512)
    a = ap.parse_args(argv)
    int_to_card, _ = api.load_id_map(a.id_map)
    model = api.get_model(a.model_dir)
    indices, dists = similarity_table(model, a.N, rows_per_launch=a.rows_per_launch)
    names = np.array([int_to_card.get(i, '') for i in range(indices.shape[0])])
    np.savez(a.out, indices=indices, dists=dists, names=names)
    print_fn(f'{a.out}: {indices.shape[0]} cards x {indices.shape[1]} neighbours')
    return indices, dists, names


if __name__ == '__main__':
    main()
