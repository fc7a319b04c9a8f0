#!/usr/bin/env python3
"""Drop-in for src/scripts/recommend.py: `recommend.py cube_name [amount]`.

Same arguments, files and output as the reference (recommend.py:20-67): the cube list is fetched,
output/full_adj_mtx.npy and output/int_to_card.json are read, and the `amount` (default 100) best
missing cards are printed as "<rank>: <name>".  The column sums and the ranking run on the GPU
(GraphRecommender; any amount: above the select path's limit every card is sorted on the
device).  Extra optional flags: --adj, --id-map, --root."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from cubecobrarecommender_amd import api, graphrec  # noqa: E402


def load(a, print_fn=print):
    """The steps both graph scripts share -> (GraphRecommender, cube_indices, int_to_card)."""
    print_fn('Getting Cube List . . . \n')
    names = api.fetch_cube_list(a.cube_name, a.root)
    print_fn('Loading Adjacency Matrix . . . \n')
    rec = graphrec.GraphRecommender(np.load(a.adj))
    print_fn('Loading Card Name Lookup . . . \n')
    int_to_card, card_to_int = api.load_id_map(a.id_map)
    print_fn('Creating Cube Vector . . . \n')
    return rec, api.cube_indices_of(names, card_to_int), int_to_card


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('cube_name')
    ap.add_argument('amount', nargs='?', type=int, default=100)
    ap.add_argument('--adj', default='output/full_adj_mtx.npy')
    ap.add_argument('--id-map', default='output/int_to_card.json')
    ap.add_argument('--root', default=api.ROOT)
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    rec, cube_indices, int_to_card = load(a)
    print('Generating Recommendations . . . \n')
    out = api.graph_recommend(rec, cube_indices, a.amount, int_to_card)
    for i, name in enumerate(out['additions']):
        print(str(i + 1) + ':', name)
    return out


if __name__ == '__main__':
    main()
