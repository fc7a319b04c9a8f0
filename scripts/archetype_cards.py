#!/usr/bin/env python3
"""`archetype_cards.py name k [--m M] [--kind rate|lift|avoid] [--min-count C] [--seed S]
[--max-iter T] [--n-init R]`: the cubes in k archetypes, and the cards that make each.

Loads ml_files/<name> and the cubes the way scripts/cluster_cubes.py does (data/maps/nameToId.json +
data/cube/*.json, or --synthetic C V), clusters them (CubeIndex.cluster) and counts, per archetype
and card, the cubes that hold the card (CubeClusters.signature_cards: integer counts on the GPU,
the same on every run).  Per archetype one line `cluster size`, then its top M signature cards by
name with their rate (share of the archetype's cubes holding the card) and lift (rate minus the
corpus's share).  --kind rate lists the staples, lift (default) what sets the archetype apart,
avoid what the rest of the corpus plays and the archetype does not; --min-count drops cards held
by fewer cubes."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('name')
    ap.add_argument('k', type=int)
    ap.add_argument('--m', type=int, default=10, help='cards per archetype')
    ap.add_argument('--kind', choices=('rate', 'lift', 'avoid'), default='lift')
    ap.add_argument('--min-count', type=int, default=1)
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
    int_to_card = None
    if a.synthetic:
        C, V = a.synthetic
        indptr, idx = synthetic_cubes(C, V, seed=a.seed)
    else:
        V, name_lookup, card_to_int, int_to_card = D.get_card_maps(os.path.join(a.data_dir, 'maps', 'nameToId.json'))
        indptr, idx = D.lists_to_csr(D.build_cube_lists(os.path.join(a.data_dir, 'cube'), name_lookup, card_to_int))
    if V != model.N:
        raise SystemExit(f'the model has {model.N} cards, the data {V}')
    cubes = [idx[indptr[c]:indptr[c + 1]] for c in range(len(indptr) - 1)]
    res = model.cube_index(cubes).cluster(a.k, seed=a.seed, max_iter=a.max_iter, n_init=a.n_init)
    rows = api.archetype_cards(res, cubes, a.m, int_to_card=int_to_card, kind=a.kind, min_count=a.min_count)
    for row in rows:
        print_fn(row['id'], row['size'])
        for card, rate, lift in row['cards']:
            print_fn(f'    {card}  rate {rate:.4f}  lift {lift:+.4f}')
    return rows


if __name__ == '__main__':
    main()
