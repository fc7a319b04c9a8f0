#!/usr/bin/env python3
"""`card_audience.py name CARD [CARD ...] [--k K]`: the cubes that most want a card.

Loads ml_files/<name> and the cubes the way scripts/similar_cubes.py does (data/maps/nameToId.json
+ data/cube/*.json, or --synthetic C V with the same seed argument), runs every cube's forward pass
on the GPU into a resident corpus (CubeCorpus) and ranks, per card, the cubes that do not play it
yet by p(card | cube) (every cube with --include-members).  A card is a name of the map, or a
card id with --synthetic.
Prints one JSON document: {card: {"members", "candidates", "above", "cubes": [[cube id, p], ...]}},
members the cubes that hold the card, candidates the cubes ranked, above those among them with
p >= --threshold."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('name')
    ap.add_argument('cards', nargs='+', metavar='CARD')
    ap.add_argument('--k', type=int, default=20, help='cubes per card')
    ap.add_argument('--include-members', action='store_true', help='rank the cubes that hold the card, too')
    ap.add_argument('--threshold', type=float, default=0.5)
    ap.add_argument('--synthetic', nargs=2, type=int, metavar=('C', 'V'))
    ap.add_argument('--data-dir', default='./data')
    ap.add_argument('--out-dir', default='./ml_files')
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args(argv)
    if not 0.0 <= a.threshold <= 1.0:
        ap.error('--threshold must lie in [0, 1]')
    if a.synthetic:
        try:
            a.cards = [int(c) for c in a.cards]
        except ValueError:
            ap.error('with --synthetic a CARD is a card id')
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
        ids = a.cards
    else:
        V, name_lookup, card_to_int, _ = D.get_card_maps(os.path.join(a.data_dir, 'maps', 'nameToId.json'))
        indptr, idx = D.lists_to_csr(D.build_cube_lists(os.path.join(a.data_dir, 'cube'), name_lookup, card_to_int))
        unknown = [c for c in a.cards if c not in card_to_int]
        if unknown:
            raise SystemExit(f'unknown card {unknown[0]!r}')
        ids = [card_to_int[c] for c in a.cards]
    if V != model.N:
        raise SystemExit(f'the model has {model.N} cards, the data {V}')
    cubes = [idx[indptr[c]:indptr[c + 1]] for c in range(len(indptr) - 1)]
    out = model.cube_corpus(cubes).audience(ids, a.k, include_members=a.include_members, threshold=a.threshold)
    doc = {}
    for t, card in enumerate(a.cards):
        found = int(out['found'][t])
        doc[str(card)] = {'members': int(out['members'][t]), 'candidates': int(out['candidates'][t]),
                          'above': int(out['above'][t]),
                          'cubes': [[int(j), float(p)] for j, p in zip(out['cubes'][t, :found], out['probs'][t, :found])]}
    print_fn(json.dumps(doc))
    return doc


if __name__ == '__main__':
    main()
