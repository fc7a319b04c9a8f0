#!/usr/bin/env python3
"""`recommend_diverse.py CUBE AMOUNT [ROOT]`: AMOUNT recommendations for a cube, re-ranked so that
near-substitutes do not crowd the list.

CUBE is a cube name (loaded the way scripts/ml_recommend.py does) or a file of card names, one per
line.  Prints one line per card in the order picked: name, its probability, the cosine to the
nearest card picked before it, its position in the plain ranking (Recommender.recommend_diverse:
greedy maximal marginal relevance on the device).  --trade T in [0, 1] weighs probability against
redundancy (1: the plain ranking); --candidates M re-ranks the first M cards of the plain ranking;
--pool FILE (card names, one per line) takes the cards from that list alone.  Flags: --model-dir,
--id-map."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('cube')
    ap.add_argument('amount', type=int)
    ap.add_argument('root', nargs='?', default='https://cubecobra.com')
    ap.add_argument('--trade', type=float, default=0.7)
    ap.add_argument('--candidates', type=int, default=None)
    ap.add_argument('--pool', default=None, metavar='FILE')
    ap.add_argument('--model-dir', default='ml_files/neg')
    ap.add_argument('--id-map', default='ml_files/recommender_id_map.json')
    return ap.parse_args(argv)


def main(argv=None, print_fn=print):
    a = parse_args(argv)
    from cubecobrarecommender_amd import api
    if os.path.isfile(a.cube):
        with open(a.cube, 'r', encoding='utf8') as fh:
            names = fh.read().split('\n')
    else:
        names = api.fetch_cube_list(a.cube, a.root)
    int_to_card, card_to_int = api.load_id_map(a.id_map)
    cube_indices = api.cube_indices_of(names, card_to_int)
    model = api.get_model(a.model_dir)
    pool = None
    if a.pool:
        ids, n_unknown = api.load_pool(a.pool, card_to_int)
        if n_unknown:
            print(f'{n_unknown} pool lines name no card the model knows', file=sys.stderr)
        pool = model.recommender().card_pool(ids)
    out = api.recommend_diverse(model, cube_indices, a.amount, int_to_card, trade=a.trade, candidates=a.candidates,
                                pool=pool)
    for name, p in out['additions'].items():
        print_fn(name, p, out['redundancy'][name], out['base_rank'][name])
    return out


if __name__ == '__main__':
    main()
