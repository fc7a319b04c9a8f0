#!/usr/bin/env python3
"""`complete_cube.py CUBE SIZE [ROOT]`: fill a cube up to SIZE cards, the cube re-scored after
every pick.

CUBE is a cube name (loaded the way scripts/ml_recommend.py does) or a file of card names, one per
line.  Prints one line per added card in the order picked: name, the probability it had when it
was picked (Recommender.complete: greedy completion on the device).  --per-step M lets the best M
cards join per forward pass (1: exact greedy); --pool FILE (card names, one per line) takes the
cards from that list alone.  Flags: --model-dir, --id-map."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('cube')
    ap.add_argument('size', type=int)
    ap.add_argument('root', nargs='?', default='https://cubecobra.com')
    ap.add_argument('--pool', default=None, metavar='FILE')
    ap.add_argument('--per-step', type=int, default=1)
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
    out = api.complete_cube(model, cube_indices, a.size, int_to_card, pool=pool, per_step=a.per_step)
    for name, p in out['additions'].items():
        print_fn(name, p)
    return out


if __name__ == '__main__':
    main()
