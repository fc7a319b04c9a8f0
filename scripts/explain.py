#!/usr/bin/env python3
"""`explain.py CUBE TARGET... [--top N] [--root ROOT]`: which cube cards make the model recommend
a card?

Loads the cube and the model the way scripts/ml_recommend.py does.  For every TARGET (a card name)
prints the name and p(target | cube), then the N cube cards whose removal lowers that probability
most, one line each: name, p(target | cube) - p(target | cube without the card)
(Recommender.leave_one_out with targets).  A TARGET the model does not know is an error.
Flags: --model-dir, --id-map."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('cube_name')
    ap.add_argument('targets', nargs='+', metavar='TARGET')
    ap.add_argument('--top', type=int, default=10)
    ap.add_argument('--root', default='https://cubecobra.com')
    ap.add_argument('--model-dir', default='ml_files/neg')
    ap.add_argument('--id-map', default='ml_files/recommender_id_map.json')
    return ap.parse_args(argv)


def main(argv=None, print_fn=print):
    a = parse_args(argv)
    from cubecobrarecommender_amd import api
    from cubecobrarecommender_amd.names import normalize
    names = api.fetch_cube_list(a.cube_name, a.root)
    int_to_card, card_to_int = api.load_id_map(a.id_map)
    cube_indices = api.cube_indices_of(names, card_to_int)
    target_ids = []
    for t in a.targets:
        if normalize(t) not in card_to_int:
            raise SystemExit(f'unknown card: {t}')
        target_ids.append(card_to_int[normalize(t)])
    result = api.explain(api.get_model(a.model_dir), cube_indices, target_ids, int_to_card, top=a.top)
    for target, why in result.items():
        print_fn(target, why['base'])
        for name, gain in why['cards']:
            print_fn('  ', name, gain)
    return result


if __name__ == '__main__':
    main()
