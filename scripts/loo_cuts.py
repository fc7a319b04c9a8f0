#!/usr/bin/env python3
"""`loo_cuts.py CUBE [N [ROOT]]`: the N cube cards the rest of the cube supports least.

Loads the cube and the model the way scripts/ml_recommend.py does and prints, first cut first, one
line per card: name, p(card | cube without the card), p(card | cube).  The first number is the
leave-one-out score (Recommender.leave_one_out): the model does not see the card it is asked
about; the second is the cut value ml_recommend.py prints.  Flags: --model-dir, --id-map."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('cube_name')
    ap.add_argument('amount', nargs='?', type=int, default=100)
    ap.add_argument('root', nargs='?', default='https://cubecobra.com')
    ap.add_argument('--model-dir', default='ml_files/neg')
    ap.add_argument('--id-map', default='ml_files/recommender_id_map.json')
    return ap.parse_args(argv)


def main(argv=None, print_fn=print):
    a = parse_args(argv)
    from cubecobrarecommender_amd import api
    names = api.fetch_cube_list(a.cube_name, a.root)
    int_to_card, card_to_int = api.load_id_map(a.id_map)
    cube_indices = api.cube_indices_of(names, card_to_int)
    cuts = api.leave_one_out_cuts(api.get_model(a.model_dir), cube_indices, int_to_card)
    for name, (with_card, without) in list(cuts.items())[:max(a.amount, 0)]:
        print_fn(name, without, with_card)
    return cuts


if __name__ == '__main__':
    main()
