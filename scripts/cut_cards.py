#!/usr/bin/env python3
"""Drop-in for src/scripts/cut_cards.py: `cut_cards.py cube_name [amount]`.

Same arguments, files and output as the reference (cut_cards.py:20-67): the `amount` (default
100) cube cards that co-occur least with the rest of the cube, printed as "<rank>: <name>", first
cut first.  A cube of fewer cards prints them all (the reference raises IndexError there)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cubecobrarecommender_amd import api  # noqa: E402
from scripts import recommend as graph_cli  # noqa: E402


def main(argv=None):
    a = graph_cli.parser().parse_args(argv)
    rec, cube_indices, int_to_card = graph_cli.load(a)
    print('Generating Recommendations . . . \n')
    out = api.graph_recommend(rec, cube_indices, 1, int_to_card)
    cuts = list(out['cuts'])[:max(a.amount, 0)]
    for i, name in enumerate(cuts):
        print(str(i + 1) + ':', name)
    return {'cuts': {name: out['cuts'][name] for name in cuts}}


if __name__ == '__main__':
    main()
