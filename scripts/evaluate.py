#!/usr/bin/env python3
"""Held-out evaluation of a saved model: `evaluate.py name [K ...]` (K defaults to 10 50 100).

Loads ml_files/<name> with load_model and the cubes the way scripts/train.py does
(data/maps/nameToId.json + data/cube/*.json, or --synthetic C V with the same seed argument), hides
--hide of every cube's cards, ranks the hidden ones on the GPU and prints one JSON line:
recall@K, ndcg@K, hit_rate@K for each K, mrr, n_cubes, n_targets, hits (the device's counters).
--loss adds bce and output_1_accuracy of the whole, clean cubes (the reconstruction output's loss
and categorical accuracy, as CC_Recommender.evaluate reports them).
--baseline adds "cooccurrence": the same metrics on the same split for the co-occurrence baseline
(GraphRecommender), its graph built on the GPU from the visible parts of the cubes only: no hidden
card leaks into it.
--pool FILE (one card name per line; with --synthetic the names are the card ids in decimal) ranks
every hidden card among the file's cards alone and adds n_targets_outside_pool, the hidden cards
dropped because the file does not hold them.  The baseline has no pools: --baseline with --pool is
an error."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('name')
    ap.add_argument('ks', nargs='*', type=int, default=[10, 50, 100])
    ap.add_argument('--hide', type=float, default=0.2, help='fraction below 1, or a count')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--loss', action='store_true', help='also report bce and output_1_accuracy')
    ap.add_argument('--baseline', action='store_true', help='also report the co-occurrence baseline')
    ap.add_argument('--synthetic', nargs=2, type=int, metavar=('C', 'V'))
    ap.add_argument('--data-dir', default='./data')
    ap.add_argument('--out-dir', default='./ml_files')
    ap.add_argument('--pool', default=None, help='file of card names: rank hidden cards among these alone')
    a = ap.parse_args(argv)
    if a.pool and a.baseline:
        ap.error('--baseline has no card pools: drop --pool or --baseline')
    from cubecobrarecommender_amd import data as D
    from cubecobrarecommender_amd import graphrec
    from cubecobrarecommender_amd.evaluate import evaluate_holdout, evaluate_loss, holdout_split
    from cubecobrarecommender_amd.model import load_model
    from cubecobrarecommender_amd.synthetic import synthetic_cubes
    model = load_model(os.path.join(a.out_dir, a.name))
    if a.synthetic:
        C, V = a.synthetic
        indptr, idx = synthetic_cubes(C, V, seed=a.seed)
        card_to_int = {str(i): i for i in range(V)}
    else:
        V, name_lookup, card_to_int, _ = D.get_card_maps(os.path.join(a.data_dir, 'maps', 'nameToId.json'))
        indptr, idx = D.lists_to_csr(D.build_cube_lists(os.path.join(a.data_dir, 'cube'), name_lookup, card_to_int))
    if V != model.N:
        raise SystemExit(f'the model has {model.N} cards, the data {V}')
    cubes = [idx[indptr[c]:indptr[c + 1]] for c in range(len(indptr) - 1)]
    hide = int(a.hide) if a.hide >= 1 else a.hide
    pool, pool_info = None, {}
    if a.pool:
        from cubecobrarecommender_amd import api
        ids, n_unknown = api.load_pool(a.pool, card_to_int)
        pool = model.recommender().card_pool(ids)
        pool_info = {'pool': a.pool, 'pool_size': pool.size, 'pool_unknown_names': n_unknown}
    out = evaluate_holdout(model, cubes, ks=a.ks or [10, 50, 100], hide=hide, seed=a.seed, pool=pool)
    out = {'name': a.name, 'cubes': len(cubes), 'hide': hide, 'seed': a.seed, **pool_info, **out}
    if a.loss:
        e = evaluate_loss(model, cubes)
        out.update({'bce': e['bce'], 'output_1_accuracy': e['output_1_accuracy']})
    if a.baseline:
        visible, _ = holdout_split(cubes, hide=hide, seed=a.seed)      # evaluate_holdout's own split
        graph = graphrec.GraphRecommender.from_cubes(*D.lists_to_csr(visible), V)
        out['cooccurrence'] = evaluate_holdout(graph, cubes, ks=a.ks or [10, 50, 100], hide=hide, seed=a.seed)
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
