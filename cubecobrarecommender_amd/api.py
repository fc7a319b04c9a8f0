"""The recommend call surface of ``src/scripts/ml_recommend.py`` and ``web/ml_recommend_web.py``,
with the model resident (the reference reloads the ~390 MB SavedModel per web request,
ml_recommend_web.py:37) and the forward + ranking on the GPU (cc_infer_*_fp32 + cc_topn)."""
import json
import os
import threading
import urllib.request

import numpy as np

from .names import normalize

ROOT = 'https://cubecobra.com'
_models = {}
_lock = threading.Lock()


def load_id_map(path='ml_files/recommender_id_map.json'):
    """ml_recommend.py:34-36: {"<int>": "<name>"} -> (int_to_card, card_to_int)."""
    int_to_card = {int(k): v for k, v in json.load(open(path, 'r')).items()}
    return int_to_card, {v: k for k, v in int_to_card.items()}


def fetch_cube_list(cube_name, root=ROOT):
    """ml_recommend.py:22-30: GET <root>/cube/api/cubelist/<cube_name> -> list of names.
    A local directory (or file://) root reads <root>/cube/api/cubelist/<cube_name> from disk."""
    if root.startswith('file://'):
        root = root[len('file://'):]
    if os.path.isdir(root):
        with open(os.path.join(root, 'cube', 'api', 'cubelist', cube_name), 'rb') as fh:
            return fh.read().decode('utf8').split('\n')
    with urllib.request.urlopen(root + '/cube/api/cubelist/' + cube_name) as fp:
        return fp.read().decode('utf8').split('\n')


def cube_indices_of(card_names, card_to_int):
    """ml_recommend.py:42-47: unknown names (custom cards) are skipped; duplicates kept in order."""
    out = []
    for name in card_names:
        idx = card_to_int.get(normalize(name))
        if idx is not None:
            out.append(idx)
    return out


def load_pool(path, card_to_int):
    """A card pool file, one card name per line -> (ids, n_unknown): the ids of the names the
    model knows (normalised as cube_indices_of does, in file order, duplicates kept) and the
    number of non-empty lines it does not.  Pass the ids to Recommender.card_pool."""
    ids, n_unknown = [], 0
    with open(path, 'r', encoding='utf8') as fh:
        for line in fh:
            name = line.strip()
            if not name:
                continue
            idx = card_to_int.get(normalize(name))
            if idx is None:
                n_unknown += 1
            else:
                ids.append(idx)
    return ids, n_unknown


def get_model(path):
    """Resident model per checkpoint directory (thread-safe; Flask runs threaded)."""
    from .model import load_model
    with _lock:
        if path not in _models:
            _models[path] = load_model(path)
        return _models[path]


def recommend_many(model, cubes_indices, amount, int_to_card, pool=None):
    """`recommend` in JSON mode for many cubes at once (Recommender.recommend_many): a list of
    {"additions": {name: p}, "cuts": {name: p}}, one per cube, equal to the single-cube results.
    Any amount stays on the batched path: above cc_recommend_batch_max_amount() (the web
    endpoint's default of 30000 ranks every card) each row is sorted on the device.  pool: a
    CardPool for every cube, or one (or None) per cube: the additions come from the pool alone."""
    cubes_indices = [list(c) for c in cubes_indices]
    outs = model.recommender().recommend_many(cubes_indices, amount, pool=pool)
    result = []
    for cube_indices, out in zip(cubes_indices, outs):
        output = {'additions': {}, 'cuts': {}}
        for idx, p in zip(out['additions'].tolist(), out['add_vals'].tolist()):
            output['additions'][int_to_card[idx]] = p
        for idx, p in zip(list(cube_indices), out['cut_vals'].tolist()):
            output['cuts'][int_to_card[idx]] = p
        result.append(output)
    return result


def similar_cubes(index, cube_indices, k, cube_names=None):
    """"Cubes like this one" for one fresh cube given as card ids, against a cubesim.CubeIndex
    (model.cube_index(cubes)): [(rank, cube, dist)] for ranks 1..min(k, len(index)), nearest first;
    cube is the index's cube id, or cube_names[id] with cube_names (a sequence or a dict)."""
    idx, dists = index.neighbours_of([list(cube_indices)], k)
    return [(i + 1, int(j) if cube_names is None else cube_names[int(j)], float(dv))
            for i, (j, dv) in enumerate(zip(idx[0], dists[0]))]


def cube_clusters_report(clusters, cube_names=None, cubes=None, int_to_card=None, top=10, representatives=5):
    """The host report of a cubecluster.CubeClusters: per cluster a dict of id, size and
    representatives [(cube, similarity)], the up to `representatives` members nearest the centroid
    (cube is the index's cube id, or cube_names[id]; similarity is the cosine, -dist).  With cubes
    (the index's cubes as card-id lists, in id order) also cards [(card, share, lift)]: the up to
    `top` cards held by the largest share of the cluster's cubes (equal shares lower card id
    first; card is the id, or int_to_card[id]), lift their share over the corpus's."""
    N = clusters.N
    name = (lambda j: int(j)) if cube_names is None else (lambda j: cube_names[int(j)])
    card = (lambda c: int(c)) if int_to_card is None else (lambda c: int_to_card[int(c)])
    if cubes is not None:
        lists = [np.unique(np.asarray(c, np.int64).reshape(-1)) for c in cubes][:N]
        V = max([int(l.max()) + 1 for l in lists if len(l)], default=0)
        corpus = np.zeros(V, np.int64)
        for l in lists:
            corpus[l] += 1
    out = []
    for c in range(clusters.k):
        reps = clusters.representatives(c, representatives)
        row = dict(id=c, size=int(clusters.sizes[c]),
                   representatives=[(name(j), float(-clusters.dists[j])) for j in reps])
        if cubes is not None:
            held = np.zeros(V, np.int64)
            members = clusters.members(c)
            for j in members:
                held[lists[int(j)]] += 1
            order = np.argsort(-held, kind='stable')[:max(0, int(top))]
            row['cards'] = [(card(i), held[i] / len(members), (held[i] / len(members)) / (corpus[i] / N))
                            for i in order if held[i] > 0]
        out.append(row)
    return out


def cube_clusters(index, k, cube_names=None, cubes=None, int_to_card=None, top=10, representatives=5, **kw):
    """"What kinds of cube are there" over a cubesim.CubeIndex: index.cluster(k, **kw) (init, seed,
    max_iter, n_init) and its cube_clusters_report."""
    return cube_clusters_report(index.cluster(k, **kw), cube_names, cubes, int_to_card, top, representatives)


def archetype_cards(clusters, cubes_or_corpus, m, int_to_card=None, kind='lift', min_count=1):
    """"Which cards make this archetype" for a cubecluster.CubeClusters and its cubes (card-id lists
    in id order, or an audience.CubeCorpus of them): clusters.signature_cards and, per cluster, a
    dict of id, size and cards [(card, rate, lift)], best first; rate is the share of the cluster's
    cubes that hold the card, lift that minus the corpus's share.  card is the id, or
    int_to_card[id]."""
    res = clusters.signature_cards(cubes_or_corpus, m, kind=kind, min_count=min_count)
    card = (lambda c: int(c)) if int_to_card is None else (lambda c: int_to_card[int(c)])
    return [dict(id=g, size=int(res.sizes[g]),
                 cards=[(card(c), float(res.rate[g, i]), float(res.lift[g, i]))
                        for i, c in enumerate(res.list_of(g).tolist())])
            for g in range(res.G)]


def card_audience(corpus, card_names, k, card_to_int, cube_names=None, include_members=False):
    """"Which cubes want this card" against an audience.CubeCorpus (model.cube_corpus(cubes)): per
    card name of card_names a list of (cube, prob), the up to k cubes with the highest
    p(card | cube) among those that do not play the card yet (every cube with include_members),
    best first, equal probabilities lower cube id first.  cube is the corpus's cube id, or
    cube_names[id] with cube_names (a sequence or a dict).  Names are normalised as
    cube_indices_of does; one the model does not know raises KeyError naming it."""
    card_names = list(card_names)
    ids = []
    for name in card_names:
        idx = card_to_int.get(normalize(name))
        if idx is None:
            raise KeyError(f'unknown card {name!r}')
        ids.append(idx)
    out = corpus.audience(ids, k, include_members=include_members)
    return [[(int(j) if cube_names is None else cube_names[int(j)], float(p))
             for j, p in zip(row[:found].tolist(), prow[:found].tolist())]
            for row, prow, found in zip(out['cubes'], out['probs'], out['found'].tolist())]


def leave_one_out_cuts(model, cube_indices, int_to_card):
    """Honest cut values of one cube: {name: (with, without)} with `with` = p(c | cube), the value
    `recommend` reports under "cuts", and `without` = p(c | cube without c)
    (Recommender.leave_one_out).  Ordered first cut first: `without` ascending, equal values lower
    card id first."""
    ids = np.asarray(list(cube_indices), np.int64).reshape(-1)
    out = model.recommender().leave_one_out([ids])[0]
    result = {}
    for i in np.lexsort((ids, out['loo_vals'])).tolist():
        result.setdefault(int_to_card[int(ids[i])], (float(out['cut_vals'][i]), float(out['loo_vals'][i])))
    return result


def complete_cube(model, cube_indices, size, int_to_card, pool=None, per_step=1):
    """Fill one cube up to `size` cards (Recommender.complete): {"additions": {name: p}} in the
    order the cards were picked, p the probability a card had in the pass that picked it.
    per_step=1 re-scores the cube after every card; pool: a CardPool the cards come from."""
    out = model.recommender().complete(list(cube_indices), size, per_step=per_step, pool=pool)
    return {'additions': {int_to_card[idx]: p for idx, p in zip(out['added'].tolist(), out['added_vals'].tolist())}}


def recommend_diverse(model, cube_indices, amount, int_to_card, trade=0.7, candidates=None, pool=None):
    """`amount` recommendations for one cube, re-ranked for diversity (Recommender.recommend_diverse):
    {"additions": {name: p}, "redundancy": {name: cosine to the nearest card picked before it},
    "base_rank": {name: 0-based position in the plain ranking}}, all in the order picked.
    trade=1 is the plain ranking; pool: a CardPool the cards come from."""
    out = model.recommender().recommend_diverse(list(cube_indices), amount, trade=trade, candidates=candidates,
                                                pool=pool)
    names = [int_to_card[idx] for idx in out['additions'].tolist()]
    return {'additions': dict(zip(names, out['add_vals'].tolist())),
            'redundancy': dict(zip(names, out['redundancy'].tolist())),
            'base_rank': dict(zip(names, out['base_rank'].tolist()))}


def explain(model, cube_indices, target_ids, int_to_card, top=10):
    """Why was a card recommended?  {target name: {"base": p(t | cube), "cards": [(name, gain)]}}
    with gain = p(t | cube) - p(t | cube without c) (a float32 subtraction) for the `top` distinct
    cube cards c with the largest gain, largest first, equal gains lower card id first."""
    ids = np.asarray(list(cube_indices), np.int64).reshape(-1)
    tgt = np.asarray(list(target_ids), np.int64).reshape(-1)
    out = model.recommender().leave_one_out([ids], targets=[tgt])[0]
    cards, first = np.unique(ids, return_index=True)
    result = {}
    for t, card in enumerate(tgt.tolist()):
        base = np.float32(out['base'][t])
        gain = (base - out['without'][first, t]).astype(np.float32)
        best = np.lexsort((cards, -gain))[:max(int(top), 0)]
        result[int_to_card[card]] = {'base': float(base),
                                     'cards': [(int_to_card[int(cards[i])], float(gain[i])) for i in best.tolist()]}
    return result


def _graph_of(adj_mtx):
    """adj_mtx as a GraphRecommender: one passed in is used as it is (its graph stays resident);
    a matrix is uploaded for this call."""
    if hasattr(adj_mtx, 'recommend_many'):
        return adj_mtx
    from . import graphrec
    return graphrec.GraphRecommender(adj_mtx)


def _cube_cards(cube):
    return np.where(np.asarray(cube) == 1)[0]


def simple_recs(cube, adj_mtx, int_to_card=None):
    """src/scripts/recommend.py:7-18: dense 0/1 cube vector in, every missing card out, best
    first (ids, or names with int_to_card).  adj_mtx is the f64 graph or a GraphRecommender; the
    scores are summed and the complete list ordered on the GPU (GraphRecommender.rank_many,
    cc_graph_rank_f64): descending, equal scores higher index first, argsort(kind='stable')[::-1].
    An object that offers recommend_many alone gets its scores ordered on the host that way; the
    list is the same."""
    cube = np.asarray(cube)
    rec = _graph_of(adj_mtx)
    if hasattr(rec, 'rank_many'):
        rec_ids = [int(i) for i in rec.rank_many([_cube_cards(cube)], None, want_vals=False)[0]['additions']]
    else:
        scores = rec.recommend_many([_cube_cards(cube)], 1, want_scores=True)[0]['scores']
        missing = np.where(cube == 0)[0]
        rec_ids = [int(i) for i in missing[np.argsort(scores[missing], kind='stable')[::-1]]]
    return rec_ids if int_to_card is None else [int_to_card[i] for i in rec_ids]


def simple_recs_many(cubes_indices, adj_mtx, int_to_card=None):
    """`simple_recs` for many cubes given as card-id lists: one complete list per cube (ids, or
    names with int_to_card) from one GraphRecommender.rank_many call."""
    outs = _graph_of(adj_mtx).rank_many([list(c) for c in cubes_indices], None, want_vals=False)
    lists = [[int(i) for i in o['additions']] for o in outs]
    return lists if int_to_card is None else [[int_to_card[i] for i in ids] for ids in lists]


def simple_cuts(cube, adj_mtx, int_to_card=None):
    """src/scripts/cut_cards.py:7-18: dense 0/1 cube vector in, the cube's cards out, first cut
    first (ascending score, equal scores lower index first).  Unlike the reference this does not
    zero the caller's diagonal: the kernel never reads it as a value."""
    rec_ids = [int(i) for i in _graph_of(adj_mtx).recommend_many([_cube_cards(cube)], 1)[0]['cuts']]
    return rec_ids if int_to_card is None else [int_to_card[i] for i in rec_ids]


def graph_rec_max_amount():
    """cc_graph_rec_max_amount(): the most additions the graph's select path returns."""
    from . import _lib
    return int(_lib.lib().cc_graph_rec_max_amount())


def graph_recommend(rec, cube_indices, amount, int_to_card):
    """The co-occurrence baseline in `recommend`'s JSON shape: {"additions": {name: score},
    "cuts": {name: score}} from GraphRecommender `rec`, the additions best first (`amount` of
    them), the cuts first cut first (every distinct cube card).  An amount above
    cc_graph_rec_max_amount() goes through rec.rank_many where `rec` offers it."""
    if hasattr(rec, 'rank_many') and int(amount) > graph_rec_max_amount():
        out = rec.rank_many([list(cube_indices)], amount)[0]
    else:
        out = rec.recommend_many([list(cube_indices)], amount)[0]
    output = {'additions': {}, 'cuts': {}}
    for idx, s in zip(out['additions'].tolist(), out['add_vals'].tolist()):
        output['additions'][int_to_card[idx]] = s
    for idx, s in zip(out['cuts'].tolist(), out['cut_vals'].tolist()):
        output['cuts'][int_to_card[idx]] = s
    return output


def recommend(model, cube_indices, amount, int_to_card, non_json=False, print_fn=print, print_cuts=True,
              pool=None):
    """ml_recommend.py:78-116 / ml_recommend_web.py:39-67 on the GPU.  Returns
    {"additions": {name: p}, "cuts": {name: p}} (additions empty in non_json mode, as the reference
    prints instead of storing them).  print_cuts: in non_json mode also print the lowest-scoring
    cuts — the CLI does (ml_recommend.py:110-116), the web function does not
    (ml_recommend_web.py:50-67 prints only the additions).  pool: a CardPool; the additions then
    come from the pool alone (the cuts are every cube card's, as without one)."""
    out = model.recommender().recommend(cube_indices, amount, pool=pool)
    output = {'additions': {}, 'cuts': {}}
    for idx, p in zip(out['additions'].tolist(), out['add_vals'].tolist()):
        card = int_to_card[idx]
        if non_json:
            print_fn(card)
        else:
            output['additions'][card] = p
    for idx, p in zip(list(cube_indices), out['cut_vals'].tolist()):
        output['cuts'][int_to_card[idx]] = p
    if non_json and print_cuts:   # ml_recommend.py:110-116: lowest-scoring cuts
        cards = list(output['cuts'].keys())
        vals = list(output['cuts'].values())
        rank_cuts = np.argsort(np.array(vals), kind='stable')
        print_fn('\n')
        for i in range(min(int(amount), len(cards))):
            print_fn(cards[rank_cuts[i]], vals[rank_cuts[i]])
    return output
