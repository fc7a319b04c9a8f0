"""CPU tests of leave-one-out's host side: the two bindings against the header, the argument checks
of cc_leave_one_out_fp32 with never-dereferenced pointers, the planning of derived rows (slicing a
cube across launches, out_ptr, the scatter into input order with duplicates, target splitting)
against a small pure-Python restatement, api.explain / api.leave_one_out_cuts on a stub
recommender, and the checks that come before any launch."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd import api, leaveoneout
from cubecobrarecommender_amd.leaveoneout import Plan, chunk_slots, plan_rows, target_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_args(name):
    hdr = open(os.path.join(ROOT, 'include', 'ccrec.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    args = re.search(r'\b' + name + r'\s*\(([^)]*)\)', hdr).group(1)
    return [a.strip() for a in args.split(',') if a.strip() and a.strip() != 'void']


def test_signatures_match_the_header():
    i32, P, SZ = C.c_int32, C.c_void_p, C.c_size_t
    assert L.SIGNATURES['cc_leave_one_out_ws_size'] == (SZ, [i32] * 5)
    assert L.SIGNATURES['cc_leave_one_out_fp32'] == (
        C.c_int, [P, i32, i32, i32, P, P, i32, i32, P, P, P, P, P, P, P, SZ, P])
    lib = L.lib()
    for name, count in (('cc_leave_one_out_ws_size', 5), ('cc_leave_one_out_fp32', 17)):
        args = header_args(name)
        assert len(L.SIGNATURES[name][1]) == len(args) == count, name
        for ctype, decl in zip(L.SIGNATURES[name][1], args):       # a pointer where the header has one
            assert (ctype is P) == ('*' in decl), (name, decl)
        assert hasattr(lib, name)
    assert lib.cc_abi_version() == 2


def test_workspace_is_bounded_by_rows_and_the_largest_cube():
    ws = lambda d, c, n, r: int(L.lib().cc_leave_one_out_ws_size(22000, d, c, n, r))      # noqa: E731
    d = 512
    # the formula: two rectangles of chunk partials, then e1, zlat, h3 and one_ptr per row
    for c, n, r in ((1, 0, 1), (1, 360, 361), (11, 360, 3971), (3, 97, 7), (1, 10000, 4096)):
        exact = 2 * c * chunk_slots(n) * d * 4 + r * (2 * d + 64) * 4 + (r + 1) * 4
        assert exact <= ws(d, c, n, r) <= exact + 6 * 256 and ws(d, c, n, r) % 256 == 0
    # a cube of 10,000 cards sliced into launches of 4096 rows never takes 10,001 rows of workspace
    assert ws(d, 1, 10000, 4096) < ws(d, 1, 10000, 10001) // 2
    # every launch the planner makes stays within rows_per_launch // 8 slots or the one largest cube
    ns = [10000] + [1] * 300 + [360] * 20
    for rpl in (1, 7, 512, 4096):
        for slices in plan_rows(ns, rpl):
            cubes = sorted({c for c, _, _ in slices})
            cap = max(chunk_slots(ns[c]) for c in cubes)
            assert len(cubes) * cap <= max(4, rpl // 8) or len(cubes) == 1
            assert sum(q1 - q0 for _, q0, q1 in slices) <= rpl


def test_argument_checks_without_a_gpu():
    lib = L.lib()
    one = C.c_void_p(4096)                       # never dereferenced: every call fails or launches nothing
    need = int(lib.cc_leave_one_out_ws_size(100, 64, 2, 40, 50))

    def call(params=one, V=100, d=64, n_cubes=2, row_ptr=one, idx=one, max_n=40, rows=50, row_cube=one, row_pos=one,
             tgt_ptr=None, tgt=None, out_ptr=one, out=one, ws=one, ws_bytes=need):
        return lib.cc_leave_one_out_fp32(params, V, d, n_cubes, row_ptr, idx, max_n, rows, row_cube, row_pos, tgt_ptr,
                                         tgt, out_ptr, out, ws, ws_bytes, None)

    def failed(what):
        msg = lib.cc_last_error_string()
        return b'cc_leave_one_out_fp32' in msg and what in msg
    bad = [(dict(params=None), b'null'), (dict(row_ptr=None), b'null'), (dict(idx=None), b'null'),
           (dict(row_cube=None), b'null'), (dict(row_pos=None), b'null'), (dict(out_ptr=None), b'null'),
           (dict(out=None), b'null'), (dict(ws=None), b'null'), (dict(tgt_ptr=one), b'null'),
           (dict(d=0), b'd must be'), (dict(d=96), b'd must be'), (dict(d=2048), b'd must be'),
           (dict(max_n=101), b'max_n'), (dict(max_n=-1), b'max_n'), (dict(V=0), b'V'), (dict(rows=-1), b'rows'),
           (dict(n_cubes=-1), b'n_cubes'), (dict(ws=C.c_void_p(4096 + 64)), b'aligned'),
           (dict(ws_bytes=need - 1), b'workspace'), (dict(ws_bytes=0), b'workspace'),
           (dict(n_cubes=0, ws_bytes=need), b'without cubes')]
    for kw, what in bad:
        assert call(**kw) == -1 and failed(what), kw
    # rows == 0: CC_OK, nothing launched
    assert call(rows=0) == 0 and call(rows=0, n_cubes=0) == 0 and call(rows=0, tgt_ptr=one, tgt=one) == 0


# ---------------------------------------------------------------------------- planning
def plan_restated(ns, rows_per_launch):
    """plan_rows row by row: [(cube, q)] per launch."""
    step, launches, cur = max(1, rows_per_launch), [], []
    slots = max(4, step // 8)
    for c, n in enumerate(ns):
        for q in range(n + 1):
            inside = {cc for cc, _ in cur}
            grown = max([chunk_slots(ns[cc]) for cc in inside | {c}])
            if cur and (len(cur) == step or (c not in inside and (len(inside) + 1) * grown > slots)):
                launches.append(cur)
                cur = []
            cur.append((c, q))
    return launches + ([cur] if cur else [])


def test_plan_rows_against_the_restatement():
    rng = np.random.default_rng(0)
    cases = [[0], [1], [5, 0, 0, 3], [97, 2, 33], [300, 1, 1, 1, 64, 65], list(rng.integers(0, 80, 40))]
    for ns in cases:
        for rpl in (0, 1, 7, 32, 33, 100, 4096):
            got = [[(c, q) for c, q0, q1 in sl for q in range(q0, q1)] for sl in plan_rows(ns, rpl)]
            assert got == plan_restated(ns, rpl), (ns, rpl)
            assert [x for launch in got for x in launch] == [(c, q) for c, n in enumerate(ns) for q in range(n + 1)]
    sliced = plan_rows([97], 7)                                   # 98 rows in 14 launches of one slice
    assert [sl[0][1:] for sl in sliced] == [(q, q + 7) for q in range(0, 98, 7)] and all(len(sl) == 1 for sl in sliced)


def test_target_chunks():
    assert target_chunks(0, 10) == []
    assert target_chunks(5, 10, budget_bytes=4 * 10 * 5) == [(0, 5)]
    assert target_chunks(5, 10, budget_bytes=4 * 10 * 2) == [(0, 2), (2, 4), (4, 5)]
    assert target_chunks(3, 10, budget_bytes=1) == [(0, 1), (1, 2), (2, 3)]         # at least one target
    assert target_chunks(22000, 4096) == [(0, 8192), (8192, 16384), (16384, 22000)]


def fake(total, card):
    """Stands in for p(card | cube whose ids sum to total): distinct float32 values."""
    return np.float32(((int(total) * 7919 + int(card) * 104729) % 1000003) / 1000003.0)


def device_restated(a):
    """What the kernels would write for one launch's arrays, with `fake` as the model."""
    out = np.full(int(a['out_ptr'][-1]), np.nan, np.float32)
    for r in range(a['rows']):
        c, pos = int(a['row_cube'][r]), int(a['row_pos'][r])
        assert 0 <= c < a['n_cubes']
        ids = a['idx'][a['row_ptr'][c]:a['row_ptr'][c + 1]].astype(np.int64)
        assert -1 <= pos < len(ids) <= a['max_n'] and np.all(np.diff(ids) > 0)
        total = ids.sum() - (ids[pos] if pos >= 0 else 0)
        if a['tgt_ptr'] is None:
            cards = ids if pos < 0 else ids[pos:pos + 1]
        else:
            cards = a['tgt'][a['tgt_ptr'][c]:a['tgt_ptr'][c + 1]]
        lo, hi = a['out_ptr'][r], a['out_ptr'][r + 1]
        assert hi - lo == len(cards)
        out[lo:hi] = [fake(total, t) for t in cards]
    assert not np.isnan(out).any()
    return out


CUBES = [[5, 3, 9], [], [7], [40, 2, 40, 11, 2, 2, 30], list(range(60, 130)), [1, 0]]


@pytest.mark.parametrize('rpl', [1, 2, 7, 33, 10 ** 6])
def test_self_mode_lands_in_input_order(rpl):
    plan = Plan(CUBES, None, 200, rpl)
    for i in range(len(plan.items)):
        a = plan.arrays(i)
        assert a['rows'] <= rpl and a['row_cube'].dtype == a['row_pos'].dtype == a['out_ptr'].dtype == np.int32
        plan.take(i, a['out_ptr'], device_restated(a))
    got = plan.results()
    assert len(got) == len(CUBES)
    for cube, g in zip(CUBES, got):
        total = sum(set(cube))
        assert g['loo_vals'].dtype == g['cut_vals'].dtype == np.float32
        assert g['loo_vals'].tolist() == [fake(total - c, c) for c in cube]
        assert g['cut_vals'].tolist() == [fake(total, c) for c in cube]


@pytest.mark.parametrize('rpl,budget', [(1, None), (7, None), (10 ** 6, None), (7, 4 * 7 * 2), (10 ** 6, 1)])
def test_targets_mode_lands_in_input_order(rpl, budget):
    per_cube = [[9, 150, 9], [1], [], [2, 2, 199, 0, 40], [61], [3, 1, 4, 1, 5, 9, 2, 6]]
    for targets in (per_cube, [9, 150, 9, 5], np.array([0, 7])):
        plan = Plan(CUBES, targets, 200, rpl, budget_bytes=budget)
        if budget == 1:                                            # one target per launch
            assert all(t1 - t0 == 1 for _, t0, t1 in plan.items)
        for i in range(len(plan.items)):
            a = plan.arrays(i)
            if budget:
                assert int(a['out_ptr'][-1]) * 4 <= max(budget, 4 * a['rows'])
            plan.take(i, a['out_ptr'], device_restated(a))
        got = plan.results()
        for r, (cube, g) in enumerate(zip(CUBES, got)):
            tg = targets[r] if targets is per_cube else list(targets)
            total = sum(set(cube))
            assert g['base'].tolist() == [fake(total, t) for t in tg]
            assert g['without'].shape == (len(cube), len(tg)) and g['without'].dtype == np.float32
            assert g['without'].tolist() == [[fake(total - c, t) for t in tg] for c in cube]


# ---------------------------------------------------------------------------- checks before a launch
class NoLaunch:
    """What leave_one_out reads off a Recommender before it launches anything."""
    V, d, dev, stream, params = 50, 64, 'cuda', None, None


def test_bad_ids_raise_before_any_launch(monkeypatch):
    used = []
    monkeypatch.setattr(leaveoneout.L, 'lib', lambda: used.append('lib'))
    for cubes, targets in (([[1, 2]], [[3, 50]]), ([[1, 2]], [3, -1]), ([[1, 2], [3]], [[3], [4], [5]]),
                           ([[1, 50]], None), ([[-1]], [[1]])):
        with pytest.raises(ValueError):
            leaveoneout.leave_one_out(NoLaunch(), cubes, targets)
    with pytest.raises(ValueError, match='target card 50'):
        leaveoneout.leave_one_out(NoLaunch(), [[1]], [50])
    assert leaveoneout.leave_one_out(NoLaunch(), []) == [] and leaveoneout.leave_one_out(NoLaunch(), [], []) == []
    assert used == []


# ---------------------------------------------------------------------------- api
class StubModel:
    def __init__(self, out):
        self.out, self.calls = out, []

    def recommender(self):
        return self

    def leave_one_out(self, cubes, targets=None):
        self.calls.append(([list(map(int, c)) for c in cubes], None if targets is None else [list(map(int, t)) for t in targets]))
        return [self.out]


NAMES = {i: f'card {i}' for i in range(20)}


def test_leave_one_out_cuts_orders_by_without_then_id():
    f = np.float32
    cube = [7, 3, 9, 3, 1]
    model = StubModel({'loo_vals': np.array([.5, .25, .25, .25, .75], f), 'cut_vals': np.array([.9, .8, .7, .8, .6], f)})
    got = api.leave_one_out_cuts(model, iter(cube), NAMES)
    assert list(got.items()) == [('card 3', (float(f(.8)), .25)), ('card 9', (float(f(.7)), .25)),
                                 ('card 7', (float(f(.9)), .5)), ('card 1', (float(f(.6)), .75))]
    assert model.calls == [([cube], None)]
    assert api.leave_one_out_cuts(StubModel({'loo_vals': np.zeros(0, f), 'cut_vals': np.zeros(0, f)}), [], NAMES) == {}


def test_explain_orders_by_gain_then_id():
    f = np.float32
    cube, targets = [7, 3, 9, 3, 1], [12, 4]
    base = np.array([.75, .5], f)
    without = np.array([[.5, .5], [.25, .125], [.25, .75], [.25, .125], [.7, .5]], f)       # rows in input order
    model = StubModel({'base': base, 'without': without})
    got = api.explain(model, cube, iter(targets), NAMES, top=3)
    assert model.calls == [([cube], [targets])]
    assert list(got) == ['card 12', 'card 4']
    assert got['card 12'] == {'base': .75, 'cards': [('card 3', .5), ('card 9', .5), ('card 7', .25)]}
    assert got['card 4'] == {'base': .5, 'cards': [('card 3', .375), ('card 1', 0.0), ('card 7', 0.0)]}
    gain = got['card 12']['cards'][2][1]
    assert gain == float(f(.75) - f(.5))                           # a float32 subtraction
    every = api.explain(model, cube, targets, NAMES, top=10)['card 4']['cards']
    assert [n for n, _ in every] == ['card 3', 'card 1', 'card 7', 'card 9'] and every[-1][1] == -.25
    assert api.explain(model, cube, targets, NAMES, top=0)['card 4']['cards'] == []


def test_cli_arguments():
    sys.path.insert(0, ROOT)
    from scripts import explain, loo_cuts
    a = explain.parse_args(['my cube', 'Lightning Bolt', 'Counterspell', '--top', '3'])
    assert (a.cube_name, a.targets, a.top, a.model_dir) == ('my cube', ['Lightning Bolt', 'Counterspell'], 3, 'ml_files/neg')
    assert explain.parse_args(['c', 't']).top == 10
    a = loo_cuts.parse_args(['my cube', '25'])
    assert (a.cube_name, a.amount, a.root, a.id_map) == ('my cube', 25, 'https://cubecobra.com',
                                                         'ml_files/recommender_id_map.json')
    assert loo_cuts.parse_args(['c']).amount == 100
    for mod, bad in ((explain, ['c']), (explain, []), (loo_cuts, []), (loo_cuts, ['c', 'many'])):
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
