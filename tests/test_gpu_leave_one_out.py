"""Leave-one-out scores (cc_leave_one_out_fp32 / Recommender.leave_one_out) against the pinned-order
CPU oracle on the shorter list (tests/loo_ref.py): every value BIT-EXACT (np.array_equal, no
tolerances), and equal to the existing device path on the derived cubes."""
import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.layout import Layout
from cubecobrarecommender_amd.leaveoneout import Plan
from cubecobrarecommender_amd.recommender import Recommender
from oracle import infer_ref, model_ref
from tests import loo_ref, tile_cases

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 31, 32, 33, 64, 65, 97)
_models = {}
_ref = {}


def model_of(V, d):
    if (V, d) not in _models:
        P = model_ref.init_params(V, d, seed=V + d, bias_std=0.01)
        _models[(V, d)] = (P, Recommender(Layout(V, d).pack(P), V, d))
    return _models[(V, d)]


def sized_batch(V):
    """One cube of each size of SIZES (capped at V), one unsorted cube with duplicates, two identical
    cubes."""
    rng = np.random.default_rng(V)
    cubes = [rng.choice(V, min(n, V), replace=False) for n in SIZES]
    base = rng.choice(V, min(V, 40), replace=False)
    cubes.append(rng.permutation(np.concatenate([base, base[:9], base[3:5]])))
    twin = rng.choice(V, min(V, 21), replace=False)
    cubes += [twin, twin.copy()]
    return cubes


def small_batch(V):
    """n = 0, 1, 33, 65 (capped at V) and an unsorted cube with duplicates."""
    rng = np.random.default_rng(V + 1)
    cubes = [rng.choice(V, min(n, V), replace=False) for n in (0, 1, 33, 65)]
    base = rng.choice(V, 12, replace=False)
    return cubes + [rng.permutation(np.concatenate([base, base[:5]]))]


def ref_self(tag, P, cubes):
    """The oracle's (loo_vals, cut_vals) of every cube, computed once per tag and shared."""
    if tag not in _ref:
        _ref[tag] = [loo_ref.loo_self(P, c) for c in cubes]
    return _ref[tag]


def same(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize('V,d', [(63, 64), (1001, 128)])
def test_self_mode_bit_exact(V, d):
    P, rec = model_of(V, d)
    cubes = sized_batch(V)
    want = ref_self(('sized', V, d), P, cubes)
    outs = rec.leave_one_out(cubes)
    many = rec.recommend_many(cubes, 1)
    assert len(outs) == len(cubes)
    for r, cube in enumerate(cubes):
        assert sorted(outs[r]) == ['cut_vals', 'loo_vals']
        assert same(outs[r]['loo_vals'], want[r][0]), r
        assert same(outs[r]['cut_vals'], want[r][1]), r
        assert same(outs[r]['cut_vals'], many[r]['cut_vals']), r
    assert np.array_equal(outs[-1]['loo_vals'], outs[-2]['loo_vals'])     # the identical cubes


def test_wide_model():
    """d = 1024: 16 k-chunks in every dot."""
    V, d = 4100, 1024
    P, rec = model_of(V, d)
    rng = np.random.default_rng(3)
    cubes = [rng.choice(V, n, replace=False) for n in (33, 40)]
    want = ref_self(('wide', V, d), P, cubes)
    outs = rec.leave_one_out(cubes)
    many = rec.recommend_many(cubes, 1)
    for r in range(2):
        assert same(outs[r]['loo_vals'], want[r][0]) and same(outs[r]['cut_vals'], want[r][1])
        assert same(outs[r]['cut_vals'], many[r]['cut_vals'])


def test_targets_every_card():
    """T = V: a `without` row is the whole oracle row of the shorter cube."""
    V, d = 63, 64
    P, rec = model_of(V, d)
    cubes = small_batch(V)
    outs = rec.leave_one_out(cubes, targets=np.arange(V))
    many = rec.recommend_many(cubes, 1, want_probs=True)
    for r, cube in enumerate(cubes):
        u = np.unique(cube)
        rows = np.stack([infer_ref.recommend_probs(P, loo_ref.without(u, j)) for j in range(len(u))]) \
            if len(u) else np.zeros((0, V), np.float32)
        assert same(outs[r]['without'], rows[np.searchsorted(u, cube)]), r
        assert same(outs[r]['base'], many[r]['probs']), r


def test_tile_shapes():
    """d = 192 (three chunks of k), T = V = 299 targets (five target tiles, the last of 43 cards: no
    multiple of 4) and 61 derived rows, of which the second cube's, 21..54, straddle the first row
    tile; both modes."""
    V, d = 299, 192
    P, rec = tile_cases.params(V, d), tile_cases.recommender(V, d)
    rng = np.random.default_rng(V + d)
    cubes = [rng.choice(V, n, replace=False) for n in (20, 33, 5)]
    outs = rec.leave_one_out(cubes, targets=np.arange(V))
    for r, cube in enumerate(cubes):
        base, rows = loo_ref.loo_targets(P, cube, np.arange(V))
        assert same(outs[r]['base'], base) and same(outs[r]['without'], rows), r
    outs = rec.leave_one_out(cubes)
    for r, cube in enumerate(cubes):
        loo, cut = loo_ref.loo_self(P, cube)
        assert same(outs[r]['loo_vals'], loo) and same(outs[r]['cut_vals'], cut), r


def test_targets_short_lists():
    """Per-cube lists: a cube card (which is the left-out card of one row), a repeated id, an
    outside card; an empty list and a cube without cards among them."""
    V, d = 63, 64
    P, rec = model_of(V, d)
    cubes = small_batch(V)
    targets = []
    for r, cube in enumerate(cubes):
        outside = np.setdiff1d(np.arange(V), cube)
        inside = cube[:2] if len(cube) else outside[:1]
        targets.append(np.concatenate([outside[:2], inside, outside[:1], inside[:1]]) if r != 2 else [])
    outs = rec.leave_one_out(cubes, targets=targets)
    for r, cube in enumerate(cubes):
        base, rows = loo_ref.loo_targets(P, cube, targets[r])
        assert same(outs[r]['base'], base) and same(outs[r]['without'], rows), r
    assert outs[2]['without'].shape == (len(cubes[2]), 0)


def test_results_do_not_depend_on_the_launches(monkeypatch):
    """rows_per_launch 1 and 7 (7 slices cubes mid-chunk) against one launch; targets split by a
    small staging budget as well."""
    from cubecobrarecommender_amd import leaveoneout
    V, d = 1001, 128
    _, rec = model_of(V, d)
    cubes = small_batch(V)
    tgt = [5, 900, int(cubes[2][0]), 5]
    whole_s, whole_t = rec.leave_one_out(cubes, rows_per_launch=10 ** 6), \
        rec.leave_one_out(cubes, targets=tgt, rows_per_launch=10 ** 6)
    assert len(Plan(cubes, None, V, 10 ** 6).items) == 1
    for rpl in (1, 7):
        got_s = rec.leave_one_out(cubes, rows_per_launch=rpl)
        got_t = rec.leave_one_out(cubes, targets=tgt, rows_per_launch=rpl)
        for r in range(len(cubes)):
            assert same(got_s[r]['loo_vals'], whole_s[r]['loo_vals']), (rpl, r)
            assert same(got_s[r]['cut_vals'], whole_s[r]['cut_vals']), (rpl, r)
            assert same(got_t[r]['base'], whole_t[r]['base']), (rpl, r)
            assert same(got_t[r]['without'], whole_t[r]['without']), (rpl, r)
    monkeypatch.setattr(leaveoneout, 'LOO_STAGING_BYTES', 4 * 3 * 40)     # three targets at 40 rows
    got_t = rec.leave_one_out(cubes, targets=tgt, rows_per_launch=40)
    for r in range(len(cubes)):
        assert same(got_t[r]['base'], whole_t[r]['base']) and same(got_t[r]['without'], whole_t[r]['without']), r


def test_results_do_not_depend_on_the_order_of_cubes():
    V, d = 1001, 128
    _, rec = model_of(V, d)
    cubes = sized_batch(V)
    fwd, back = rec.leave_one_out(cubes), rec.leave_one_out(cubes[::-1])[::-1]
    alone = rec.leave_one_out([cubes[7]])[0]
    for r in range(len(cubes)):
        assert same(fwd[r]['loo_vals'], back[r]['loo_vals']) and same(fwd[r]['cut_vals'], back[r]['cut_vals']), r
    assert same(alone['loo_vals'], fwd[7]['loo_vals']) and same(alone['cut_vals'], fwd[7]['cut_vals'])


def test_agrees_with_recommend_many_on_the_derived_cubes():
    V, d = 1001, 128
    _, rec = model_of(V, d)
    cube = np.random.default_rng(65).choice(V, 65, replace=False)
    u = np.unique(cube)
    derived = [loo_ref.without(u, j) for j in range(len(u))]
    probs = rec.recommend_many(derived, 0, want_probs=True)
    diagonal = np.array([probs[j]['probs'][u[j]] for j in range(len(u))], np.float32)
    got = rec.leave_one_out([cube])[0]['loo_vals']
    assert same(got, diagonal[np.searchsorted(u, cube)])


def _direct(rec, cubes, targets=None, ws_short=0, tail=5):
    """cc_leave_one_out_fp32 itself over one launch, outputs and workspace pre-filled with junk;
    `tail` junk words behind the last row's."""
    V, d, dev = rec.V, rec.d, rec.dev
    plan = Plan(cubes, targets, V, 10 ** 6)
    assert len(plan.items) == 1
    a = plan.arrays(0)
    up = lambda x: torch.from_numpy(x if len(x) else np.zeros(1, np.int32)).to(dev)      # noqa: E731
    t = {k: up(a[k]) for k in ('row_ptr', 'idx', 'row_cube', 'row_pos', 'out_ptr')}
    tp, tg = (None, None) if targets is None else (up(a['tgt_ptr']), up(a['tgt']))
    need = int(L.lib().cc_leave_one_out_ws_size(V, d, a['n_cubes'], a['max_n'], a['rows']))
    ws = torch.full((need // 4 + 64,), -1, device=dev, dtype=torch.int32)
    total = int(a['out_ptr'][-1])
    out = torch.full((total + tail,), 7.0, device=dev)
    rc = L.lib().cc_leave_one_out_fp32(L.ptr(rec.params), V, d, a['n_cubes'], L.ptr(t['row_ptr']), L.ptr(t['idx']),
                                       a['max_n'], a['rows'], L.ptr(t['row_cube']), L.ptr(t['row_pos']), L.ptr(tp),
                                       L.ptr(tg), L.ptr(t['out_ptr']), L.ptr(out), L.ptr(ws), need - ws_short,
                                       L.stream_ptr())
    torch.cuda.synchronize()
    return rc, plan, a, out.cpu().numpy()


def test_direct_call_writes_every_wanted_word_and_no_other():
    V, d = 63, 64
    P, rec = model_of(V, d)
    cubes = small_batch(V)
    rc, plan, a, out = _direct(rec, cubes)
    total = int(a['out_ptr'][-1])
    assert rc == 0 and total == sum(2 * len(np.unique(c)) for c in cubes)
    assert np.all(out[total:] == 7.0)
    plan.take(0, a['out_ptr'], out[:total])
    for r, got in enumerate(plan.results()):
        loo, cut = loo_ref.loo_self(P, cubes[r])
        assert same(got['loo_vals'], loo) and same(got['cut_vals'], cut), r
    tgt = [3, 3, int(cubes[3][0]), 62]
    rc, plan, a, out = _direct(rec, cubes, targets=tgt)
    total = int(a['out_ptr'][-1])
    assert rc == 0 and total == 4 * sum(len(np.unique(c)) + 1 for c in cubes)
    assert np.all(out[total:] == 7.0)
    plan.take(0, a['out_ptr'], out[:total])
    for r, got in enumerate(plan.results()):
        base, rows = loo_ref.loo_targets(P, cubes[r], tgt)
        assert same(got['base'], base) and same(got['without'], rows), r


def test_direct_call_refuses_a_short_workspace():
    V, d = 63, 64
    _, rec = model_of(V, d)
    rc, _, a, out = _direct(rec, small_batch(V), ws_short=4)
    assert rc == -1 and b'workspace' in L.lib().cc_last_error_string()     # CC_ERR_ARG, no launch
    assert np.all(out == 7.0)
