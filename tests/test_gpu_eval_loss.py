"""cc_recommend_batch_loss_fp32 / Recommender.reconstruction_loss / evaluate_loss /
CC_Recommender.evaluate / fit(validation_data): the validation loss reduced on the device.

The row losses are float64 bit patterns and the predictions integers: np.array_equal against the
host restatement of the pinned arithmetic (tests/eval_loss_ref.py; tests/test_eval_loss_host.py
holds that one to the fp64 oracle), no tolerances."""
import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.evaluate import evaluate_loss
from cubecobrarecommender_amd.generator import DataGenerator
from cubecobrarecommender_amd.layout import Layout
from cubecobrarecommender_amd.model import CC_Recommender
from cubecobrarecommender_amd.recommender import Recommender, pack_cubes
from tests import eval_loss_ref as E
from tests import tile_cases
from tests.gpu_helpers import problem

pytestmark = pytest.mark.gpu

SHAPES, KINDS = E.SHAPES, E.KINDS


_recs = {}


def case(V, d, kind):
    """reference_case plus the resident model: (P, rec, cubes, targets, ref)."""
    P, cubes, targets, ref = E.reference_case(V, d, kind)
    if (V, d, kind) not in _recs:
        _recs[(V, d, kind)] = Recommender(Layout(V, d).pack(P), V, d)
    return P, _recs[(V, d, kind)], cubes, targets, ref


def _direct(rec, cubes, targets, ws=None, R=None, null_loss=False, ws_shift=0):
    """cc_recommend_batch_loss_fp32 itself, outputs and (a fresh) workspace pre-filled with junk."""
    V, d, dev = rec.V, rec.d, rec.dev
    row_ptr, idx, max_n, _, _ = pack_cubes(cubes, V)
    tgt_ptr = np.zeros(len(cubes) + 1, np.int32)
    tgt_ptr[1:] = np.cumsum([len(t) for t in targets])
    tgt = (np.concatenate([np.asarray(t, np.int64) for t in targets]) if len(targets) else np.zeros(0)).astype(np.int32)
    n = len(cubes)
    R = n if R is None else R

    def dev_of(a):
        return torch.from_numpy(a if len(a) else np.zeros(1, np.int32)).to(dev)
    rp, ix, tp, tg = dev_of(row_ptr), dev_of(idx), dev_of(tgt_ptr), dev_of(tgt)
    need = int(L.lib().cc_recommend_batch_loss_ws_size(V, d, n, max_n)) // 4 + 64
    if ws is None:
        ws = torch.full((need,), -1, device=dev, dtype=torch.int32)
    assert ws.numel() >= need and ws.data_ptr() % 256 == 0
    loss = torch.full((max(n, 1),), 7.0, device=dev, dtype=torch.float64)
    pred = torch.full((max(n, 1),), 77, device=dev, dtype=torch.int32)
    rc = L.lib().cc_recommend_batch_loss_fp32(
        L.ptr(rec.params), V, d, R, L.ptr(rp), L.ptr(ix), max_n, L.ptr(tp), L.ptr(tg),
        L.C.c_void_p(ws.data_ptr() + ws_shift), None if null_loss else L.ptr(loss), L.ptr(pred), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, loss.cpu().numpy(), pred.cpu().numpy(), ws


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def check_wide(V, cubes, targets, ref):
    """What the wide model must provide, asserted on the reference alone."""
    loss, pred, zs, ys = ref
    z, y = np.stack(zs), np.stack(ys)
    assert np.any(z >= E.SIG_SAT)
    for yy in (1.0, 0.0):
        assert np.any((z > 10) & (y == yy)) and np.any((z < -10) & (y == yy)), yy
    p = [E.probs_sat(zr) for zr in zs]
    tied = [int(np.count_nonzero(pr == pr.max())) > 1 for pr in p]
    assert any(tied) and not all(tied)
    hit = pred == E.first_targets(targets, V)
    assert hit.any() and not hit.all()
    assert all(pred[r] == int(np.argmax(p[r])) for r in range(len(zs)))    # the tree is numpy's first maximum


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('V,d', SHAPES)
def test_direct_call(V, d, kind):
    P, rec, cubes, targets, ref = case(V, d, kind)
    if kind == 'wide':
        check_wide(V, cubes, targets, ref)
    hit = ref[1] == E.first_targets(targets, V)
    assert hit[6] and not hit[7]
    n = len(cubes)
    # R = 1 / 33 / 65 / 130: each rows-per-tile variant (2, 4, 8) and a second row tile
    for R in ((n, 1, 33, 65, 130) if V == 63 else (n,)):
        rows = [r % n for r in range(R)]
        rc, loss, pred, _ = _direct(rec, [cubes[r] for r in rows], [targets[r] for r in rows])
        assert rc == 0
        assert same_bits(loss, ref[0][rows]), (R, loss, ref[0][rows])
        assert np.array_equal(pred, ref[1][rows]), R


_tile_refs = {}


@pytest.mark.parametrize('V,d,R', tile_cases.TILE_CASES)
def test_direct_call_tile_shapes(V, d, R):
    """The loss tile's edges (tests/tile_cases.py); every row's targets are its cube."""
    rec, cubes = tile_cases.recommender(V, d), tile_cases.cubes(V, R)
    if (V, d) not in _tile_refs:
        _tile_refs[(V, d)] = E.reference(tile_cases.params(V, d), tile_cases.cubes(V, tile_cases.MAX_ROWS))
    ref = _tile_refs[(V, d)]
    rc, loss, pred, _ = _direct(rec, cubes, cubes)
    assert rc == 0
    assert same_bits(loss, ref[0][:R])
    assert np.array_equal(pred, ref[1][:R])


@pytest.mark.parametrize('kind', KINDS)
def test_rows_do_not_depend_on_their_company(kind):
    """A row alone, in the batch and with rows_per_launch=7 has the same bits; so has a smaller
    batch run afterwards in the workspace a larger one has used."""
    V, d = 1001, 128
    P, rec, cubes, targets, ref = case(V, d, kind)
    n = len(cubes)
    rows = [r % n for r in range(20)]
    cs, ts = [cubes[r] for r in rows], [targets[r] for r in rows]
    whole = rec.reconstruction_loss(cs, ts)
    assert whole[0].dtype == np.float64 and whole[1].dtype == np.int32
    assert same_bits(whole[0], ref[0][rows]) and np.array_equal(whole[1], ref[1][rows])
    split = rec.reconstruction_loss(cs, ts, rows_per_launch=7)
    assert same_bits(split[0], whole[0]) and np.array_equal(split[1], whole[1])
    for r in range(n):
        one = rec.reconstruction_loss([cubes[r]], [targets[r]])
        assert same_bits(one[0], ref[0][r:r + 1]) and one[1][0] == ref[1][r]
    rc, loss, pred, ws = _direct(rec, cs, ts)
    assert rc == 0 and same_bits(loss, whole[0])
    rc, loss, pred, _ = _direct(rec, cs[2:7], ts[2:7], ws=ws)      # the used workspace, fewer rows
    assert rc == 0 and same_bits(loss, whole[0][2:7]) and np.array_equal(pred, whole[1][2:7])


def test_targets_default_to_the_cubes_and_guards():
    V, d = 63, 64
    P, rec, cubes, targets, ref = case(V, d, 'default')
    a = rec.reconstruction_loss(cubes)
    b = rec.reconstruction_loss(cubes, cubes)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert same_bits(a[0][[1, 8]], ref[0][[1, 8]])                  # the rows whose targets are the cube
    empty = rec.reconstruction_loss([])
    assert empty[0].shape == (0,) and empty[1].shape == (0,)
    lib = L.lib()
    for kw, word in ((dict(ws_shift=4), b'aligned'), (dict(null_loss=True), b'null')):
        rc, loss, pred, _ = _direct(rec, cubes, targets, **kw)
        assert rc == -1 and word in lib.cc_last_error_string()     # CC_ERR_ARG
        assert np.all(loss == 7.0) and np.all(pred == 77)           # nothing launched
    rc, loss, pred, _ = _direct(rec, cubes, targets, R=0)
    assert rc == 0 and np.all(loss == 7.0) and np.all(pred == 77)
    with pytest.raises(ValueError, match='outside'):
        rec.reconstruction_loss(cubes, [[V]] * len(cubes))
    with pytest.raises(ValueError, match='outside'):
        rec.reconstruction_loss([[1, -2]])


def test_evaluate_surfaces_agree():
    V, d = 1001, 128
    P, rec, cubes, targets, ref = case(V, d, 'wide')
    got = evaluate_loss(rec, cubes, targets)
    hit = ref[1] == E.first_targets(targets, V)
    assert got == {'bce': float(np.sum(ref[0])) / len(cubes), 'output_1_accuracy': float(hit.sum()) / len(cubes),
                   'n_cubes': len(cubes)}
    model = CC_Recommender(V, d=d, params_flat=Layout(V, d).pack(P))
    assert model.evaluate(cubes, targets) == got
    assert model.evaluate(cubes, targets, batch_size=4) == got
    dense_x, dense_y = np.zeros((len(cubes), V)), np.zeros((len(cubes), V))
    for r in range(len(cubes)):
        dense_x[r, cubes[r]] = 1
        dense_y[r, targets[r]] = 1
    assert model.evaluate(dense_x, dense_y) == got                  # dense 0/1 matrices, as Keras takes them
    assert model.evaluate(cubes) == evaluate_loss(rec, cubes)


def test_fit_with_validation_data_trains_the_same_and_reports_evaluate():
    V, d, C = 600, 64, 128
    lists, Mt, ns = problem(13, C, V, (15, 40, 90))
    train, held = lists[:96], lists[96:]
    runs = []
    for val in (None, held):
        gen = DataGenerator(Mt.astype(np.float32), train, batch_size=32, noise=0.2, seed=4)
        model = CC_Recommender(V, d=d, seed=2)
        model.compile(loss_weights=[1.0, 0.1], metrics=['accuracy'])
        model.fit(gen, epochs=2, verbose=0, validation_data=val, validation_ks=(10,) if val is not None else ())
        runs.append((model._current_flat(), model._m, model._v, model._step, model))
    a, b = runs
    assert a[3] == b[3] == 2 * (96 // 32)
    for k in range(3):                                              # parameters, m, v: bit for bit
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert all(not k.startswith('val_') for h in a[4].history for k in h)
    model = b[4]
    assert len(model.history) == 2
    for h in model.history:
        assert {'val_bce', 'val_output_1_accuracy', 'val_recall@10', 'val_mrr'} <= set(h)
    e = model.evaluate(held)
    assert model.history[-1]['val_bce'] == e['bce']
    assert model.history[-1]['val_output_1_accuracy'] == e['output_1_accuracy']
    assert model.history[0]['val_bce'] != model.history[1]['val_bce']       # each epoch's own weights
    pair = CC_Recommender(V, d=d, seed=2)
    pair.compile(loss_weights=[1.0, 0.1])
    gen = DataGenerator(Mt.astype(np.float32), train, batch_size=32, noise=0.2, seed=4)
    lines = []
    pair.fit(gen, epochs=1, verbose=1, log=lines.append, validation_data=(held, [c[:3] for c in held]))
    assert pair.history[0]['val_bce'] == pair.evaluate(held, [c[:3] for c in held])['bce']
    assert len(lines) == 1 and f"val_bce: {pair.history[0]['val_bce']:.6f}" in lines[0]     # the epoch's log line
