"""CPU tests of the validation loss's host side: the restatement of the device arithmetic
(tests/eval_loss_ref.py) against the fp64 oracle, evaluate_loss on a stub recommender, the
argument checks that come before any launch, the two bindings, and scripts/train.py's split."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.evaluate import evaluate_loss
from cubecobrarecommender_amd.model import CC_Recommender
from cubecobrarecommender_amd.recommender import Recommender
from oracle import model_ref
from tests import eval_loss_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# largest relative difference |restatement - fp64| / fp64 over the case's rows, measured on the
# CPU (x86-64, numpy float64); the bound of the test is 4x this
MEASURED = {(63, 64, 'default'): 2.97e-9, (63, 64, 'wide'): 1.65e-7,
            (1001, 128, 'default'): 8.53e-11, (1001, 128, 'wide'): 9.46e-8,
            (1001, 192, 'default'): 2.20e-10, (1001, 192, 'wide'): 9.58e-8}


@pytest.mark.parametrize('kind', E.KINDS)
@pytest.mark.parametrize('V,d', E.SHAPES)
def test_restatement_against_the_fp64_oracle(V, d, kind):
    """Row by row against model_ref.train_forward_backward(mode='fp64')'s bce: the only difference
    is the fp32 logits (the terms and their sum are fp64 on both sides).  Measured: 2.97e-9 /
    8.53e-11 / 2.20e-10 for the default models at (63, 64) / (1001, 128) / (1001, 192), and
    1.65e-7 / 9.46e-8 / 9.58e-8 for the wide ones (logits over +-20 and beyond, where a rounding
    of z is an absolute error of the term); each bound is 4x its measured value."""
    P, cubes, targets, ref = E.reference_case(V, d, kind)
    worst = 0.0
    for r, (c, t) in enumerate(zip(cubes, targets)):
        want = model_ref.train_forward_backward(P, [np.unique(c)], [np.unique(t)], V, d, mode='fp64')[0]['bce']
        worst = max(worst, abs(ref[0][r] - want) / want)
    print(f'restatement vs fp64 at {(V, d, kind)}: {worst:.3e}')
    assert worst <= 4 * MEASURED[(V, d, kind)]


def test_the_reduction_tree_is_a_sum_and_a_first_argmax():
    """The tile tree adds every term exactly once (against math.fsum, to rounding) and its
    tie rule is numpy's first maximum, ties included."""
    import math
    rng = np.random.default_rng(5)
    for V in (1, 3, 63, 64, 65, 1001):
        z = rng.normal(0, 8, V).astype(np.float32)
        y = (rng.random(V) < 0.3).astype(np.float64)
        t = E.terms64(z, y)
        assert E.row_loss(z, y) == pytest.approx(math.fsum(t) / V, rel=1e-14)
        z[rng.integers(0, V, 3)] = 40.0                             # several cards at exactly 1.0
        assert E.row_pred(z) == int(np.argmax(E.probs_sat(z))) == int(np.flatnonzero(z >= E.SIG_SAT)[0])
    assert E.probs_sat(np.float32([15.7243833541870117]))[0] == 1.0
    assert E.probs_sat(np.float32([15.72]))[0] < 1.0


class StubRecommender:
    """reconstruction_loss with fixed results: evaluate_loss's own arithmetic, nothing else."""

    def __init__(self, row_loss, row_pred):
        self.row_loss, self.row_pred, self.calls = row_loss, row_pred, []

    def reconstruction_loss(self, cubes, targets=None, rows_per_launch=512):
        self.calls.append((cubes, targets, rows_per_launch))
        return np.asarray(self.row_loss, np.float64), np.asarray(self.row_pred, np.int32)


def test_evaluate_loss_means_and_hit_rule():
    cubes = [[5, 2, 9], [4], [], [7, 7, 3], [0, 1]]
    targets = [[9, 2], [], [6], [8, 3, 3], [1]]
    stub = StubRecommender([0.5, 0.25, 1.0, 2.0, 0.125], [2, 0, 6, 8, 0])
    out = evaluate_loss(stub, cubes, targets, rows_per_launch=3)
    # first (lowest) targets 2, (none -> 0), 6, 3, 1: rows 0, 1, 2 hit
    assert out == {'bce': (0.5 + 0.25 + 1.0 + 2.0 + 0.125) / 5, 'output_1_accuracy': 3 / 5, 'n_cubes': 5}
    assert stub.calls[0][2] == 3 and stub.calls[0][1] is targets
    out = evaluate_loss(stub, cubes)                                # the cubes are the targets
    # first targets 2, 4, (none -> 0), 3, 0: rows 0 and 4 hit
    assert out['output_1_accuracy'] == 2 / 5 and stub.calls[1][1] is None
    assert isinstance(out['bce'], float) and isinstance(out['output_1_accuracy'], float)
    assert evaluate_loss(StubRecommender([], []), []) == {'bce': 0.0, 'output_1_accuracy': 0.0, 'n_cubes': 0}


def test_ids_outside_the_range_raise_before_any_launch():
    rec = Recommender.__new__(Recommender)                          # no device, no weights: nothing can launch
    rec.V, rec.d, rec.dev = 50, 64, None
    with pytest.raises(ValueError, match=r'cube 1.*outside'):
        rec.reconstruction_loss([[1, 2], [3, 50]])
    with pytest.raises(ValueError, match='outside'):
        rec.reconstruction_loss([[1, 2], [3]], [[4], [-1]])
    with pytest.raises(ValueError, match='target lists'):
        rec.reconstruction_loss([[1, 2], [3]], [[4]])
    loss, pred = rec.reconstruction_loss([])
    assert loss.shape == (0,) and loss.dtype == np.float64 and pred.shape == (0,) and pred.dtype == np.int32


def test_fit_refuses_validation_data_under_data_parallel():
    model = CC_Recommender(50, d=64)
    with pytest.raises(ValueError, match='world'):
        model.fit(None, epochs=1, world=2, validation_data=[[1, 2, 3]])      # before the generator is touched


def header_arg_count(name):
    hdr = open(os.path.join(ROOT, 'include', 'ccrec.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    args = re.search(r'\b' + name + r'\s*\(([^)]*)\)', hdr).group(1)
    return len([a for a in args.split(',') if a.strip() and a.strip() != 'void'])


def test_lib_declares_the_two_symbols_and_checks_arguments_without_a_gpu():
    i32, P = C.c_int32, C.c_void_p
    size, entry = 'cc_recommend_batch_loss_ws_size', 'cc_recommend_batch_loss_fp32'
    assert L.SIGNATURES[size] == (C.c_size_t, [i32, i32, i32, i32])
    assert L.SIGNATURES[entry] == (C.c_int, [P, i32, i32, i32, P, P, i32, P, P, P, P, P, P])
    assert len(L.SIGNATURES[size][1]) == header_arg_count(size) == 4
    assert len(L.SIGNATURES[entry][1]) == header_arg_count(entry) == 13
    lib = L.lib()
    assert lib.cc_abi_version() == 2
    # the forward's buffers, the masks and three words per (tile, row): nothing of size R x V x 4
    # (16 bytes per 64 cards where the recommend chain keeps 4 bytes per card)
    for V, d, R, max_n in ((1001, 128, 11, 500), (20884, 512, 512, 540)):
        assert int(lib.cc_recommend_batch_loss_ws_size(V, d, R, max_n)) < int(lib.cc_recommend_batch_ws_size(V, d, R, max_n))
        assert int(lib.cc_recommend_batch_loss_ws_size(V, d, R, max_n)) % 256 == 0
    one = C.c_void_p(4096)                           # never dereferenced: every call fails or has R == 0
    f = lib.cc_recommend_batch_loss_fp32

    def call(R=2, loss=one, pred=one, ws=one, d=64, max_n=3):
        return f(one, 63, d, R, one, one, max_n, one, one, ws, loss, pred, None)
    assert call(loss=None) == -1 and b'null' in lib.cc_last_error_string()
    assert call(pred=None) == -1
    assert call(R=-1) == -1
    assert call(d=96) == -1
    assert call(ws=C.c_void_p(4096 + 4)) == -1 and b'aligned' in lib.cc_last_error_string()
    assert call(max_n=64) == -1 and b'max_n' in lib.cc_last_error_string()
    assert call(R=0) == 0                            # CC_OK, nothing launched


def test_train_script_validation_split():
    from scripts import train as cli
    C_ = 103
    keep, held = cli.validation_split(C_, 0.2, seed=7)
    assert len(held) == 20 and len(keep) == 83                      # floor(0.2 * 103)
    assert len(np.intersect1d(keep, held)) == 0
    assert np.array_equal(np.sort(np.concatenate([keep, held])), np.arange(C_))
    assert np.array_equal(keep, np.sort(keep))                      # the training cubes keep their order
    assert np.array_equal(held, np.random.default_rng(7).permutation(C_)[-20:])
    keep2, held2 = cli.validation_split(C_, 0.2, seed=7)
    assert np.array_equal(keep, keep2) and np.array_equal(held, held2)
    assert not np.array_equal(held, cli.validation_split(C_, 0.2, seed=8)[1])
    keep0, held0 = cli.validation_split(C_, 0.0, seed=7)
    assert np.array_equal(keep0, np.arange(C_)) and len(held0) == 0
    assert len(cli.validation_split(9, 0.1, seed=0)[1]) == 0         # floor(0.9)
    with pytest.raises(ValueError):
        cli.validation_split(C_, 1.0, seed=0)
