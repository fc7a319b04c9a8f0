"""CPU tests of batched card similarity's host side: the three bindings against the header, the
workspace size, every argument check of cc_similar_cards_batch with never-dereferenced pointers
(each call either fails or has Q == 0: nothing is launched), and similar_many's own checks with
the library call replaced by a recorder."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd import similarity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = b'cc_similar_cards_batch'


def header_arg_count(name):
    hdr = open(os.path.join(ROOT, 'include', 'ccrec.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    args = re.search(r'\b' + name + r'\s*\(([^)]*)\)', hdr).group(1)
    return len([a for a in args.split(',') if a.strip() and a.strip() != 'void'])


def test_signatures_match_the_header():
    i32, P = C.c_int32, C.c_void_p
    assert L.SIGNATURES['cc_similar_batch_max_n'] == (i32, [])
    assert L.SIGNATURES['cc_similar_batch_ws_size'] == (C.c_size_t, [i32, i32, i32, i32])
    assert L.SIGNATURES['cc_similar_cards_batch'] == (C.c_int, [P, i32, i32, i32, P, i32, P, P, P, P, P])
    assert L.SIGNATURES['cc_similar_cards_batch_timed'] == (C.c_int, [P, i32, i32, i32, P, i32, P, P, P, P, P, P])
    for name, count in (('cc_similar_batch_max_n', 0), ('cc_similar_batch_ws_size', 4),
                        ('cc_similar_cards_batch', 11), ('cc_similar_cards_batch_timed', 12)):
        assert len(L.SIGNATURES[name][1]) == header_arg_count(name) == count
    assert L.lib().cc_abi_version() == 2


def test_cap_and_workspace_size():
    lib = L.lib()
    cap = int(lib.cc_similar_batch_max_n())
    assert cap >= 1024
    for V, K, Q in ((1, 1, 1), (63, 5, 7), (300, 70, 130), (22000, 64, 512)):
        for N in sorted({1, min(V, 40), V}):
            size = int(lib.cc_similar_batch_ws_size(V, K, Q, N))
            assert size % 256 == 0 and size >= V * K * 4 + Q * V * 4, (V, K, Q, N)
    V, K, Q = 22000, 64, 512
    at_cap, above = (int(lib.cc_similar_batch_ws_size(V, K, Q, N)) for N in (cap, cap + 1))
    assert int(lib.cc_similar_batch_ws_size(V, K, Q, 1)) == at_cap       # the select needs no more
    assert above >= at_cap + 2 * Q * V * 8                                # the sort's two pair buffers
    assert int(lib.cc_similar_batch_ws_size(V, K, Q, V)) == above


def test_argument_checks_without_a_gpu():
    lib = L.lib()
    one = C.c_void_p(4096)                           # never dereferenced: every call fails or has Q == 0
    entry = lib.cc_similar_cards_batch

    def call(emb=one, V=63, K=64, Q=2, queries=one, N=10, ws=one, out_idx=one, out_dist=one, dist_all=None):
        return entry(emb, V, K, Q, queries, N, ws, out_idx, out_dist, dist_all, None)

    def failed(what):
        msg = lib.cc_last_error_string()
        return ENTRY in msg and what in msg
    for null in ('emb', 'queries', 'ws', 'out_idx', 'out_dist'):
        assert call(**{null: None}) == -1 and failed(b'null'), null
        assert call(**{null: None}, Q=0) == -1 and failed(b'null'), null
    for V, K in ((0, 64), (-1, 64), (63, 0), (63, -5)):
        assert call(V=V, K=K, N=1) == -1 and failed(b'V/K'), (V, K)
    assert call(Q=-1) == -1 and failed(b'Q')
    assert call(Q=(1 << 22) + 1) == -1 and failed(b'Q')
    for N in (0, -3, 64):
        assert call(N=N) == -1 and failed(b'N must be'), N
    assert call(ws=C.c_void_p(4096 + 8)) == -1 and failed(b'aligned')
    assert call(ws=C.c_void_p(4096 + 128)) == -1 and failed(b'aligned')
    # the first failing check wins whatever else is wrong, and a failing call with Q == 0 still fails
    assert call(N=0, Q=0) == -1 and failed(b'N must be')
    assert call(ws=C.c_void_p(4096 + 8), Q=0) == -1 and failed(b'aligned')
    # Q == 0: CC_OK, nothing launched (any N in range, with and without dist_all)
    assert call(Q=0) == 0 and call(Q=0, N=63) == 0 and call(Q=0, N=1, dist_all=one) == 0
    assert call(Q=0, V=1, K=1, N=1) == 0
    # the measuring entry runs the same checks under its own name
    timed = lib.cc_similar_cards_batch_timed
    ms = (C.c_float * 3)(1, 1, 1)
    assert timed(one, 63, 64, 2, one, 10, one, one, one, None, None, None) == -1
    assert b'cc_similar_cards_batch_timed' in lib.cc_last_error_string()
    assert timed(None, 63, 64, 2, one, 10, one, one, one, None, ms, None) == -1 and failed(b'null')
    assert b'cc_similar_cards_batch_timed' in lib.cc_last_error_string()
    assert timed(one, 63, 64, 2, one, 64, one, one, one, None, ms, None) == -1 and failed(b'N must be')


class Recorder:
    """Stands in for the _lib module inside similarity: every use of the library is recorded."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def record(*args):
            self.calls.append((name, args))
            raise AssertionError(f'the library was used: {name}')
        return record


def test_similar_many_checks_ids_before_any_library_call(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(similarity, 'L', rec)
    emb = torch.zeros(50, 64)
    for bad in ([3, 50], [-1], [0, 1, 2, 10**6], np.array([49, 50])):
        with pytest.raises(ValueError, match='outside'):
            similarity.similar_many(emb, bad, 10)
    with pytest.raises(ValueError, match=r'query 1.*50'):
        similarity.similar_many(emb, [3, 50, -1], 10)
    with pytest.raises(ValueError, match='outside'):       # the id check comes first, whatever N is
        similarity.similar_many(emb, [50], 0)
    assert rec.calls == []


def test_similar_many_empty_results_need_no_library(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(similarity, 'L', rec)
    emb = torch.zeros(50, 64)
    for N in (0, -4):
        idx, dist = similarity.similar_many(emb, [1, 2, 2], N)
        assert idx.shape == (3, 0) and idx.dtype == np.int64
        assert dist.shape == (3, 0) and dist.dtype == np.float32
    idx, dist = similarity.similar_many(emb, [], 10)
    assert idx.shape == (0, 10) and idx.dtype == np.int64 and dist.shape == (0, 10) and dist.dtype == np.float32
    idx, dist = similarity.similar_many(emb, [], 80)       # n = min(N, V)
    assert idx.shape == (0, 50) and dist.shape == (0, 50)
    idx, dist = similarity.similarity_table(emb, 0)
    assert idx.shape == (50, 0) and idx.dtype == np.int32 and dist.shape == (50, 0) and dist.dtype == np.float32
    assert rec.calls == []
