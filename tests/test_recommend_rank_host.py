"""CPU tests of the full-ranking batched recommend's host side: the two cc_recommend_batch_rank_*
bindings, the workspace size (a host function) and the rows-per-launch cap."""
import ctypes as C

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.recommender import RANK_STAGING_BYTES, rank_rows_per_launch

SHAPES = [(63, 64, 1, 0), (1001, 128, 11, 500), (4100, 128, 130, 4100), (20884, 512, 512, 720),
          (22000, 1024, 64, 22000)]


def test_bindings():
    p, i32 = C.c_void_p, C.c_int32
    assert L.SIGNATURES['cc_recommend_batch_rank_ws_size'] == (C.c_size_t, [i32, i32, i32, i32])
    assert L.SIGNATURES['cc_recommend_batch_rank_fp32'] == (
        C.c_int, [p, i32, i32, i32, p, p, i32, i32, p, p, p, p, p, p, p])
    lib = L.lib()
    assert lib.cc_recommend_batch_rank_ws_size.restype is C.c_size_t
    assert lib.cc_recommend_batch_rank_fp32.restype is C.c_int


def test_workspace_size():
    lib = L.lib()
    for V, d, R, max_n in SHAPES:
        rank = int(lib.cc_recommend_batch_rank_ws_size(V, d, R, max_n))
        batch = int(lib.cc_recommend_batch_ws_size(V, d, R, max_n))
        assert rank >= batch
        assert rank >= batch + 2 * R * V * 4          # two (key, id) ping-pong buffers on top
        assert rank % 256 == 0
        assert int(lib.cc_recommend_batch_rank_ws_size(V, d, R + 1, max_n)) >= rank
        assert int(lib.cc_recommend_batch_rank_ws_size(V + 1, d, R, max_n)) >= rank
    sizes = [int(lib.cc_recommend_batch_rank_ws_size(4100, 128, R, 100)) for R in range(1, 140)]
    assert sizes == sorted(sizes)
    sizes = [int(lib.cc_recommend_batch_rank_ws_size(V, 128, 11, 60)) for V in range(60, 4200, 7)]
    assert sizes == sorted(sizes)


def test_rows_per_launch_cap():
    for V in (1, 63, 1001, 20884, 22000):
        for A in (1, 2049, V):
            for rows in (1, 32, 512, 4096):
                for budget in (0, 1, 1 << 20, RANK_STAGING_BYTES, 1 << 40):
                    got = rank_rows_per_launch(V, A, rows, budget)
                    assert 1 <= got <= rows
                    # staging per row: n_add + A additions + A values + at most V cut values
                    assert got == 1 or got * 4 * (1 + 2 * A + V) <= budget
    V = 22000
    got = rank_rows_per_launch(V, V, 512)              # the default budget
    assert 1 <= got <= 512 and got * 4 * (1 + 3 * V) <= RANK_STAGING_BYTES
    assert rank_rows_per_launch(V, V, 512, 1 << 40) == 512
    assert rank_rows_per_launch(V, V, 0) == 1 and rank_rows_per_launch(V, V, -3, 0) == 1
