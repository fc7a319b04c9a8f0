"""The host launch pipeline (cubecobrarecommender_amd/launches.py) without a GPU or the library:
the order of pipelined's calls, the spans, the target slices, and the growth rules of Workspace and
Staging on the CPU device."""
import numpy as np
import pytest
import torch

from cubecobrarecommender_amd.launches import Staging, Workspace, pipelined, row_spans, slice_targets


class Done:
    """A fake event: records its synchronize."""

    def __init__(self, log, k):
        self.log, self.k = log, k

    def synchronize(self):
        self.log.append(('sync', self.k))


def run(spans, fail_at=None):
    """pipelined over `spans` with recording fakes -> (log, turns seen by launch)."""
    log, turns, number = [], [], {s: k for k, s in enumerate(spans)}

    def launch(r0, r1, turn):
        k = number[(r0, r1)]
        if k == fail_at:
            raise RuntimeError(f'launch {k}')
        log.append(('launch', k))
        turns.append(turn)
        return ('payload', k), Done(log, k)

    def collect(r0, r1, payload):
        assert payload == ('payload', number[(r0, r1)])
        log.append(('collect', number[(r0, r1)]))

    try:
        last = pipelined(spans, launch, collect)
        assert last == (('payload', len(spans) - 1) if spans else None)   # the caller's to hold
    except RuntimeError as e:
        log.append(('raised', str(e)))
    return log, turns


def expected_order(n):
    """launch 0, launch 1, sync 0, collect 0, launch 2, sync 1, collect 1, ..., sync and collect last."""
    want = []
    for k in range(n):
        want.append(('launch', k))
        if k:
            want += [('sync', k - 1), ('collect', k - 1)]
    if n:
        want += [('sync', n - 1), ('collect', n - 1)]
    return want


@pytest.mark.parametrize('n', [0, 1, 2, 5])
def test_pipelined_call_order(n):
    spans = row_spans(3 * n, 3)
    assert len(spans) == n
    log, turns = run(spans)
    assert log == expected_order(n)
    assert turns == list(range(n))
    for k in range(n):
        at = log.index(('sync', k))
        assert log[at + 1] == ('collect', k)                      # waited for, then unpacked
        if k + 1 < n:
            assert log.index(('launch', k + 1)) < at              # behind the next launch


def test_pipelined_passes_an_exception_on():
    log, turns = run(row_spans(4, 1), fail_at=2)
    assert log == [('launch', 0), ('launch', 1), ('sync', 0), ('collect', 0), ('raised', 'launch 2')]
    assert turns == [0, 1]

    def collect(r0, r1, payload):
        raise KeyError(r0)
    calls = []
    with pytest.raises(KeyError):
        pipelined([(0, 1), (1, 2), (2, 3)], lambda r0, r1, turn: (calls.append(r0), Done([], r0)), collect)
    assert calls == [0, 1]                                        # nothing after the failed collect


def test_row_spans():
    assert row_spans(0, 512) == [] and row_spans(0, 0) == []
    assert row_spans(1, 512) == [(0, 1)] and row_spans(1, 1) == [(0, 1)]
    for step, count in ((512, 1), (64, 3), (7, 19), (1, 130)):
        spans = row_spans(130, step)
        assert len(spans) == count and spans[0][0] == 0 and spans[-1][1] == 130
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))            # [0, R) tiled exactly
        assert all(0 < r1 - r0 <= step for r0, r1 in spans)
        assert all(r1 - r0 == step for r0, r1 in spans[:-1])
    assert row_spans(130, 7)[-1] == (126, 130)
    for step in (0, -3):
        assert row_spans(5, step) == row_spans(5, 1) == [(r, r + 1) for r in range(5)]


def test_slice_targets():
    lens = [0, 0, 3, 1, 0, 0, 4, 2, 0]                            # empty rows at both ends and inside
    tgt_ptr = np.zeros(len(lens) + 1, np.int32)
    tgt_ptr[1:] = np.cumsum(lens)
    tgt = np.arange(100, 100 + tgt_ptr[-1], dtype=np.int32)
    for step in (1, 2, 4, 9, 512):
        parts = []
        for r0, r1 in row_spans(len(lens), step):
            tp, tg = slice_targets(tgt_ptr, tgt, r0, r1)
            assert tp.dtype == np.int32 and tg.dtype == np.int32
            assert tp[0] == 0 and len(tp) == r1 - r0 + 1 and tp[-1] == len(tg)
            assert np.diff(tp).tolist() == lens[r0:r1]
            parts.append(tg)
        assert np.array_equal(np.concatenate(parts), tgt)
    tp, tg = slice_targets(tgt_ptr, tgt, 0, 2)
    assert tp.tolist() == [0, 0, 0] and len(tg) == 0


def test_workspace_grows_only_when_needed():
    ws = Workspace()
    assert ws.buf is None
    a = ws.get(4000, 'cpu')
    assert a.dtype == torch.int32 and a.numel() == 4000 // 4 + 64 and ws.buf is a
    assert ws.get(4000, 'cpu') is a and ws.get(0, 'cpu') is a and ws.get(4003, 'cpu') is a
    assert ws.get(4 * (a.numel() - 64), 'cpu') is a                # the largest request it still serves
    b = ws.get(4 * (a.numel() - 64) + 4, 'cpu')
    assert b is not a and b.numel() == a.numel() + 1 and ws.buf is b
    assert ws.get(16, 'cpu') is b                                  # kept: never shrinks


def test_staging_fresh_and_kept():
    st = Staging(pin=False)
    t = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    f1, f2 = st.fresh(t), st.fresh(t)
    assert f1.data_ptr() != f2.data_ptr() and torch.equal(f1, t) and f1.shape == t.shape and not st.bufs
    k0 = st.kept(t, (0, 'vals'))
    assert torch.equal(k0, t) and k0.shape == t.shape and k0.dtype == t.dtype
    base = st.bufs[(0, 'vals')]
    assert base.numel() == 12 and k0.data_ptr() == base.data_ptr()
    small = torch.full((2, 3), 7.0, dtype=torch.float64)
    k1 = st.kept(small, (0, 'vals'))                               # a smaller request: the same storage
    assert st.bufs[(0, 'vals')] is base and k1.data_ptr() == base.data_ptr() and torch.equal(k1, small)
    assert k0.reshape(-1)[:6].tolist() == [7.0] * 6                # ... which the earlier view shares
    other = st.kept(t, (1, 'vals'))                                # the other set: a buffer of its own
    assert set(st.bufs) == {(0, 'vals'), (1, 'vals')} and other.data_ptr() != base.data_ptr()
    assert st.bufs[(0, 'vals')] is base
    big = st.kept(torch.zeros(13, dtype=torch.float64), (0, 'vals'))          # grown only past its size
    assert st.bufs[(0, 'vals')] is not base and big.numel() == 13 and st.bufs[(1, 'vals')].numel() == 12
