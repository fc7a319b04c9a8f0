"""Archetype card profiles: which cards make a group of cubes, and which does it
avoid?  A group-by of cubes by an integer label into card counts per group (cc_group_cards_count:
LDS-privatised histograms per group, streamed in spans) and per group the m cards with the largest
integer rank key (cc_group_cards_top).  Nothing on the device is floating point: every returned
integer is fixed by the cubes and the labels, and the rates are derived from them here in float64."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .launches import Workspace, mark, pipelined, row_spans, upload
from .recommender import pack_cubes

KINDS = {'rate': 0, 'lift': 1, 'avoid': 2}      # CC_GROUP_RATE, CC_GROUP_LIFT, CC_GROUP_AVOID
MAX_CUBES, MAX_V, MAX_M = 1 << 22, 1 << 18, 1024
SPAN_ROWS = 1 << 22                             # rows of one cc_group_cards_count


def check_args(R, labels, V, m, kind, min_count, G):
    """(labels int32 [R], V, m, kind, min_count, G), or ValueError: before any device call."""
    if kind not in KINDS:
        raise ValueError(f'kind {kind!r} is none of {sorted(KINDS)}')
    V, m, min_count = int(V), int(m), int(min_count)
    if not 1 <= m <= MAX_M:
        raise ValueError(f'm = {m} outside [1, {MAX_M}]')
    if not 1 <= V <= MAX_V:
        raise ValueError(f'V = {V} outside [1, {MAX_V}]')
    if min_count < 0:
        raise ValueError(f'min_count = {min_count} is negative')
    lab = np.asarray(labels, np.int64).reshape(-1)
    if len(lab) != R:
        raise ValueError(f'{len(lab)} labels for {R} cubes')
    G = (max(int(lab.max()) + 1, 1) if len(lab) else 1) if G is None else int(G)
    cap = int(L.lib().cc_group_cards_max_groups())
    if not 1 <= G <= cap:
        raise ValueError(f'G = {G} outside [1, cc_group_cards_max_groups() = {cap}]')
    bad = np.flatnonzero((lab < -1) | (lab >= G))
    if len(bad):
        raise ValueError(f'cube {int(bad[0])}: label {int(lab[bad[0]])} outside [-1, {G})')
    N = int((lab >= 0).sum())
    if N > MAX_CUBES:
        raise ValueError(f'{N} labelled cubes are above the {MAX_CUBES} the rank keys admit')
    return lab.astype(np.int32), V, m, kind, min_count, G


class GroupCards:
    """Per group g of G its signature cards, m columns each:
      cards int32 [G, m], card_count uint32 [G, m]   the first found[g] entries are the group's list
          (candidates by key descending, equal keys lower card first) and each card's count in the
          group; then -1 / 0
      found int32 [G]; sizes int32 [G] (cubes per group); totals uint32 [V] (cubes per card over all
      groups); N (labelled cubes)
      rate, base, lift float64 [G, m]   count / size, total / N and their difference (0 past found)
      counts uint32 [G, V]   only when asked for, else None
      kind, min_count        what ranked the lists"""

    def __init__(self, cards, card_count, found, sizes, totals, kind, min_count, counts=None):
        self.cards, self.card_count, self.found = cards, card_count, found
        self.sizes, self.totals, self.counts = sizes, totals, counts
        self.kind, self.min_count = kind, min_count
        self.G, self.m, self.V = cards.shape[0], cards.shape[1], len(totals)
        self.N = int(sizes.astype(np.int64).sum())
        live = cards >= 0
        s = np.maximum(sizes.astype(np.float64), 1.0)[:, None]
        self.rate = np.where(live, card_count.astype(np.float64) / s, 0.0)
        self.base = np.where(live, totals[np.maximum(cards, 0)].astype(np.float64) / max(self.N, 1), 0.0)
        self.lift = self.rate - self.base

    def _group(self, g):
        g = int(g)
        if not 0 <= g < self.G:
            raise ValueError(f'group {g} outside [0, {self.G})')
        return g

    def list_of(self, g):
        """Group g's reported cards, best first."""
        g = self._group(g)
        return self.cards[g, :int(self.found[g])]

    def missing(self, g, cube, n):
        """The first n cards of group g's list that `cube` (card ids) does not hold: what the
        archetype plays and the cube does not."""
        row = self.list_of(g)
        held = np.asarray(cube, np.int64).reshape(-1)
        return row[~np.isin(row, held)][:max(0, int(n))]


def _finish(lib, count, size, total, V, G, m, kind, min_count, ws, want_counts, stage):
    """cc_group_cards_top over the device counts and the copies back -> GroupCards; the caller has
    queued every count launch on the current stream."""
    dev = count.device
    cards = torch.empty(G, m, device=dev, dtype=torch.int32)
    ccnt = torch.empty(G, m, device=dev, dtype=torch.int32)
    found = torch.empty(G, device=dev, dtype=torch.int32)
    L.call('cc_group_cards_top', L.ptr(count), L.ptr(size), L.ptr(total), V, G, KINDS[kind], min_count, m, L.ptr(ws),
           L.ptr(cards), L.ptr(ccnt), L.ptr(found), L.stream_ptr())
    host = [stage(t) for t in (cards, ccnt, found, size, total)] + ([stage(count)] if want_counts else [])
    torch.cuda.current_stream().synchronize()
    out = [h.numpy().copy() for h in host]
    del host
    return GroupCards(out[0], out[1].view(np.uint32), out[2], out[3], out[4].view(np.uint32), kind, min_count,
                      out[5].view(np.uint32).reshape(G, V) if want_counts else None)


def _tables(G, V, dev):
    return (torch.empty(G * V, device=dev, dtype=torch.int32), torch.empty(G, device=dev, dtype=torch.int32),
            torch.empty(V, device=dev, dtype=torch.int32))


def _stage(t):
    return torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True)


def group_cards(cubes, labels, V, m, kind='lift', min_count=1, G=None, counts=False, rows_per_launch=65536,
                device='cuda'):
    """Cubes (card-id lists) grouped by labels (one per cube, -1: ignored) -> GroupCards with m
    cards per group ranked by kind:
      'rate'   the cards most of the group's cubes hold (its staples),
      'lift'   the in-group rate minus the corpus rate (what makes the group itself),
      'avoid'  the reverse: what the rest of the corpus plays and this group does not.
    Only cards that min_count cubes of the group hold (avoid: of the corpus) are listed.  G: the
    number of groups (default max(labels) + 1).  The cubes are packed once and uploaded in spans of
    rows_per_launch; the result's every integer is the same whatever the span.  A label outside
    [-1, G), a label count other than len(cubes), m outside [1, 1024], an unknown kind, V above
    2^18, more than 2^22 labelled cubes and a card outside [0, V) raise ValueError before anything
    is launched."""
    cubes = cubes if hasattr(cubes, '__len__') else list(cubes)
    lab, V, m, kind, min_count, G = check_args(len(cubes), labels, V, m, kind, min_count, G)
    row_ptr, idx, _, _, _ = pack_cubes(cubes, V)
    R, dev, lib = len(lab), torch.device(device), L.lib()
    step = min(max(1, int(rows_per_launch)), SPAN_ROWS)
    with torch.cuda.device(dev):
        count, size, total = _tables(G, V, dev)
        ws = Workspace().get(lib.cc_group_cards_ws_size(min(step, max(R, 1)), V, G, m), dev)

        def launch(r0, r1, turn):
            lo, hi = int(row_ptr[r0]), int(row_ptr[r1])
            rp_d = upload((row_ptr[r0:r1 + 1] - row_ptr[r0]).astype(np.int32), dev)
            ix_d, lab_d = upload(idx[lo:hi], dev), upload(lab[r0:r1], dev)      # alive until the call is queued
            L.call('cc_group_cards_count', L.ptr(rp_d), L.ptr(ix_d), r1 - r0, V, L.ptr(lab_d), G, 1 if turn else 0, 0,
                   L.ptr(ws), L.ptr(count), L.ptr(size), L.ptr(total), L.stream_ptr())
            return None, mark()

        spans = row_spans(R, step)
        if not spans:               # no cubes: the zeroing alone
            L.call('cc_group_cards_count', L.ptr(ws), L.ptr(ws), 0, V, L.ptr(ws), G, 0, 0, L.ptr(ws), L.ptr(count),
                   L.ptr(size), L.ptr(total), L.stream_ptr())
        pipelined(spans, launch, lambda r0, r1, payload: None)
        return _finish(lib, count, size, total, V, G, m, kind, min_count, ws, counts, _stage)


def corpus_group_cards(corpus, labels, m, kind='lift', min_count=1, G=None, counts=False, rows_per_launch=1 << 20):
    """CubeCorpus.group_cards (audience.py documents it)."""
    lab, V, m, kind, min_count, G = check_args(len(corpus), labels, corpus.V, m, kind, min_count, G)
    dev, lib = torch.device(corpus.dev), L.lib()
    step = min(max(1, int(rows_per_launch)), SPAN_ROWS)
    with corpus.lock, torch.cuda.device(dev):
        if len(lab) != corpus.N:
            raise ValueError(f'{len(lab)} labels for {corpus.N} cubes')
        R = corpus.N
        count, size, total = _tables(G, V, dev)
        ws = corpus._ws.get(lib.cc_group_cards_ws_size(min(step, max(R, 1)), V, G, m), dev)
        lab_d = upload(lab, dev)
        if R == 0:
            L.call('cc_group_cards_count', L.ptr(ws), L.ptr(ws), 0, V, L.ptr(ws), G, 0, 0, L.ptr(ws), L.ptr(count),
                   L.ptr(size), L.ptr(total), L.stream_ptr())
        else:
            base = corpus._buf.data_ptr()
            ptr0 = base + int(lib.cc_audience_corpus_ptr_offset(corpus.capacity, corpus.d))
            ids = C.c_void_p(base + int(lib.cc_audience_corpus_ids_offset(corpus.capacity, corpus.d)))
            for turn, (r0, r1) in enumerate(row_spans(R, step)):      # resident: nothing to upload or unpack
                L.call('cc_group_cards_count', C.c_void_p(ptr0 + 4 * r0), ids, r1 - r0, V,
                       C.c_void_p(lab_d.data_ptr() + 4 * r0), G, 1 if turn else 0, 0, L.ptr(ws), L.ptr(count),
                       L.ptr(size), L.ptr(total), L.stream_ptr())
        return _finish(lib, count, size, total, V, G, m, kind, min_count, ws, counts, _stage)
