"""The host pipeline behind every batched call: spans of rows, one launch queued
ahead of the one being unpacked, a kept device workspace, uploads, and the landing of results in
pinned memory.  Pure plumbing: it knows no kernel, and the callers keep their locks and streams."""
from types import SimpleNamespace

import numpy as np
import torch


def row_spans(R, rows_per_launch):
    """[(r0, r1)] tiling [0, R) in steps of rows_per_launch (below 1 counts as 1)."""
    step = max(1, int(rows_per_launch))
    return [(r0, min(R, r0 + step)) for r0 in range(0, R, step)]


def pipelined(spans, launch, collect):
    """launch(r0, r1, turn) -> (payload, done) queues span number `turn` and the copies of its
    results without waiting; collect(r0, r1, payload) unpacks them once done.synchronize() has
    returned.  A span is unpacked while the next one runs: launch 0, launch 1, collect 0, launch 2,
    collect 1, ..., collect last.  An exception propagates; what is queued is not waited for.
    Returns the last payload (None without spans): freeing a pinned tensor records an event on the
    stream that filled it, so a caller that waits for its stream afterwards holds the payload until
    it has waited; every other caller drops it."""
    def finish(r0, r1, payload, done):
        done.synchronize()
        collect(r0, r1, payload)

    pending = None
    for turn, (r0, r1) in enumerate(spans):
        queued = (r0, r1, *launch(r0, r1, turn))
        if pending is not None:
            finish(*pending)
        pending = queued
    if pending is not None:
        finish(*pending)
        return pending[2]


def mark(stream=None):
    """An event recorded on `stream` (None: the current one) behind what is queued there."""
    done = torch.cuda.Event()
    done.record(stream)
    return done


def upload(arr, dev):
    """The numpy array on `dev`, without waiting; an empty one as one zero of its dtype (every
    entry wants a non-NULL pointer)."""
    return torch.from_numpy(arr if len(arr) else np.zeros(1, arr.dtype)).to(dev, non_blocking=True)


def ws_elems(nbytes):
    """int32 elements of a workspace of nbytes: the one place of the 256 bytes of slack."""
    return int(nbytes) // 4 + 64


class Workspace:
    """A device int32 buffer, grown when needed and kept: `buf`, None until the first get."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, dev):
        """At least ws_elems(nbytes) elements: the kept buffer itself unless the request is
        larger."""
        need = ws_elems(nbytes)
        if self.buf is None or self.buf.numel() < need:
            self.buf = torch.empty(need, device=dev, dtype=torch.int32)
        return self.buf


class Staging:
    """Host landing buffers of device results (pinned, unless pin=False).  With kept buffers a
    caller alternates two sets, the turn's parity in the key: a set is free again once the launch
    before last has been collected, which `pipelined` guarantees before it queues the next.  What
    a call returns must be copied out of a kept buffer: a later launch overwrites it."""

    def __init__(self, pin=True):
        self.pin, self.bufs = pin, {}

    def fresh(self, t):
        """A new host tensor receiving `t`; no waiting."""
        return torch.empty(t.shape, dtype=t.dtype, pin_memory=self.pin).copy_(t, non_blocking=True)

    def kept(self, t, key):
        """A view of the kept buffer `key` (grown when needed) receiving `t`; no waiting."""
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < t.numel():
            buf = self.bufs[key] = torch.empty(t.numel(), dtype=t.dtype, pin_memory=self.pin)
        return buf[:t.numel()].view(t.shape).copy_(t, non_blocking=True)


def slice_targets(tgt_ptr, tgt, r0, r1):
    """Rows r0..r1 of a target CSR: (pointers rebased to start at 0, their targets)."""
    return tgt_ptr[r0:r1 + 1] - tgt_ptr[r0], tgt[tgt_ptr[r0]:tgt_ptr[r1]]


def target_ranks_rows(pack, inputs, V, tgt_ptr, tgt, cutoffs, rows_per_launch, dev, stream, staging,
                      val_dtype, call):
    """The body of both target_ranks methods; the caller holds its lock and has made `stream`
    current.  pack is recommender.pack_cubes, handed in because this module imports no caller.
    Per span the cubes are packed and uploaded with the span's targets, then call(s) makes the
    entry call.  The fields of s (nt targets and nnz cube cards in the span):
      r0, r1, Rc, max_n   ints: the span, its rows r1 - r0, its longest cube
      rp [Rc + 1], ix [nnz]   int32, the cubes as CSR;  tp [Rc + 1], tg [nt]   int32, the targets
      nk   int, the number of cutoffs;  cut [nk] int32 and hits [nk + 2] int64 (zeroed once per
           call, summed over the spans), both None when nk == 0
      rk [nt] int32 and tv [nt] val_dtype   outputs, returned;  cuts [nnz] val_dtype   scratch
    All tensors are on `dev`; an empty one has one element.  Returns (ranks, vals, hits) as
    target_ranks documents them."""
    nk = len(cutoffs)
    cut_d = torch.tensor(cutoffs, device=dev, dtype=torch.int32) if nk else None
    hits_d = torch.zeros(nk + 2, device=dev, dtype=torch.int64) if nk else None
    ranks, vals = [], []

    def launch(r0, r1, turn):
        row_ptr, idx, max_n, _, _ = pack(inputs[r0:r1], V)
        tp, tg = slice_targets(tgt_ptr, tgt, r0, r1)
        s = SimpleNamespace(r0=r0, r1=r1, Rc=r1 - r0, max_n=max_n, nk=nk, cut=cut_d, hits=hits_d,
                            rp=upload(row_ptr, dev), ix=upload(idx, dev), tp=upload(tp, dev), tg=upload(tg, dev))
        s.rk = torch.empty(max(len(tg), 1), device=dev, dtype=torch.int32)
        s.tv = torch.empty(max(len(tg), 1), device=dev, dtype=val_dtype)
        s.cuts = torch.empty(max(len(idx), 1), device=dev, dtype=val_dtype)   # the chain's; not returned
        call(s)
        return (staging.fresh(s.rk).numpy(), staging.fresh(s.tv).numpy(), tp), mark(stream)

    def collect(r0, r1, payload):
        rk, tv, tp = payload
        for lo, hi in zip(tp[:-1].tolist(), tp[1:].tolist()):
            ranks.append(rk[lo:hi].copy())
            vals.append(tv[lo:hi].copy())

    pipelined(row_spans(len(inputs), rows_per_launch), launch, collect)
    return ranks, vals, (hits_d.cpu().numpy().view(np.uint64) if nk else None)
