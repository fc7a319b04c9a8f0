"""Greedy cube completion: fill cubes up to a target size on the device, the best
per_step cards joining the cube per forward pass (cc_complete_fp32, csrc/complete.hip).

A launch carries its rows through every pass without a host round trip: the host packs the cubes
once, works out how many passes the slowest row needs and how many picks the largest row can take,
and unpacks n_added / added / added_vals at the end.  Everything but `complete_many` itself is pure
host code."""
import numpy as np
import torch

from . import _lib as L
from .launches import mark, pipelined, row_spans, upload
from .recommender import check_card_ids, pack_cubes, resolve_pools


def per_cube_sizes(sizes, R):
    """The `sizes` argument -> int64 [R]: one int serves every cube, else one per cube.  Raises
    ValueError for another number of sizes."""
    if np.ndim(sizes) == 0:
        return np.full(R, int(sizes), np.int64)
    out = np.asarray(list(sizes), np.int64).reshape(-1)
    if len(out) != R:
        raise ValueError(f'{len(out)} sizes for {R} cubes')
    return out


def plan_passes(ns, sizes, per_step, V):
    """Rows of ns[r] distinct cards filled to sizes[r] -> (target_n int32 [R], passes, A, max_n) as
    cc_complete_fp32 takes them: the targets capped at V; the passes the slowest row needs,
    ceil(room / per_step) with room = max(0, target - n) (0: nothing to add anywhere); the output
    pitch A, the largest room (at least 1); max_n, the longest row at any time."""
    ns = np.asarray(ns, np.int64)
    target = np.clip(np.asarray(sizes, np.int64), 0, int(V))
    room = np.maximum(target - ns, 0)
    most = int(room.max()) if len(room) else 0
    max_n = int(np.maximum(ns, target).max()) if len(ns) else 0
    return target.astype(np.int32), -(-most // int(per_step)), max(most, 1), max_n


def complete_many(rec, cubes, sizes, per_step=1, pool=None, rows_per_launch=512):
    """The body of Recommender.complete_many (documented there)."""
    V, d, dev = rec.V, rec.d, rec.dev
    per_step = int(per_step)
    if per_step < 1:
        raise ValueError(f'per_step is {per_step}: at least 1')
    inputs = [np.asarray(c, np.int64).reshape(-1) for c in cubes]
    R = len(inputs)
    sizes = per_cube_sizes(sizes, R)
    pools, pool_of_row = resolve_pools(pool, R, V)
    check_card_ids(inputs, V)
    if R == 0:
        return []
    lib = L.lib()
    if per_step > int(lib.cc_complete_max_per_step()):
        raise ValueError(f'per_step is {per_step}: above cc_complete_max_per_step() = '
                         f'{int(lib.cc_complete_max_per_step())}')
    out = []

    def launch(r0, r1, turn):
        row_ptr, idx, _, _, _ = pack_cubes(inputs[r0:r1], V)
        Rc = r1 - r0
        target, passes, A, max_n = plan_passes(np.diff(row_ptr), sizes[r0:r1], per_step, V)
        if passes == 0:                       # every row is at or above its size
            return None, mark(rec.stream)
        ws = rec._batch_ws.get(lib.cc_complete_ws_size(V, d, Rc, max_n, per_step), dev)
        rp_d, ix_d, tn_d = upload(row_ptr, dev), upload(idx, dev), upload(target, dev)
        ints = torch.empty(Rc * (1 + A), device=dev, dtype=torch.int32)      # n_added, added
        vals = torch.empty(Rc * A, device=dev, dtype=torch.float32)
        por_d = upload(pool_of_row[r0:r1], dev) if pools is not None else None
        pool_args = rec._pool_args(table, por_d, none=(None, 0, None))
        L.call('cc_complete_fp32', L.ptr(rec.params), V, d, Rc, L.ptr(rp_d), L.ptr(ix_d), max_n, L.ptr(tn_d),
               per_step, passes, *pool_args, A, L.ptr(ints), L.ptr(ints[Rc:]), L.ptr(vals), L.ptr(ws),
               ws.numel() * 4, L.stream_ptr(rec.stream))
        return (A, rec._rank_pins.fresh(ints).numpy(), rec._rank_pins.fresh(vals).numpy()), mark(rec.stream)

    def collect(r0, r1, payload):
        Rc = r1 - r0
        if payload is None:
            out.extend({'added': np.zeros(0, np.int32), 'added_vals': np.zeros(0, np.float32)} for _ in range(Rc))
            return
        A, ints, vals = payload
        nadd, adds, addv = ints[:Rc].tolist(), ints[Rc:].reshape(Rc, A), vals.reshape(Rc, A)
        for r in range(Rc):
            out.append({'added': adds[r, :nadd[r]].copy(), 'added_vals': addv[r, :nadd[r]].copy()})

    with rec.lock, torch.cuda.stream(rec.stream):
        table = rec._pool_table(pools) if pools is not None else None
        pipelined(row_spans(R, rows_per_launch), launch, collect)
    return out
