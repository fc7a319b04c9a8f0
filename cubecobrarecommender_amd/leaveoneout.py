"""Leave-one-out scores: p(c | cube without c) for every cube card, and the same
derived rows read at chosen target cards (cc_leave_one_out_fp32, csrc/loo.hip).

A cube of n distinct cards has n + 1 derived rows, q = 0 .. n: row 0 is the base row (nothing left
out), row q leaves out the id at sorted position q - 1.  Everything but `leave_one_out` itself is
pure host code: rows are dealt to launches in cube order, a cube larger than one launch is sliced
by positions, and a launch's results are laid out by `out_ptr`."""
import numpy as np
import torch

from . import _lib as L
from .launches import mark, pipelined, upload
from .recommender import check_card_ids, cuts_in_input_order, pack_cubes

GATHER_CHUNK = 32                  # ids per E1 chunk (csrc/infer.hip)
LOO_STAGING_BYTES = 128 << 20      # result bytes staged per launch; more targets than fit are split


def chunk_slots(n):
    """E1 chunk partials a cube of n distinct cards takes in the workspace (at least 1)."""
    return max(1, -(-int(n) // GATHER_CHUNK))


def plan_rows(ns, rows_per_launch):
    """Derived rows of cubes with ns[c] distinct cards -> launches, each a list of slices
    (cube, q0, q1): rows q0 .. q1 - 1 of that cube.  Rows go out in cube order, at most
    rows_per_launch (below 1 counts as 1) per launch.  The chunk partials of a launch are a
    rectangle cubes x chunk_slots(longest cube): a further cube joins a launch only while that
    rectangle stays within max(4, rows_per_launch // 8) slots, so the workspace is bounded by the
    rows per launch and by the one largest cube, never by their product."""
    step = max(1, int(rows_per_launch))
    slots = max(4, step // 8)
    launches, cur, used, ncubes, cap = [], [], 0, 0, 0
    for c, n in enumerate(ns):
        q, total, ccap = 0, int(n) + 1, chunk_slots(n)
        while q < total:
            new_cube = not cur or cur[-1][0] != c
            if cur and (used == step or (new_cube and (ncubes + 1) * max(cap, ccap) > slots)):
                launches.append(cur)
                cur, used, ncubes, cap, new_cube = [], 0, 0, 0, True
            take = min(total - q, step - used)
            cur.append((c, q, q + take))
            if new_cube:
                ncubes, cap = ncubes + 1, max(cap, ccap)
            used, q = used + take, q + take
    if cur:
        launches.append(cur)
    return launches


def launch_rows(slices):
    """One launch's slices -> (c0, c1, row_cube, row_pos): its cubes are [c0, c1), row_cube int32
    counts from c0, row_pos int32 is the sorted position left out, -1 for a base row."""
    c0, c1 = slices[0][0], slices[-1][0] + 1
    row_cube = np.concatenate([np.full(q1 - q0, c - c0, np.int32) for c, q0, q1 in slices])
    row_pos = np.concatenate([np.arange(q0 - 1, q1 - 1, dtype=np.int32) for _, q0, q1 in slices])
    return c0, c1, row_cube, row_pos


def out_offsets(counts):
    """Result words per derived row -> out_ptr int32 [rows + 1]."""
    out_ptr = np.zeros(len(counts) + 1, np.int64)
    out_ptr[1:] = np.cumsum(counts, dtype=np.int64)
    if out_ptr[-1] >= 2 ** 31:
        raise ValueError('more than 2^31 results in one launch: lower rows_per_launch')
    return out_ptr.astype(np.int32)


def target_chunks(T, rows, budget_bytes=None):
    """[(t0, t1)] tiling [0, T) so that rows x (t1 - t0) float32 results stay within budget_bytes
    (LOO_STAGING_BYTES); at least one target per chunk."""
    budget = LOO_STAGING_BYTES if budget_bytes is None else int(budget_bytes)
    step = max(1, budget // (4 * max(int(rows), 1)))
    return [(t0, min(T, t0 + step)) for t0 in range(0, T, step)]


def per_cube_targets(targets, C, V):
    """The `targets` argument -> C int64 arrays: one flat list of ids serves every cube, else one
    list per cube.  Raises ValueError for another number of lists or an id outside [0, V)."""
    flat = isinstance(targets, np.ndarray) and targets.ndim == 1
    if not flat:
        targets = list(targets)
        flat = all(np.ndim(t) == 0 for t in targets)
    if flat:
        one = np.asarray(targets, np.int64).reshape(-1)
        if len(one) and (one.min() < 0 or one.max() >= V):
            raise ValueError(f'target card {int(one[(one < 0) | (one >= V)][0])} outside [0, {V})')
        return [one] * C
    tl = [np.asarray(t, np.int64).reshape(-1) for t in targets]
    if len(tl) != C:
        raise ValueError(f'{len(tl)} target lists for {C} cubes')
    check_card_ids(tl, V)
    return tl


class Plan:
    """One leave_one_out call on the host: the checked and packed arguments, the launches
    (`items`: (slices, t0, t1), targets [t0, t1) of every cube's list; 0, 0 in self mode), the
    arrays each launch takes (`arrays`), and the place every result word lands (`take`, `results`).
    Raises ValueError for an id outside [0, V) in cubes or targets."""

    def __init__(self, cubes, targets, V, rows_per_launch, budget_bytes=None):
        row_ptr, self.idx, _, self.inputs, self.slot = pack_cubes(list(cubes), V)
        C = len(self.inputs)
        self.tl = tl = None if targets is None else per_cube_targets(targets, C, V)
        self.row_ptr = row_ptr.astype(np.int64)
        self.ns = ns = np.diff(self.row_ptr)
        self.items = []
        for slices in plan_rows(ns, rows_per_launch):
            if tl is None:
                self.items.append((slices, 0, 0))
                continue
            rows = sum(q1 - q0 for _, q0, q1 in slices)
            T = max(len(tl[c]) for c in range(slices[0][0], slices[-1][0] + 1))
            self.items += [(slices, t0, t1) for t0, t1 in target_chunks(T, rows, budget_bytes)]
        nnz = int(self.row_ptr[-1])
        if tl is None:
            self.loo, self.cut = np.zeros(nnz, np.float32), np.zeros(nnz, np.float32)
        else:
            self.base = [np.zeros(len(t), np.float32) for t in tl]
            self.without = [np.zeros((int(n), len(t)), np.float32) for n, t in zip(ns, tl)]

    def arrays(self, i):
        """Launch i as cc_leave_one_out_fp32 takes it: n_cubes, max_n, rows (ints) and row_ptr,
        idx, row_cube, row_pos, tgt_ptr, tgt, out_ptr (int32 arrays; the targets None in self
        mode, where a base row returns its cube's n cut values and a derived row one word)."""
        slices, t0, t1 = self.items[i]
        c0, c1, row_cube, row_pos = launch_rows(slices)
        lo, ns = self.row_ptr[c0], self.ns[c0:c1]
        a = {'n_cubes': c1 - c0, 'max_n': int(ns.max()), 'rows': len(row_cube), 'row_cube': row_cube,
             'row_pos': row_pos, 'row_ptr': (self.row_ptr[c0:c1 + 1] - lo).astype(np.int32),
             'idx': self.idx[lo:self.row_ptr[c1]], 'tgt_ptr': None, 'tgt': None}
        if self.tl is None:
            counts = np.where(row_pos < 0, ns[row_cube], 1)
        else:
            tgs = [self.tl[c][t0:t1] for c in range(c0, c1)]
            Tc = np.fromiter((len(t) for t in tgs), np.int64, c1 - c0)
            a['tgt_ptr'] = np.zeros(c1 - c0 + 1, np.int32)
            a['tgt_ptr'][1:] = np.cumsum(Tc)
            a['tgt'] = np.concatenate(tgs).astype(np.int32)
            counts = Tc[row_cube]
        a['out_ptr'] = out_offsets(counts)
        return a

    def take(self, i, out_ptr, out):
        """File launch i's results `out` (float32, laid out by its out_ptr)."""
        slices, t0, t1 = self.items[i]
        r = 0
        for c, q0, q1 in slices:
            k, lo, n = q1 - q0, int(self.row_ptr[c]), int(self.ns[c])
            seg = out[out_ptr[r]:out_ptr[r + k]]
            r += k
            p0 = max(q0 - 1, 0)                     # the first left-out position of the slice
            if self.tl is None:
                if q0 == 0:
                    self.cut[lo:lo + n], seg = seg[:n], seg[n:]
                self.loo[lo + p0:lo + p0 + len(seg)] = seg
                continue
            Tc = len(self.tl[c][t0:t1])
            if Tc == 0:
                continue
            block = seg.reshape(k, Tc)
            if q0 == 0:
                self.base[c][t0:t0 + Tc], block = block[0], block[1:]
            self.without[c][p0:p0 + len(block), t0:t0 + Tc] = block

    def results(self):
        """One dict per cube, in the cubes' input order (duplicated ids repeat their value)."""
        if self.tl is None:
            loo = cuts_in_input_order(self.loo, self.slot, self.inputs)
            cut = cuts_in_input_order(self.cut, self.slot, self.inputs)
            return [{'loo_vals': a, 'cut_vals': b} for a, b in zip(loo, cut)]
        ends = np.cumsum([len(ci) for ci in self.inputs])
        return [{'base': self.base[c], 'without': self.without[c][self.slot[e - len(ci):e] - self.row_ptr[c]]}
                for c, (ci, e) in enumerate(zip(self.inputs, ends))]


def leave_one_out(rec, cubes, targets=None, rows_per_launch=4096):
    """The body of Recommender.leave_one_out (documented there)."""
    V, d, dev = rec.V, rec.d, rec.dev
    plan = Plan(cubes, targets, V, rows_per_launch)
    if not plan.items:
        return plan.results()
    lib = L.lib()

    def launch(i, _, turn):
        a = plan.arrays(i)
        ws = rec._batch_ws.get(lib.cc_leave_one_out_ws_size(V, d, a['n_cubes'], a['max_n'], a['rows']), dev)
        out = torch.empty(max(int(a['out_ptr'][-1]), 1), device=dev, dtype=torch.float32)
        t = {k: upload(a[k], dev) for k in ('row_ptr', 'idx', 'row_cube', 'row_pos', 'out_ptr')}
        tp, tg = (None, None) if a['tgt_ptr'] is None else (upload(a['tgt_ptr'], dev), upload(a['tgt'], dev))
        L.call('cc_leave_one_out_fp32', L.ptr(rec.params), V, d, a['n_cubes'], L.ptr(t['row_ptr']), L.ptr(t['idx']),
               a['max_n'], a['rows'], L.ptr(t['row_cube']), L.ptr(t['row_pos']), L.ptr(tp), L.ptr(tg),
               L.ptr(t['out_ptr']), L.ptr(out), L.ptr(ws), ws.numel() * 4, L.stream_ptr(rec.stream))
        return (a['out_ptr'], rec._rank_pins.fresh(out).numpy()), mark(rec.stream)

    with rec.lock, torch.cuda.stream(rec.stream):
        pipelined([(i, i + 1) for i in range(len(plan.items))], launch,
                  lambda i, _, payload: plan.take(i, *payload))
    return plan.results()
