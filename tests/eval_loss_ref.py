"""Host restatement of cc_recommend_batch_loss_fp32's pinned arithmetic (test infrastructure only).

  logit   oracle/infer_ref's fp32 forward (encode32, the decoder tower, dense32 without ReLU)
  term    fp64, every operation separately rounded, with oracle.detmath:
          t = (max(z, 0) - z*y) + det_log(1 + det_exp(-|z|));  a card >= V contributes +0.0
  tile    64 cards = 16 lanes x 4 consecutive cards: a lane sums ((t0 + t1) + t2) + t3, the lanes
          combine by an xor butterfly, offsets 1, 2, 4, 8: a = a + a[lane ^ off]
  row     tile partials added from 0.0 in ascending tile order, then / float(V)
  pred    first index of the maximum of p' = 1 where z >= SIG_SAT, else det_sigmoid32(z); the
          same tree with ties to the lower index (within a lane, across the butterfly, across
          tiles), which is numpy's argmax
"""
import numpy as np

from oracle import infer_ref, model_ref
from oracle.detmath import det_exp, det_log, det_sigmoid32

SIG_SAT = np.float32(15.7243833541870117)   # Eigen's logistic is exactly 1 from here on
TILE, LANES, PER_LANE = 64, 16, 4


def hidden32(P, cube):
    """h3 [d] of one cube: the input of the output layer."""
    h = infer_ref.encode32(P, cube)
    for nm in infer_ref.TOWER[3:]:
        h = infer_ref.dense32(h, P[nm + '/kernel'], P[nm + '/bias'])
    return h


def logits32(P, cube, h3=None):
    """fp32 logits [V] of one cube: what out_tile_kernel computes before the sigmoid."""
    h = hidden32(P, cube) if h3 is None else h3
    return infer_ref.dense32(h, P['decoder/reconstruct/kernel'], P['decoder/reconstruct/bias'], relu=False)


def target_mask(targets, V):
    """0/1 float64 [V]; ids outside [0, V) are ignored, duplicates collapse."""
    t = np.asarray(targets, np.int64).reshape(-1)
    y = np.zeros(V, np.float64)
    y[t[(t >= 0) & (t < V)]] = 1.0
    return y


def terms64(z, y):
    z64 = np.asarray(z, np.float32).astype(np.float64)
    a = np.maximum(z64, 0.0) - z64 * y
    return a + det_log(1.0 + det_exp(-np.abs(z64)))


def probs_sat(z):
    z = np.asarray(z, np.float32)
    return np.where(z >= SIG_SAT, np.float32(1.0), det_sigmoid32(z)).astype(np.float32)


def _tiles(a, fill):
    """[V] -> [tiles, 16 lanes, 4 cards], padded with `fill`."""
    V = len(a)
    n = -(-V // TILE)
    out = np.full(n * TILE, fill, a.dtype)
    out[:V] = a
    return out.reshape(n, LANES, PER_LANE)


def row_loss(z, y):
    """The row's loss as the device reduces it (float64)."""
    V = len(z)
    t = _tiles(terms64(z, y), 0.0)
    lane = ((t[:, :, 0] + t[:, :, 1]) + t[:, :, 2]) + t[:, :, 3]
    ids = np.arange(LANES)
    for off in (1, 2, 4, 8):
        lane = lane + lane[:, ids ^ off]
    total = np.float64(0.0)
    for part in lane[:, 0]:
        total = total + part
    return total / np.float64(V)


def row_pred(z):
    """First index of the maximum of p', reduced in the device's order."""
    V = len(z)
    p = _tiles(probs_sat(z), np.float32(-1.0))
    idx = _tiles(np.arange(V, dtype=np.int64), np.int64(2 ** 31 - 1))
    bp, bi = p[:, :, 0].copy(), idx[:, :, 0].copy()
    for e in range(1, PER_LANE):
        take = p[:, :, e] > bp
        bp, bi = np.where(take, p[:, :, e], bp), np.where(take, idx[:, :, e], bi)
    ids = np.arange(LANES)
    for off in (1, 2, 4, 8):
        op, oi = bp[:, ids ^ off], bi[:, ids ^ off]
        take = (op > bp) | ((op == bp) & (oi < bi))
        bp, bi = np.where(take, op, bp), np.where(take, oi, bi)
    best_p, best_i = np.float32(-1.0), 0
    for t in range(bp.shape[0]):
        if bp[t, 0] > best_p:
            best_p, best_i = bp[t, 0], int(bi[t, 0])
    return best_i


def reference(P, cubes, targets=None):
    """(row_loss float64 [R], row_pred int32 [R], logits [R] of fp32 [V], masks [R] of 0/1 [V])."""
    targets = cubes if targets is None else targets
    V = P['decoder/reconstruct/kernel'].shape[1]
    zs = [logits32(P, c) for c in cubes]
    ys = [target_mask(t, V) for t in targets]
    loss = np.array([row_loss(z, y) for z, y in zip(zs, ys)], np.float64).reshape(len(zs))
    pred = np.array([row_pred(z) for z in zs], np.int32).reshape(len(zs))
    return loss, pred, zs, ys


def first_targets(targets, V):
    """tf.argmax of the multi-hot rows: the lowest valid target id, 0 for a row without one."""
    out = np.zeros(len(targets), np.int64)
    for r, t in enumerate(targets):
        t = np.asarray(t, np.int64).reshape(-1)
        t = t[(t >= 0) & (t < V)]
        out[r] = t.min() if len(t) else 0
    return out


# ---------------------------------------------------------------- the tests' shared cases
# one partial tile with V % 4 != 0; 16 tiles with a partial last one and two 64-wide chunks; three chunks
SHAPES = [(63, 64), (1001, 128), (1001, 192)]
KINDS = ['default', 'wide']
_cache = {}


def mixed_cubes(V):
    """The input rows the kernel's edges need (the targets come with the reference, below)."""
    rng = np.random.default_rng(V)
    n = min(V, 40)
    return [np.zeros(0, np.int64),                                   # 0: an empty cube
            rng.choice(V, n // 2, replace=False),                    # 1: targets = the cube
            rng.choice(V, n, replace=False),                         # 2: empty targets
            rng.choice(V, n // 3, replace=False),                    # 3: targets != cube
            rng.permutation(V),                                      # 4: all V cards
            rng.choice(V, n // 2, replace=False),                    # 5: duplicated, unsorted targets
            rng.choice(V, 5, replace=False),                         # 6: first target = the prediction (a hit)
            rng.choice(V, 9, replace=False),                         # 7: first target != the prediction (a miss)
            rng.choice(V, n, replace=True)]                          # 8: duplicates in the cube


def reference_case(V, d, kind):
    """(P, cubes, targets, ref) with ref = (row_loss, row_pred, logits, masks) of the restatement
    (host only); computed once per (shape, model) and shared, never changed."""
    key = (V, d, kind)
    if key in _cache:
        return _cache[key]
    P = model_ref.init_params(V, d, seed=V + d, bias_std=0.01)
    cubes = mixed_cubes(V)
    h3 = [hidden32(P, c) for c in cubes]                           # the output layer's input: both models'
    a, b = V // 3, V // 3 + 17                                       # the wide model's two cards at +50
    if kind == 'wide':
        # logits spread over +-20 and wider: the output kernel scaled so that the largest
        # |z - bias| on these rows becomes 20, a bias of N(0, 4), and two biases at +50 whose cards
        # tie at exactly 1.0.  The second one's column is set against row 6's h3, so that in row 6
        # (and in the rows more aligned with it) it falls below the saturation and out of the tie,
        # while in the empty cube's row, whose h3 is short, both stay at 1.0
        zs = [logits32(P, c, h) for c, h in zip(cubes, h3)]
        spread = max(float(np.abs(z - P['decoder/reconstruct/bias']).max()) for z in zs)
        rng = np.random.default_rng(V * d)
        P = dict(P)
        Wo = P['decoder/reconstruct/kernel'] * np.float32(20.0 / spread)
        bo = rng.normal(0.0, 2.0, V).astype(np.float32)
        bo[a] = bo[b] = 50.0
        u = h3[6].astype(np.float64)
        Wo[:, b] = (-(50.0 - 5.0) * u / (u @ u)).astype(np.float32)
        P['decoder/reconstruct/kernel'], P['decoder/reconstruct/bias'] = Wo.astype(np.float32), bo
    zs = [logits32(P, c, h) for c, h in zip(cubes, h3)]
    pred = [row_pred(z) for z in zs]
    rng = np.random.default_rng(V + 7 * d)
    t5 = rng.choice(V, 12, replace=False)
    other = [c for c in range(V) if c > pred[6]][:3]
    z4 = zs[4].copy()
    z4[[a, b]] = 0.0                                                 # row 4's extreme logits among the ordinary cards
    targets = [np.array([3, 1, min(V - 1, 70)]),                     # 0
               cubes[1],                                             # 1
               np.zeros(0, np.int64),                                # 2
               rng.choice(V, 25, replace=False),                     # 3
               np.concatenate([rng.choice(V, 7, replace=False), [int(np.argmax(z4)), int(np.argmin(z4))]]),   # 4
               rng.permutation(np.concatenate([t5, t5[:7], t5[2:4]])),   # 5
               np.array(other + [pred[6]], np.int64),                # 6: lowest id = the prediction
               np.array([c for c in range(V) if c != pred[7]][:2][::-1], np.int64),   # 7
               cubes[8]]                                             # 8
    ys = [target_mask(t, V) for t in targets]
    loss = np.array([row_loss(z, y) for z, y in zip(zs, ys)], np.float64)
    _cache[key] = (P, cubes, targets, (loss, np.array(pred, np.int32), zs, ys))
    return _cache[key]
