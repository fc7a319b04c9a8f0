"""CPU: where the tower weight gradients ride in the W1-gradient launch (StepPlan.dw_in_w1) and the
launch geometry that leaves CUs free for their rider workgroups (cc_embed_grad_cs_geometry)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from record_step_plans import dataset_inputs, load_table   # noqa: E402

from cubecobrarecommender_amd import _lib as L   # noqa: E402
from cubecobrarecommender_amd.plan import _cdf, plan_step   # noqa: E402
from cubecobrarecommender_amd.trainer import TrainConfig   # noqa: E402

TABLE = load_table(os.path.join(ROOT, 'tests', 'golden', 'step_plans.json'))
BENCH = dict(V=22000, d=256, batch_size=512, dtype='bf16', fuse_w1_adam=True, wo_adam_in_tower=True)


def _plan(**kw):
    cfg = TrainConfig(**{**BENCH, **kw})
    return plan_step(cfg, data_reg_rows=(0, cfg.V) if cfg.reg > 0 else None)


def test_bench_step_rides_by_default():
    p = _plan()
    assert p.fuse_w1 and p.tower_dw == 'direct' and p.has_wpack and p.dw_in_w1 == 16
    assert _plan(reg=0.1).dw_in_w1 == 0            # the sampled regulariser: measured slower, off unless asked
    assert _plan(reg=0.1, dw_in_w1=16).dw_in_w1 == 16             # (by index: 9 tower layers)
    assert _plan(reg=0.1, dw_in_w1=24, reg_by_index=False).dw_in_w1 == 24
    assert _plan(dw_in_w1=24).dw_in_w1 == 24       # the rider count is the config's
    assert _plan(batch_size=1024).dw_in_w1 == 16   # 1024 rows: still one wave per tile


@pytest.mark.parametrize('kw', [dict(dw_in_w1=0), dict(fuse_w1_adam=False), dict(dtype='fp32'),
                                dict(reg=0.1, reg_mode='full', dw_in_w1=16), dict(force_dp=True), dict(world=2),
                                dict(fused_tower=False), dict(prefetch_noise=False),
                                dict(batch_size=1024, reg=0.1, dw_in_w1=16)], ids=str)
def test_other_steps_keep_the_two_launches(kw):
    """Off without W1's Adam in its gradient kernel (unfused, data parallel, fp32, generic towers),
    in full mode, and where a chain has 2048 rows or more (its dW is split by rows)."""
    assert _plan(**kw).dw_in_w1 == 0


def test_field_follows_its_conditions_over_the_recorded_grid():
    """Every recorded config, asking for 16 riders: on exactly with fuse_w1, the direct dW from the
    packed images, not full mode, fewer than 2048 rows; by default (measured per mode) only the
    BCE-only steps of those."""
    on = 0
    for row in TABLE['rows']:
        if 'selection' not in row:
            continue
        ns, rows = dataset_inputs(row)
        p = plan_step(TrainConfig(**row['cfg'], dw_in_w1=16), cdf=_cdf(ns), data_reg_rows=rows)
        want = p.fuse_w1 and p.tower_dw == 'direct' and p.has_wpack and not p.full_reg and p.R < 2048
        assert p.dw_in_w1 == (16 if want else 0), row['cfg']
        auto = plan_step(TrainConfig(**row['cfg']), cdf=_cdf(ns), data_reg_rows=rows)
        assert auto.dw_in_w1 == (16 if want and not p.use_reg else 0), row['cfg']
        on += bool(want)
    assert on >= 10


def _geometry(V, d, R, riders):
    c, t, w = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    nb = L.lib().cc_embed_grad_cs_geometry(V, d, R, riders, ctypes.byref(c), ctypes.byref(t), ctypes.byref(w))
    return int(nb), c.value, t.value, w.value


@pytest.mark.parametrize('riders', [1, 8, 16, 24])
@pytest.mark.parametrize('V', [2500, 8184, 20884, 22000])
@pytest.mark.parametrize('d,R', [(256, 512), (256, 1024), (128, 256), (512, 512)])
def test_reserve_mode_geometry(V, d, R, riders):
    """With riders the W1 workgroups and the riders fit the 256 CUs together, no wave takes more
    tiles than its registers hold, the chunks cover every 32-row tile (bias row included) exactly
    once, the tickets of cc_embed_grad_cs_tickets cover the chunks, and a grid that already leaves
    the CUs free is the plain call's."""
    tiles, nsl = (V + 1 + 31) // 32, d // 32
    nb0, c0, t0, w0 = _geometry(V, d, R, 0)
    nb, c, t, w = _geometry(V, d, R, riders)
    assert nb == c * nsl and w == w0 and t <= 8 * w    # 8 waves per workgroup
    assert (c - 1) * t < tiles <= c * t                # every chunk non-empty, every tile in one chunk
    assert c <= int(L.lib().cc_embed_grad_cs_tickets(V, d, R))
    fits = -(-tiles // ((256 - riders) // nsl)) <= 8 * w   # some chunking leaves the CUs free
    if nb0 + riders <= 256 or not fits:
        assert (nb, c, t) == (nb0, c0, t0)
    else:
        assert t > t0 and nb + riders <= 256               # the finest chunking that fits:
        assert -(-tiles // (t - 1)) * nsl + riders > 256   # one tile fewer per chunk does not
    if d <= 256:
        assert nb + riders <= 256


def test_headline_geometry():
    """V = 22,000, d = 256, B = 512: 688 tiles; 32 chunks of 22 fill the chip, 16 riders re-chunk it
    to 30 chunks of 23 (240 W1 workgroups); V = 8184: 256 one-chunk-per-CU workgroups re-chunked."""
    assert _geometry(22000, 256, 512, 0)[:3] == (256, 32, 22)
    assert _geometry(22000, 256, 512, 16)[:3] == (240, 30, 23)
    assert _geometry(8184, 256, 512, 0)[0] == 256 and _geometry(8184, 256, 512, 16)[0] <= 240
    assert _geometry(2504, 256, 128, 16) == _geometry(2504, 256, 128, 0) and _geometry(2504, 256, 128, 0)[0] == 216
    assert _geometry(0, 256, 512, 16)[0] == 0
