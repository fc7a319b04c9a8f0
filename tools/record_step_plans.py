"""Record which kernel path every part of the training step takes, per config, into
tests/golden/step_plans.json (the table tests/test_step_plan.py pins plan.plan_step to).

    python tools/record_step_plans.py --cpu [--out tests/golden/step_plans.json]

For every config of GRID it constructs a Trainer and reads the selection off its attributes
(attributes and the three query methods only, so the script runs unchanged on either side of a
change to how the selection is made).  The table is a record of a *parent* commit: check that
commit out, run this, and commit the result with the change; the CPU test then holds the new code
to what the parent selected.

--cpu: no GPU.  Trainer.__init__'s decisions touch no device result, so the kernel launches
(_lib.call), the stream helpers and torch.cuda.Stream are stubbed, the buffers are host memory
(zero pages, never written) and the library is loaded only for its host-side size queries.  Without
--cpu the trainers are constructed on cuda:0 (no step runs).  The file says which way it was made.

Samplers are recipes ('zipf': neg_sampler ∝ 1/(1+i); 'uniform'), so a row's inputs — the config,
the sampler's CDF, the M~ rows the dataset holds — rebuild from the file alone.
"""
import argparse
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# plain attributes of the trainer: flags and static quantities
FLAGS = ('dp', 'use_reg', 'full_reg', 'owner', 'Breg', 'R', 'RP', 'reg_rows', 'kl_row_scale', 'kl_loss_scale',
         'reg_by_index', 'xt_rows', 'mx8', 'dtype', 'fused_tower', 'embed_mfma', 'dx_glds', 'fused_out', 'dz1_ld',
         'fused_reg', 'd3q_in_tower', 'mx8_bce_q', 'reg_logits_paired', 'prefetch', 'prefetch_dp', 'xt_in_gather',
         'xt_in_tower', 'adam_packs', 'w1_off', 'fuse_w1', 'wo_ranges', 'rest_ranges', 'wo_range', 'f_in_tower',
         'splits', 'splits_reg', 'tsplits', 'early_reg_out')
# "this buffer exists": selection key -> attribute that is a tensor or None
EXISTS = {'has_wpack': 'wpack', 'has_D3p': 'D3p', 'has_gpre1p': 'gpre1p', 'has_w1_cs': 'eg_tickets',
          'has_WoP': 'WoP', 'has_y_img': 'y_img', 'has_x_bits': 'x_bits', 'has_Z2': 'Z2'}
QUERIES = ('dp_defer_out_ok', 'bucket_hook_names', 'f_bucket_name')


def sampler(kind, V):
    p = 1.0 / (1.0 + np.arange(V)) if kind == 'zipf' else np.ones(V)
    return p / p.sum()


def plain(x):
    """JSON-plain value: tuples as lists, numpy scalars as Python's, flags as 0 / 1."""
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, (bool, np.bool_)):
        return int(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x)
    return x


def layout_facts(lay):
    return [lay.align, int(lay.group_biases), int(lay.total), plain(getattr(lay, 'w1_chunks', None))]


def load_table(path):
    """The table with every row's selection as a dict again."""
    with open(path) as f:
        doc = json.load(f)
    for r in doc['rows']:
        if 'selection' in r:
            r['selection'] = dict(zip(doc['keys'], r['selection']))
    return doc


def selection_of(tr):
    """The recorded selection of a constructed Trainer."""
    from cubecobrarecommender_amd import _lib as L
    from cubecobrarecommender_amd.trainer import dx_splitk_fits
    cfg = tr.cfg
    sel = {k: plain(getattr(tr, k)) for k in FLAGS}
    sel.update({k: int(getattr(tr, a) is not None) for k, a in EXISTS.items()})
    for q in QUERIES:
        sel[q] = plain(getattr(tr, q)())
    lay = tr.layout
    sel['layout'] = layout_facts(lay)
    # the tower dW launch: straight from the packed images / LDS-staged, or slabs + their reduce
    bf16 = tr.dtype == L.CC_BF16
    sel['tower_dw'] = (None if not tr.fused_tower else
                       'direct' if bf16 and (tr.hpt is not None or max(tr.R, cfg.batch_size) <= 1184) else 'slab')
    # the decoder dX launch of each branch: 'pair' = cc_gemm_pair with the branch's dW (the fused
    # output kernels leave dX alone: the LDS-DMA split-K kernels where the shape fits)
    dx = []
    for k, nr in enumerate(tr.branch_rows()):
        if not tr.fused_tower:
            dx.append('gemm')
        elif not ((k == 0 and tr.fused_out) or (k == 1 and tr.fused_reg)):
            dx.append('pair')
        elif k == 1 and tr.WoP is not None and nr % 128 == 0 and dx_splitk_fits(nr, cfg.V, cfg.d):
            dx.append('dx_splitk_pk')
        elif (tr.dx_glds and not tr.mx8 and nr % 128 == 0 and cfg.d % 128 == 0 and cfg.V % 8 == 0
              and dx_splitk_fits(nr, cfg.V, cfg.d)):
            dx.append('dx_splitk')
        else:
            dx.append('gemm')
    sel['dx_kernels'] = dx
    return sel


def C(data=None, **cfg):
    return {'cfg': cfg, 'data': dict(data or {})}


def grid():
    """The configs: the baseline and bench shapes, model.fit's, the GPU tests', and both sides of
    every threshold the selection has."""
    g = []
    bench = dict(fuse_w1_adam=True, wo_adam_in_tower=True)
    shard = {'shard': True}
    big = dict(V=22000, d=256, batch_size=512)
    # BASELINE.json configs 2-5 (config 1 constructs no trainer) at their own shapes, plain and as
    # bench.py configures them
    for sw in ({}, bench):
        g += [C(**big, **sw), C(**big, reg=0.1, **sw), C(**big, reg=0.1, reg_mode='full', **sw)]
        g += [C(V=22000, d=1024, batch_size=512, dtype='fp8', reg=r, **sw) for r in (0.0, 0.1)]
        for rank in (0, 7) if sw else (0,):   # (the one-process switches do nothing on 8 ranks)
            g.append(C(shard, **big, reg=0.1, world=8, rank=rank, reg_shard=True, **sw))
            g.append(C(shard, V=22000, d=1024, batch_size=512, dtype='fp8', reg=0.1, world=8, rank=rank,
                       reg_shard=True, **sw))
        g.append(C(**big, reg=0.1, world=8, rank=3, **sw))
        g.append(C(shard, **big, reg=0.1, reg_mode='full', world=8, rank=7, **sw))
    # bench.py --force-dp (reg_shard follows --reg), its switches one at a time
    g += [C(**big, force_dp=True, **bench), C(shard, **big, reg=0.1, force_dp=True, reg_shard=True, **bench),
          C(**big, reg=0.1, force_dp=True, **bench),
          C(shard, **big, reg=0.1, force_dp=True, reg_shard=True, dp_graph=False, **bench),
          C(shard, **big, reg=0.1, reg_mode='full', force_dp=True, **bench),
          C(shard, V=22000, d=1024, batch_size=512, dtype='fp8', reg=0.1, force_dp=True, reg_shard=True, **bench)]
    g += [C(**big, reg=0.1, f_in_tower=True, **bench), C(**big, reg=0.1, wo_tower_frac=0.3, **bench)]
    g.append(C(**big, reg=0.1, reg_mode='full', dx_packed_wo=False, **bench))
    # model.fit: the fused Adam placements in one process, metrics on request
    for dtype in ('bf16', 'fp32'):
        for reg in (0.0, 1.0):
            for metrics in (False, True):
                V, d, B = (2500, 256, 128) if dtype == 'bf16' else (700, 64, 32)
                g.append(C(V=V, d=d, batch_size=B, reg=reg, dtype=dtype, metrics=metrics, **bench))
    g += [C(V=700, d=64, batch_size=32, reg=1.0, world=2, rank=1), C(V=600, d=64, batch_size=16, reg=0.1, dtype='fp32')]
    # the GPU tests' configs (tests/test_gpu_*.py)
    for dtype in ('fp32', 'bf16'):
        for reg in (0.0, 0.1):
            for V, d, B, fused in ((700, 64, 32, True), (2500, 128, 64, True), (2500, 256, 64, True),
                                   (700, 64, 32, False), (2500, 128, 48, True), (2500, 256, 128, True),
                                   (2504, 256, 128, True), (2500, 512, 128, True), (2500, 256, 256, True),
                                   (2500, 256, 512, True), (1500, 128, 128, True)):
                g.append(C(V=V, d=d, batch_size=B, reg=reg, dtype=dtype, fused_tower=fused))
            g.append(C(V=700, d=64, batch_size=32, reg=reg, dtype=dtype, prefetch_noise=False))
    for reg in (0.0, 0.1):
        for V, d, B in ((1500, 128, 128), (2500, 1024, 128), (3000, 1024, 128), (2500, 1024, 64)):
            g.append(C(V=V, d=d, batch_size=B, reg=reg, dtype='fp8'))
            g.append(C(V=V, d=d, batch_size=B, reg=reg, dtype='fp8', fuse_w1_adam=True))
        g.append(C(V=2500, d=1024, batch_size=64, reg=reg))
        for fuse, wo, ft in ((False, False, False), (True, False, False), (True, True, False), (True, True, True)):
            for B in (128, 256):
                g.append(C(V=2500, d=256, batch_size=B, reg=reg, fuse_w1_adam=fuse, wo_adam_in_tower=wo, f_in_tower=ft))
        g.append(C(V=2500, d=256, batch_size=128, reg=reg, fuse_w1_adam=True, wo_adam_in_tower=True, graph_steps=4))
    for dtype, V, d, B in (('fp32', 700, 64, 32), ('bf16', 1500, 256, 128), ('bf16', 1500, 512, 128),
                           ('bf16', 5000, 256, 256), ('bf16', 2500, 256, 128), ('bf16', 2502, 256, 128),
                           ('bf16', 2504, 256, 128), ('bf16', 300, 128, 128), ('fp8', 1500, 128, 128)):
        g.append(C(V=V, d=d, batch_size=B, reg=0.3, dtype=dtype, reg_mode='full'))
        if V in (700, 1500) and d != 512:   # (tests/test_gpu_train.py's metrics cases)
            g.append(C(V=V, d=d, batch_size=B, reg=0.1, dtype=dtype, reg_mode='full', metrics=True))
    for V, B, d in ((2500, 128, 256), (3001, 256, 256), (2500, 128, 512), (2504, 128, 256), (2504, 256, 256),
                    (700, 512, 256)):
        g.append(C(V=V, d=d, batch_size=B, reg=0.1))
        g.append(C(V=V, d=d, batch_size=B))
    for d, dtype in ((256, 'bf16'), (512, 'bf16'), (1024, 'fp8')):
        for fused in (True, False):
            for by_index in (True, False):
                g.append(C(V=2500, d=d, batch_size=128, reg=0.1, dtype=dtype, reg_by_index=by_index,
                           fuse_w1_adam=fused, prefetch_noise=fused))
    g += [C(V=700, d=128, batch_size=128, reg=0.1), C(V=2504, d=256, batch_size=128, **bench, f_in_tower=True),
          C(V=300, d=64, batch_size=32, reg=0.1, dtype='fp32'), C(V=700, d=128, batch_size=128, reg=0.1, dtype='fp8'),
          C(V=300, d=128, batch_size=128, reg=0.1, reg_mode='full')]
    # data parallel (tests/test_gpu_dp.py): gloo ranks, the bench shape, one-rank RCCL, fp8
    for rank in (0, 1):
        for reg, rs in ((0.0, False), (0.1, False), (0.1, True)) if rank == 0 else ((0.1, True),):
            g.append(C(V=700, d=64, batch_size=32, reg=reg, dtype='fp32', world=2, rank=rank, reg_shard=rs))
            g.append(C(V=2500, d=256, batch_size=128, reg=reg, world=2, rank=rank, reg_shard=rs))
            g.append(C(V=700, d=64, batch_size=16, reg=reg, dtype='fp32', world=2, rank=rank))
        for rs in (False, True):
            g.append(C(V=3000, d=1024, batch_size=128, reg=0.1, dtype='fp8', world=2, rank=rank, reg_shard=rs))
            for fw in (True, False):
                g.append(C(shard if rs else None, **big, reg=0.1, world=2, rank=rank, reg_shard=rs, fuse_w1_adam=fw))
    for V, d, dtype in ((2500, 256, 'bf16'), (2500, 1024, 'fp8')):
        for reg, rs in ((0.0, False), (0.1, False), (0.1, True)):
            for kw in ({}, {'w1_chunks': 2}, {'w1_chunks': 3}, {'dp_graph': False}):
                g.append(C(V=V, d=d, batch_size=128, reg=reg, dtype=dtype, force_dp=True, reg_shard=rs, **kw))
    # thresholds: dtype x d
    for dtype in ('bf16', 'fp32', 'fp8'):
        for d in (64, 128, 256, 512, 1024, 2048):
            g.append(C(V=1024, d=d, batch_size=128, reg=0.1, dtype=dtype))
            g.append(C(V=1024, d=d, batch_size=128, reg=0.1, dtype=dtype, **bench, f_in_tower=True))
            g.append(C(V=1024, d=d, batch_size=128, reg=0.1, dtype=dtype, force_dp=True, reg_shard=True))
            g.append(C(V=1024, d=d, batch_size=128, reg=0.1, dtype=dtype, reg_mode='full'))
    # ... B: off the 32-row blocks, the fused D1 shapes (128 / 256 / 512), the quantiser launches
    # above 512, more W1-product rows than 2048
    for dtype in ('bf16', 'fp8', 'fp32'):
        for B in (16, 48, 128, 256, 512, 640, 1024, 1152, 2176):
            for reg in (0.0, 0.1) if dtype == 'bf16' else (0.1,):
                g.append(C(V=1024, d=128, batch_size=B, reg=reg, dtype=dtype, **bench))
        g.append(C(V=1024, d=128, batch_size=1024, reg=0.1, dtype=dtype, reg_by_index=False))
        g.append(C(V=1024, d=128, batch_size=2048, reg=0.1, dtype=dtype, reg_by_index=False))
    # ... Breg: <= 512, <= 1024, above (full mode's row count follows V), Breg % 128
    for V in (500, 512, 1000, 1024, 1056, 1280):
        for dtype in ('bf16', 'fp8'):
            g.append(C(V=V, d=256, batch_size=128, reg=0.1, dtype=dtype, reg_mode='full'))
        g.append(C(V=V, d=256, batch_size=128, reg=0.1, reg_mode='full', dx_packed_wo=False))
    for B in (512, 1024):
        for world in (2, 8):
            g.append(C(V=4096, d=256, batch_size=B, reg=0.1, world=world, rank=1, reg_shard=True))
            g.append(C({'sampler': 'uniform'}, V=4096, d=256, batch_size=B, reg=0.1, world=world, rank=1, reg_shard=True))
    # ... V: V % 8, fewer than 32 K-splits of 512
    for V in (300, 512, 1025, 4100, 16383, 16384, 16388):
        for dtype in ('bf16', 'fp8', 'fp32'):
            for reg in (0.0, 0.1) if dtype == 'bf16' else (0.1,):
                g.append(C(V=V, d=256, batch_size=128, reg=reg, dtype=dtype))
    g.append(C(V=4100, d=256, batch_size=128, reg=0.1, reg_mode='full'))
    # ... the fused D2 kernel's 32-bit extent of M~ (hi * V * 4 bytes): the last row shard of 8
    for V in (23170, 23171):
        g.append(C(shard, V=V, d=128, batch_size=128, reg=0.1, reg_mode='full', world=8, rank=7))
        g.append(C(shard, V=V, d=128, batch_size=128, reg=0.1, world=8, rank=7, reg_shard=True))
        g.append(C(shard, V=V, d=128, batch_size=128, reg=0.1, world=8, rank=0, reg_shard=True))
    # ... world: 8 with and without the row shards, 3 (not a power of two), every regulariser mode
    for world, rank in ((8, 5), (3, 2)):
        for dtype, d in (('bf16', 256), ('fp32', 64), ('fp8', 1024)):
            g.append(C(V=3000, d=d, batch_size=128, dtype=dtype, world=world, rank=rank))
            for rs in (False, True):
                g.append(C(V=3000, d=d, batch_size=128, reg=0.1, dtype=dtype, world=world, rank=rank, reg_shard=rs))
            g.append(C(shard, V=3000, d=d, batch_size=128, reg=0.1, dtype=dtype, world=world, rank=rank,
                       reg_mode='full'))
    # ... each boolean switch against the bench configuration, both regulariser states; w1_chunks
    base = dict(V=2504, d=256, batch_size=256)
    for reg in (0.0, 0.1):
        for dp in (False, True) if reg else (False,):
            on = dict(base, reg=reg, force_dp=dp, reg_shard=dp and reg > 0, **bench)
            g.append(C(**on))
            for sw, v in (('fused_tower', False), ('prefetch_noise', False), ('fuse_w1_adam', False),
                          ('wo_adam_in_tower', False), ('f_in_tower', True), ('dx_packed_wo', False),
                          ('dp_defer_out', False), ('dp_graph', False), ('dp_f_in_adam', False), ('dz_pad', False),
                          ('metrics', True), ('reg_by_index', False), ('reg_shard', not on['reg_shard']),
                          ('w1_chunks', 2), ('wo_tower_frac', 0.0), ('wo_tower_frac', 1.0), ('wo_tower_frac', 1e-5)):
                g.append(C(**dict(on, **{sw: v})))
    g.append(C(V=2504, d=1024, batch_size=256, reg=0.1, force_dp=True, w1_chunks=2))
    g.append(C(V=2504, d=1024, batch_size=256, reg=0.1, force_dp=True))
    g.append(C(V=2504, d=1024, batch_size=256, reg=0.1, reg_mode='full', force_dp=True, w1_chunks=2))
    # ... what the plan rejects
    g += [C(V=1024, d=96, batch_size=128), C(V=1024, d=192, batch_size=128), C(V=1024, d=256, batch_size=128, dtype='fp16'),
          C(V=1024, d=256, batch_size=128, reg=0.1, reg_mode='all'),
          C({'matrix': False}, V=1024, d=256, batch_size=128, reg=0.1),
          C(V=1024, d=64, batch_size=128, dtype='fp8'), C(V=1024, d=128, batch_size=96, dtype='fp8'),
          C(V=1024, d=128, batch_size=64, dtype='fp8'), C(V=1024, d=128, batch_size=64, dtype='fp8', reg=0.1),
          C(V=1000, d=128, batch_size=128, dtype='fp8', reg=0.1, reg_mode='full'),
          C(V=1024, d=128, batch_size=128, dtype='fp8', fused_tower=False),
          C(V=1024, d=2048, batch_size=128, dtype='fp8', reg=0.1),
          C({'rows': [0, 512]}, V=1024, d=128, batch_size=128, reg=0.1, world=2, rank=1, reg_shard=True),
          C({'rows': [0, 512]}, V=1024, d=128, batch_size=128, reg=0.1),
          C(V=64, d=128, batch_size=128, reg=0.1, world=8, rank=0, reg_shard=True),      # an empty mass shard
          C(V=1024, d=128, batch_size=128, reg=0.1, reg_mode='all', dtype='fp16')]
    seen, out = set(), []
    for row in g:
        key = json.dumps(row, sort_keys=True)
        if key not in seen:
            seen.add(key)
            out.append(row)
    return out


def dataset_inputs(row):
    """(neg_sampler, the M~ rows the dataset holds or None) of a grid row."""
    from cubecobrarecommender_amd.trainer import TrainConfig, reg_rows_for
    cfg = TrainConfig(**row['cfg'])
    d = row['data']
    ns = sampler(d.get('sampler', 'zipf'), cfg.V)
    if not d.get('matrix', cfg.reg > 0):
        return ns, None
    if 'rows' in d:
        return ns, tuple(d['rows'])
    if d.get('shard'):
        return ns, reg_rows_for(ns, cfg.world, cfg.rank, cfg.reg_mode)
    return ns, (0, cfg.V)


def record_row(row, device):
    import torch
    from cubecobrarecommender_amd.trainer import DeviceDataset, TrainConfig, Trainer
    cfg = TrainConfig(**row['cfg'])
    try:
        ns, rows = dataset_inputs(row)
        y = torch.zeros(rows[1] - rows[0], cfg.V) if rows is not None else None
        data = DeviceDataset(csr=([0, 2, 4], [0, 1, 1, 2]), num_cards=cfg.V, neg_sampler=ns, y_mtx=y,
                             reg_rows=rows, device=device)
        return dict(row, selection=selection_of(Trainer(cfg, data, device=device)))
    except (ValueError, AssertionError) as e:
        return dict(row, error={'type': type(e).__name__, 'message': str(e)})


def stub_device():
    """--cpu: launches and streams do nothing; the library's host-side size queries stay real."""
    import ctypes
    import torch
    from cubecobrarecommender_amd import _lib as L
    L.call = lambda name, *args: None
    L.stream_ptr = lambda stream=None: ctypes.c_void_p(0)
    torch.cuda.Stream = lambda *a, **kw: None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cpu', action='store_true', help='no GPU: stub the launches, host buffers')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'step_plans.json'))
    args = ap.parse_args()
    if args.cpu:
        stub_device()
    commit = subprocess.run(['git', '-C', ROOT, 'rev-parse', 'HEAD'], capture_output=True, text=True).stdout.strip()
    dirty = bool(subprocess.run(['git', '-C', ROOT, 'status', '--porcelain', '--', 'cubecobrarecommender_amd'],
                                capture_output=True, text=True).stdout.strip())
    rows = [record_row(r, 'cpu' if args.cpu else 'cuda') for r in grid()]
    doc = {'recorded_at_commit': commit, 'package_modified': dirty,
           'made': ('on a CPU: launches, stream helpers and torch.cuda.Stream stubbed, device="cpu"' if args.cpu
                    else 'on a GPU: trainers constructed on cuda:0, no step run'),
           'tool': 'tools/record_step_plans.py', 'rows': rows}
    # one row per line; a selection as the list of its values in the order of "keys" (flags 0 / 1)
    keys = sorted(next(r['selection'] for r in rows if 'selection' in r))
    doc['keys'] = keys
    packed = [{k: ([r[k][n] for n in keys] if k == 'selection' else v) for k, v in r.items()} for r in rows]
    with open(args.out, 'w') as f:
        f.write('{\n')
        for k in ('recorded_at_commit', 'package_modified', 'made', 'tool', 'keys'):
            f.write(f' {json.dumps(k)}: {json.dumps(doc[k])},\n')
        f.write(' "rows": [\n' + ',\n'.join('  ' + json.dumps(r, sort_keys=True, separators=(',', ':'))
                                            for r in packed) + '\n ]\n}\n')
    errs = sum('error' in r for r in rows)
    print(f'{len(rows)} rows ({errs} rejected) at {commit[:7]} -> {args.out}')


if __name__ == '__main__':
    main()
