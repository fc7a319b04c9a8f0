"""GPU: the tower weight gradients as rider workgroups of the W1 gradient + Adam launch
(cc_embed_grad_cs_adam_dw / cc_embed_grad_cs_adam_reg_dw, TrainConfig.dw_in_w1) against the two
launches they replace (cc_tower_bwd_dw_direct, then cc_embed_grad_cs_adam[_reg]): every result bit
for bit — a W1 tile and a dW job are each one wave's work, whichever launch and chunking runs them."""
import ctypes

import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.layout import Layout
from cubecobrarecommender_amd.trainer import DeviceDataset, TrainConfig, Trainer
from oracle import model_ref
from tests.gpu_helpers import problem

pytestmark = pytest.mark.gpu

ADAM = (1e-3, 0.9, 0.999, 1e-7)


def _inputs(V, d, R, Bt, Rt, nreg, seed):
    """Random operands of both products.  W1: R bit rows over V cards, the dPre1 image of pitch RP
    (reg rows, if any, behind the R cube rows), W1's p / m / v.  Towers: batch Bt, Rt rows in all
    (Rt > Bt: the regulariser branch's three layers too); any bf16 contents are valid packed images."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    bf = lambda n, s=0.2: (torch.randn(n, device='cuda', generator=g) * s).to(torch.bfloat16)
    RP = (R + nreg + 63) // 64 * 64
    X = torch.rand(V, R, device='cuda', generator=g) < 0.05
    w = (X.view(V, R // 32, 32).to(torch.int64) << torch.arange(32, device='cuda')).sum(-1)
    xt = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)            # [V][R / 32] bit words
    inp = dict(RP=RP, xt=xt, dpre=bf(d * RP, 0.1), p=torch.randn(V * d, device='cuda', generator=g) * 0.05,
               m=torch.randn(V * d, device='cuda', generator=g) * 1e-3,
               v=torch.rand(V * d, device='cuda', generator=g) * 1e-5,
               state=torch.tensor([4, 0, 0, 0], device='cuda', dtype=torch.int64),
               hpt=[bf(Rt * k) for k in (d, 256, 128, 64, 128, 256)],
               gpt=[bf(Rt * n) for n in (256, 128, 64, 128, 256, d)], rid=None)
    if nreg:
        rid = torch.randint(0, V, (nreg,), device='cuda', generator=g, dtype=torch.int32)
        rid[::7] = -1        # padding rows (owner-computes slots without a draw)
        rid[1:9] = V - 1     # a popular card: one tile with many reg k-steps
        inp['rid'] = rid
    return inp


def _run(fused, riders, V, d, R, Bt, Rt, nreg, packed, inp):
    dims = [(d, 256), (256, 128), (128, 64), (64, 128), (128, 256), (256, d)]
    nl = 9 if Rt > Bt else 6
    gw = [torch.full((k * n,), 7.0, device='cuda') for k, n in (dims[l if l < 6 else l - 3] for l in range(nl))]
    gb = [torch.full((n,), 7.0, device='cuda') for _, n in (dims[l if l < 6 else l - 3] for l in range(nl))]
    t = L.TowerArgs(dtype=L.CC_BF16, d=d, B=Bt, R=Rt)
    dummy = torch.zeros(16, device='cuda')       # (checked non-null; the packed dW job reads hpt / gpt only)
    t.gD3 = dummy.data_ptr()
    for a in range(5):
        t.gact[a] = dummy.data_ptr()
    for a in range(6):
        t.hpt[a], t.gpt[a] = inp['hpt'][a].data_ptr(), inp['gpt'][a].data_ptr()
    for l in range(nl):
        t.gw[l], t.gb[l] = gw[l].data_ptr(), gb[l].data_ptr()
    xt, p, m, v = (inp[k].clone() for k in ('xt', 'p', 'm', 'v'))
    shadow = torch.zeros(V * d, device='cuda', dtype=torch.bfloat16)
    bg = torch.full((d,), 7.0, device='cuda')
    tickets = torch.zeros(int(L.lib().cc_embed_grad_cs_tickets(V, d, R)), device='cuda', dtype=torch.int32)
    s = L.stream_ptr()
    w1 = (L.ptr(inp['dpre']), packed, V, d, R, inp['RP'], L.ptr(xt), L.ptr(bg), L.ptr(tickets), L.ptr(p), L.ptr(m),
          L.ptr(v), L.ptr(shadow), L.ptr(inp['state']), *ADAM)
    reg = (L.ptr(inp['rid']), nreg, R // 16) if nreg else ()
    name = 'cc_embed_grad_cs_adam_reg' if nreg else 'cc_embed_grad_cs_adam'
    if fused:
        L.call(name + '_dw', *w1, *reg, ctypes.byref(t), riders, s)
    else:
        L.call('cc_tower_bwd_dw_direct', ctypes.byref(t), s)
        L.call(name, *w1, *reg, s)
    torch.cuda.synchronize()
    assert int(xt.abs().sum().item()) == 0 and int(tickets.abs().sum().item()) == 0   # consumed, tickets reset
    out = {f'gw{l}': gw[l] for l in range(nl)}
    out.update({f'gb{l}': gb[l] for l in range(nl)})
    out.update(p=p, m=m, v=v, shadow=shadow, bias_grad=bg)
    return {k: x.cpu() for k, x in out.items()}


def _geometry(V, d, R, riders):
    c, tp = ctypes.c_int32(), ctypes.c_int32()
    return int(L.lib().cc_embed_grad_cs_geometry(V, d, R, riders, ctypes.byref(c), ctypes.byref(tp), None)), tp.value


def _compare(V, d, R, Bt, Rt, nreg, packed, rider_counts, seed):
    inp = _inputs(V, d, R, Bt, Rt, nreg, seed)
    base = _run(False, 0, V, d, R, Bt, Rt, nreg, packed, inp)
    assert not any(bool((base[k] == 7.0).all()) for k in base if k[0] == 'g' or k == 'bias_grad')   # all written
    assert not torch.equal(base['p'], inp['p'].cpu())
    for riders in rider_counts:
        got = _run(True, riders, V, d, R, Bt, Rt, nreg, packed, inp)
        bad = [k for k in base if not torch.equal(base[k], got[k])]
        assert not bad, (riders, bad)


# V = 2504: 27 chunks x 8 slices = 216 W1 workgroups, room for the riders as it is; V = 8184, R = 512:
# 256 tiles, one per CU — the reserve mode re-chunks; d = 128: the unpacked dPre1^T source, 4 slices;
# V = 2500: a partial last tile (the bias row inside it) and a short last chunk; R = 1024: the
# rider form of the 32-word instance (1024 tower rows: still one wave per dW tile)
@pytest.mark.parametrize('V,d,R', [(2504, 256, 128), (8184, 256, 512), (8184, 128, 256), (2500, 256, 128),
                                   (2504, 256, 1024)])
def test_fused_launch_matches_the_two_launches(V, d, R):
    """All six tower gw / gb, W1's p / m / v / shadow and the W1 bias gradient, with 1 rider (it
    walks all 208 jobs at d = 256) and the default 16."""
    if (V, d, R) == (8184, 256, 512):
        (nb0, t0), (nb, t1) = _geometry(V, d, R, 0), _geometry(V, d, R, 16)
        assert nb0 == 256 and nb + 16 <= 256 and t1 > t0
    _compare(V, d, R, R, R, 0, 1 if d == 256 else 0, (1, 16), seed=V + d + R)


def test_fused_launch_matches_reg_by_index():
    """The reg-by-index form: 128 cube rows in the bit matrix, 128 reg rows by card id (padding ids
    and a popular card among them); the towers carry all 256 rows (9 layers' dW)."""
    _compare(2504, 256, 128, 128, 256, 128, 1, (1, 16), seed=77)


def test_tall_chain_is_refused():
    """Where cc_tower_bwd_dw_direct splits the rows (2048 rows with a slab) the fused entry says so
    and launches nothing."""
    V, d, R = 2504, 256, 128
    inp = _inputs(V, d, R, 2048, 2048, 0, 5)
    t = L.TowerArgs(dtype=L.CC_BF16, d=d, B=2048, R=2048)
    keep = [torch.zeros(k * n + n, device='cuda') for k, n in [(d, 256), (256, 128), (128, 64), (64, 128), (128, 256), (256, d)]]
    slab = torch.zeros((2048 // 32) * int(L.lib().cc_tower_slab_elems(d)), device='cuda')
    t.gD3, t.slab = keep[0].data_ptr(), slab.data_ptr()
    for a in range(5):
        t.gact[a] = keep[0].data_ptr()
    for a in range(6):
        t.hpt[a], t.gpt[a] = inp['hpt'][a].data_ptr(), inp['gpt'][a].data_ptr()
        t.gw[a], t.gb[a] = keep[a].data_ptr(), keep[a].data_ptr()
    p0 = inp['p'].clone()
    shadow = torch.zeros(V * d, device='cuda', dtype=torch.bfloat16)
    bg = torch.zeros(d, device='cuda')
    tickets = torch.zeros(int(L.lib().cc_embed_grad_cs_tickets(V, d, R)), device='cuda', dtype=torch.int32)
    rc = L.lib().cc_embed_grad_cs_adam_dw(L.ptr(inp['dpre']), 1, V, d, R, inp['RP'], L.ptr(inp['xt']), L.ptr(bg),
                                          L.ptr(tickets), L.ptr(inp['p']), L.ptr(inp['m']), L.ptr(inp['v']),
                                          L.ptr(shadow), L.ptr(inp['state']), *ADAM, ctypes.byref(t), 16,
                                          L.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b'two launches' in L.lib().cc_last_error_string()
    assert torch.equal(inp['p'], p0)


@pytest.mark.parametrize('reg', [0.0, 0.1])
def test_trainer_with_riders_matches_without(reg):
    """bench.py's TrainConfig at V = 2504, d = 256, B = 128: dw_in_w1 on (16 riders; with the
    regulariser by request, its default there is off) against off over two eager steps, capture, step_many(11) in graphs of 4 steps, flush — parameters, moments,
    shadow, device counters and the losses."""
    V, d, B = 2504, 256, 128
    out = {}
    for riders in (0, 16):
        lists, Mt, ns = problem(19, 1024, V, (20, 40, 80))
        P = model_ref.init_params(V, d, seed=19, bias_std=0.01)
        cfg = TrainConfig(V=V, d=d, batch_size=B, reg=reg, dtype='bf16', seed=19, fuse_w1_adam=True,
                          wo_adam_in_tower=True, graph_steps=4, dw_in_w1=riders)
        tr = Trainer(cfg, DeviceDataset(lists, V, y_mtx=Mt.astype(np.float32) if reg > 0 else None, neg_sampler=ns),
                     params_flat=Layout(V, d).pack(P))
        tr.set_epoch_permutation(np.random.default_rng(19).permutation(1024).astype(np.int32))
        assert tr.dw_in_w1 == riders and tr.fuse_w1 and tr.reg_by_index == (reg > 0)
        losses = []
        for _ in range(2):
            tr.step()
            losses.append(tr.losses())
        acc = torch.zeros(2, dtype=torch.float64, device='cuda')
        tr.capture(loss_acc=acc)
        tr.step_many(11, loss_acc=acc)
        tr.flush()
        torch.cuda.synchronize()
        tr.check_status()
        out[riders] = (tr.params.cpu(), tr.m.cpu(), tr.v.cpu(), tr.shadow.cpu(), tr.state.cpu(), acc.cpu(), losses)
    for i, (a, b) in enumerate(zip(out[0][:6], out[16][:6])):
        assert torch.equal(a, b), i
    assert out[0][6] == out[16][6] and float(out[16][5][0]) > 0
