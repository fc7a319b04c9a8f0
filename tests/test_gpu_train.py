"""GPU training-step parity vs the CPU oracle (oracle/model_ref.py): loss within 1e-4 relative at
fp32; the bf16 MFMA path vs the oracle emulating the same bf16 operand rounding."""
import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.layout import Layout
from cubecobrarecommender_amd.trainer import DeviceDataset, TrainConfig, Trainer
from oracle import model_ref, noise_ref
from tests.gpu_helpers import problem, record_errors, rel_err

pytestmark = pytest.mark.gpu

# bf16 / MX-FP8 bars against the oracle that emulates the same operand roundings (what is left is
# summation order): ~3x the largest error observed on MI355X over these tests (CCREC_PARITY_LOG
# runs, tools/gpu_parity.sh).  fp32: the north_star's 1e-4.
# observed maxima (r03q, 49 tests): fp32 loss 7.2e-8 / grad 7.2e-7; bf16 6.5e-7 / 2.5e-3 (full mode's
# 1,500 identity rows into W1: 6.7e-3); MX-FP8 4.4e-8 / 2.0e-3
TOL = {'fp32': (3e-7, 3e-6), 'bf16': (2e-6, 8e-3), 'bf16_full': (2e-6, 2e-2),
       'mx8': (1.5e-7, 6e-3)}   # (loss, gradient) relative


def _errs(name, step, got, losses, grads, gflat, reg):
    e = {'loss/bce': abs(got['bce'] - losses['bce']) / losses['bce']}
    if reg > 0:
        e['loss/kl'] = abs(got['kl'] - losses['kl']) / losses['kl']
    e.update({k: rel_err(gflat[k], grads[k]) for k in grads if reg or not k.startswith('decoder_for_reg')})
    record_errors(name, step, e)
    return e


def _assert_within(e, tol, step):
    lt, gt = tol
    bad = {k: v for k, v in e.items() if not v < (lt if k.startswith('loss/') else gt)}
    assert not bad, (step, bad)


def _setup(V, d, B, C, reg, dtype, seed=3, sizes=(20, 40, 80), fused_tower=True, prefetch=True, **kw):
    lists, Mt, ns = problem(seed, C, V, sizes)
    P = model_ref.init_params(V, d, seed=seed, bias_std=0.01)
    lay = Layout(V, d)
    cfg = TrainConfig(V=V, d=d, batch_size=B, reg=reg, dtype=dtype, seed=seed, fused_tower=fused_tower,
                      prefetch_noise=prefetch, **kw)
    data = DeviceDataset(lists, V, y_mtx=Mt.astype(np.float32) if reg > 0 else None, neg_sampler=ns)
    tr = Trainer(cfg, data, params_flat=lay.pack(P))
    perm = np.random.default_rng(seed).permutation(C).astype(np.int32)
    tr.set_epoch_permutation(perm)
    return tr, lists, Mt, ns, P, perm


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('reg', [0.0, 0.1])
@pytest.mark.parametrize('V,d,B,fused', [(700, 64, 32, True), (2500, 128, 64, True), (2500, 256, 64, True),
                                         (700, 64, 32, False), (2500, 128, 48, True), (2500, 256, 128, True),
                                         (2504, 256, 128, True),
                                         (2500, 128, 128, True), (2500, 512, 128, True)])
def test_train_steps_match_oracle(dtype, reg, V, d, B, fused):
    C = 4 * B
    tr, lists, Mt, ns, P, perm = _setup(V, d, B, C, reg, dtype, fused_tower=fused)
    assert tr.fused_tower == (fused and B % 32 == 0 and (dtype == 'bf16' or d <= 256))
    if dtype == 'bf16' and B in (128, 256, 512) and d in (128, 256, 512):
        # the bench's path: fused D1 output kernel reading Wo, packed tower and D3 images
        assert tr.fused_out and tr.wpack is not None and tr.D3p is not None
    cdf = noise_ref.cdf_of(ns)
    Mo = {k: np.zeros_like(v) for k, v in P.items()}
    Vo = {k: np.zeros_like(v) for k, v in P.items()}
    mode = 'bf16' if dtype == 'bf16' else 'fp64'
    for step in range(3):
        tr.forward_backward()
        torch.cuda.synchronize()
        xs, ys, reg_idx = tr.batch_lists()
        cubes = [lists[c] for c in perm[step * B:(step + 1) * B]]
        oxs, oys, oreg, _ = noise_ref.philox_noise_batch(cubes, cdf, ns, tr.cfg.seed, step)
        for b in range(B):   # F is bit-exact
            assert np.array_equal(xs[b], oxs[b]) and np.array_equal(ys[b], oys[b])
        if reg > 0:
            assert np.array_equal(reg_idx, oreg)
        losses, grads = model_ref.train_forward_backward(
            P, oxs, oys, V, d, reg=reg, reg_idx=oreg, y_reg=Mt[oreg] if reg > 0 else None, mode=mode)
        e = _errs(f'train_{dtype}_{reg}_{V}_{d}_{B}_{fused}', step, tr.losses(), losses, grads,
                  tr.layout.unpack(tr.grads.cpu().numpy()), reg)
        _assert_within(e, TOL[dtype], step)
        tr.apply()
        # advance the oracle with the oracle's own gradients (TF Adam in fp32)
        G = {k: grads[k] for k in grads}
        P, Mo, Vo = model_ref.adam_tf(P, Mo, Vo, G, t=step + 1)
        torch.cuda.synchronize()
        # keep the two trajectories on identical weights (Adam sign-noise on ~0 grads otherwise
        # diverges the comparison, not the math): copy oracle params into the GPU trainer
        got_p = tr.layout.unpack(tr.params.cpu().numpy())
        for k in ('encoder/encoded_2/kernel', 'decoder/reconstruct/kernel'):
            assert rel_err(got_p[k], P[k]) < (1e-3 if dtype == 'fp32' else 5e-2)
        tr.params.copy_(torch.from_numpy(tr.layout.pack(P)))
        tr.m.copy_(torch.from_numpy(tr.layout.pack(Mo)))
        tr.v.copy_(torch.from_numpy(tr.layout.pack(Vo)))
        tr.refresh_shadow()


def test_adam_matches_tf_formula():
    import ctypes
    from cubecobrarecommender_amd import _lib as L
    rng = np.random.default_rng(0)
    n = 10007
    p = rng.standard_normal(n).astype(np.float32)
    g = rng.standard_normal(n).astype(np.float32)
    m = np.zeros(n, np.float32)
    v = np.zeros(n, np.float32)
    dp, dm, dv, dg = (torch.from_numpy(a.copy()).cuda() for a in (p, m, v, g))
    st = torch.tensor([4, 0, 0, 0], dtype=torch.int64, device='cuda')   # t = 5
    L.call('cc_adam_dense', L.ptr(dp), L.ptr(dm), L.ptr(dv), L.ptr(dg), None, n, L.ptr(st),
           1e-3, 0.9, 0.999, 1e-7, L.stream_ptr())
    torch.cuda.synchronize()
    P, Mo, Vo = model_ref.adam_tf({'a': p}, {'a': m}, {'a': v}, {'a': g}, t=5)
    assert np.max(np.abs(dp.cpu().numpy() - P['a'])) < 1e-6
    assert rel_err(dm.cpu().numpy(), Mo['a']) < 1e-6 and rel_err(dv.cpu().numpy(), Vo['a']) < 1e-6


@pytest.mark.parametrize('bpe', [0, 3])
def test_adam_fused_transposes_and_counters(bpe):
    """cc_adam_dense_t == cc_adam_dense + bf16 shadow + transposed copies of the regions
    (bit-exact), and the completion-ticket state advance."""
    rng = np.random.default_rng(7)
    shapes = [(64, 256), (256, 130), (128, 64), (256, 700)]     # partial 64-tiles included
    gap = 68
    offs, n = [], 100
    for r, c in shapes:
        offs.append(n)
        n += r * c + gap
    n = (n + 3) // 4 * 4
    p, m, g = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    v = rng.random(n).astype(np.float32)
    outs = []
    for fused in (False, True):
        dp, dm, dv, dg = (torch.from_numpy(a.copy()).cuda() for a in (p, m, v, g))
        sh = torch.zeros(n, dtype=torch.int16, device='cuda')
        st = torch.tensor([4, 2, 0, 0], dtype=torch.int64, device='cuda')
        dsts = [torch.zeros(c, r, dtype=torch.int16, device='cuda') for r, c in shapes]
        if fused:
            arr = (L.AdamTRegion * len(shapes))()
            for i, ((r, c), o) in enumerate(zip(shapes, offs)):
                arr[i].off, arr[i].rows, arr[i].cols, arr[i].dst = o, r, c, dsts[i].data_ptr()
            L.call('cc_adam_dense_t', L.ptr(dp), L.ptr(dm), L.ptr(dv), L.ptr(dg), L.ptr(sh), n,
                   L.ptr(st), 1e-3, 0.9, 0.999, 1e-7, arr, len(shapes), bpe, L.stream_ptr())
        else:
            L.call('cc_adam_dense', L.ptr(dp), L.ptr(dm), L.ptr(dv), L.ptr(dg), L.ptr(sh), n,
                   L.ptr(st), 1e-3, 0.9, 0.999, 1e-7, L.stream_ptr())
            for (r, c), o, dst in zip(shapes, offs, dsts):
                dst.copy_(sh[o:o + r * c].view(r, c).t())
            if bpe:
                L.call('cc_state_advance', L.ptr(st), bpe, L.stream_ptr())
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (dp, dm, dv, sh, st, *dsts)])
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    assert outs[1][4].tolist() == ([5, 0, 1, 0] if bpe else [4, 2, 0, 0])


def test_graph_replay_matches_eager_and_epochs_roll_over():
    V, d, B, C = 700, 64, 32, 128          # 4 batches per epoch
    # batch_lists() after step() must show that step's batch: no F prefetch here
    tr_e, lists, Mt, ns, P, _ = _setup(V, d, B, C, 0.1, 'bf16', prefetch=False)
    tr_g, *_ = _setup(V, d, B, C, 0.1, 'bf16', prefetch=False)
    rng = np.random.default_rng(1)
    perms = np.stack([rng.permutation(C) for _ in range(2)]).astype(np.int32)
    tr_e.set_epoch_permutations(perms)
    tr_g.set_epoch_permutations(perms)
    tr_g.capture()
    cdf = noise_ref.cdf_of(ns)
    for step in range(6):
        tr_e.step()
        tr_g.step()
        torch.cuda.synchronize()
        assert tr_e.losses() == tr_g.losses()
        xs, ys, _ = tr_g.batch_lists()
        ep, bi = divmod(step, 4)
        cubes = [lists[c] for c in perms[ep % 2][bi * B:(bi + 1) * B]]
        oxs, oys, _, _ = noise_ref.philox_noise_batch(cubes, cdf, ns, tr_g.cfg.seed, step)
        assert all(np.array_equal(a, b) for a, b in zip(xs[:B], oxs))
    assert torch.equal(tr_e.params, tr_g.params)
    tr_g.flush()            # the last step's counters run at the head of the next step
    assert tr_g.state.cpu().tolist()[:3] == [6, 2, 1]


@pytest.mark.parametrize('reg', [0.0, 0.1])
def test_noise_prefetch_is_exact(reg):
    """F drawn in the previous step's Adam launch (cc_adam_noise) == F at the head of the step:
    identical parameters and losses over epoch roll-overs, eager and as graph replays; and F drawn
    in the previous step's tower backward launch (f_in_tower, cc_tower_bwd_chain_noise)."""
    V, d, B, C = 700, 64, 32, 128          # 4 batches per epoch
    perms = np.stack([np.random.default_rng(s).permutation(C) for s in (1, 2)]).astype(np.int32)
    trs = []
    for prefetch, graphs, ft in ((False, False, False), (True, False, False), (True, True, False),
                                 (True, False, True), (True, True, True)):
        tr, *_ = _setup(V, d, B, C, reg, 'bf16', prefetch=prefetch, f_in_tower=ft)
        assert tr.prefetch == prefetch and tr.f_in_tower == ft
        tr.set_epoch_permutations(perms)
        if graphs:
            tr.capture()
        trs.append(tr)
    for step in range(7):
        for tr in trs:
            tr.step()
        torch.cuda.synchronize()
        assert all(tr.losses() == trs[0].losses() for tr in trs[1:])
    for tr in trs:
        tr.flush()
    for tr in trs[1:]:
        assert torch.equal(tr.params, trs[0].params)
        assert torch.equal(tr.state, trs[0].state)


@pytest.mark.parametrize('reg', [0.0, 0.1])
def test_data_parallel_equivalence(reg):
    """W ranks of batch B == one process of batch W*B: same cubes, same F draws (Philox slots),
    averaged gradients equal the single-process gradients (the all-reduce is the only exchange)."""
    V, d, B, C, W = 700, 64, 32, 256, 2
    lists, Mt, ns = problem(3, C, V, (20, 40, 80))
    P = model_ref.init_params(V, d, seed=3, bias_std=0.01)
    lay = Layout(V, d)
    perms = np.random.default_rng(4).permutation(C)[None, :]

    def make(b, rank, world):
        cfg = TrainConfig(V=V, d=d, batch_size=b, reg=reg, dtype='fp32', seed=3, rank=rank, world=world)
        data = DeviceDataset(lists, V, y_mtx=Mt.astype(np.float32) if reg else None, neg_sampler=ns)
        tr = Trainer(cfg, data, params_flat=lay.pack(P))
        tr.set_epoch_permutations(perms)
        return tr

    single = make(W * B, 0, 1)
    ranks = [make(B, r, W) for r in range(W)]
    for step in range(2):
        single.forward_backward()
        for t in ranks:
            t.forward_backward()
        torch.cuda.synchronize()
        xs, _, _ = single.batch_lists()
        got = [t.batch_lists()[0][:B] for t in ranks]
        assert all(np.array_equal(a, b) for a, b in zip(xs[:W * B], got[0] + got[1]))
        # ranks use the bucket-aligned layout (zero.py); compare in the standard layout
        avg = (ranks[0].standard(ranks[0].grads) + ranks[1].standard(ranks[1].grads)) / np.float32(W)
        n = lay.total if reg else lay.main_total
        assert rel_err(avg[:n], single.grads[:n].cpu().numpy()) < 1e-5
        lw = [t.losses()['loss'] for t in ranks]
        assert abs(np.mean(lw) - single.losses()['loss']) / single.losses()['loss'] < 1e-6
        for t in ranks:          # every rank applies the same averaged update
            t.load_standard(t.grads, avg)
            t.apply()
        single.apply()
        torch.cuda.synchronize()
        assert rel_err(ranks[0].standard(ranks[0].params), single.params.cpu().numpy()) < 1e-5


@pytest.mark.parametrize('reg', [0.0, 0.1])
@pytest.mark.parametrize('V,d,B', [(1500, 128, 128), (2500, 1024, 128)])
def test_fp8_decoder_steps_track_oracle(reg, V, d, B):
    """Config 5: MX-FP8 decoder output / regulariser GEMMs, everything else bf16.
    Against the MX-FP8-emulating oracle (model_ref mode='mx8': the same e4m3fn + E8M0 quantisation
    of the same bf16 operands along each product's K axis): F bit-exact, losses within 1e-3 and
    gradients within 3e-2 relative L2 (an operand that rounds one bf16 ulp differently can land in
    the neighbouring fp8 code, 2^-3 apart)."""
    C = 4 * B
    tr, lists, Mt, ns, P, perm = _setup(V, d, B, C, reg, 'fp8')
    assert tr.mx8 and tr.fused_tower and tr.d3q_in_tower == (d > 256)
    cdf = noise_ref.cdf_of(ns)
    for step in range(2):
        tr.forward_backward()
        torch.cuda.synchronize()
        if tr.d3q_in_tower:   # the wide tower forward's D3 MX-FP8 images == cc_quant_mx8 of D3, bit for bit
            R = tr.R
            q, qs = torch.empty_like(tr.D3q), torch.empty_like(tr.D3qs)
            qt, qts = torch.empty_like(tr.D3tq), torch.empty_like(tr.D3tqs)
            L.call('cc_quant_mx8', L.CC_BF16, L.ptr(tr.D3), R, d, d, 0, L.ptr(q), d, L.ptr(qs), None, L.stream_ptr())
            L.call('cc_quant_mx8', L.CC_BF16, L.ptr(tr.D3), R, d, d, 1, L.ptr(qt), R, L.ptr(qts), None, L.stream_ptr())
            torch.cuda.synchronize()
            assert torch.equal(q, tr.D3q) and torch.equal(qs, tr.D3qs)
            assert torch.equal(qt, tr.D3tq) and torch.equal(qts, tr.D3tqs)
        xs, ys, reg_idx = tr.batch_lists()
        cubes = [lists[c] for c in perm[step * B:(step + 1) * B]]
        oxs, oys, oreg, _ = noise_ref.philox_noise_batch(cubes, cdf, ns, tr.cfg.seed, step)
        for b in range(B):
            assert np.array_equal(xs[b], oxs[b]) and np.array_equal(ys[b], oys[b])
        losses, grads = model_ref.train_forward_backward(
            P, oxs, oys, V, d, reg=reg, reg_idx=oreg, y_reg=Mt[oreg] if reg > 0 else None, mode='mx8')
        e = _errs(f'fp8_{reg}_{V}_{d}_{B}', step, tr.losses(), losses, grads,
                  tr.layout.unpack(tr.grads.cpu().numpy()), reg)
        _assert_within(e, TOL['mx8'], step)
        tr.apply()
        torch.cuda.synchronize()
        P = tr.layout.unpack(tr.params.cpu().numpy())   # follow the GPU trajectory


@pytest.mark.parametrize('reg', [0.0, 0.1])
def test_wide_d1024_bf16_steps_match_oracle(reg):
    """d = 1024 (config 5's width) through the fused towers at bf16."""
    V, d, B = 2500, 1024, 64
    tr, lists, Mt, ns, P, perm = _setup(V, d, B, 4 * B, reg, 'bf16')
    assert tr.fused_tower
    cdf = noise_ref.cdf_of(ns)
    tr.forward_backward()
    torch.cuda.synchronize()
    cubes = [lists[c] for c in perm[:B]]
    oxs, oys, oreg, _ = noise_ref.philox_noise_batch(cubes, cdf, ns, tr.cfg.seed, 0)
    losses, grads = model_ref.train_forward_backward(
        P, oxs, oys, V, d, reg=reg, reg_idx=oreg, y_reg=Mt[oreg] if reg > 0 else None, mode='bf16')
    e = _errs(f'wide1024_{reg}', 0, tr.losses(), losses, grads, tr.layout.unpack(tr.grads.cpu().numpy()), reg)
    _assert_within(e, TOL['bf16'], 0)


def test_adam_pack_images_and_counters():
    """cc_adam_noise_pack (one-process step at the bench's shape class): after eager and graph
    steps, the packed tower images written by the Adam launch equal a fresh repack of the bf16
    shadow, and the counters advanced by the next E1 gather equal the step count."""
    tr = _setup(2500, 256, 128, 1024, 0.0, 'bf16')[0]
    assert tr.adam_packs and tr.fused_out
    for _ in range(3):
        tr.step()
    tr.capture()
    for _ in range(5):
        tr.step()
    torch.cuda.synchronize()
    got = tr.wpack.clone()
    tr.flush()
    st = tr.state.cpu().numpy()
    assert st[0] == 8 and st[1] == 8 % tr.batches_per_epoch and st[2] == 8 // tr.batches_per_epoch, st
    tr.transpose_tower()
    torch.cuda.synchronize()
    assert torch.equal(got, tr.wpack)


@pytest.mark.parametrize('reg', [0.0, 0.1])
def test_fused_w1_adam_matches_unfused(reg):
    """TrainConfig(fuse_w1_adam=True) — bench.py's step: TF Adam on W1 in the column-slice W1-gradient
    kernel's epilogue, the main Adam launch starting after W1 — gives bit-identical parameters,
    bf16 shadow, Adam moments and losses to the unfused step (same cc_adam::elem update, same
    gradient values), over eager steps and graph replays.  With wo_adam_in_tower as well: the
    output layers' trailing parts (Wo, and Wo_reg with the regulariser) updated in the tower
    backward launch (cc_tower_bwd_chain_adam, cc_adam::range_u) and the rest in two ranges of the
    Adam + F launch (cc_adam_noise_pack2) — the same bits again; and with f_in_tower, the next step's
    F drawn by the tower backward launch (cc_tower_bwd_chain_noise, two cubes per workgroup) and the
    Adam launch without it (cc_adam_pack2)."""
    out = {}
    for fuse, wo, ft in ((False, False, False), (True, False, False), (True, True, False), (True, True, True),
                         (True, False, True)):
        lists, Mt, ns = problem(11, 1024, 2500, (20, 40, 80))
        P = model_ref.init_params(2500, 256, seed=11, bias_std=0.01)
        lay = Layout(2500, 256)
        cfg = TrainConfig(V=2500, d=256, batch_size=256, reg=reg, dtype='bf16', seed=11, fuse_w1_adam=fuse,
                          wo_adam_in_tower=wo, f_in_tower=ft)
        tr = Trainer(cfg, DeviceDataset(lists, 2500, y_mtx=Mt.astype(np.float32) if reg > 0 else None,
                                        neg_sampler=ns), params_flat=lay.pack(P))
        tr.set_epoch_permutation(np.random.default_rng(11).permutation(1024).astype(np.int32))
        assert tr.fuse_w1 == fuse and tr.adam_packs and (tr.wo_range is not None) == wo and tr.f_in_tower == ft
        losses = []
        for _ in range(2):
            tr.step()
            losses.append(tr.losses())
        tr.capture()
        for _ in range(3):
            tr.step()
            losses.append(tr.losses())
        tr.flush()
        torch.cuda.synchronize()
        out[fuse, wo, ft] = (tr.params.cpu(), tr.m.cpu(), tr.v.cpu(), tr.shadow.cpu(), losses)
    base = out[False, False, False]
    for key in ((True, False, False), (True, True, False), (True, True, True), (True, False, True)):
        for a, b in zip(base[:4], out[key][:4]):
            assert torch.equal(a, b), key
        assert base[4] == out[key][4], key


@pytest.mark.parametrize('reg,ft', [(0.0, False), (0.1, False), (0.0, True), (0.1, True)])
def test_step_many_multi_graph_matches_single_steps(reg, ft):
    """step_many — graph_steps (here 4; remainders by the graphs of its halves) whole steps per captured graph replay, the loss
    accumulated inside the graph — gives bit-identical parameters, moments, shadow, device
    counters and accumulated losses to the same number of single step() calls (bench.py's
    configuration: fused W1 / Wo Adam placement)."""
    out = {}
    for multi in (False, True):
        lists, Mt, ns = problem(13, 1024, 2500, (20, 40, 80))
        P = model_ref.init_params(2500, 256, seed=13, bias_std=0.01)
        lay = Layout(2500, 256)
        cfg = TrainConfig(V=2500, d=256, batch_size=128, reg=reg, dtype='bf16', seed=13, fuse_w1_adam=True,
                          wo_adam_in_tower=True, f_in_tower=ft, graph_steps=4 if multi else 1)
        tr = Trainer(cfg, DeviceDataset(lists, 2500, y_mtx=Mt.astype(np.float32) if reg > 0 else None,
                                        neg_sampler=ns), params_flat=lay.pack(P))
        tr.set_epoch_permutation(np.random.default_rng(13).permutation(1024).astype(np.int32))
        acc = torch.zeros(2, dtype=torch.float64, device='cuda')
        tr.capture(loss_acc=acc)
        assert (tr.g_multi is not None) == multi
        tr.step_many(11, loss_acc=acc)   # 1 single (reaching the steady state) + 4 + 4 + 2 (the half graph)
        tr.flush()
        torch.cuda.synchronize()
        out[multi] = (tr.params.cpu(), tr.m.cpu(), tr.v.cpu(), tr.shadow.cpu(), tr.state.cpu(), acc.cpu())
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('dtype,V,d,B', [('fp32', 700, 64, 32), ('bf16', 1500, 256, 128), ('bf16', 1500, 512, 128),
                                         ('bf16', 5000, 256, 256)])
def test_full_mode_regulariser_matches_oracle(dtype, V, d, B):
    """reg_mode='full' (README.md:27: KL(M~, D2(E(I))) over ALL |V| identity rows every step):
    the rows are static (x row = {card}, reg_idx = card, padded rows masked), their W1 gradient is
    added row by row (cc_embed_identity_add), the KL is the mean over V rows — against the oracle
    with reg_idx = arange(V), y_reg = M~, for two steps with Adam between them.  bf16: dWo by the
    separate kl_dwo_kernel over the stored dZ (V = 1,500: 4-B staged rows; V = 5,000: 16-B)."""
    C = 4 * B
    lists, Mt, ns = problem(5, C, V, (20, 40, 80))
    P = model_ref.init_params(V, d, seed=5, bias_std=0.01)
    lay = Layout(V, d)
    cfg = TrainConfig(V=V, d=d, batch_size=B, reg=0.3, dtype=dtype, seed=5, reg_mode='full')
    tr = Trainer(cfg, DeviceDataset(lists, V, y_mtx=Mt.astype(np.float32), neg_sampler=ns), params_flat=lay.pack(P))
    assert tr.full_reg and tr.Breg >= V and tr.Breg % 32 == 0 and tr.R == B + tr.Breg
    perm = np.random.default_rng(5).permutation(C).astype(np.int32)
    tr.set_epoch_permutation(perm)
    tr.capture()
    cdf = noise_ref.cdf_of(ns)
    mode = 'fp64' if dtype == 'fp32' else 'bf16'
    for step in range(2):
        Pk = lay.unpack(tr.standard(tr.params))
        tr.step()
        torch.cuda.synchronize()
        cubes = [lists[c] for c in perm[step * B:(step + 1) * B]]
        oxs, oys, _, _ = noise_ref.philox_noise_batch(cubes, cdf, ns, 5, step, with_reg=False)
        losses, grads = model_ref.train_forward_backward(Pk, oxs, oys, V, d, reg=0.3, reg_idx=np.arange(V),
                                                         y_reg=Mt, mode=mode)
        e = _errs(f'full_{dtype}_{V}_{d}_{B}', step, tr.losses(), losses, grads,
                  lay.unpack(tr.standard(tr.grads)), 0.3)
        _assert_within(e, TOL['fp32' if dtype == 'fp32' else 'bf16_full'], step)
    tr.check_status()


@pytest.mark.parametrize('V,B,d', [(2500, 128, 256), (3001, 256, 256), (2500, 128, 512), (2504, 128, 256)])
def test_fused_regulariser_clip_fix_path(V, B, d):
    """The fused D2 kernels' exact-clip path (csrc/decreg.hip): a decoder_for_reg bias spread
    pushes part of every softmax row below 1e-7, so TF's clip gradient mask matters (S shrinks by
    the excluded target mass) — the main kernel flags it and the fix kernels correct dZ, dWo, dbo.
    Against the bf16-emulating oracle; a V not a multiple of the 96-column slices included; d = 512
    runs the 64-column slices."""
    tr, lists, Mt, ns, P, perm = _setup(V, d, B, 4 * B, 0.5, 'bf16')
    assert tr.fused_reg
    rng = np.random.default_rng(V)
    P['decoder_for_reg/reconstruct/bias'] = np.linspace(-40, 6, V)[rng.permutation(V)].astype(np.float32)
    tr.params.copy_(torch.from_numpy(tr.layout.pack(P)))
    tr.refresh_shadow()
    cdf = noise_ref.cdf_of(ns)
    tr.forward_backward()
    torch.cuda.synchronize()
    cubes = [lists[c] for c in perm[:B]]
    oxs, oys, oreg, _ = noise_ref.philox_noise_batch(cubes, cdf, ns, tr.cfg.seed, 0)
    losses, grads = model_ref.train_forward_backward(P, oxs, oys, V, d, reg=0.5, reg_idx=oreg, y_reg=Mt[oreg],
                                                     mode='bf16')
    e = _errs(f'clipfix_{V}_{B}', 0, tr.losses(), losses, grads, tr.layout.unpack(tr.grads.cpu().numpy()), 0.5)
    _assert_within({k: e[k] for k in ('loss/kl', 'decoder_for_reg/reconstruct/kernel',
                                      'decoder_for_reg/reconstruct/bias', 'decoder_for_reg/decoded_3/kernel',
                                      'encoder/encoded_1/kernel')}, TOL['bf16'], 0)


@pytest.mark.parametrize('V,spread', [(2500, True), (2502, True), (2504, True), (2504, False)])
def test_full_mode_clip_fix_path(V, spread):
    """Full mode (all |V| identity rows, several 512-row tiles per slice) with the exact-clip
    path live: the bias spread of the clip test above pushes part of every softmax row below
    1e-7.  Against the bf16-emulating oracle over reg_idx = arange(V) (spread off: no clip), then
    dWo's 96-column kernel (cc_dec_kl_args.flags = CC_KL_DWO_NARROW) against the default: at
    V % 8 == 0 the default is kl_dwo2_kernel (two row halves added), the 96-column kernel sums all
    rows in one pass — every other output identical, dWo equal to float rounding."""
    d, B = 256, 128

    def run(flags):
        tr, lists, Mt, ns, P, perm = _setup(V, d, B, 4 * B, 0.5, 'bf16', reg_mode='full')
        assert tr.full_reg and tr.fused_reg
        rng = np.random.default_rng(V)
        if spread:
            P['decoder_for_reg/reconstruct/bias'] = np.linspace(-40, 6, V)[rng.permutation(V)].astype(np.float32)
        tr.params.copy_(torch.from_numpy(tr.layout.pack(P)))
        tr.refresh_shadow()
        tr.kl_flags = flags
        tr.forward_backward()
        torch.cuda.synchronize()
        return tr, lists, Mt, ns, P, perm

    tr, lists, Mt, ns, P, perm = run(0)
    cdf = noise_ref.cdf_of(ns)
    cubes = [lists[c] for c in perm[:B]]
    oxs, oys, _, _ = noise_ref.philox_noise_batch(cubes, cdf, ns, tr.cfg.seed, 0, with_reg=False)
    losses, grads = model_ref.train_forward_backward(P, oxs, oys, V, d, reg=0.5, reg_idx=np.arange(V), y_reg=Mt,
                                                     mode='bf16')
    e = _errs(f'fullclip_{V}_{int(spread)}', 0, tr.losses(), losses, grads, tr.layout.unpack(tr.grads.cpu().numpy()), 0.5)
    # (the KL loss: most terms at the ln(1e-7) floor, a large total summed in fp32 lanes — 2.3e-6
    # relative at V = 2,500, the same with M~ in registers: checked bit for bit below)
    _assert_within({k: e[k] for k in ('decoder_for_reg/reconstruct/kernel', 'decoder_for_reg/reconstruct/bias',
                                      'decoder_for_reg/decoded_3/kernel', 'encoder/encoded_1/kernel')},
                   TOL['bf16_full'], 0)
    assert e['loss/kl'] < 5e-6, e['loss/kl']
    g1 = tr.layout.unpack(tr.grads.cpu().numpy())
    dwo = 'decoder_for_reg/reconstruct/kernel'
    for flags in (L.CC_KL_DWO_NARROW,):
        tr2 = run(flags)[0]
        g2 = tr.layout.unpack(tr2.grads.cpu().numpy())
        diff = {k: float(np.abs(g1[k] - g2[k]).max()) for k in g1 if not np.array_equal(g1[k], g2[k])}
        narrow = V % 8 == 0 and flags & L.CC_KL_DWO_NARROW
        if narrow and dwo in diff:   # one K order vs two row halves: float rounding only
            scale = float(np.abs(g1[dwo]).max())
            assert diff.pop(dwo) <= 2e-6 * scale, (flags, scale)
        assert torch.equal(tr2.dZout, tr.dZout) and not diff, (flags, diff)
        assert tr2.losses() == tr.losses(), (flags, tr2.losses(), tr.losses())


# Eigen's float logistic (TF 2.5's CPU sigmoid) is exactly 1 from this logit on (metrics.hip)
SIG_SAT = 15.7243833541870117


def keras_out1_pred_argmax(z):
    """argmax over the row of the fp32 sigmoid output, first index on ties (tf.argmax)."""
    p = torch.where(z >= SIG_SAT, torch.ones_like(z), torch.sigmoid(z))
    return torch.argmax(p, dim=1)


@pytest.mark.parametrize('dtype,reg,mode', [('bf16', 0.1, 'sampled'), ('fp32', 0.1, 'sampled'),
                                            ('bf16', 0.1, 'full'), ('bf16', 0.0, 'sampled')])
def test_accuracy_metrics_match_torch(dtype, reg, mode):
    """TrainConfig(metrics=True) — compile(metrics=['accuracy']) (train.py:87), resolved as TF 2.5
    does (categorical for both [B, |V|] outputs): output 1's argmax of the fp32 sigmoid (Eigen's
    saturation at 1.0, first index on ties) vs the first set target bit, output 2's argmax of the
    logits vs argmax of the M~ row — counted on the device == the same counts from torch fp32 logits
    of the step's own operands (D3, the bf16 / fp32 output-layer weights), over two steps."""
    V, d, B, C = 2500, 256, 128, 1024
    lists, Mt, ns = problem(21, C, V, (20, 40, 80))
    P = model_ref.init_params(V, d, seed=21, bias_std=0.01)
    # a spread of output-1 biases: some logits saturate the sigmoid (ties at 1.0: the first wins)
    P['decoder/reconstruct/bias'] = np.random.default_rng(5).uniform(-4, 17, V).astype(np.float32)
    lay = Layout(V, d)
    cfg = TrainConfig(V=V, d=d, batch_size=B, reg=reg, dtype=dtype, seed=21, metrics=True, reg_mode=mode)
    Mt32 = Mt.astype(np.float32)
    tr = Trainer(cfg, DeviceDataset(lists, V, y_mtx=Mt32 if reg > 0 else None, neg_sampler=ns),
                 params_flat=lay.pack(P))
    tr.set_epoch_permutation(np.random.default_rng(21).permutation(C).astype(np.int32))
    t_am = torch.from_numpy(np.argmax(Mt32, axis=1)).cuda()
    want = np.zeros(3)
    for _ in range(2):
        tr.forward_backward()
        torch.cuda.synchronize()
        flat = (tr.shadow if tr.shadow is not None else tr.params).float()
        D3 = tr.D3.float()

        def logits(pre, rows):
            o = lay.offset(pre + '/reconstruct/kernel')
            ob = lay.offset(pre + '/reconstruct/bias')
            return D3[rows] @ flat[o:o + d * V].view(d, V) + tr.params[ob:ob + V]
        z1 = logits('decoder', slice(0, B))
        yb = tr.y_bits[:B].to(torch.int64) & 0xFFFFFFFF
        y = ((yb.unsqueeze(-1) >> torch.arange(32, device='cuda')) & 1).reshape(B, -1)[:, :V]
        want[0] += float((keras_out1_pred_argmax(z1) == torch.argmax(y, dim=1)).sum())
        if reg > 0:
            idx = tr.reg_idx[:tr.Breg].long()
            live = idx >= 0
            z2 = logits('decoder_for_reg', slice(B, B + tr.Breg))[live]
            want[1] += float((torch.argmax(z2, dim=1) == t_am[idx[live]]).sum())
            want[2] += float(live.sum())
        tr.apply()
    torch.cuda.synchronize()
    got = tr.acc_counts.cpu().numpy().astype(np.float64)
    # top logits within a rounding of each other may order differently between cc_gemm's and
    # torch's summation orders (and the device's and torch's exp): a couple of rows at most
    assert 0 < want[0] < 2 * B and abs(got[0] - want[0]) <= 2, (got, want)
    assert got[2] == want[2] and abs(got[1] - want[1]) <= 2, (got, want)
    m = tr.take_metrics(2)
    assert abs(m['output_1_accuracy'] - got[0] / (2 * B)) < 1e-12 and tr.acc_counts.sum().item() == 0
    assert ('output_2_accuracy' in m) == (reg > 0)


def test_metric_counts_exact_after_capture():
    """capture()'s eager warm-up step must not leave its counts behind: after capture +
    step_many(n) the device has counted exactly n steps' rows (output 2's row count = n * B)."""
    V, d, B, C = 2500, 256, 128, 1024
    lists, Mt, ns = problem(22, C, V, (20, 40, 80))
    P = model_ref.init_params(V, d, seed=22, bias_std=0.01)
    cfg = TrainConfig(V=V, d=d, batch_size=B, reg=0.1, dtype='bf16', seed=22, metrics=True, graph_steps=4)
    tr = Trainer(cfg, DeviceDataset(lists, V, y_mtx=Mt.astype(np.float32), neg_sampler=ns),
                 params_flat=Layout(V, d).pack(P))
    tr.set_epoch_permutation(np.random.default_rng(22).permutation(C).astype(np.int32))
    tr.capture()
    assert tr.acc_counts.sum().item() == 0
    tr.step_many(6)
    torch.cuda.synchronize()
    c = tr.acc_counts.cpu().numpy()
    assert c[2] == 6 * B and 0 <= c[0] <= 6 * B and 0 <= c[1] <= c[2], c
    m = tr.take_metrics(6)
    assert 0.0 <= m['output_1_accuracy'] <= 1.0 and 0.0 <= m['output_2_accuracy'] <= 1.0


def test_capture_keeps_the_cycle_collector_out():
    """trainer._capture: dead cycles are collected before the capture begins and Python's cycle
    collector stays off until it ends (a collection inside a capture finalises GPU objects with
    HIP calls no capture allows); the collector's state is restored afterwards, also on an error."""
    import gc
    import weakref
    from cubecobrarecommender_amd.trainer import _capture

    class Node:
        pass

    a = Node()
    a.me = a                          # a dead cycle once `a` is gone
    dead = weakref.ref(a)
    del a
    x = torch.zeros(64, device='cuda')
    x += 1                            # (the add kernel's module loads outside any capture)
    x.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    assert gc.isenabled()
    with _capture(g):
        assert dead() is None and not gc.isenabled()
        x += 1
    assert gc.isenabled()
    g.replay()
    torch.cuda.synchronize()
    assert x.sum().item() == 64
    with pytest.raises(ZeroDivisionError):
        with _capture(torch.cuda.CUDAGraph()):
            x += 1
            1 / 0
    assert gc.isenabled()
    gc.disable()                      # a caller that runs with the collector off keeps it off
    try:
        with _capture(torch.cuda.CUDAGraph()):
            x += 1
        assert not gc.isenabled()
    finally:
        gc.enable()


def test_sigmoid_cat_accuracy_tie_rules():
    """cc_sigmoid_cat_accuracy's claimed tie rules (ccrec.h; parity against TF's Eigen sigmoid is
    unpinned below the saturation point): logits past 15.7243833541870117 saturate to
    1.0 so the FIRST saturated column is the argmax even when a later logit is larger; an all-zero
    target row maps to index 0."""
    V, Bt = 100, 4
    Z = np.full((Bt, V), -3.0, np.float32)
    Z[0, 10], Z[0, 40] = 16.0, 30.0        # both saturate: column 10 wins; target bit 10 -> correct
    Z[1, 10], Z[1, 40] = 15.0, 30.0        # only 40 saturates: argmax 40; target 10 -> wrong
    Z[2, 0], Z[2, 7] = 2.0, 1.0            # argmax 0; all-zero target row -> index 0 -> correct
    Z[3, 5], Z[3, 6] = 40.0, 40.0          # exact tie at 1.0: column 5; target bits {6, 5} -> first 5
    y = np.zeros((Bt, 128), np.uint8)
    y[0, 10] = y[1, 10] = 1
    y[3, 5] = y[3, 6] = 1
    yw = torch.from_numpy(np.packbits(y, axis=1, bitorder='little').view(np.int32)).cuda()
    cnt = torch.zeros(3, dtype=torch.int64, device='cuda')
    L.call('cc_sigmoid_cat_accuracy', L.ptr(torch.from_numpy(Z).cuda()), V, L.ptr(yw), Bt, V, L.ptr(cnt),
           L.stream_ptr())
    torch.cuda.synchronize()
    assert int(cnt[0]) == 3, cnt          # rows 0, 2, 3 correct; row 1 not


@pytest.mark.parametrize('d,dtype', [(256, 'bf16'), (512, 'bf16'), (1024, 'fp8')])
@pytest.mark.parametrize('fused', [True, False])
def test_reg_rows_by_index_bit_identical(d, dtype, fused):
    """The sampled regulariser's one-card rows by index in the W1 gradient (cc_embed_grad_cs_reg /
    _adam_reg: only the reg k-steps that touch a tile, from the rows' card list) == the same step with
    those rows as bits of a B + Breg-row bit matrix (TrainConfig(reg_by_index=False)): parameters,
    moments, gradients and losses bit for bit over eager steps and graph replays.  fused: W1's Adam in
    the gradient kernel with F prefetched (bench.py's configuration); else the gradient stored (F's
    direct xt atomics, which skip the reg rows)."""
    V, B, C = 2500, 128, 512
    lists, Mt, ns = problem(17, C, V, (20, 40, 80))
    P = model_ref.init_params(V, d, seed=17, bias_std=0.01)
    out = []
    for by_index in (True, False):
        cfg = TrainConfig(V=V, d=d, batch_size=B, reg=0.1, dtype=dtype, seed=17, reg_by_index=by_index,
                          fuse_w1_adam=fused, prefetch_noise=fused)
        tr = Trainer(cfg, DeviceDataset(lists, V, y_mtx=Mt.astype(np.float32), neg_sampler=ns),
                     params_flat=Layout(V, d).pack(P))
        assert tr.reg_by_index == by_index and tr.xt_rows == (B if by_index else 2 * B)
        assert tr.fuse_w1 == fused
        tr.set_epoch_permutation(np.random.default_rng(17).permutation(C).astype(np.int32))
        losses = []
        for _ in range(2):
            tr.step()
            tr.flush()
            torch.cuda.synchronize()
            losses.append(tr.losses())
        g = tr.grads.cpu().numpy().copy()
        tr.capture()
        for _ in range(3):
            tr.step()
        tr.flush()
        torch.cuda.synchronize()
        losses.append(tr.losses())
        tr.check_status()
        out.append((tr.params.cpu().numpy(), tr.m.cpu().numpy(), tr.v.cpu().numpy(), g, losses))
    (p1, m1, v1, g1, l1), (p0, m0, v0, g0, l0) = out
    assert l1 == l0, (l1, l0)
    np.testing.assert_array_equal(g1, g0)
    np.testing.assert_array_equal(p1, p0)
    np.testing.assert_array_equal(m1, m0)
    np.testing.assert_array_equal(v1, v0)


@pytest.mark.parametrize('V,B', [(2500, 128), (2504, 256), (700, 512)])
def test_tower_forward_writes_target_mask_image(V, B):
    """The tower forward launch's extra blocks write the fused D1 kernel's target-mask image
    (cc_tower_args.y_img): y_bits word-column major, every 32-row block's rows in accumulator-
    register order (dword 2r + h = row (r & 3) + 8 (r >> 2) + 4h) — checked against that transform
    of the step's own y_bits after a forward/backward."""
    tr, *_ = _setup(V, 256, B, 4 * B, 0.0, 'bf16')
    assert tr.y_img is not None
    tr.forward_backward()
    torch.cuda.synchronize()
    pos = torch.arange(32)
    row = 8 * (pos >> 3) + 4 * (pos & 1) + ((pos >> 1) & 3)
    want = tr.y_bits[(torch.arange(B // 32)[:, None] * 32 + row[None, :]).reshape(-1).cuda()].t().contiguous()
    assert torch.equal(tr.y_img.view((V + 31) // 32, B), want)


_HAS = {'has_wpack': 'wpack', 'has_D3p': 'D3p', 'has_gpre1p': 'gpre1p', 'has_w1_cs': 'eg_tickets',
        'has_WoP': 'WoP', 'has_y_img': 'y_img', 'has_x_bits': 'x_bits', 'has_Z2': 'Z2'}


@pytest.mark.parametrize('dtype,V,d,B,reg,kw', [
    ('bf16', 700, 128, 128, 0.1, {}),
    ('bf16', 2504, 256, 128, 0.0, dict(fuse_w1_adam=True, wo_adam_in_tower=True, f_in_tower=True)),
    ('fp32', 300, 64, 32, 0.1, {}),
    ('fp8', 700, 128, 128, 0.1, {}),
    ('bf16', 300, 128, 128, 0.1, dict(reg_mode='full'))])
def test_trainer_runs_the_planned_paths(dtype, V, d, B, reg, kw):
    """The trainer is what plan.plan_step decided (tests/test_step_plan.py pins the plan itself on
    the CPU): after construction and one step, every plan flag equals the attribute of the same name
    and every has_* flag says whether its buffer exists."""
    import dataclasses
    tr, *_ = _setup(V, d, B, 4 * B, reg, dtype, **kw)
    tr.step()
    torch.cuda.synchronize()
    tr.check_status()
    assert np.isfinite(tr.losses()['loss'])
    plain = lambda x: [plain(v) for v in x] if isinstance(x, (list, tuple)) else x   # noqa: E731
    for f in dataclasses.fields(tr.plan):
        want = getattr(tr.plan, f.name)
        if f.name in _HAS:
            assert (getattr(tr, _HAS[f.name]) is not None) == want, f.name
        elif f.name in ('dp_defer_out_ok', 'bucket_hook_names', 'f_bucket_name'):
            assert getattr(tr, f.name)() == want, f.name
        elif f.name in ('layout', 'std_layout'):
            assert getattr(tr, f.name) is want, f.name
        elif f.name not in ('tower_dw', 'dx_kernels'):   # (read from the plan at their launches)
            assert plain(getattr(tr, f.name)) == plain(want), f.name
