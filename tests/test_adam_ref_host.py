"""CPU: tests/adam_ref.py (the fp64 reference, bounds, fp32 emulation, layouts and regimes behind
tests/test_gpu_adam_elem.py) held to two independent statements of the update, to its own bounds with
a right fp32 kernel simulated in numpy, and to nine single-fault mutations of that kernel, each of which
must fail the check on a named regime."""
import numpy as np
import pytest
import torch

from oracle import model_ref
from tests import adam_ref as AR
from tests import tower_ref as TR

f32 = np.float32
N = 10007
HPS = (AR.HP_DEFAULT, AR.HP_SECOND)


def _ref(regime, step, hp=AR.HP_DEFAULT, n=N):
    inp = AR.inputs(regime, n)
    return inp, AR.reference(inp.p, inp.m, inp.v, inp.g, step, hp)


def test_regimes_are_what_they_claim():
    for r in AR.REGIMES:
        inp = AR.inputs(r, N)
        assert all(np.all(np.isfinite(x)) for x in (inp.p, inp.m, inp.v, inp.g)) and np.all(inp.v >= 0)
        assert len(inp.probes) == 4 and np.all(inp.m[inp.probes] == 1) and np.all(inp.p[inp.probes] == 0)
        assert AR.same_bits(inp.p, AR.inputs(r, N).p)                       # seeded
    a = AR.inputs('absent', N)
    gone = a.g == 0
    tiny = np.finfo(f32).tiny
    assert 0.85 < gone.mean() < 0.95
    assert np.any((np.abs(a.m[gone]) < tiny) & (a.m[gone] != 0)) and np.any((a.v[gone] < tiny) & (a.v[gone] != 0))
    assert np.any(np.signbit(a.m[gone]) & (a.m[gone] == 0)) and np.any(~np.signbit(a.m[gone]) & (a.m[gone] == 0))
    assert np.any(np.signbit(a.v[gone]) & (a.v[gone] == 0)) and np.any(~np.signbit(a.v[gone]) & (a.v[gone] == 0))
    e = AR.inputs('eps_band', N)
    s = np.sqrt(e.v.astype(np.float64))
    assert np.mean(s < 1e-7) > 0.2 and np.mean(s > 1e-7) > 0.2
    w = AR.inputs('wide', N)
    assert np.abs(w.g).max() > 1e14 and np.abs(w.g).min() < 1e-19 and np.all(np.isfinite(w.g * w.g))
    t = AR.inputs('ties', N, probes=False)
    u = t.p.view(np.uint32)
    assert np.all(((u & 0xFFFF) == 0x8000) | (t.p == 0)) and np.sum(t.p == 0) == 2       # +0.0 and -0.0
    hi = u >> 16
    assert np.any(hi & 1) and np.any(~hi & 1 == 1) and np.any(u == 0x80000000) and np.any(np.signbit(t.p))
    assert np.any((np.abs(t.p) < tiny) & (t.p != 0))
    up = AR.bf16_rne(t.p).astype(np.uint32) - hi          # a tie goes to the even neighbour
    assert np.array_equal(up, hi & 1)


@pytest.mark.parametrize('hp', HPS, ids=['default', 'second'])
def test_reference_matches_model_ref_adam_tf(hp):
    """oracle/model_ref.adam_tf (float32 numpy) lies inside every bound, every regime and step."""
    worst = {}
    for regime in AR.REGIMES:
        for step in AR.STEPS:
            inp, ref = _ref(regime, step, hp)
            with np.errstate(under='ignore'):
                P, M, V = model_ref.adam_tf({'a': inp.p.copy()}, {'a': inp.m.copy()}, {'a': inp.v.copy()}, {'a': inp.g},
                                            t=step + 1, lr=hp[0], beta1=hp[1], beta2=hp[2], eps=hp[3])
            r = AR.ratios(ref, P['a'], M['a'], V['a'])
            assert AR.passes(r), (regime, step, r)
            worst = {k: max(v, worst.get(k, 0)) for k, v in r.items()}
    print('model_ref.adam_tf error / bound', worst)


@pytest.mark.parametrize('hp', HPS, ids=['default', 'second'])
def test_reference_matches_torch_adam_float64(hp):
    """torch.optim.Adam in float64.  torch divides by sqrt(v) / sqrt(1 - b2^t) + eps_torch; with
    eps_torch = eps / sqrt(1 - b2^t) that is TF's m alpha / (sqrt(v) + eps) exactly, so p, m and v
    are all compared (1e-12 relative: two fp64 evaluation orders)."""
    lr, b1, b2, eps = AR.hp64(hp)
    for regime in AR.REGIMES:
        for step in AR.STEPS:
            inp, ref = _ref(regime, step, hp, n=1027)
            t = float(step) + 1.0
            with np.errstate(under='ignore'):
                eps_t = eps / np.sqrt(1.0 - np.power(b2, t))
            p = torch.tensor(inp.p.astype(np.float64), requires_grad=True)
            opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=float(eps_t))
            opt.state[p] = {'step': torch.tensor(float(step)), 'exp_avg': torch.tensor(inp.m.astype(np.float64)),
                            'exp_avg_sq': torch.tensor(inp.v.astype(np.float64))}
            p.grad = torch.tensor(inp.g.astype(np.float64))
            opt.step()
            st = opt.state[p]
            for name, got, want in (('p', p.detach(), ref.p), ('m', st['exp_avg'], ref.m), ('v', st['exp_avg_sq'], ref.v)):
                got = got.numpy()
                scale = np.abs(want) + (np.abs(inp.p.astype(np.float64)) if name == 'p' else 0)
                assert np.all(np.abs(got - want) <= 1e-12 * scale + 1e-300), (regime, step, name)


def test_right_kernel_inside_every_bound():
    """emulate() with numpy's fp32 alpha: inside every bound at every element, every regime, step and
    both hyperparameter sets; alpha inside its own bound.  Prints the largest error / bound."""
    worst, worst_a = {}, 0.0
    for hp in HPS:
        for step in AR.STEPS:
            a = AR.alpha32(step, hp)
            alpha, ra = AR.alpha_ref(step, hp)
            worst_a = max(worst_a, abs(float(a) - alpha) / alpha / ra)
            for regime in AR.REGIMES:
                for n in (1, 5, 1027, N):
                    inp, ref = _ref(regime, step, hp, n)
                    r = AR.ratios(ref, *AR.emulate(inp.p, inp.m, inp.v, inp.g, a, hp))
                    assert AR.passes(r), (regime, step, n, r)
                    worst = {k: max(v, worst.get(k, 0)) for k, v in r.items()}
    print('emulate error / bound', worst, 'alpha', worst_a)
    assert worst_a <= 1 and min(worst.values()) > 0.3          # the bounds are the roundings' own size
    assert float(AR.alpha32(2 ** 31, AR.HP_DEFAULT)) == float(f32(1e-3))    # b^t = 0: alpha is lr


def test_alpha_candidates_contain_alpha():
    for hp in HPS:
        for step in AR.STEPS:
            a = AR.alpha32(step, hp)
            inp = AR.probe_inputs(4)
            p1, m1, v1 = AR.emulate(inp.p, inp.m, inp.v, inp.g, a, hp)
            assert np.all(m1 == 1) and np.all(v1 == 1) and len(set(p1.tolist())) == 1
            c = AR.alpha_candidates(p1[0], hp)
            assert 1 <= len(c) <= 3 and a in c


# ---- single-fault mutations of the kernel: (name, regime it must fail on, step, the mutated update)
def _mutant(fault, inp, step, hp):
    lr, b1, b2, eps = (f32(x) for x in hp)
    p, m, v, g = inp.p, inp.m, inp.v, inp.g
    alpha = AR.alpha32(step, hp)
    omb1, omb2 = f32(1) - b1, f32(1) - b2
    if fault == 'no_bias_correction':
        alpha = lr
    elif fault == 't_is_step':
        alpha = AR.alpha32(step - 1, hp)
    elif fault == 'b1_b2_exchanged':
        alpha = AR.alpha32(step, (hp[0], hp[2], hp[1], hp[3]))
        omb1, omb2 = omb2, omb1
    with np.errstate(under='ignore', invalid='ignore', divide='ignore'):
        m1 = m + (g - m) * omb1
        v1 = v + ((g if fault == 'v_from_g' else g * g) - v) * omb2
        den = np.sqrt(v1 + eps) if fault == 'eps_inside_sqrt' else np.sqrt(v1) + eps
        p1 = p - ((m if fault == 'p_from_old_m' else m1) * alpha) / den
    if fault == 'tail_untouched':
        k = len(p) // 4 * 4
        p1[k:], m1[k:], v1[k:] = p[k:], m[k:], v[k:]
    sh = AR.bf16_rne(p if fault == 'shadow_from_old_p' else p1)
    if fault == 'shadow_truncated':
        sh = (p1.view(np.uint32) >> 16).astype(np.uint16)
    return p1, m1, v1, sh


MUTATIONS = [('eps_inside_sqrt', 'eps_band', 4), ('no_bias_correction', 'fresh', 4), ('t_is_step', 'trained', 4),
             ('b1_b2_exchanged', 'trained', 4), ('v_from_g', 'trained', 4), ('p_from_old_m', 'trained', 4),
             ('tail_untouched', 'trained', 4), ('shadow_truncated', 'ties', 4), ('shadow_from_old_p', 'trained', 4)]


def _check(inp, ref, p1, m1, v1, sh):
    return AR.passes(AR.ratios(ref, p1, m1, v1)) and np.array_equal(sh, AR.bf16_rne(p1))


def test_unmutated_kernel_passes_the_mutation_check():
    for _, regime, step in MUTATIONS:
        inp, ref = _ref(regime, step)
        assert _check(inp, ref, *_mutant(None, inp, step, AR.HP_DEFAULT))


@pytest.mark.parametrize('fault,regime,step', MUTATIONS, ids=[f'{m[0]}-fails_on-{m[1]}' for m in MUTATIONS])
def test_mutation_fails(fault, regime, step):
    inp, ref = _ref(regime, step)
    assert N % 4 == 3
    assert not _check(inp, ref, *_mutant(fault, inp, step, AR.HP_DEFAULT)), f'{fault} passes on {regime}'


# ---- layouts
@pytest.mark.parametrize('K,N_', [(32, 32), (64, 32), (32, 96), (160, 64)])
def test_images_self_inverse_and_match_tower_ref(K, N_):
    W = np.arange(K * N_, dtype=np.uint16).reshape(K, N_)
    f, b = AR.image_fwd(W), AR.image_bwd(W)
    assert sorted(f.tolist()) == list(range(K * N_)) and sorted(b.tolist()) == list(range(K * N_))
    assert np.array_equal(AR.unimage_fwd(f, K, N_), W) and np.array_equal(AR.unimage_bwd(b, K, N_), W)
    assert np.array_equal(f, TR.pack_t(W)) and np.array_equal(b, TR.pack_t(np.ascontiguousarray(W.T)))
    assert not np.array_equal(f, b)


@pytest.mark.parametrize('rows,cols', [(1, 4), (2, 130), (36, 2), (64, 64), (65, 68), (256, 130)])
def test_transposed_region_self_inverse(rows, cols):
    flat = np.arange(7 + rows * cols + 5, dtype=np.uint16)
    dst = AR.transposed_region(flat, 7, rows, cols)
    assert dst.shape == (cols, rows) and dst[cols - 1, 0] == 7 + cols - 1
    assert np.array_equal(AR.untransposed_region(dst, rows, cols), flat[7:7 + rows * cols])
    assert np.array_equal(dst, TR.transpose_ld(flat[7:7 + rows * cols].reshape(rows, cols)))


def test_bf16_rne_matches_tower_ref_bits():
    x = np.concatenate([AR.inputs(r, 1027).p for r in AR.REGIMES])
    assert np.array_equal(AR.bf16_rne(x), TR.bits(x))
    assert AR.bf16_rne(np.array([1.0, -0.0], f32)).tolist() == [0x3F80, 0x8000]
