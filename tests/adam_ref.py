"""fp64 reference, derived per-element bounds, fp32 emulation, layouts and input regimes for the TF
Adam update of csrc/adam.hpp (cc_adam::elem and the constants of range() / range_u()).  Pure numpy;
tests/test_adam_ref_host.py holds it to oracle/model_ref.adam_tf, to torch.optim.Adam in float64 and
to nine single-fault mutations; tests/test_gpu_adam_elem.py holds the kernels to it.

The update, as adam.hpp states it (t = state[0] + 1; lr, b1, b2, eps the fp32 values the kernel
receives, widened to fp64):
  alpha = lr sqrt(1 - b2^t) / (1 - b1^t)
  m' = m + (g - m)(1 - b1);   v' = v + (g g - v)(1 - b2);   p' = p - m' alpha / (sqrt(v') + eps)
1 - b1 and 1 - b2 are exact in fp32 for 0.5 <= b <= 1 (Sterbenz), so the reference uses the exact
differences of the fp32 values.

Bounds (u = 2^-24, eta = 2^-150: half the smallest fp32 denormal, added once per rounding so that a
denormal result is covered; hats are the kernel's fp32 values).  elem() has contraction off and no FMA,
so every operation rounds once, in the order written:
  m'   d = g - m, e = d (1 - b1), m' = m + e: three roundings.
       |m^' - m'| <= bm = (2 u |e| + u |m'| + 3 eta)(1 + 4u)
       (d's error passes through the product, which adds its own: 2 u |e|; the sum's: u |m'|)
  v'   q = g g, d = q - v, e = d (1 - b2), v' = v + e: FOUR roundings (the issue text counts three;
       the square is a rounding of its own, its error reaches v' scaled by 1 - b2).
       |v^' - v'| <= bv = (u (1 - b2) q + 2 u |e| + u |v'| + 4 eta)(1 + 4u)
  p'   N = m' alpha, s = sqrt(v'), D = s + eps, Q = N / D, p' = p - Q: five roundings on top of
       the propagated errors of m', v' and alpha (ra = the relative bound on alpha below):
       eN = (alpha bm + |N| (ra + u))(1 + 4u) + eta
       es = min(sqrt(bv), bv / sqrt(v')) + u sqrt(v') (1 + 4u) + eta     (|sqrt a - sqrt b| <= both)
       eD = es + u D (1 + 4u) + eta
       A  = (eN + |Q| eD) / (D - eD);   eQ = A + u (|Q| + A) + eta       (D >= eps > eD always: asserted)
       |p^' - p'| <= bp = eQ + u (|p'| + eQ) + eta
  every bound is multiplied by 1 + 2^-20 for the fp64 reference's own rounding.
  alpha  rel(alpha) <= ra = K u (b2^t / (2 (1 - b2^t)) + b1^t / (1 - b1^t)) + 4u  [+ the rounding of t
       to fp32 past 2^24: |fl(t) - t| |ln b| times the same two amplification factors]
       K = 16: the OpenCL conformance limit of powf, which the device maths library is built to; not a
       measurement.  The first term is powf's error amplified by the cancellation in 1 - b^t (at
       t = 1, b2 = 0.999: one ulp of b2^t moves alpha by 324 ulp).  4u covers the roundings of
       1 - b2^t (halved by the square root), sqrt, the product with lr, 1 - b1^t and the divide; the
       strict worst case of those five is 4.5u (1 - b^t is exact for b^t >= 0.5 and within u / 2
       absolute below), the formula is kept as the issue states it.
The bounds are derived; nothing here was fitted to what a device returns.

emulate() is the same update in numpy float32, operation for operation.  The HIP build is -O3 with no
fast-math, fp32 denormals on (the code object's metadata), so / and sqrtf are correctly
rounded and * + - are IEEE: given the device's alpha, the device's m', v', p' equal emulate()'s bits.
"""
import functools
from collections import namedtuple

import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -150
K_POWF = 16
REF_SLACK = 1.0 + 2.0 ** -20

HP_DEFAULT = (1e-3, 0.9, 0.999, 1e-7)
HP_SECOND = (3e-4, 0.8, 0.99, 1e-8)
STEPS = (0, 1, 4, 99, 999, 6930, 10 ** 5, 2 ** 24 - 1, 2 ** 31)
REGIMES = ('fresh', 'trained', 'absent', 'eps_band', 'wide', 'ties')
FUSED_REGIMES = ('trained', 'absent', 'eps_band', 'ties')
FUSED_STEPS = (0, 4, 6930)

f32 = np.float32


def hp64(hp):
    """The hyperparameters as the kernel receives them (fp32), widened to fp64."""
    return tuple(float(f32(x)) for x in hp)


# ------------------------------------------------------------------ alpha
def alpha_ref(step, hp):
    """(alpha, relative bound ra) in fp64; t = step + 1."""
    lr, b1, b2, _ = hp64(hp)
    t = float(step) + 1.0                       # exact in fp64 for every step used (< 2^53)
    dt = abs(float(f32(t)) - t)                 # the kernel's (float)(step + 1)
    with np.errstate(under='ignore'):
        b1p, b2p = np.power(b1, t), np.power(b2, t)
    alpha = lr * np.sqrt(1.0 - b2p) / (1.0 - b1p)
    amp = b2p / (2.0 * (1.0 - b2p)) + b1p / (1.0 - b1p)
    amp_t = b2p / (2.0 * (1.0 - b2p)) * abs(np.log(b2)) + b1p / (1.0 - b1p) * abs(np.log(b1))
    return float(alpha), float(K_POWF * U * amp + 4.0 * U + dt * amp_t)


def alpha32(step, hp):
    """alpha as range() computes it, in numpy float32 (numpy's powf, not the device's)."""
    lr, b1, b2, _ = (f32(x) for x in hp)
    t = f32(step + 1)
    with np.errstate(under='ignore'):
        b1p, b2p = np.power(b1, t, dtype=f32), np.power(b2, t, dtype=f32)
    return f32(lr * np.sqrt(f32(1) - b2p) / (f32(1) - b1p))


def alpha_candidates(probe_p, hp):
    """The fp32 values a with fl(a / fl(1 + eps)) == -probe_p (a probe's p': p = 0, m = g = v = 1)."""
    r = f32(-probe_p)
    D = f32(f32(1) + f32(hp[3]))
    a = f32(r * D)
    lo = a
    for _ in range(3):
        lo = np.nextafter(lo, f32(-np.inf), dtype=f32)
    out, c = [], lo
    for _ in range(7):
        if f32(c / D) == r:
            out.append(f32(c))
        c = np.nextafter(c, f32(np.inf), dtype=f32)
    assert len(out) <= 3
    return out


# ------------------------------------------------------------------ the reference and its bounds
Ref = namedtuple('Ref', 'p m v alpha ra bp bm bv')


def reference(p, m, v, g, step, hp):
    """p', m', v', alpha in fp64 and the per-element bounds bp, bm, bv (module docstring)."""
    _, b1, b2, eps = hp64(hp)
    alpha, ra = alpha_ref(step, hp)
    p, m, v, g = (np.asarray(x, np.float64) for x in (p, m, v, g))
    assert np.all(v >= 0) and all(np.all(np.isfinite(x)) for x in (p, m, v, g))
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    em = (g - m) * omb1
    m1 = m + em
    q = g * g
    ev = (q - v) * omb2
    v1 = v + ev
    s = np.sqrt(v1)
    D = s + eps
    N = m1 * alpha
    Q = N / D
    p1 = p - Q
    k = 1.0 + 4.0 * U
    bm = (2 * U * np.abs(em) + U * np.abs(m1) + 3 * ETA) * k
    bv = (U * omb2 * q + 2 * U * np.abs(ev) + U * np.abs(v1) + 4 * ETA) * k
    eN = (alpha * bm + np.abs(N) * (ra + U)) * k + ETA
    with np.errstate(divide='ignore', invalid='ignore'):
        es = np.where(s > 0, np.minimum(np.sqrt(bv), bv / s), np.sqrt(bv)) + U * s * k + ETA
    eD = es + U * D * k + ETA
    assert np.all(eD < D)
    A = (eN + np.abs(Q) * eD) / (D - eD)
    eQ = A + U * (np.abs(Q) + A) + ETA
    bp = eQ + U * (np.abs(p1) + eQ) + ETA
    return Ref(p1, m1, v1, alpha, ra, bp * REF_SLACK, bm * REF_SLACK, bv * REF_SLACK)


def ratios(ref, p, m, v):
    """Largest error / bound of p', m', v' over every element (nothing is left out; NaN counts as inf)."""
    out = {}
    for k, got, want, b in (('p', p, ref.p, ref.bp), ('m', m, ref.m, ref.bm), ('v', v, ref.v, ref.bv)):
        r = np.abs(np.asarray(got, np.float64) - want) / b
        out[k] = float(np.max(np.where(np.isnan(r), np.inf, r))) if r.size else 0.0
    return out


def passes(r):
    return all(x <= 1.0 for x in r.values())


# ------------------------------------------------------------------ fp32, operation for operation
def emulate(p, m, v, g, alpha, hp):
    """elem() in numpy float32 given alpha (fp32): (p', m', v')."""
    _, b1, b2, eps = (f32(x) for x in hp)
    p, m, v, g = (np.asarray(x, f32) for x in (p, m, v, g))
    omb1, omb2 = f32(1) - b1, f32(1) - b2
    with np.errstate(under='ignore', over='ignore'):
        m1 = m + (g - m) * omb1
        v1 = v + (g * g - v) * omb2
        p1 = p - (m1 * f32(alpha)) / (np.sqrt(v1) + eps)
    assert p1.dtype == f32 and m1.dtype == f32 and v1.dtype == f32
    return p1, m1, v1


def bf16_rne(x):
    """fp32 -> bf16 bit patterns (uint16), round to nearest even as common.hpp's f2bf does it."""
    u = np.ascontiguousarray(x, dtype=f32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------ layouts
def frag_index(rows, red):
    """The packed tower image of a [rows][red] operand (rows: output features, red: the reduction),
    as adam.hpp's frag_off describes it: 32-row tiles t, 16-deep reduction steps j, and inside a
    fragment lane = (row & 31) + 32 ((r >> 3) & 1) holding 8 consecutive reduction elements:
    flat offset (((t (red / 16) + j) 64 + lane) 8 + (r & 7).  Returns [rows][red] offsets."""
    n, r = np.meshgrid(np.arange(rows), np.arange(red), indexing='ij')
    lane = (n & 31) + 32 * ((r >> 3) & 1)
    return (((n >> 5) * (red // 16) + (r >> 4)) * 64 + lane) * 8 + (r & 7)


def image_fwd(W):
    """Forward image of a layer W [K][N] (row-major in the flat buffer): rows n, reduction k."""
    K, N = W.shape
    out = np.empty(K * N, W.dtype)
    out[frag_index(N, K).reshape(-1)] = W.T.reshape(-1)
    return out


def image_bwd(W):
    """Backward image of W [K][N]: rows k, reduction n."""
    K, N = W.shape
    out = np.empty(K * N, W.dtype)
    out[frag_index(K, N).reshape(-1)] = W.reshape(-1)
    return out


def unimage_fwd(img, K, N):
    return np.ascontiguousarray(img[frag_index(N, K)].T)


def unimage_bwd(img, K, N):
    return np.ascontiguousarray(img[frag_index(K, N)])


def transposed_region(flat, off, rows, cols):
    """cc_adam_dense_t's copy of region [rows][cols] at `off`: dst [cols][rows]."""
    return np.ascontiguousarray(flat[off:off + rows * cols].reshape(rows, cols).T)


def untransposed_region(dst, rows, cols):
    return np.ascontiguousarray(dst.reshape(cols, rows).T).reshape(-1)


# ------------------------------------------------------------------ input regimes
Inputs = namedtuple('Inputs', 'regime n p m v g probes')
_SEEDS = {r: 101 + i for i, r in enumerate(REGIMES)}


def probe_positions(n):
    """Fixed positions of the alpha probes inside a range of n elements (none below n = 16: there a
    call on n probe elements alone reads alpha)."""
    return np.array([0, n // 3, (2 * n) // 3, n - 1]) if n >= 16 else np.zeros(0, np.int64)


def _logu(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _sign(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0)


def _trained(rng, n):
    return (0.05 * rng.standard_normal(n), 1e-3 * rng.standard_normal(n), 1e-5 * rng.random(n),
            1e-3 * rng.standard_normal(n))


def _ties_p(rng, n):
    """fp32 values exactly halfway between neighbouring bf16 values: low half 0x8000; the high half
    (even: the tie rounds down in magnitude, odd: up) random with the exponent field in [0, 0xF0]:
    denormals included, no inf / NaN; -0.0 and +0.0 themselves and both neighbours' parities placed."""
    hi = (rng.integers(0, 2, n).astype(np.uint32) << 15) | (rng.integers(0, 0xF1, n).astype(np.uint32) << 7) \
        | rng.integers(0, 128, n).astype(np.uint32)
    u = (hi << 16) | np.uint32(0x8000)
    fixed = np.array([0x80000000, 0x00000000, 0x00008000, 0x00018000, 0x80008000, 0x80018000, 0x3F808000,
                      0x3F818000, 0xBF808000, 0xBF818000], np.uint32)       # -0, +0, denormal ties, +-1.00x ties
    first = 1 if n >= 16 else 0                  # element 0 is an alpha probe from n = 16 on
    k = min(n - first, len(fixed))
    u[first:first + k] = fixed[:k]
    return u.view(f32)


@functools.lru_cache(maxsize=64)
def inputs(regime, n, probes=True):
    """Seeded fp32 inputs of a regime at n elements; alpha probes (p = 0, m = g = v = 1) at
    probe_positions(n) unless probes is False."""
    rng = np.random.default_rng(1000 * _SEEDS[regime] + n % 1000 + n // 1000)
    if regime == 'fresh':
        p, g = rng.standard_normal(n), rng.standard_normal(n)
        m, v = np.zeros(n), np.zeros(n)
    elif regime == 'trained':
        p, m, v, g = _trained(rng, n)
    elif regime == 'absent':
        p, m, v, g = _trained(rng, n)
        gone = rng.random(n) < 0.9
        m = np.where(gone, _sign(rng, n) * _logu(rng, 1e-44, 1e-3, n), m)
        v = np.where(gone, _logu(rng, 1e-44, 1e-5, n), v)
        z = gone & (rng.random(n) < 0.1)                 # exact zeros of either sign
        m = np.where(z, np.where(rng.random(n) < 0.5, -0.0, 0.0), m)
        z = gone & (rng.random(n) < 0.1)
        v = np.where(z, np.where(rng.random(n) < 0.5, -0.0, 0.0), v)
        g = np.where(gone, 0.0, g)
    elif regime == 'eps_band':
        p = 0.05 * rng.standard_normal(n)
        v = _logu(rng, 1e-22, 1e-10, n)
        m = 1e-8 * rng.standard_normal(n)
        g = np.sqrt(v) * rng.standard_normal(n)
    elif regime == 'wide':
        p, m, v, _ = _trained(rng, n)
        g = _sign(rng, n) * _logu(rng, 1e-20, 1e15, n)
    elif regime == 'ties':
        p = _ties_p(rng, n)
        m, g, v = np.zeros(n), np.zeros(n), np.ones(n)
    else:
        raise ValueError(regime)
    p, m, v, g = (np.ascontiguousarray(x, dtype=f32) for x in (p, m, v, g))
    pos = probe_positions(n) if probes else np.zeros(0, np.int64)
    p[pos], m[pos], v[pos], g[pos] = 0.0, 1.0, 1.0, 1.0
    for x in (p, m, v, g):
        x.setflags(write=False)
    return Inputs(regime, n, p, m, v, g, pos)


def probe_inputs(n):
    """n probe elements and nothing else."""
    one, zero = np.ones(n, f32), np.zeros(n, f32)
    return Inputs('probes', n, zero, one, one.copy(), one.copy(), np.arange(n))
