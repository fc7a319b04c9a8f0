"""Plain-numpy fp64 reference of the fused D1 output layer (csrc/decout.hip, dec_bce_dw_kernel behind
cc_dec_bce_dw / _ld / _img), the inputs, operand layouts and per-element error bounds of
tests/test_gpu_decout_elem.py.  No GPU, no torch: tests/test_decout_ref_host.py holds this module to
torch-CPU autograd in float64 and proves the bounds on a simulated kernel and six single faults.

Reference (fp64 on the operands as rounded to the kernel's formats: D3 and Wo bf16, bo fp32):
  z = D3 Wo + bo,  loss = mean(max(z, 0) - z y + log1p(exp(-|z|))),
  dz = (sigmoid(z) - y) / (B V) in the target-signed form (1 - 2y) sigmoid((1 - 2y) z) / (B V), which
  never cancels,  gW = D3^T dz,  gb = colsum dz,  and the loss sum of every slice of NB columns
  (NB = 96 for d <= 256, 64 for d = 512; slice sl = columns [sl NB, sl NB + NB)).

Bounds (u = 2^-24, UB = 2^-8 of tower_ref; scale = 1 / (B V); NJ = NB / 32; npass = ceil(B / 256)):
  eps_z = (d + 4) u (|D3| |Wo| + |bo|)   fp32 MFMA accumulation of d products and the bias in any
          order (bf16 products are exact in fp32; the bias enters exactly: three bf16 terms that sum
          to bo in fp32).
  e     = |dz| (eps_z + (|z| log2 e + 8) 2u)   the error of the fp32 dz before its rounding.  sigmoid's
          relative sensitivity to its argument is 1 - sigmoid <= 1, so eps_z of z is at most eps_z
          relative on dz.  The epilogue: z * log2e rounds twice (the constant, the product: 2u
          relative on an exponent of |z| log2 e, so that much relative on a = exp2(-|z log2 e|)),
          v_exp and v_rcp are 1 ulp = 2u each, 1 + a, a * rcp and * scale round once (u each), and
          the fp32 scale 1.0f / (float(B) * float(V)) is within 1.5 u of 1 / (B V): 8.5 u <= 16 u.
  tiny  = 2^-126 scale   the smallest normal fp32 times scale: a below 2^-126 may be flushed to zero
          or kept as a denormal, whatever the mode, and dz then moves by less than this.
  dz    |dZ - dz| <= UB (|dz| + e) + e + tiny   one round-to-nearest bf16 of the fp32 value (half an
          ulp of 8 significant bits is at most 2^-8 relative).  Where |dz| <= tiny: |dZ| <= tiny.  Where
          |dz| > tiny: the signs agree.  (A condition on the inputs, asserted by the host test: no
          |dz| lies in (tiny, 2^-120), where the fp32 dz itself would be denormal and a flush could
          lose up to 2^-126 rather than tiny; and no |z| lies within 1e-3 of a point where the fp32 a
          changes between zero and non-zero — |z| log2 e = 126 with denormals flushed, 149 or 150
          (A_ZERO_POINTS) without.  So no element is left out of any comparison.)
  gwk   |gW - D3^T dZ_kernel| <= (B + 2) u |D3|^T |dZ_kernel|   fp32 accumulation of B exact products
          in any order (the two halves of SPLIT2 included).  Separates a dWo fault from a dZ fault.
  gw    |gW - D3^T dz| <= |D3|^T dzb + (B + 2) u |D3|^T (|dz| + dzb),  dzb the dz bound above.  The first
          term is the dz bound pushed through |D3|^T; the second is there because dWo is itself an fp32
          sum of B products of the stored dZ (|dZ| <= |dz| + dzb) — the gwk error, which the first term
          does not contain.
  gb    |gb - colsum dz| <= (B + 2) u colsum |dz| + colsum (e + tiny)   the kernel sums the fp32 dz
          before its rounding, so no UB term.  tiny stands beside e for the same reason as in dz: each
          of the B summands may have lost up to tiny to a flushed a, and e, being relative to |dz|,
          does not cover an absolute loss.
  loss  per element eps_z + 6u + 2^-126, summed over the slice; + (16 NJ npass + 8) u of the slice's
          sum of terms (all terms are >= 0).  Per element: |d term / dz| <= 1 gives eps_z; max(s, 0) =
          |z| or 0 is exact; log1p(a) is taken as ln of a product of sixteen 1 + a: the rounding of
          1 + a in (1, 2] moves its ln by at most u; the error of a itself ((1 + |z| log2 e) 2u
          relative, weight a / (1 + a) <= min(a, 1/2)) by at most 1.6u; the 15 multiplies of 16 factors
          by less than u per factor; v_log's 1 ulp of log2(product) by 2u ln(1 + a) <= 1.4u: 5u, taken
          as 6u (4u — 1 + a, the product, the log — would leave out the error of a itself).  Sums: a lane
          adds at most 16 NJ npass terms in fp32, then rsum + lsum ln 2, six shuffle adds and the conversion to
          double: + 8.  The bound applies to every slice partial and (summed) to the total.
          At z near -6 the terms are ~ a = 0.0025 and the rounding of 1 + a alone is 2.4e-5 of a
          term: the bound is ~1e-4 relative there, the observed error far smaller (the roundings
          are not all one way); loss_rel, the plain relative error of the total, is recorded beside it.
"""
from collections import namedtuple

import numpy as np

from tests import tower_ref as TR
from tests.tower_ref import U, UB, ceil64, ratio  # noqa: F401  (re-exported for the two test files)

LOUD = 100.0                       # rows B .. ldt of every D3 image: loud if read
FTZ = 2.0 ** -126                  # the smallest normal fp32
LOG2E = 1.4426950408889634
EDGES = (0.0, 30.0, -30.0, 100.0, -100.0)   # the planted bo classes of the trained regime
REGIMES = ('mild', 'trained')
# |z| log2 e at which a = exp2(-|z log2 e|) turns to zero in fp32: below 2^-126 with denormals flushed;
# below 2^-149 (a result truncated) or 2^-150 (rounded to nearest) with denormals kept
A_ZERO_POINTS = (126.0, 149.0, 150.0)

Case = namedtuple('Case', 'B d V ldt')
# B, d, V, ldt: the smallest set that reaches every instantiation the host entry can launch — the generic
# kernel at all nine (d, B), the DMA and DMA+IMG kernels (Wo given, V % 8 == 0) at the six (d <= 256, B) —
# and every edge (tests/test_gpu_decout_elem.py says what each row reaches)
CASES = [Case(128, 128, 1, 128), Case(128, 128, 33, 256), Case(256, 128, 97, 512), Case(512, 128, 200, 1024),
         Case(128, 256, 96, 128), Case(256, 256, 1001, 512), Case(512, 256, 1000, 1024), Case(512, 256, 768, 512),
         Case(512, 256, 1001, 1024), Case(128, 512, 65, 256), Case(256, 512, 709, 512), Case(512, 512, 712, 1024),
         Case(128, 128, 104, 256), Case(256, 128, 40, 512), Case(256, 256, 200, 512)]


def nb_of(d):
    """Columns per slice (csrc/decout.hip nb_of)."""
    return 96 if d <= 256 else 64


def n_slices(d, V):
    return -(-V // nb_of(d))


def ldz_of(V):
    """The trainer's padded dZ row pitch ceil64(V); one 64-column step more where V is a multiple of
    64 itself, so that every case has pad columns to watch (the GPU test also runs the trainer's own
    pitch ceil64(V) == V there)."""
    return ceil64(V + 1)


# ------------------------------------------------------------------ inputs
Inputs = namedtuple('Inputs', 'case regime D3 Wo bo y ybits scale zero_rows planted')


def plant_columns(V):
    """The planted columns of the trained regime: up to ten, evenly spread over the first 64 columns
    (both 32-column tiles of the first slice at every d; every later slice is the plain trained
    regime, so its loss partial measures the small terms alone) and never the last column, which stays
    an ordinary one, where reading the neighbour's weights shows (a saturated column would hide it) —
    as (column, class index into EDGES)."""
    cols = np.unique(np.linspace(0, min(max(V - 2, 0), 63), min(V, 10)).astype(int))
    return [(int(c), i % len(EDGES)) for i, c in enumerate(cols)]


def make_inputs(case, regime, seed):
    """D3 = relu(N(0, 1)) (a ReLU output: non-negative, about half exactly zero), Wo = N(0, 0.8^2 2 / d)
    (logit std ~0.8 at every d), both rounded to bf16; bo fp32.
    mild:    bo = N(0, 0.1^2), target density 0.1.
    trained: bo = -6 + N(0, 1), target density 0.02, and the planted edges — four all-zero D3 rows (z ==
             bo exactly there) and up to ten columns with bo = 0 (-0.0 the second time), +-30, +-100.  Their
             targets: density 0.5 at bo = 0, the sign of bo elsewhere (what a trained model has learnt),
             and 0, 1, 0, 1 down the zero rows — so every class meets both target values, the wrong one
             on a few elements only, and their terms of 30 and 100 do not drown the rest of the loss."""
    B, d, V, ldt = case
    assert regime in REGIMES
    rng = np.random.default_rng(seed)
    D3 = TR.round_bf16(np.maximum(rng.standard_normal((B, d)), 0.0))
    Wo = TR.round_bf16(rng.standard_normal((d, V)) * (0.8 * np.sqrt(2.0 / d)))
    zero_rows, planted = (), []
    if regime == 'mild':
        bo = rng.standard_normal(V) * 0.1
        y = rng.random((B, V)) < 0.1
    else:
        bo = -6.0 + rng.standard_normal(V)
        y = rng.random((B, V)) < 0.02
        zero_rows = (1, 37, B // 2 + 5, B - 1)
        D3[list(zero_rows)] = 0.0
        planted = plant_columns(V)
        for i, (c, k) in enumerate(planted):
            bo[c] = -0.0 if (k == 0 and i >= len(EDGES)) else EDGES[k]
            y[:, c] = rng.random(B) < 0.5 if EDGES[k] == 0 else EDGES[k] > 0
            y[list(zero_rows), c] = [False, True, False, True]
    bo = bo.astype(np.float32).astype(np.float64)
    return Inputs(case, regime, D3, Wo, bo, y, y_bits_of(y, rng), 1.0 / (B * V), zero_rows, planted)


def case_inputs(case, regime):
    """The inputs every test of (case, regime) uses (one seed per pair)."""
    B, d, V, ldt = case
    return make_inputs(case, regime, 1000 * d + 7 * V + B + ldt + 500009 * REGIMES.index(regime))


# ------------------------------------------------------------------ the reference, fp64
Ref = namedtuple('Ref', 'z terms loss dz gW gb slice_sums eps_z e')


def sigmoid(s):
    en = np.exp(-np.abs(s))
    return np.where(s >= 0, 1.0 / (1.0 + en), en / (1.0 + en))


def slice_sums(terms, d):
    """Per-slice sums of a [B][V] array."""
    NB, V = nb_of(d), terms.shape[1]
    return np.array([terms[:, n0:n0 + NB].sum() for n0 in range(0, V, NB)])


def reference(inp, y=None, Wo=None):
    """fp64 on the rounded operands (y / Wo: replacements, for the host test's mutations)."""
    B, d, V, ldt = inp.case
    y = inp.y if y is None else y
    Wo = inp.Wo if Wo is None else Wo
    z = inp.D3 @ Wo + inp.bo
    terms = np.maximum(z, 0.0) - z * y + np.log1p(np.exp(-np.abs(z)))
    sgn = np.where(y, -1.0, 1.0)
    dz = sgn * sigmoid(sgn * z) * inp.scale
    eps_z = (d + 4) * U * (np.abs(inp.D3) @ np.abs(Wo) + np.abs(inp.bo))
    e = np.abs(dz) * (eps_z + (np.abs(z) * LOG2E + 8.0) * 2.0 * U)
    return Ref(z, terms, terms.mean(), dz, inp.D3.T @ dz, dz.sum(0), slice_sums(terms, d), eps_z, e)


# ------------------------------------------------------------------ bounds and the comparison
def tiny_of(inp):
    return FTZ * inp.scale


def dz_bound(inp, ref):
    return UB * (np.abs(ref.dz) + ref.e) + ref.e + tiny_of(inp)


def loss_bounds(inp, ref):
    """Bound of every slice's loss sum (unscaled)."""
    B, d, V, ldt = inp.case
    NJ, npass = nb_of(d) // 32, -(-B // 256)
    return slice_sums(ref.eps_z + 6.0 * U + FTZ, d) + (16 * NJ * npass + 8) * U * ref.slice_sums


def compare(inp, ref, dZ, gW, gb, part, loss):
    """Error / bound of every check (module docstring) for one set of outputs: dZ [B][V] (the stored
    bf16 values), gW [d][V], gb [V], part [n_slices] (unscaled slice sums), loss (scaled by 1 / (B V)).
    dz_tiny: the largest |dZ| / tiny among the elements with |dz| <= tiny; dz_sign: the number of
    elements with |dz| > tiny whose sign differs; loss_rel, loss_part_rel: the plain relative error of
    the total and the largest one of a slice partial."""
    B, d, V, ldt = inp.case
    tiny = tiny_of(inp)
    aD3, adz = np.abs(inp.D3), np.abs(ref.dz)
    dzb = dz_bound(inp, ref)
    small = adz <= tiny
    out = {'dz': ratio(np.abs(dZ - ref.dz), dzb),
           'dz_tiny': float(np.max(np.abs(dZ[small])) / tiny) if small.any() else 0.0,
           'dz_sign': float(np.count_nonzero(np.sign(dZ[~small]) != np.sign(ref.dz[~small])))}
    acc = (B + 2) * U
    out['gwk'] = ratio(np.abs(gW - inp.D3.T @ dZ), acc * (aD3.T @ np.abs(dZ)))
    out['gw'] = ratio(np.abs(gW - ref.gW), aD3.T @ dzb + acc * (aD3.T @ (adz + dzb)))
    out['gb'] = ratio(np.abs(gb - ref.gb), acc * adz.sum(0) + (ref.e + tiny).sum(0))
    lb = loss_bounds(inp, ref)
    out['loss_part'] = ratio(np.abs(np.asarray(part, np.float64) - ref.slice_sums), lb)
    out['loss'] = float(abs(loss - ref.loss) / (lb.sum() * inp.scale))
    out['loss_rel'] = float(abs(loss - ref.loss) / abs(ref.loss))
    out['loss_part_rel'] = float(np.max(np.abs(np.asarray(part, np.float64) - ref.slice_sums) / ref.slice_sums))
    return out


BOUNDED = ('dz', 'dz_tiny', 'gwk', 'gw', 'gb', 'loss_part', 'loss')   # each must be <= 1; dz_sign must be 0


def passes(errs):
    return all(errs[k] <= 1 for k in BOUNDED) and errs['dz_sign'] == 0


def input_conditions(inp, ref):
    """What the comparison relies on (docstring: dz), as a list of violated conditions."""
    bad = []
    for p in A_ZERO_POINTS:
        if np.any(np.abs(np.abs(ref.z) - p / LOG2E) < 1e-3):
            bad.append(f'|z| within 1e-3 of {p} ln 2, where the fp32 a changes between zero and non-zero')
    adz = np.abs(ref.dz)
    if np.any((adz > tiny_of(inp)) & (adz < 2.0 ** -120)):
        bad.append('a dz that is denormal in fp32 but above tiny')
    return bad


# ------------------------------------------------------------------ layouts (uint16 bf16 bit patterns, uint32 words)
def y_bits_of(y, rng=None):
    """y [B][V] bool -> y_bits [B][ceil(V / 32)] uint32, bit l of word w = column 32 w + l; the bits of the
    last word at positions >= V are random (rng given) or zero."""
    B, V = y.shape
    VW = (V + 31) // 32
    full = np.zeros((B, VW * 32), bool)
    if rng is not None:
        full[:, V:] = rng.random((B, VW * 32 - V)) < 0.5
    full[:, :V] = y
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder='little')).view(np.uint32).reshape(B, VW)


def unpack_y_bits(ybits, V):
    return np.unpackbits(np.ascontiguousarray(ybits).view(np.uint8), axis=1, bitorder='little')[:, :V].astype(bool)


def y_img_of(ybits):
    """cc_tower_args.y_img (include/ccrec.h): [ceil(V / 32)][B]; dword 2r + h of a 32-row block is the
    block's row (r & 3) + 8 (r >> 2) + 4h."""
    B, VW = ybits.shape
    img = np.zeros((VW, B), np.uint32)
    for blk in range(B // 32):
        for r in range(16):
            for h in range(2):
                img[:, 32 * blk + 2 * r + h] = ybits[32 * blk + (r & 3) + 8 * (r >> 2) + 4 * h]
    return img


Images = namedtuple('Images', 'D3 D3t D3p D3tp Wo WoT')


def operand_images(inp, ldt=None):
    """Every operand image of one call as bf16 bit patterns, from an ldt-row D3 buffer whose rows
    B .. ldt hold LOUD: D3 [ldt][d], D3t [d][ldt], D3p = act6p [ldt/32][d/16][2][32][8], D3tp = act6tp
    [d/32][ldt/16][2][32][8] (both flat), Wo [d][V], WoT [V][d]."""
    B, d, V, _ = inp.case
    ldt = inp.case.ldt if ldt is None else ldt
    loud = TR.bits(np.float32(LOUD)).reshape(())
    rows = np.full((ldt, d), loud, np.uint16)
    rows[:B] = TR.bits(inp.D3)
    wo = TR.bits(inp.Wo)
    return Images(rows, TR.transpose_ld(rows[:B], ldt, loud), TR.pack_rows(rows), TR.pack_t(rows[:B], ldt, loud),
                  wo, np.ascontiguousarray(wo.T))
