"""CPU: the argument checks of the six cc_embed_grad_cs* entries and of cc_tower_bwd_chain_adam /
cc_tower_bwd_chain_noise.  They run on the host before any launch, so every case here is a
rejection: fake (aligned, non-null, never dereferenced) addresses, exactly one condition violated,
the return code and the whole message asserted.  No case passes a fully valid argument set — that
would reach the launch."""
import ctypes

import pytest

from cubecobrarecommender_amd import _lib as L

ARG, UNSUPPORTED = -1, -3
FORMS = ('cc_embed_grad_cs', 'cc_embed_grad_cs_adam', 'cc_embed_grad_cs_reg', 'cc_embed_grad_cs_adam_reg',
         'cc_embed_grad_cs_adam_dw', 'cc_embed_grad_cs_adam_reg_dw')
ADAM_FORMS = tuple(f for f in FORMS if '_adam' in f)
REG_FORMS = tuple(f for f in FORMS if '_reg' in f)
DW_FORMS = tuple(f for f in FORMS if f.endswith('_dw'))
PLAIN_FORMS = tuple(f for f in FORMS if '_adam' not in f)

# a valid call of every form (never made as it stands): V = 777 cards, d = 128, 96 cube rows, 64 reg
# rows behind them in a 256-row dPre1 image
BASE = dict(dpre=0x10000, packed=1, V=777, d=128, R=96, ld_t=256, xt_bits=0x20000, grad=0x30000, bias_grad=0x40000,
            tickets=0x50000, p=0x60000, m=0x70000, v=0x80000, shadow=0x90000, state=0xA0000, lr=1e-3, beta1=0.9,
            beta2=0.999, eps=1e-7, reg_idx=0xB0000, nreg=64, reg_k0=6, card0=0, n_riders=16, stream=None)
W1 = ('dpre', 'packed', 'V', 'd', 'R', 'ld_t', 'xt_bits')
ADAM = ('p', 'm', 'v', 'shadow', 'state', 'lr', 'beta1', 'beta2', 'eps')
REG = ('reg_idx', 'nreg', 'reg_k0')


def _fields(form):
    if '_adam' not in form:
        return W1 + ('grad', 'bias_grad', 'tickets') + (REG + ('card0',) if '_reg' in form else ()) + ('stream',)
    return (W1 + ('bias_grad', 'tickets') + ADAM + (REG if '_reg' in form else ()) +
            (('tower', 'n_riders') if form.endswith('_dw') else ()) + ('stream',))


def _tower(**kw):
    """A tower the rider forms accept: bf16, d = 128, 96 rows, the packed hpt / gpt images."""
    t = L.TowerArgs(dtype=L.CC_BF16, d=128, B=96, R=96)
    t.gD3 = 0xC0000
    for a in range(5):
        t.gact[a] = 0xC1000
    for a in range(6):
        t.hpt[a], t.gpt[a], t.gw[a], t.gb[a] = 0xD0000 + 0x100 * a, 0xE0000 + 0x100 * a, 0xF0000, 0xF1000
    for k, val in kw.items():
        if isinstance(val, tuple):
            getattr(t, k)[val[0]] = val[1]
        else:
            setattr(t, k, val)
    return t


def _call(form, over):
    a = {**BASE, **over}
    t = a.pop('tower', _tower())
    a['tower'] = None if t is None else ctypes.byref(t)
    lib = L.lib()
    rc = getattr(lib, form)(*(a[f] for f in _fields(form)))
    return rc, lib.cc_last_error_string().decode()


NULL = '{who}: null pointer'
ALIGN_G = '{who}: grad / bias_grad 16-B aligned'
ALIGN_A = '{who}: p, m, v, bias_grad 16-B aligned, shadow 8-B aligned'
DMSG = '{who}: d must be a multiple of 32'
VR = '{who}: V > 0, R in 1..2048'
VR_REG = 'cc_embed_grad_cs_reg: V > 0, R in 1..2048, card0 >= 0'
LDT = '{who}: ld_t must be a multiple of 64 covering R, dPre1 image 16-B aligned'
REG_N = '{who}: reg_idx non-null, nreg in 1..512'
REG_ROWS = ('{who}: reg rows past the product\'s rows and inside the dPre1 image (16 reg_k0 >= R, '
            '16 (reg_k0 + ceil(nreg / 16)) <= ld_t)')
RIDERS = '{who}: n_riders in 1..64'
LDS = 'cc_embed_grad_cs: R too large for the LDS stage'
DW_PACKED = ('{who}: needs the packed transposed hpt / gpt images (16-B aligned, B and R multiples of 16) of the '
             'bf16 fast / wide chains')
DW_TALL = ('{who}: tall chain (its dW is split by rows): run cc_tower_bwd_dw_direct and the W1 gradient as two '
           'launches')

# (forms, overrides of BASE, return code, message; {who}: the called entry)
CASES = []


def case(forms, msg, rc=ARG, **over):
    CASES.extend((f, over, rc, msg if f != 'cc_embed_grad_cs_reg' or msg != VR else VR_REG) for f in forms)


for name in ('dpre', 'xt_bits'):
    case(FORMS, NULL, **{name: None})
case(PLAIN_FORMS, NULL, grad=None)
for name in ('p', 'm', 'v', 'shadow', 'state'):
    case(ADAM_FORMS, NULL, **{name: None})
case(PLAIN_FORMS, ALIGN_G, grad=BASE['grad'] + 4)
case(PLAIN_FORMS, ALIGN_G, bias_grad=BASE['bias_grad'] + 8)
for name in ('p', 'm', 'v', 'bias_grad'):
    case(ADAM_FORMS, ALIGN_A, **{name: BASE[name] + 4})
case(ADAM_FORMS, ALIGN_A, shadow=BASE['shadow'] + 4)
for d in (48, 16, 4128):
    case(FORMS, DMSG, d=d)
case(FORMS, VR, V=0)
case(FORMS, VR, R=0)
case(FORMS, VR, R=2049, ld_t=2240, reg_k0=129)
case(('cc_embed_grad_cs_reg',), VR_REG, card0=-1)
case(FORMS, LDT, ld_t=224)                      # covers R and the reg rows; no multiple of 64
case(FORMS, LDT, ld_t=64)                       # a multiple of 64 below R = 96
case(FORMS, LDT, dpre=BASE['dpre'] + 8)
case(REG_FORMS, REG_N, reg_idx=None)
case(REG_FORMS, REG_N, nreg=0)
case(REG_FORMS, REG_N, nreg=513, ld_t=640)
case(REG_FORMS, REG_ROWS, reg_k0=5)             # 80 < R
case(REG_FORMS, REG_ROWS, ld_t=128)             # rows 96 .. 159 of a 128-row image
case(DW_FORMS, RIDERS, n_riders=0)
case(DW_FORMS, RIDERS, n_riders=65)
case(DW_FORMS, 'cc_tower: null args', tower=None)
case(DW_FORMS, 'cc_tower: d out of range for the fused towers', rc=UNSUPPORTED, tower=_tower(d=2048))
case(DW_FORMS, '{who}: bf16 only', tower=_tower(dtype=L.CC_F32))
case(DW_FORMS, '{who}: null gD3', tower=_tower(gD3=None))
case(DW_FORMS, '{who}: null gw/gb', tower=_tower(gb=(5, None)))
case(DW_FORMS, DW_PACKED, tower=_tower(gpt=(3, None)))
case(DW_FORMS, DW_PACKED, tower=_tower(hpt=(0, 0xD0008)))
case(DW_FORMS, DW_TALL, tower=_tower(B=2048, R=2048, slab=0xC8000))
# the Adam epilogue's re-layout tiles leave no room for a 1024 < R slice: 131072 + 16384 + 36864 bytes
case(ADAM_FORMS, LDS, R=1025, ld_t=1088, reg_k0=65, nreg=16)


def _id(c):
    form, over = c[0], c[1]
    return form[len('cc_embed_grad_'):] + '-' + ','.join(
        k if not isinstance(x, int) or isinstance(x, bool) or x > 0xFFFF else f'{k}={x}' for k, x in over.items())


@pytest.mark.parametrize('form,over,rc,msg', CASES, ids=[f'{i}-{_id(c)}' for i, c in enumerate(CASES)])
def test_w1_gradient_entry_rejects(form, over, rc, msg):
    assert _call(form, over) == (rc, msg.format(who=form))


def test_every_form_meets_every_kind_of_check():
    seen = {}
    for form, over, _, msg in CASES:
        seen.setdefault(form, set()).add(msg)
    assert set(seen) == set(FORMS)
    for form in FORMS:
        want = {NULL, DMSG, LDT, VR_REG if form == 'cc_embed_grad_cs_reg' else VR,
                ALIGN_A if form in ADAM_FORMS else ALIGN_G}
        want |= {REG_N, REG_ROWS} if form in REG_FORMS else set()
        want |= {RIDERS, DW_PACKED, DW_TALL} if form in DW_FORMS else set()
        want |= {LDS} if form in ADAM_FORMS else set()
        assert want <= seen[form], form


# ---- cc_tower_bwd_chain_adam / cc_tower_bwd_chain_noise: the chains' launch with TF Adam over two ranges

CHAIN_BASE = dict(p=0x60000, m=0x70000, v=0x80000, g=0x90000, shadow=0xA0000, lo0=0, n0=64, lo1=128, n1=64,
                  state=0xB0000, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, stream=None, bpe=10)
CHAIN_ADAM = ('p', 'm', 'v', 'g', 'shadow', 'lo0', 'n0', 'lo1', 'n1', 'state', 'lr', 'beta1', 'beta2', 'eps', 'stream')


def _noise(**kw):
    """cc_noise_fwd's arguments as the chains' launch accepts them for the next step's F."""
    n = L.NoiseArgs(V=777, B=96, x_cap=64, with_reg=0, batch_stride=96, num_perms=1, num_cubes=1000)
    for i, f in enumerate(('cube_ptr', 'cube_idx', 'perm', 'cdf', 'neg_sampler', 'state', 'x_cnt', 'x_idx', 'y_bits',
                           'status')):
        setattr(n, f, 0x100000 + 0x1000 * i)
    for k, val in kw.items():
        setattr(n, k, val)
    return n


def _chain_call(entry, over):
    a = {**CHAIN_BASE, **over}
    t, nx = a.pop('tower', _tower()), a.pop('next', _noise())
    head = [None if t is None else ctypes.byref(t)]
    if entry.endswith('_noise'):
        head += [None if nx is None else ctypes.byref(nx), a['bpe']]
    lib = L.lib()
    rc = getattr(lib, entry)(*head, *(a[f] for f in CHAIN_ADAM))
    return rc, lib.cc_last_error_string().decode()


CHAINS = ('cc_tower_bwd_chain_adam', 'cc_tower_bwd_chain_noise')
FAST = '{who}: the bf16 fast chains (d <= 256) only'
C_NULL = {'cc_tower_bwd_chain_adam': 'cc_tower_bwd_chain_adam: null pointer',
          'cc_tower_bwd_chain_noise': 'cc_tower_bwd_chain_noise: null Adam pointer'}
C_ALIGN = '{who}: buffers must be 16-byte aligned, range starts multiples of 4'
C_SHADOW = '{who}: shadow must be 8-byte aligned'
C_RANGES = '{who}: ranges'
F_ARGS = 'cc_tower_bwd_chain_noise: F arguments'
F_XT = 'cc_tower_bwd_chain_noise: F may not set xt bits here (the W1 gradient still reads them)'
F_PERMS = 'cc_tower_bwd_chain_noise: num_perms / num_cubes / batches_per_epoch'
F_V = 'cc_tower_bwd_chain_noise: V too large'

CHAIN_CASES = []


def chain_case(msg, entries=CHAINS, **over):
    CHAIN_CASES.extend((e, over, msg[e] if isinstance(msg, dict) else msg) for e in entries)


chain_case(FAST, tower=None)
chain_case(FAST, tower=_tower(dtype=L.CC_F32))
chain_case(FAST, tower=_tower(d=512))
for name in ('p', 'm', 'v', 'g', 'state'):
    chain_case(C_NULL, **{name: None})
for name in ('p', 'm', 'v', 'g'):
    chain_case(C_ALIGN, **{name: CHAIN_BASE[name] + 8})
chain_case(C_ALIGN, lo0=2)
chain_case(C_ALIGN, lo1=130)
chain_case(C_SHADOW, shadow=CHAIN_BASE['shadow'] + 4)
chain_case(C_RANGES, lo0=-4)
chain_case(C_RANGES, n0=-4)
chain_case(C_RANGES, n1=-4)
chain_case(C_RANGES, lo1=32)                    # the second range starts inside the first
NOISE = CHAINS[1:]
chain_case(F_ARGS, NOISE, next=None)
for name in ('V', 'B', 'x_cap', 'cube_ptr', 'cube_idx', 'perm', 'cdf', 'neg_sampler', 'state', 'x_cnt', 'x_idx', 'y_bits',
             'status'):
    chain_case(F_ARGS, NOISE, next=_noise(**{name: 0}))
chain_case(F_ARGS, NOISE, next=_noise(with_reg=1))          # with_reg without reg_idx
chain_case(F_XT, NOISE, next=_noise(xt_bits=0x200000))
chain_case(F_PERMS, NOISE, next=_noise(num_perms=0))
chain_case(F_PERMS, NOISE, next=_noise(num_cubes=95))       # fewer cubes than one batch stride
chain_case(F_PERMS, NOISE, bpe=0)
chain_case(F_V, NOISE, next=_noise(V=50_000_000))


def _chain_id(c):
    entry, over = c[0], c[1]
    return entry[len('cc_tower_bwd_chain_'):] + '-' + ','.join(
        k if not isinstance(x, int) or x > 0xFFFF else f'{k}={x}' for k, x in over.items())


@pytest.mark.parametrize('entry,over,msg', CHAIN_CASES, ids=[f'{i}-{_chain_id(c)}' for i, c in enumerate(CHAIN_CASES)])
def test_chain_adam_entry_rejects(entry, over, msg):
    assert _chain_call(entry, over) == (ARG, msg.format(who=entry))
