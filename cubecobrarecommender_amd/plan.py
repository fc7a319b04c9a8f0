"""Path selection of the training step: which kernel each part of a step runs and which buffers
those kernels need, decided once from the config and a few host-side facts about the dataset.

plan_step() is pure — no torch device, no library call, nothing allocated — so what a config
selects can be read (and is pinned, tests/test_step_plan.py against tests/golden/step_plans.json)
without a GPU.  Trainer.__init__ builds the plan, allocates what it names and copies its fields to
the attributes the step methods, zero.py, bench.py and the tests read.  Sizes that come from the
library (tickets, slabs, workspaces, fragment images) stay with the allocations in trainer.py.

Each decision is written once, in dependency order; a later one names the earlier flag instead of
restating its conditions (fused_out implies bf16 operands, the fused towers and no fp8, and so on).
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from ._lib import CC_BF16, CC_F32
from .layout import Layout


def reg_row_shards(cdf, world):
    """Row shards of M~ for the sampled regulariser (owner computes): boundaries
    b[0..world] at equal cumulative neg_sampler mass — shard r = cards whose CDF value lies in
    (r/world, (r+1)/world] — and each shard's mass m_r = cdf[b_{r+1}-1] - cdf[b_r-1].  Rank r holds
    rows [b_r, b_{r+1}) of M~ only; every rank draws the step's world*B global reg rows (the same
    draws one process of batch world*B makes) and computes the KL terms of the rows it owns
    (cc_reg_rows), so the summed gradient is exactly the one-process gradient; equal mass balances
    the expected rows per rank."""
    cdf = np.asarray(cdf, np.float64)
    V = len(cdf)
    b = np.searchsorted(cdf, np.arange(world + 1) / float(world), side='right')
    b[0], b[world] = 0, V
    b = np.maximum.accumulate(np.minimum(b, V))
    lo_mass = np.where(b[:-1] > 0, cdf[np.maximum(b[:-1] - 1, 0)], 0.0)
    hi_mass = np.where(b[1:] > 0, cdf[np.maximum(b[1:] - 1, 0)], 0.0)
    mass = hi_mass - lo_mass
    if np.any(b[1:] <= b[:-1]) or np.any(mass <= 0):
        raise ValueError(f'reg_row_shards: a shard of {world} is empty (one card holds > 1/{world} '
                         'of the neg_sampler mass); use the replicated M~ (reg_shard=False)')
    return b.astype(np.int64), mass


def owner_capacity(mass, B, world, align=32, sigmas=6.0):
    """Reg rows each rank reserves under owner computes: the world*B global draws land in shard r
    Binomial(world*B, m_r) times; capacity = max over ranks of mean + 6 sigma (+1), rounded up to
    `align` (an overflow sets the device status bit 2 and Trainer.check_status raises)."""
    n = world * B
    m = np.asarray(mass, np.float64)
    need = np.max(n * m + sigmas * np.sqrt(n * m * (1.0 - m)) + 1.0)
    return int(min(n, int(np.ceil(need / align)) * align))


def full_rows(V, world, rank):
    """Full mode: rank r owns identity rows [r*ceil(V/W), (r+1)*ceil(V/W)) ∩ [0, V)."""
    per = -(-V // world)
    return min(V, rank * per), min(V, (rank + 1) * per)


def fused_reg_fits(hi, V, Breg):
    """cc_dec_softmax_kl_dw's 32-bit buffer extents (decreg.hip: mt_bytes < 2^31 for M~ rows up to
    `hi`, the Breg x V bf16 dZ < 2^32 bytes)."""
    return hi * V * 4 <= 0x7FFFFFFF and Breg * V * 2 <= 0xFFFFFFFF


def dx_splitk_fits(M, V, d):
    """cc_gemm_dx_splitk's operand extents (dxgemm.hip: M*V and d*V bf16 elements < 2 GB)."""
    return M * V * 2 < (1 << 31) and d * V * 2 < (1 << 31)


def _cdf(neg_sampler):
    cdf = np.cumsum(np.asarray(neg_sampler, np.float64))
    return cdf / cdf[-1]


def reg_rows_for(neg_sampler, world, rank, reg_mode='sampled'):
    """Rank's M~ row shard [lo, hi): equal neg_sampler mass (sampled) or equal rows (full)."""
    if reg_mode == 'full':
        return full_rows(len(neg_sampler), world, rank)
    b, _ = reg_row_shards(_cdf(neg_sampler), world)
    return int(b[rank]), int(b[rank + 1])


def branches_of(use_reg):
    return ('decoder', 'decoder_for_reg') if use_reg else ('decoder',)


Range = Tuple[int, int]


@dataclass(frozen=True)
class StepPlan:
    """What plan_step decided.  Flags carry the names the trainer's attributes have; has_* say that
    a buffer exists where its existence is itself a decision."""
    # layout and rows
    layout: Layout                 # the flat parameter layout (data parallel: bucket-aligned)
    std_layout: Layout             # the standard cc_param_layout (checkpoints)
    dp: bool                       # zero.py's sharded step (buckets, collectives)
    use_reg: bool
    full_reg: bool                 # all |V| identity rows every step
    owner: bool                    # data parallel, M~ row-sharded: owner computes
    reg_rows: Range                # M~ rows [lo, hi) this rank reads
    Breg: int                      # regulariser rows: rows [B, B + Breg) of every row-indexed buffer
    R: int                         # B + Breg
    RP: int                        # R rounded up to 64 (dPre1^T's pitch)
    kl_row_scale: float            # dZ weight of a regulariser row
    kl_loss_scale: float
    # operand formats
    mx8: bool                      # fp8: MX-FP8 decoder output / regulariser GEMMs
    dtype: int                     # CC_F32 or CC_BF16 (fp8 keeps bf16 everywhere else)
    # towers and the W1 gradient
    fused_tower: bool              # tower.hip row-block kernels (else per-layer cc_gemm launches)
    reg_by_index: bool             # sampled reg rows enter the W1 product by index
    xt_rows: int                   # rows of the W1-gradient bit matrix
    embed_mfma: bool               # the W1 gradient on MFMA, by column slices, from dPre1^T
    has_w1_cs: bool                # ... its tickets (cc_embed_grad_cs; else cc_embed_scatter_bwd)
    has_wpack: bool                # fragment-packed tower weight images
    has_D3p: bool                  # D3 as packed operand images of the fused output kernels
    has_gpre1p: bool               # dPre1 as packed transposed fragments
    tower_dw: Optional[str]        # 'direct' | 'slab' (+ cc_tower_reduce) | None without the fused towers
    tsplits: int                   # the generic tower dW's K-splits
    # decoder output layers
    dx_glds: bool                  # decoder dX on the LDS-DMA pipelined split-K kernel's dtype
    fused_out: bool                # D1: logits + BCE + dZ + dWo in one kernel (decout.hip)
    dz1_ld: int                    # ... its dZ row pitch
    fused_reg: bool                # D2: logits + softmax + KL + dZ + dWo in one kernel (decreg.hip)
    has_Z2: bool                   # materialised fp32 D2 logits (the unfused regulariser)
    has_WoP: bool                  # full mode: Wo as its MFMA fragment image for dX
    d3q_in_tower: bool             # fp8: the tower forward writes D3's MX-FP8 images
    mx8_bce_q: bool                # fp8: the BCE product writes dZ's MX-FP8 images
    reg_logits_paired: bool        # fp8: the regulariser logits ride in the BCE product's launch
    splits: int                    # decoder dX K-splits
    splits_reg: int                # ... of the regulariser branch
    dx_kernels: Tuple[str, ...]    # per branch: 'dx_splitk_pk' | 'dx_splitk' | 'gemm' | 'pair' (with dW)
    # F and Adam placement
    prefetch: bool                 # one process: the next step's F in the Adam launch
    prefetch_dp: bool              # data parallel: the next step's F off the forward's critical path
    xt_in_gather: bool             # F writes x rows as bitmasks; a later launch transposes them
    has_x_bits: bool
    xt_in_tower: bool              # ... the tower forward launch (fast chains) instead of the E1 gather
    has_y_img: bool                # the fused D1 kernel's target masks in accumulator row order
    adam_packs: bool               # the Adam + F launch rewrites the packed tower images
    w1_off: int                    # W1's padded size (the Adam range starts here with fuse_w1)
    fuse_w1: bool                  # TF Adam on W1 inside its gradient kernel
    wo_ranges: Optional[Tuple[Range, ...]]     # output-layer tails updated in the tower backward launch
    rest_ranges: Optional[Tuple[Range, ...]]   # ... and what the Adam launch keeps
    wo_range: Optional[Range]
    f_in_tower: bool               # the next step's F in the tower backward launch
    dw_in_w1: int                  # > 0: the tower dW jobs ride in the W1-gradient launch, on this many riders
    # data parallel (zero.py)
    early_reg_out: bool            # both output layers are one early bucket
    dp_defer_out_ok: bool          # the output layers' all-gather may wait for the next step's head
    bucket_hook_names: Tuple[str, ...]   # buckets forward_backward_b finalises one by one
    f_bucket_name: str             # the bucket whose sharded Adam launch also draws the next F


def plan_step(cfg, cdf=None, data_reg_rows=None):
    """The StepPlan of a TrainConfig.  cdf: the dataset's neg_sampler CDF (read only for the
    owner-computes row shards); data_reg_rows: the M~ rows (lo, hi) the dataset holds, None without
    the matrix.  Raises what Trainer(cfg, data) raises for a config it cannot run."""
    V, d, B, W = cfg.V, cfg.d, cfg.batch_size, cfg.world
    assert d % 64 == 0 and (d // 64) & (d // 64 - 1) == 0, 'd must be 64 * 2^k'
    bf16 = cfg.dtype != 'fp32'     # bf16 operands (fp8 too); an unknown dtype is rejected below
    mx8 = cfg.dtype == 'fp8'
    dp = W > 1 or cfg.force_dp
    # data-parallel: gradient buckets aligned to world*64 so every rank owns an equal shard (with
    # a bf16 shadow the biases are grouped so zero.py all-gathers the kernels' bf16 shadow); W1's
    # gradient in row chunks by the exchange model: 1 at d <= 512, 2 above
    std_layout = Layout(V, d)
    layout = (Layout(V, d, align=W * 64, group_biases=bf16,
                     w1_chunks=(1 if cfg.reg_mode == 'full' else cfg.w1_chunks if cfg.w1_chunks > 0
                                else 1 if d <= 512 else 2))
              if dp else std_layout)
    use_reg = cfg.reg > 0
    if use_reg and data_reg_rows is None:
        raise ValueError('reg > 0 needs the M~ matrix on the device')
    if cfg.reg_mode not in ('sampled', 'full'):
        raise ValueError(f"reg_mode {cfg.reg_mode!r}: 'sampled' or 'full'")
    full_reg = use_reg and cfg.reg_mode == 'full'
    owner = use_reg and not full_reg and cfg.reg_shard and dp
    # regulariser rows of this rank: rows [B, B + Breg) of every row-indexed buffer.
    #   sampled: B draws per step (slot b of cube b), dz weight reg/B;
    #   owner (data parallel, M~ row-sharded): the world*B global draws that fall in this
    #     rank's shard, padded to a static capacity, masked rows reg_idx = -1; weight reg/B
    #     (the zero.py average over ranks makes it reg/(world*B) per global row);
    #   full: identity rows [lo, hi) (all of V on one GPU), weight reg*world/V.
    ralign = 128 if mx8 else 32
    reg_rows, Breg = (0, V), (B if use_reg else 0)
    kl_row_scale, kl_loss_scale = cfg.reg / B, 1.0 / B
    if full_reg:
        reg_rows = full_rows(V, W, cfg.rank)
        Breg = -(-(reg_rows[1] - reg_rows[0]) // ralign) * ralign
        kl_row_scale, kl_loss_scale = cfg.reg * W / V, W / V
    elif owner:
        bnd, mass = reg_row_shards(cdf, W)
        reg_rows = (int(bnd[cfg.rank]), int(bnd[cfg.rank + 1]))
        Breg = owner_capacity(mass, B, W, align=ralign)
    R = B + Breg
    if use_reg and data_reg_rows != reg_rows and data_reg_rows != (0, V):   # (all of M~: the trainer cuts it)
        raise ValueError(f'dataset holds M~ rows {data_reg_rows}, rank needs {reg_rows}')
    if cfg.dtype not in ('bf16', 'fp32', 'fp8'):
        raise ValueError(f'dtype {cfg.dtype!r}: bf16, fp32 or fp8')
    if mx8 and (d % 128 or R % 128 or B % 32):
        raise ValueError('fp8 (MX) decoder GEMMs need d and the row count (B, 2B with reg) multiples of 128')
    # fused 32-row-block towers (tower.hip) when the widths fit; generic GEMMs otherwise
    fused_tower = cfg.fused_tower and B % 32 == 0 and d <= (1024 if bf16 else 256)
    if mx8 and not fused_tower:
        raise ValueError('fp8 needs the fused towers (fused_tower=True, B % 32 == 0)')
    # the bf16 tower kernels' fragment-packed images (weights, D3, every layer's input and
    # output-gradient): d <= 256 fast chains, 256 < d <= 1024 wide
    pack = fused_tower and bf16
    fast = pack and d <= 256
    # the sampled reg rows (one card each) by index in the W1 gradient (cc_embed_grad_cs_reg), not
    # as bits of a 2B-row bit matrix (not with f_in_tower: the next step's F, drawn in the tower
    # backward launch, rewrites the reg cards before the W1 gradient reads them)
    reg_by_index = bool(cfg.reg_by_index and use_reg and not full_reg and pack and d % 128 == 0
                        and 0 < Breg <= 512 and not cfg.f_in_tower)
    # rows of the MFMA W1-gradient product (its bit matrix): the cubes only when the regulariser
    # rows enter by index (full mode: cc_embed_identity_add; sampled: cc_embed_grad_cs_reg)
    xt_rows = B if (full_reg or reg_by_index) else R
    # the W1 gradient on MFMA by column slices (cc_embed_grad_cs) from dPre1^T bf16 [d][RP] written
    # by the tower backward chain; otherwise the row kernel (cc_embed_scatter_bwd)
    embed_mfma = pack and d % 128 == 0 and xt_rows <= 2048
    assert not reg_by_index or embed_mfma, 'reg_by_index needs the column-slice W1 gradient'
    # D1 output layer fused (logits + BCE + dZ + dWo, csrc/decout.hip) where its shape fits; its dZ
    # rows at a pitch of whole 64-element (128-B) groups (DESIGN: measured r04u)
    fused_out = pack and not mx8 and d in (128, 256, 512) and B in (128, 256, 512)
    dz1_ld = -(-V // 64) * 64 if fused_out and cfg.dz_pad else V
    # D2 output layer fused (logits twice -> softmax -> KL -> dZ -> dWo, csrc/decreg.hip): the same
    # shape class; its buffer descriptors address M~ up to row hi and the Breg x V bf16 dZ with
    # 32-bit extents — larger card pools take the Z2 path instead of failing
    fused_reg = (use_reg and pack and not mx8 and d in (128, 256, 512) and Breg % 32 == 0
                 and fused_reg_fits(reg_rows[1], V, Breg))
    # the full-mode regulariser's dX takes Wo as its MFMA B-fragment image (cc_gemm_dx_splitk_pk)
    has_WoP = bool(full_reg and fused_reg and d % 256 == 0 and V % 8 == 0 and Breg % 128 == 0
                   and cfg.dx_packed_wo)
    # config 5: on the wide chains the tower forward writes D3's MX-FP8 images itself; the BCE
    # product makes dZ's MX-FP8 images and the bias gradient in its epilogue (cc_gemm_mx8_bce_q2,
    # B <= 512; larger batches keep the quantiser launches), the regulariser logits as extra blocks
    # of the same launch
    d3q_in_tower = mx8 and d > 256
    mx8_bce_q = mx8 and B <= 512
    reg_logits_paired = mx8_bce_q and use_reg
    # decoder dX K-splits over K = V (measured: 32 bf16; fp8's 256 x 256 tiles 16); the regulariser
    # branch with thousands of rows (full mode) fills the chip with its output tiles: 4
    # (tools/micro/dx_full_micro.py, the 128 x 256-tile kernel of dxgemm.hip for tall M)
    splits = max(1, min(16 if mx8 else 32, V // 512))
    splits_reg = splits if Breg <= 1024 else 4
    tsplits = max(1, min(8, B // 128))             # tower dW: K = rows (B or 2B)
    # each branch's dX launch.  Behind a fused output kernel (which made dWo) dX runs alone: the
    # LDS-DMA pipelined split-K kernel (dxgemm.hip) on the shapes it takes, the full-mode
    # regulariser's with Wo's fragment image, else cc_gemm's register-staged NT path (same
    # partials).  Otherwise dX and dW are one grouped launch, cc_gemm_pair ('pair'; the side-stream
    # alternative was measured slower — r03: the tower dW beside the W1 gradient, 166.5 -> 181.7 us
    # per step, every kernel of the graph slower).  Without the fused towers: plain cc_gemm.
    def dx_kernel(k, nr):
        if not fused_tower:
            return 'gemm'
        if not (fused_reg if k else fused_out):
            return 'pair'
        if nr % 128 or not dx_splitk_fits(nr, V, d):
            return 'gemm'
        if k == 1 and has_WoP:
            return 'dx_splitk_pk'
        return 'dx_splitk' if V % 8 == 0 else 'gemm'
    dx_kernels = tuple(dx_kernel(k, nr) for k, nr in enumerate((B, Breg) if use_reg else (B,)))
    # F for the next step in the Adam launch (cc_adam_noise): Adam is HBM-bound, F latency-bound;
    # data parallel: beside the exchange of the last gradient buckets (zero.py)
    prefetch = cfg.prefetch_noise and not dp
    prefetch_dp = cfg.prefetch_noise and dp
    # one process: F writes its x rows as bitmasks and the next E1 gather launch bit-transposes
    # them into the W1-gradient bitmask (cc_embed_gather_fwd_xt) — or the tower forward launch
    # where its fast kernel runs (its 16-32 chain blocks leave the other CUs idle)
    xt_in_gather = prefetch and bf16
    xt_in_tower = xt_in_gather and fast
    # the fused D1 kernel's target masks as an image in accumulator-register row order, transposed
    # from F's y words by the tower forward launch's extra blocks
    has_y_img = fused_out and fast
    # one process, packed tower images: the Adam + F launch also rewrites them and advances the
    # step counters (cc_adam_noise_pack) — the next step starts without a counters/transposes launch
    adam_packs = prefetch and pack
    # TF Adam on W1 in the W1-gradient kernel's epilogue (cc_embed_grad_cs_adam): one process only
    # (DP reduces the gradient first), the column-slice kernel, not the full-mode regulariser (its
    # identity rows add to the W1 gradient after that kernel); W1 is the first tensor of the layout
    w1_off = layout.offset('encoder/encoded_1/bias')   # = W1's padded size
    fuse_w1 = (cfg.fuse_w1_adam and adam_packs and embed_mfma and not full_reg
               and layout.offset('encoder/encoded_1/kernel') == 0)
    # TF Adam on the trailing wo_tower_frac of the decoder output layers in extra workgroups of the
    # tower backward launch (cc_tower_bwd_chain_adam; < 0: measured per mode — 0.6 BCE only, 0.55
    # with the sampled regulariser).  wo_ranges: the tower launch's [lo, hi) flat ranges;
    # rest_ranges: the Adam launch's (W1 end onwards)
    wo_ranges = rest_ranges = None
    if cfg.wo_adam_in_tower and fuse_w1 and fused_out and (not use_reg or fused_reg) and fast:
        frac = cfg.wo_tower_frac if cfg.wo_tower_frac >= 0 else (0.55 if use_reg else 0.6)
        frac = min(max(float(frac), 0.0), 1.0)
        spans = [(layout.offset('decoder/reconstruct/kernel'), layout.main_total)]
        if use_reg:
            spans.append((layout.offset('decoder_for_reg/reconstruct/kernel'), layout.total))
        wo = tuple((hi - int((hi - lo) * frac) // 256 * 256, hi) for lo, hi in spans)
        if all(a < b for a, b in wo):
            wo_ranges = wo
            rest, lo = [], w1_off
            for a, b in wo:        # the complement inside [W1 end, end of the Adam range)
                rest.append((lo, a))
                lo = b
            rest_ranges = tuple(rest)
    # the next step's F in the tower backward launch: one process with F prefetched and the xt bits
    # made by the tower forward's transpose (so F sets none the W1 gradient still reads)
    f_in_tower = bool(cfg.f_in_tower and adam_packs and xt_in_tower and not full_reg)
    # the tower weight gradients as rider workgroups of the W1 gradient + Adam launch
    # (cc_embed_grad_cs_adam_dw) instead of their own launch between the backward chain and it:
    # with tower_dw == 'direct' from the packed hpt / gpt images (pack) only, and neither the
    # full-mode regulariser nor any chain of 2048 rows or more (tower.hip splits a tall chain's dW
    # by rows: its own two launches).  The value is the rider count (cfg.dw_in_w1 < 0: measured
    # per mode — 16 riders BCE only, 147.2 -> 143.0 us per step; with the sampled regulariser the
    # 1024-row chains' jobs outlast the W1 product on the 16 - 24 CUs it can spare: off).
    riders = int(cfg.dw_in_w1) if cfg.dw_in_w1 >= 0 else (0 if use_reg else 16)
    dw_in_w1 = riders if fuse_w1 and pack and not full_reg and R < 2048 else 0
    assert 0 <= dw_in_w1 <= 64, 'dw_in_w1: 0 (off) or 1..64 rider workgroups'
    # zero.py: the bf16 / fp8 layout's output layers are one early bucket (its exchange waits for
    # the regulariser branch too); it may defer their all-gather to the next step's head when
    # nothing between this step's Adam and the next D1 launch reads their shadow (the fused kernels
    # read Wo straight from it; no Wo^T, MX-FP8 or fragment image is refreshed from it)
    early_reg_out = dp and layout.group_biases and use_reg
    dp_defer_out_ok = bool(cfg.dp_defer_out and fused_out and (not use_reg or fused_reg) and not has_WoP)
    nchunks = len(layout.w1_chunks) if layout.group_biases else 0
    return StepPlan(
        layout=layout, std_layout=std_layout, dp=dp, use_reg=use_reg, full_reg=full_reg, owner=owner,
        reg_rows=reg_rows, Breg=Breg, R=R, RP=(R + 63) // 64 * 64, kl_row_scale=kl_row_scale,
        kl_loss_scale=kl_loss_scale, mx8=mx8, dtype=CC_BF16 if bf16 else CC_F32, fused_tower=fused_tower,
        reg_by_index=reg_by_index, xt_rows=xt_rows, embed_mfma=embed_mfma, has_w1_cs=embed_mfma, has_wpack=pack,
        has_D3p=pack, has_gpre1p=embed_mfma and d == 256,
        tower_dw=None if not fused_tower else 'direct' if bf16 else 'slab', tsplits=tsplits, dx_glds=bf16,
        fused_out=fused_out, dz1_ld=dz1_ld, fused_reg=fused_reg, has_Z2=use_reg and not fused_reg, has_WoP=has_WoP,
        d3q_in_tower=d3q_in_tower, mx8_bce_q=mx8_bce_q, reg_logits_paired=reg_logits_paired, splits=splits,
        splits_reg=splits_reg, dx_kernels=dx_kernels, prefetch=prefetch, prefetch_dp=prefetch_dp,
        xt_in_gather=xt_in_gather, has_x_bits=xt_in_gather, xt_in_tower=xt_in_tower, has_y_img=has_y_img,
        adam_packs=adam_packs, w1_off=w1_off, fuse_w1=fuse_w1, wo_ranges=wo_ranges, rest_ranges=rest_ranges,
        wo_range=wo_ranges[0] if wo_ranges else None, f_in_tower=f_in_tower, dw_in_w1=dw_in_w1,
        early_reg_out=early_reg_out,
        dp_defer_out_ok=dp_defer_out_ok,
        bucket_hook_names=tuple(f'w1_{i}' for i in range(nchunks)),
        f_bucket_name=f'w1_{nchunks - 1}' if layout.group_biases else 'towers_e1')
