"""TEST INFRASTRUCTURE ONLY: host restatements the training-step tests compare the HIP step with.  Plain numpy / torch on the CPU, no GPU.

1. The dropout mask of conformer_ocr_amd/csrc/train_enc.hip.h (`drop_keep`) and the site numbers of train_step.hip.h (`drop_site`), restated
   bit for bit; tests/test_train_ref_host.py checks the restatement's statistics.
2. `DroppedOracle`: the float64 oracle (oracle/conformer_ref.py) with those masks installed at the reference's six dropout sites;
   tests/golden/tiny_train_drop.npz (the REFERENCE's own modules with the same masks) pins the placement.
3. `MediumOracle`: the same with every Linear / pointwise-conv product restating the step's 'medium' matmul precision (bf16-rounded operands
   in the forward, the weight gradient and the input gradient; everything else in the oracle's dtype).

Index conventions (read from the kernels): the five activation sites use the flat row-major index over (line, frame, channel) of the
(M, width) activation; the attention weights use ((line * heads + head) * T + query) * T + key -- k_attn_fwd / k_attn_bwd_rows / k_attn_bwd_cols
(`row * T + j`), k_attn_softmax / k_attn_softmax_bwd (`row * T + j` although the row stride of the buffer is Tk) and k_btranspose
(`(z * T + r) * T + c`).  In every case that is the row-major index of the tensor as the oracle holds it.
"""
from __future__ import annotations

import functools
import json
import os
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from conformer_ocr_amd import synth
from oracle.conformer_ref import Oracle

_M64 = (1 << 64) - 1
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_C1 = np.uint64(0xBF58476D1CE4E5B9)
_C2 = np.uint64(0x94D049BB133111EB)

# train_step.hip.h: enum DropSite, DROP_SITE_INPUT
DROP_SITE_INPUT = 1
DROP_FF_HIDDEN, DROP_FF_OUT, DROP_ATTN_WEIGHTS, DROP_ATTN_OUT, DROP_CONV_OUT = 2, 3, 4, 5, 6
SITE_KIND = {'ff_hidden': DROP_FF_HIDDEN, 'ff_out': DROP_FF_OUT, 'attn_weights': DROP_ATTN_WEIGHTS, 'attn_out': DROP_ATTN_OUT, 'conv_out': DROP_CONV_OUT}


def drop_site(l: int, kind: int, which: int = 0) -> int:
    """train_step.hip.h `drop_site`: block l, site kind, which = 0 / 1 for the block's first / second feed-forward module."""
    return 16 * l + kind + 8 * which


def drop_keep(seed: int, site: int, idx, p: float) -> np.ndarray:
    """train_enc.hip.h `drop_keep`: the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 (idx + 1) + (site << 48) modulo 2^64; its top 24
    bits times 2^-24, compared `>= p` in float32.  idx: any integer array; returns a bool array of its shape."""
    idx = np.asarray(idx).astype(np.uint64)
    z = np.full(idx.shape, int(seed) & _M64, dtype=np.uint64) + _GOLDEN * (idx + np.uint64(1))
    z = z + np.full(idx.shape, (int(site) << 48) & _M64, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * _C1
    z = (z ^ (z >> np.uint64(27))) * _C2
    z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)          # (24-bit integers: exact in float32)
    return u >= np.float32(p)


def drop_scale(p: float) -> float:
    """1 / (1 - p) computed in float32, as every kernel computes it."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def site_of(site: str, l: int = 0, which: int = 0) -> int:
    return DROP_SITE_INPUT if site == 'input' else drop_site(l, SITE_KIND[site], which)


def site_p(site: str, p4: Sequence[float]) -> float:
    """p4 = (input, feed_forward, attention, conv), the reference's four probabilities (encoder.py:144-147)."""
    return float({'input': p4[0], 'ff_hidden': p4[1], 'ff_out': p4[1], 'attn_weights': p4[2], 'attn_out': p4[2], 'conv_out': p4[3]}[site])


def drop_factor(shape, seed: int, site: int, p: float, dtype=torch.float64) -> torch.Tensor:
    """keep / (1 - p) over the row-major indices of a tensor of `shape`."""
    n = int(np.prod(shape))
    keep = drop_keep(seed, site, np.arange(n, dtype=np.uint64), p).reshape(tuple(shape))
    return torch.from_numpy(keep).to(dtype) * drop_scale(p)


class DroppedOracle(Oracle):
    """The oracle's train mode with the device's masks at the six sites."""

    def __init__(self, hp, state, p4, seed, dtype=torch.float64):
        super().__init__(hp, state, dtype)
        self.p4, self.seed = tuple(float(p) for p in p4), int(seed)

    def dropout(self, x, site, l=0, which=0):
        p = site_p(site, self.p4)
        if not self.training or p <= 0.0:
            return x
        return x * drop_factor(x.shape, self.seed, site_of(site, l, which), p, self.dtype)


# ---- 'medium' matmul precision: lin_fwd / lin_bwd_bf16 / lin_bwd of train_step.hip.h, restated ---------------------------------------------
def _rb(x: torch.Tensor) -> torch.Tensor:
    """fp32 value -> bf16 (nearest even) -> back: the device rounds the fp32 value it holds."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def medium_rules(Nc: int, Kr: int) -> Tuple[bool, bool]:
    """(forward on bf16 operands, input gradient on bf16 operands) of a Linear with Nc outputs and Kr inputs, as the code decides them:
    a Linear whose two dimensions are multiples of 8 runs lin_fwd's bf16 branch and lin_bwd_bf16 (both True).  Any other goes through
    `gemm`, which rounds its operands whenever both leading dimensions and the depth are multiples of 8: the forward's depth is Kr; the input
    gradient's is Nc padded to a multiple of 4.  The weight gradient is on bf16 operands in every case (its depth, the padded row count, is a
    multiple of 64 under 'medium', in `gemm` and in the split-K form alike) and the bias gradient sums the unrounded dY."""
    if Nc % 8 == 0 and Kr % 8 == 0:
        return True, True
    return Kr % 8 == 0, ((Nc + 3) // 4 * 4) % 8 == 0


class _MediumLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        fwd16, dx16 = medium_rules(w.shape[0], w.shape[1])
        ctx.dx16, ctx.has_b = dx16, b is not None
        ctx.save_for_backward(x, w)
        y = (_rb(x) @ _rb(w).t()) if fwd16 else x @ w.t()
        return y if b is None else y + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dyr = _rb(dy)
        dw = dyr.reshape(-1, w.shape[0]).t() @ _rb(x).reshape(-1, w.shape[1])
        dx = (dyr @ _rb(w)) if ctx.dx16 else dy @ w
        db = dy.reshape(-1, w.shape[0]).sum(0) if ctx.has_b else None
        return dx, dw, db


class MediumOracle(DroppedOracle):
    """DroppedOracle whose Linear / pointwise-conv products follow the step's 'medium' precision.  (The attention's own products stay exact:
    the step runs them in fp32 in both precisions.)"""

    def linear(self, x, w, b=None):
        return _MediumLinear.apply(x, w, b)


# ---- one training step through an oracle -------------------------------------------------------------------------------------------------------
def train_grads(o: Oracle, image, lens, targets):
    """Loss, probits, d loss / d parameter and the BatchNorm batch statistics of the reference's training step (model.py:119,129-142) through
    oracle `o` in train mode + torch autograd."""
    params = {k: v for k, v in o.w.items() if v.is_floating_point() and 'running_' not in k}
    for v in params.values():
        v.requires_grad_(True)
    probits, ol = o.forward_train(torch.from_numpy(image).to(o.dtype), torch.from_numpy(np.asarray(lens)))
    target = torch.tensor([c for s in targets for c in s], dtype=torch.long)
    tl = torch.tensor([len(s) for s in targets], dtype=torch.long)
    loss = torch.nn.functional.ctc_loss(torch.nn.functional.log_softmax(probits, -1).transpose(0, 1), target, ol.long(), tl,
                                        reduction='sum', zero_infinity=True)
    loss.backward()
    return float(loss.detach()), probits.detach().numpy(), {k: v.grad.numpy() for k, v in params.items()}, o.bn_batch_stats


def oracle_train_grads_dropped(hp, state, image, lens, targets, p4, seed, dtype=torch.float64):
    return train_grads(DroppedOracle(hp, state, p4, seed, dtype), image, lens, targets)


def oracle_train_grads_medium(hp, state, image, lens, targets, p4=(0.0, 0.0, 0.0, 0.0), seed=0, dtype=torch.float64):
    return train_grads(MediumOracle(hp, state, p4, seed, dtype), image, lens, targets)


def medium_e_ref(hp, state, image, lens, targets, p4=(0.0, 0.0, 0.0, 0.0), seed=0):
    """How far MediumOracle in float32 lands from MediumOracle in float64 -- the measure the 'medium' bounds of tests/test_hip_train_pin.py
    (E_REF, E_BN) are taken from.  Returns (e_ref, per-tensor e_ref, e_bn): per tensor max|g32 - g64| / max|g64| (tensors whose float64 gradient
    is zero -- the key projection's bias -- left out), e_ref its largest value, e_bn the largest absolute difference of the running statistics
    after the step."""
    _, p64, g64, bn64 = oracle_train_grads_medium(hp, state, image, lens, targets, p4, seed, torch.float64)
    _, _, g32, bn32 = oracle_train_grads_medium(hp, state, image, lens, targets, p4, seed, torch.float32)
    per = {k: float(np.abs(g32[k].astype(np.float64) - g64[k]).max() / np.abs(g64[k]).max()) for k in g64 if np.abs(g64[k]).max() > 1e-9}
    M = p64.shape[0] * p64.shape[1]
    r64, r32 = bn_running(state, bn64, M), bn_running(state, bn32, M)
    return max(per.values()), per, max(float(np.abs(r64[k] - r32[k]).max()) for k in r64)


def perturbed_state(state, rng: np.random.Generator):
    """A copy of the state with every parameter entry moved to its float32 neighbour above or below (one ulp, random sign): another float32
    evaluation of the same step, as a different summation order or split would be, in which other operands round to the other bf16 neighbour."""
    out = {}
    for k, v in state.items():
        v = np.asarray(v)
        if v.dtype == np.float32 and 'running_' not in k:
            v = np.nextafter(v, np.where(rng.integers(0, 2, v.shape) == 1, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        out[k] = v
    return out


def medium_e_ref_sampled(hp, state, image, lens, targets, p4=(0.0, 0.0, 0.0, 0.0), seed=0, runs=16, perturb_seed=0):
    """`medium_e_ref` per tensor over `runs` float32 evaluations instead of one: MediumOracle in float32 on `perturbed_state` copies against
    MediumOracle in float64 on the unperturbed state.  One float32 run is too small a sample of a late tensor's own error (whether an operand
    upstream of it rounds the other way is a rare event per run).  Returns (per tensor: the largest max|g32 - g64| / max|g64| over the runs,
    per run: {tensor: figure})."""
    _, _, g64, _ = oracle_train_grads_medium(hp, state, image, lens, targets, p4, seed, torch.float64)
    rng = np.random.default_rng(perturb_seed)
    each = []
    for _ in range(runs):
        _, _, g32, _ = oracle_train_grads_medium(hp, perturbed_state(state, rng), image, lens, targets, p4, seed, torch.float32)
        each.append({k: float(np.abs(g32[k].astype(np.float64) - g64[k]).max() / np.abs(g64[k]).max()) for k in g64 if np.abs(g64[k]).max() > 1e-9})
    return {k: max(r[k] for r in each) for k in each[0]}, each


def medium_e_ref_runs(hp, state, image, lens, targets, p4=(0.0, 0.0, 0.0, 0.0), seed=0, perturbed=2, perturb_seed=0):
    """[(e_ref, e_bn)] of 1 + `perturbed` float32 evaluations against ONE float64 one: the first is `medium_e_ref`'s own pair (the unperturbed
    state), the others run on `perturbed_state` copies.  For the larger models, where a float64 run per sample would cost seconds."""
    _, p64, g64, bn64 = oracle_train_grads_medium(hp, state, image, lens, targets, p4, seed, torch.float64)
    M = p64.shape[0] * p64.shape[1]
    r64 = bn_running(state, bn64, M)
    rng, out = np.random.default_rng(perturb_seed), []
    for i in range(1 + perturbed):
        _, _, g32, bn32 = oracle_train_grads_medium(hp, state if i == 0 else perturbed_state(state, rng), image, lens, targets, p4, seed, torch.float32)
        r32 = bn_running(state, bn32, M)
        out.append((max(float(np.abs(g32[k].astype(np.float64) - g64[k]).max() / np.abs(g64[k]).max()) for k in g64 if np.abs(g64[k]).max() > 1e-9),
                    max(float(np.abs(r64[k] - r32[k]).max()) for k in r64)))
    return out


def bn_running(state, bn: Dict[int, tuple], M: int) -> Dict[str, np.ndarray]:
    """The BatchNorm running statistics a step leaves: momentum 0.1, unbiased batch variance over the M = N T positions."""
    out = {}
    for l, (mu, var) in bn.items():
        p = f'encoder.layers.{l}.sequential.2.module.sequential.5.'
        out[p + 'running_mean'] = 0.9 * state[p + 'running_mean'].astype(np.float64) + 0.1 * mu.numpy().astype(np.float64)
        out[p + 'running_var'] = 0.9 * state[p + 'running_var'].astype(np.float64) + 0.1 * var.numpy().astype(np.float64) * M / (M - 1)
    return out


# ---- the cases and recorded figures of tests/test_hip_train_pin.py and tests/test_hip_train_shapes.py (here so that non-GPU tests can use them without the engine) -------------------
P4 = (0.1, 0.2, 0.3, 0.4)          # (input, feed_forward, attention, conv): four distinct values, as in tiny_train_drop.npz
DROP_SEED = 20240229
NO_DROP = (0.0, 0.0, 0.0, 0.0)

CASES = {
    # the reference's own fixture configuration (tiny_train.npz), ragged widths: tests/test_hip_train_full.py's 'tiny'
    'tiny': dict(hp=lambda: synth.hparams('tiny'), seed=4321, n=3, W=64, widths=[64, 37, 50], targets=[[3, 1, 4], [1, 5], [9, 2, 6, 5]]),
    # the shapes of test_medium_matmul_precision_stays_close_to_the_exact_step
    'cfg2x2_232': dict(hp=lambda: synth.hparams('cfg2', num_encoder_layers=2), seed=5, lines_seed=9, n=3, W=232, widths=[232, 137, 200],
                       targets=[[5, 9, 9, 3], [17], [2, 2, 40]]),
    # M = 750: the cfg2 Linears split their weight gradients over 32 x 64 rows (rp = 2048): splits 0..10 hold rows, split 11 46 rows and
    # padding, the rest zeros
    'cfg2x2_1000': dict(hp=lambda: synth.hparams('cfg2', num_encoder_layers=2), seed=5, lines_seed=23, n=3, W=1000, widths=[1000, 612, 333],
                        targets=[[5, 9, 9, 3], [17, 2], [2, 40, 7]]),
    # M = 2096 > 2048 (Mp = 4096; rp = 4096 over 32 splits: 128 rows each, the 17th holds 48 rows and padding, splits 18..32 are empty -- a last
    # split that holds rows is 'rows_full' below; 66 column-sum chunks of 32 rows: k_colsum_final4 / the deferred finals, both colsum_final16), frontend rows 8 x 524 x 16 = 67072 > 65536 (256-row chunks) and 8 x 262 x 8 = 16768 > 16384 (64-row chunks)
    'rows': dict(hp=lambda: synth.hparams('cfg2', num_encoder_layers=1, height=32), seed=31, lines_seed=32, n=8, W=1048,
                 widths=[1048, 700, 333, 1043, 64, 900, 517, 1000],
                 targets=[[5, 9, 9, 3], [17], [2, 2], [40, 7, 7], [1], [3, 1, 4, 1], [59, 26], [5, 35, 8]]),
    # M = 2000, just under 2048: EVERY split of every weight gradient holds rows and the last one is partly padding -- 32 splits of 64 rows (the
    # last: 16 rows), the frontend's output linear 16 splits of 128 (the last: 80), its pointwise conv 16000 rows in 32 splits of 512 (the last: 128)
    'rows_full': dict(hp=lambda: synth.hparams('cfg2', num_encoder_layers=1, height=32), seed=31, lines_seed=33, n=8, W=1000,
                      widths=[1000, 700, 333, 997, 64, 900, 517, 960],
                      targets=[[5, 9, 9, 3], [17], [2, 2], [40, 7, 7], [1], [3, 1, 4, 1], [59, 26], [5, 35, 8]]),
}

# ---- one case per kernel form that the model's dimensions select (tests/test_hip_train_shapes.py; what each one must keep selecting:
# SHAPE_PRE below).  One encoder block each, at most 75 output frames; heights other than 96 only shrink the frontend.
SHAPE_CASES = {
    # the reference's default model: row attention at dh = 36 with T = 75 > 64 (a lane walks two keys), D = 144 / ff = 576 / 2 D = 288 (partial
    # 128-wide tiles in every weight gradient), 32 conv channels, the <31> depthwise kernels with 144 of 256 lanes live
    'cfg1_1': dict(hp=lambda: synth.hparams('cfg1', num_encoder_layers=1), seed=41, n=3, W=300, widths=[300, 137, 222],
                   targets=[[5, 9, 9, 3], [17], [2, 2, 40]]),
    # dh = 72: the second pass of every `d += 64` loop of the row kernels, per-wave LDS rows of 72 floats
    'cfg1_h2': dict(hp=lambda: synth.hparams('cfg1', num_encoder_layers=1, num_attention_heads=2, height=32), seed=42, n=2, W=280, widths=[280, 171],
                    targets=[[5, 9, 9, 3], [17, 2]]),
    # dh = 18: the scalar path of the row kernels (dh % 4 != 0)
    'cfg1_h8': dict(hp=lambda: synth.hparams('cfg1', num_encoder_layers=1, num_attention_heads=8, height=32), seed=43, n=2, W=280, widths=[280, 171],
                    targets=[[5, 9, 9, 3], [17, 2]]),
    # dh = 32: batched attention with ONE 32-wide k-chunk; T = 70, Tk = 96, Rk = 160: every padded dimension is padded
    'h8': dict(hp=lambda: synth.hparams('cfg2', num_encoder_layers=1, num_attention_heads=8, height=32), seed=44, n=2, W=280, widths=[280, 171],
               targets=[[5, 9, 9, 3], [17, 2]]),
    # dh = 128, the largest head: batched attention with four k-chunks
    'h2': dict(hp=lambda: synth.hparams('cfg2', num_encoder_layers=1, num_attention_heads=2, height=32), seed=45, n=2, W=280, widths=[280, 171],
               targets=[[5, 9, 9, 3], [17, 2]]),
    # kernel 15 at D = 256: k_dw1d_rows<., 0> / k_dw1d_bwd_w<0> with every lane live; T = 35 = two 16-frame chunks and one of 3 frames, halos
    # of 7 frames crossing chunk and line ends
    'k15': dict(hp=lambda: synth.hparams('cfg2', num_encoder_layers=1, conv_kernel_size=15, height=32), seed=46, n=2, W=140, widths=[140, 93],
                targets=[[5, 9, 3], [17]]),
    # kernel 33 > 32: the flat depthwise kernels (forward, input gradient with flip = 1, tap gradient)
    'k33': dict(hp=lambda: synth.hparams('cfg2', num_encoder_layers=1, conv_kernel_size=33, height=32), seed=47, n=2, W=280, widths=[280, 171],
                targets=[[5, 9, 9, 3], [17, 2]]),
    # D = 512: two column blocks in the depthwise / column-sum / BatchNorm kernels, 8 heads of 64, 8 splits in the feed-forward weight gradients
    'd512k7': dict(hp=lambda: synth.hparams('cfg4', num_encoder_layers=1, conv_kernel_size=7, height=32), seed=48, n=2, W=140, widths=[140, 93],
                   targets=[[5, 9, 3], [17]]),
    # the full-step feed-forward residual (ffr = 1), expansion 2 (ff = 512), 97 classes (nclp = 100: k_pad_cols, scalar column sums k_colsum_partial<CS_ONE, float>, `gemm`'s own
    # rounding rule under 'medium')
    'nohalf97ff2': dict(hp=lambda: synth.hparams('cfg2', num_encoder_layers=1, half_step_residual=False, num_classes=97,
                                                 feed_forward_expansion_factor=2, height=32), seed=49, n=2, W=140, widths=[140, 93],
                        targets=[[5, 9, 3], [96]]),
    # D = 1024, the widest accepted: four column blocks, dh = 128, the frontend's output linear (1024, 16384) = 1024 tiles -> splits == 1 (the
    # weight gradient written directly), feed-forward (4096, 1024) -> 2 splits, F (C + 1) 4 = 65664 > 65536 bytes -> the flat tfc
    'widest': dict(hp=lambda: synth.hparams('cfg4', num_encoder_layers=1, encoder_dim=1024, num_attention_heads=8, subsampling_conv_channels=512,
                                            height=128, conv_kernel_size=15), seed=50, n=2, W=140, widths=[140, 93], targets=[[5, 9, 3], [17]]),
}
CASES.update(SHAPE_CASES)
MEDIUM_SHAPE_CASES = ('cfg1_1', 'd512k7', 'nohalf97ff2', 'widest')


def train_wg_splits(Nc: int, Kr: int) -> int:
    """train_step.hip.h `train_wg_splits`: `tiles = ceil_div(Nc, SPLITK_BM) * ceil_div(Kr, SPLITK_BN)` with 128 x 128 tiles,
    `max(1, min(32, 512 / tiles))`."""
    tiles = -(-Nc // 128) * -(-Kr // 128)
    return max(1, min(32, 512 // tiles))


def shape_facts(name) -> Dict[str, int]:
    """The dimensions train_plan (train_step.hip.h) derives for a case, from its hyper-parameters and padded width alone."""
    hp, W = CASES[name]['hp'](), CASES[name]['W']
    stages = {2: 1, 4: 2, 8: 3}[hp.subsampling_factor]
    down = lambda x: functools.reduce(lambda l, _: (l - 1) // 2 + 1, range(stages), x)          # (out_len1 per stride-2 stage)
    D, C, T, F = hp.encoder_dim, hp.subsampling_conv_channels, down(W), down(hp.height)
    f = dict(D=D, C=C, T=T, F=F, K=hp.conv_kernel_size, heads=hp.num_attention_heads, dh=D // hp.num_attention_heads, ncls=hp.num_classes,
             ff=hp.feed_forward_expansion_factor * D, Tk=(T + 31) // 32 * 32, Rk=(2 * T - 1 + 31) // 32 * 32, nclp=(hp.num_classes + 3) // 4 * 4,
             col_blocks=-(-D // 256), chunks=-(-T // 16), tfc_lds=F * (C + 1) * 4, half=bool(hp.half_step_residual))
    f.update(s_up=train_wg_splits(f['ff'], D), s_down=train_wg_splits(D, f['ff']), s_dd=train_wg_splits(D, D), s_glu=train_wg_splits(2 * D, D),
             s_out=train_wg_splits(D, C * F), s_dec=train_wg_splits(hp.num_classes, D), s_cc=train_wg_splits(C, C))
    return f


# What each case exists for, as a predicate over `shape_facts`: asserted by the GPU test before it runs and by tests/test_train_ref_host.py
# without a GPU, so that a later change of shapes cannot silently lose the branch.  The code lines: p.attn_gemm = dh % 32 == 0 and
# train_wg_splits (train_step.hip.h), `d += 64` / `(dh & 3) == 0` (k_attn_* of train_enc.hip.h), K == 31 / K <= 32 / else (conv_fwd, conv_bwd),
# ceil_div(D, 256) column blocks, the LDS test of `tfc`, ffr, `Nc % 4` (lin_bwd; `Train::colsum`, which picks k_colsum_partial's float / f32x4 form).
SHAPE_PRE = {
    'cfg1_1': lambda f: f['dh'] == 36 and f['dh'] % 32 != 0 and f['dh'] % 4 == 0 and f['T'] > 64 and f['K'] == 31 and f['D'] < 256
    and all(x % 128 != 0 for x in (f['D'], f['ff'], 2 * f['D'])) and all(x % 8 == 0 for x in (f['D'], f['ff'], f['C'], f['C'] * f['F'], f['ncls']))
    and (f['s_up'], f['s_down'], f['s_dd'], f['s_glu'], f['s_out'], f['s_dec'], f['s_cc']) == (32,) * 7,
    'cfg1_h2': lambda f: f['dh'] == 72 and f['dh'] > 64 and f['dh'] % 32 != 0 and f['dh'] % 4 == 0 and f['T'] > 64,
    'cfg1_h8': lambda f: f['dh'] == 18 and f['dh'] % 4 != 0 and f['dh'] % 32 != 0 and f['T'] > 64,
    'h8': lambda f: f['dh'] == 32 and f['dh'] % 32 == 0 and f['dh'] // 32 == 1 and f['T'] > 64 and (f['T'], f['Tk'], f['Rk']) == (70, 96, 160)
    and f['T'] < f['Tk'] and 2 * f['T'] - 1 < f['Rk'],
    'h2': lambda f: f['dh'] == 128 and f['dh'] % 32 == 0 and f['T'] > 64 and f['T'] < f['Tk'],
    'k15': lambda f: f['K'] != 31 and f['K'] <= 32 and f['D'] >= 256 and f['chunks'] == 3 and f['T'] % 16 != 0 and (f['K'] - 1) // 2 > f['T'] % 16,
    'k33': lambda f: f['K'] > 32,
    'd512k7': lambda f: f['D'] > 256 and f['col_blocks'] == 2 and f['dh'] == 64 and f['K'] != 31 and f['K'] <= 32
    and (f['s_up'], f['s_down'], f['s_dd'], f['s_glu'], f['s_out']) == (8, 8, 32, 16, 8),
    'nohalf97ff2': lambda f: not f['half'] and f['ff'] == 2 * f['D'] and f['ncls'] % 4 != 0 and f['nclp'] == 100 and f['ncls'] % 8 != 0 and f['nclp'] % 8 != 0,
    'widest': lambda f: f['D'] == 1024 and f['D'] > 256 and f['col_blocks'] == 4 and f['dh'] == 128 and f['dh'] % 32 == 0 and f['K'] != 31 and f['K'] <= 32
    and f['tfc_lds'] > 64 * 1024 and (f['s_out'], f['s_up'], f['s_down'], f['s_dd'], f['s_glu']) == (1, 2, 2, 8, 4),
}


def assert_shape_selects(name):
    f = shape_facts(name)
    assert SHAPE_PRE[name](f), (name, f)
    return f


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = CASES[name]
    hp = c['hp']()
    state = synth.make_state_dict(hp, seed=c['seed'], decoder_gain=1.0)
    image, lens = synth.make_lines(c['n'], hp.height, c['W'], seed=c.get('lines_seed', c['seed']), widths=c['widths'])
    return hp, state, image, lens, c['targets']


# e_ref per 'medium' case: max over the parameter tensors of max|g32 - g64| / max|g64|, g32 / g64 the gradients of MediumOracle run in float32 /
# float64 on the CPU (`medium_e_ref`; tensors whose float64 gradient is zero -- the key projection's bias -- excluded: they get the absolute
# floor).  The bound is 4 e_ref: the margin is for the device's other summation order and splits and for roundings that flip at a bf16 tie.
# E_BN: the same measure on the BatchNorm running statistics after the step (absolute: they are O(0.1 .. 1)); their bound is the suite's 1e-5
# plus 4 E_BN.  Keys: (case, dropout on).
E_BN = {('tiny', False): 7.8e-9, ('tiny', True): 2.6e-7, ('cfg2x2_232', False): 2.42e-4, ('cfg2x2_232', True): 1.14e-4,
        ('rows', False): 9.3e-6, ('rows', True): 1.96e-5,
        ('cfg1_1', False): 2.68e-5, ('d512k7', False): 1.00e-4, ('nohalf97ff2', False): 3.94e-5, ('widest', False): 1.18e-4}
E_REF = {('tiny', False): 5.11e-3, ('tiny', True): 1.04e-2, ('cfg2x2_232', False): 5.54e-3, ('cfg2x2_232', True): 1.03e-2,
         ('rows', False): 3.09e-3, ('rows', True): 2.88e-3,
         # (SHAPE_CASES; four float32 runs on states moved by one ulp give 4.1e-3 .. 5.2e-3, 6.3e-3 .. 8.1e-3, 4.6e-3 .. 6.1e-3, 6.1e-3 .. 8.1e-3)
         ('cfg1_1', False): 4.44e-3, ('d512k7', False): 5.97e-3, ('nohalf97ff2', False): 3.48e-3, ('widest', False): 4.85e-3}


def tiny_sampled_e_ref() -> Dict[str, float]:
    """tests/golden/tiny_medium_e_ref.json: `medium_e_ref_sampled` of 'tiny' without dropout (16 runs, perturb_seed 0), per tensor."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tiny_medium_e_ref.json')) as fp:
        return json.load(fp)['e_ref']
