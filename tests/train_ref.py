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


def bn_running(state, bn: Dict[int, tuple], M: int) -> Dict[str, np.ndarray]:
    """The BatchNorm running statistics a step leaves: momentum 0.1, unbiased batch variance over the M = N T positions."""
    out = {}
    for l, (mu, var) in bn.items():
        p = f'encoder.layers.{l}.sequential.2.module.sequential.5.'
        out[p + 'running_mean'] = 0.9 * state[p + 'running_mean'].astype(np.float64) + 0.1 * mu.numpy().astype(np.float64)
        out[p + 'running_var'] = 0.9 * state[p + 'running_var'].astype(np.float64) + 0.1 * var.numpy().astype(np.float64) * M / (M - 1)
    return out


# ---- the cases and recorded figures of tests/test_hip_train_pin.py (here so that non-GPU tests can use them without the engine) -------------------
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
    # split that holds rows is 'rows_full' below; 66 column-sum chunks of 32 rows: k_colsum_final4), frontend rows 8 x 524 x 16 = 67072 > 65536 (256-row chunks) and 8 x 262 x 8 = 16768 > 16384 (64-row chunks)
    'rows': dict(hp=lambda: synth.hparams('cfg2', num_encoder_layers=1, height=32), seed=31, lines_seed=32, n=8, W=1048,
                 widths=[1048, 700, 333, 1043, 64, 900, 517, 1000],
                 targets=[[5, 9, 9, 3], [17], [2, 2], [40, 7, 7], [1], [3, 1, 4, 1], [59, 26], [5, 35, 8]]),
    # M = 2000, just under 2048: EVERY split of every weight gradient holds rows and the last one is partly padding -- 32 splits of 64 rows (the
    # last: 16 rows), the frontend's output linear 16 splits of 128 (the last: 80), its pointwise conv 16000 rows in 32 splits of 512 (the last: 128)
    'rows_full': dict(hp=lambda: synth.hparams('cfg2', num_encoder_layers=1, height=32), seed=31, lines_seed=33, n=8, W=1000,
                      widths=[1000, 700, 333, 997, 64, 900, 517, 960],
                      targets=[[5, 9, 9, 3], [17], [2, 2], [40, 7, 7], [1], [3, 1, 4, 1], [59, 26], [5, 35, 8]]),
}


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
        ('rows', False): 9.3e-6, ('rows', True): 1.96e-5}
E_REF = {('tiny', False): 5.11e-3, ('tiny', True): 1.04e-2, ('cfg2x2_232', False): 5.54e-3, ('cfg2x2_232', True): 1.03e-2,
         ('rows', False): 3.09e-3, ('rows', True): 2.88e-3}


def tiny_sampled_e_ref() -> Dict[str, float]:
    """tests/golden/tiny_medium_e_ref.json: `medium_e_ref_sampled` of 'tiny' without dropout (16 runs, perturb_seed 0), per tensor."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tiny_medium_e_ref.json')) as fp:
        return json.load(fp)['e_ref']
