#!/usr/bin/env python3
"""Cost of the distillation term.

    python tools/distill_rate.py [--iters 200] [--steps 20]

(a) `cocr_distill_loss` (with the gradient, accumulating into the CTC gradient as the training step calls it) next to `cocr_ctc_loss` on
    32 x 300 x 256 and 32 x 300 x 97 random logits: HIP-event medians per call (table upload + kernels), and the kernel's byte floor --
    two reads, one read-modify-write of N T C floats -- at 6.3 TB/s.
(b) ms per training step of the cfg2 shapes with two blocks (32 lines of 96 x 400 px, 'medium' products) with and without teacher logits
    (a random tensor: the teacher's own forward is the serving path, measured by bench.py).
Legs alternate in one process; medians.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conformer_ocr_amd import synth  # noqa: E402
from conformer_ocr_amd.engine import HipRecognizer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=200, help='timed calls per leg of (a)')
ap.add_argument('--steps', type=int, default=20, help='timed training steps per leg of (b)')
args = ap.parse_args()
HBM_BYTES_PER_S = 6.3e12


def med(xs):
    return float(np.median(xs))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r                                       # ms


out = {'a': [], 'b': {}}
eng = HipRecognizer(synth.hparams('tiny'), torch.device('cuda:0'), 'fp32')
g = np.random.default_rng(7)
for N, T, C in ((32, 300, 256), (32, 300, 97)):
    zs = torch.from_numpy((g.standard_normal((N, T, C)) * 4.0).astype(np.float32)).cuda()
    zt = torch.from_numpy((g.standard_normal((N, T, C)) * 4.0).astype(np.float32)).cuda()
    lens = np.full(N, T, dtype=np.int32)
    tl = np.full(N, 40, dtype=np.int32)
    tg = g.integers(1, C, int(tl.sum())).astype(np.int32)
    grad = torch.zeros_like(zs)
    for _ in range(5):                                                  # warm-up: rings, scratch, code objects
        eng.ctc_loss(zs, lens, tg, tl)
        eng.distill_loss(zs, zt, lens, 2.0, grad=grad, ctc_weight=0.5, kd_weight=0.5)
    torch.cuda.synchronize()
    t_ctc, t_kd, t_kd_loss = [], [], []
    for _ in range(args.iters):
        t_ctc.append(timed(lambda: eng.ctc_loss(zs, lens, tg, tl))[0])
        t_kd.append(timed(lambda: eng.distill_loss(zs, zt, lens, 2.0, grad=grad, ctc_weight=0.5, kd_weight=0.5))[0])
        t_kd_loss.append(timed(lambda: eng.distill_loss(zs, zt, lens, 2.0, with_grad=False))[0])
    nbytes = 4 * N * T * C * 4
    out['a'].append({'shape': [N, T, C], 'iters': args.iters, 'ctc_loss_ms_median': round(med(t_ctc), 4), 'distill_loss_ms_median': round(med(t_kd), 4),
                     'distill_loss_only_ms_median': round(med(t_kd_loss), 4),
                     'distill_loss_ms_p10_p90': [round(float(np.percentile(t_kd, q)), 4) for q in (10, 90)],
                     'byte_floor_ms': round(nbytes / HBM_BYTES_PER_S * 1e3, 5), 'bytes': nbytes})

hp = synth.hparams('cfg2', num_encoder_layers=2)
state = synth.make_state_dict(hp, seed=5, decoder_gain=1.0)
N, W = 32, 400
image, lens = synth.make_lines(N, hp.height, W, seed=9)
x = torch.from_numpy(image[:, 0]).cuda()
tl = [8] * N
tg = g.integers(1, hp.num_classes, sum(tl)).tolist()
tr = HipRecognizer(hp, torch.device('cuda:0'), 'fp32')
tr.load_state(state)
tr.train_begin('medium')
tz = torch.from_numpy((g.standard_normal((N, tr.out_len(W), hp.num_classes)) * 4.0).astype(np.float32)).cuda()
drop = (0.1, 0.1, 0.1, 0.1)
for i in range(3):
    tr.train_step(x, lens, tg, tl, dropout=drop, seed=i)
    tr.train_step(x, lens, tg, tl, dropout=drop, seed=i, teacher_logits=tz, tau=2.0, distill_weight=0.5)
t_plain, t_kd = [], []
for i in range(args.steps):
    t_plain.append(timed(lambda: tr.train_step(x, lens, tg, tl, dropout=drop, seed=i))[0])
    t_kd.append(timed(lambda: tr.train_step(x, lens, tg, tl, dropout=drop, seed=i, teacher_logits=tz, tau=2.0, distill_weight=0.5))[0])
out['b'] = {'model': 'cfg2, 2 blocks', 'batch': [N, hp.height, W], 'precision': 'medium', 'steps': args.steps,
            'train_step_ms_median': round(med(t_plain), 3), 'train_step_with_teacher_ms_median': round(med(t_kd), 3),
            'added_ms': round(med(t_kd) - med(t_plain), 3)}
print(json.dumps(out))
