#!/usr/bin/env python3
"""Rate of the ground-truth training loop: synthetic pages of `synth.make_text_lines` lines pasted along straight
and rotated baselines (tests/page_synth.py), written as PNG + PAGE XML into a temporary directory, loaded by `GroundTruthDataset`, and
trained by the loop of `train.fit` (batches -> [augment] -> Trainer.training_step) at cfg2 shapes: 32 lines of 1168 px (+ 2 x 16 pad =
1200: every batch is 32 x 96 x 1200).

    python tools/gt_train_rate.py [--pages 8] [--epochs 3] [--reps 3] [--layers 0] [--matmul medium]

Prints, per leg, ms per step and lines/s of the training phase of an epoch, with augmentation off and on (alternating in one process),
and next to them the step of tools/train_bench.py (one fixed float32 batch of the same shape, `Trainer.training_step`) and the time of the
augmentation call alone (host draw + upload + kernel, HIP events).  Kernel time alone: run under `rocprofv3 --kernel-trace --stats` and
read augment_kernel."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conformer_ocr_amd import synth  # noqa: E402
from conformer_ocr_amd.augment import AugmentConfig, draw, line_keys  # noqa: E402
from conformer_ocr_amd.codec import ascii_codec  # noqa: E402
from conformer_ocr_amd.dataset import GroundTruthDataset  # noqa: E402
from conformer_ocr_amd.pred import PytorchRecognitionModel  # noqa: E402
from conformer_ocr_amd.train import Trainer  # noqa: E402
from tests import gt_synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--pages', type=int, default=8, help='pages of 8 lines each')
ap.add_argument('--epochs', type=int, default=3, help='epochs per leg and repetition')
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--layers', type=int, default=0, help='encoder blocks (0: the config\'s 12)')
ap.add_argument('--matmul', default='medium')
args = ap.parse_args()

kw = {'num_encoder_layers': args.layers} if args.layers else {}
with tempfile.TemporaryDirectory() as d:
    pages = gt_synth.make_pages(d, formats=['page'] * args.pages, lines_per_page=8, width=1168, kinds=[('line', 0.0), ('line', 1.5), ('line', -1.5)])
    data = GroundTruthDataset([x for x, _, _ in pages], evaluation_files=[pages[0][0]], format_type='xml', batch_size=32, edge=200, seed=1)
hp = synth.hparams('cfg2', num_classes=max(data.codec.max_label + 1, 2), **kw)
net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1,
                              codec=data.codec, compute_dtype='bf16')
state = synth.make_state_dict(hp, seed=1, decoder_gain=1.0)
net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
net = net.to('cuda:0').eval()
tr = Trainer(net, lr=1e-4, weight_decay=1e-2, warmup=10, matmul_precision=args.matmul)
shapes = sorted({(len(idx), w) for w, idx in data.plan(0)})

# train_bench.py's step: one fixed float32 batch of the same shape
image, lens, texts, _ = synth.make_text_lines(32, hp.height, 1200, seed=3)
fixed = {'image': torch.from_numpy(image).cuda(), 'seq_lens': torch.from_numpy(lens), 'target': torch.tensor([c for t in texts for c in t]),
         'target_lens': torch.tensor([len(t) for t in texts])}


def fit_phase(augment: bool, epoch0: int):
    data.augment = augment
    torch.cuda.synchronize()
    t0, steps, lines = time.perf_counter(), 0, 0
    for e in range(epoch0, epoch0 + args.epochs):
        for batch in data.batches(e):
            tr.training_step(batch)
            steps += 1
            lines += int(batch['image'].shape[0])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt / steps * 1e3, lines / dt


def bench_step(n: int):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        tr.training_step(fixed)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def augment_call(reps: int = 20):
    w, idx = data.plan(0)[0]
    im, sl = data._images(idx, w)
    cfg = AugmentConfig()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for r in range(reps):
        p, g = draw(line_keys(1, r, data.uids[idx]), sl, data.height, w, cfg)
        data.engine.augment(im, sl, p, g)
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, e0.elapsed_time(e1) / reps


fit_phase(False, 0)                   # warm-up: workspaces, pinned pools, the first augmentation tables
fit_phase(True, 0)
bench_step(2)
res = {'off': [], 'on': [], 'train_bench': []}
epoch = 1
for r in range(args.reps):
    for leg in ('off', 'on'):
        res[leg].append(fit_phase(leg == 'on', epoch))
        epoch += args.epochs
    res['train_bench'].append(bench_step(2 * args.epochs))
host_ms, dev_ms = augment_call()
off = float(np.median([m for m, _ in res['off']]))
on = float(np.median([m for m, _ in res['on']]))
tb = float(np.median(res['train_bench']))
print(json.dumps({
    'shapes': shapes, 'layers': hp.num_encoder_layers, 'matmul': args.matmul, 'lines': data.n_train,
    'fit_no_augment_ms_per_step': round(off, 2), 'fit_no_augment_lines_per_s': round(float(np.median([l for _, l in res['off']])), 1),
    'fit_augment_ms_per_step': round(on, 2), 'fit_augment_lines_per_s': round(float(np.median([l for _, l in res['on']])), 1),
    'train_bench_ms_per_step': round(tb, 2),
    'augment_share_of_step': round((on - off) / on, 4), 'fit_vs_train_bench': round(off / tb - 1.0, 4),
    'augment_call_host_ms': round(host_ms, 3), 'augment_call_event_ms': round(dev_ms, 3),
    'raw': {k: [[round(x, 2) for x in (v if isinstance(v, tuple) else (v,))] for v in vs] for k, vs in res.items()},
}))
