#!/usr/bin/env python3
"""Cost of the two phases of a fine-tune in one process: ms per FROZEN step (eval-mode forward on the bf16 serving
engine, CTC gradient, decoder backward, AdamW on the output layer) and per WHOLE-NETWORK step (`Trainer.training_step` as
tools/train_bench.py times it; matmul precision 'medium') on one fixed batch of 32 x 96 x 1200 at cfg2 shapes (12 blocks), and the
duration of the hand-over call (`cocr_train_adopt_decoder`) from HIP events.

    python tools/finetune_rate.py [--steps 10] [--reps 3] [--layers 0] [--matmul medium]

The legs alternate; the figures are medians over `--reps` repetitions.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_ocr_amd import synth  # noqa: E402
from conformer_ocr_amd.codec import ascii_codec  # noqa: E402
from conformer_ocr_amd.pred import PytorchRecognitionModel  # noqa: E402
from conformer_ocr_amd.train import Trainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=10, help='steps per leg and repetition')
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--layers', type=int, default=0, help='encoder blocks (0: the config\'s 12)')
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--width', type=int, default=1200)
ap.add_argument('--matmul', default='medium')
args = ap.parse_args()

hp = synth.hparams('cfg2', **({'num_encoder_layers': args.layers} if args.layers else {}))
state = synth.make_state_dict(hp, seed=1, decoder_gain=1.0)


def model():
    net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1,
                                  codec=ascii_codec(hp.num_classes), compute_dtype='bf16')
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return net.to('cuda:0').eval()


image, lens, texts, _ = synth.make_text_lines(args.batch, hp.height, args.width, seed=3)
batch = {'image': torch.from_numpy(image).cuda(), 'seq_lens': torch.from_numpy(lens), 'target': torch.tensor([c for t in texts for c in t]),
         'target_lens': torch.tensor([len(t) for t in texts])}
legs = {'frozen': Trainer(model(), lr=1e-4, weight_decay=1e-2, warmup=10, matmul_precision=args.matmul, freeze_backbone=10 ** 12),
        'full': Trainer(model(), lr=1e-4, weight_decay=1e-2, warmup=10, matmul_precision=args.matmul)}


def leg(name: str, n: int) -> float:
    tr = legs[name]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        tr.training_step(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


for name in legs:                        # warm-up: workspaces, the captured forward, the optimizer state
    leg(name, 2)
res = {name: [] for name in legs}
for _ in range(args.reps):
    for name in legs:
        res[name].append(leg(name, args.steps))

# the hand-over: the frozen leg's output layer (master copy, moments, step count) into its own whole-network state
tr = legs['frozen']
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
adopt = []
for _ in range(5):
    torch.cuda.synchronize()
    e0.record()
    tr.engine.train_adopt_decoder(tr.net._engine)
    e1.record()
    torch.cuda.synchronize()
    adopt.append(e0.elapsed_time(e1))
frozen, full = float(np.median(res['frozen'])), float(np.median(res['full']))
print(json.dumps({'layers': hp.num_encoder_layers, 'batch': args.batch, 'width': args.width, 'matmul': args.matmul,
                  'frozen_ms_per_step': round(frozen, 3), 'full_ms_per_step': round(full, 3), 'full_over_frozen': round(full / frozen, 2),
                  'frozen_is_faster': frozen < full, 'adopt_decoder_event_ms': round(float(np.median(adopt)), 4),
                  'raw': {k: [round(x, 3) for x in v] for k, v in res.items()}, 'adopt_raw_ms': [round(x, 4) for x in adopt]}))
