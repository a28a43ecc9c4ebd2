#!/usr/bin/env python3
"""Time of one training step of the whole network (cocr_train_step + the optimizer step; fp32) and a short training run on synthetic text
lines:   python tools/train_bench.py [--config cfg2] [--batch 32] [--width 1200] [--steps 5] [--fit 0] [--optimizer KIND [--dec-steps N]]
--optimizer KIND (AdamW, Adam, SGD, RMSprop; --momentum M): the Trainer steps with that optimizer, and the optimizer step ALONE is timed
with HIP events next to the whole step -- `cocr_train_optim_step` of that kind and, alternating with it in the same process,
`cocr_train_adamw` (the kernel AdamW had before the general one), each on an engine of its own holding the gradients of a real step:
--optim-rounds rounds of --optim-reps back-to-back calls between two events; the median / least / largest round per call and the
bytes per second the median implies (4 n x (vectors read + vectors written), n = the parameter count).  --dec-steps N: the output layer
N steps ahead on both engines (`train_optim_restore`), the per-tensor bias corrections as after a frozen phase.
--fit K: K steps on text lines (conformer_ocr_amd.synth.make_text_lines) from random weights, printing the loss and the greedy CER of
the trained model against the ground truth every few steps (the inference path serves the trained weights after sync).
--accumulate K / --clip-norm X: the Trainer's gradient window.  --steps then counts optimizer steps (K calls each);
`ms_per_step` stays the time per call, `ms_per_optimizer_step` is K times that.  With --clip-norm the norm call ALONE is timed on the
gradient vector of the last real step, next to one optimizer step at the same n on an engine of its own, alternating: per call the span
between two HIP events around it and the host's wall time from the call to the end of its wait (the norm call waits for its result
by itself, the optimizer call is followed by a wait on the second event); median / least / largest of --optim-rounds x 5 calls."""
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
from conformer_ocr_amd.evaluate import ErrorRate  # noqa: E402
from conformer_ocr_amd.pred import PytorchRecognitionModel  # noqa: E402
from conformer_ocr_amd.train import Trainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--config', default='cfg2')
ap.add_argument('--layers', type=int, default=0)
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--width', type=int, default=1200)
ap.add_argument('--steps', type=int, default=5)
ap.add_argument('--fit', type=int, default=0)
ap.add_argument('--lr', type=float, default=1e-3)
ap.add_argument('--optimizer', default=None, choices=('AdamW', 'Adam', 'SGD', 'RMSprop'))
ap.add_argument('--momentum', type=float, default=0.9)
ap.add_argument('--dec-steps', type=int, default=0)
ap.add_argument('--optim-reps', type=int, default=50)
ap.add_argument('--optim-rounds', type=int, default=9)
ap.add_argument('--accumulate', type=int, default=1)
ap.add_argument('--clip-norm', type=float, default=None)
ap.add_argument('--matmul', default='highest', help="'highest' (exact fp32 products) or 'medium' (bf16-rounded operands, the reference's training setting)")
args = ap.parse_args()
kw = {'num_encoder_layers': args.layers} if args.layers else {}
hp = synth.hparams(args.config, **kw)
state = synth.make_state_dict(hp, seed=1, decoder_gain=1.0)
net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1,
                              codec=ascii_codec(hp.num_classes), compute_dtype='bf16' if hp.encoder_dim in (256, 512) else 'fp32')
net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
net = net.to('cuda:0').eval()
image, lens, texts, _ = synth.make_text_lines(args.batch, hp.height, args.width, seed=3)
batch = {'image': torch.from_numpy(image).cuda(), 'seq_lens': torch.from_numpy(lens), 'target': torch.tensor([c for t in texts for c in t]),
         'target_lens': torch.tensor([len(t) for t in texts])}
tr = Trainer(net, lr=args.lr, weight_decay=1e-2, warmup=10, matmul_precision=args.matmul, optimizer=args.optimizer or 'AdamW', momentum=args.momentum,
             **({'accumulate_grad_batches': args.accumulate, 'gradient_clip_val': args.clip_norm} if args.accumulate != 1 or args.clip_norm is not None else {}))
out = {'config': args.config, 'layers': hp.num_encoder_layers, 'batch': args.batch, 'width': args.width}
for _ in range(args.accumulate):
    tr.training_step(batch)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.steps * args.accumulate):
    loss = tr.training_step(batch)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / (args.steps * args.accumulate)
out.update(ms_per_step=round(dt * 1e3, 2), lines_per_s=round(args.batch / dt, 1), last_loss=loss)
if args.accumulate != 1 or args.clip_norm is not None:
    out.update(accumulate=args.accumulate, clip_norm=args.clip_norm, ms_per_optimizer_step=round(dt * args.accumulate * 1e3, 2),
               last_grad_norm=tr.last_grad_norm)
if args.clip_norm is not None:
    from conformer_ocr_amd.engine import HipRecognizer
    side = HipRecognizer(hp, torch.device('cuda', 0), 'fp32')
    side.load_state(state)
    side.train_begin()
    side.train_grad_buffer().copy_(tr.engine.train_grad_buffer())
    kind = args.optimizer or 'AdamW'
    g = tr.engine.train_grad_buffer()
    calls = {'grad_norm': lambda: tr.engine.grad_norm(g),
             f'train_optim_step[{kind}]': lambda: side.train_optim_step(kind, args.lr, weight_decay=1e-2, momentum=args.momentum if kind in ('SGD', 'RMSprop') else 0.0)}
    spans = {k: ([], []) for k in calls}
    for fn in calls.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.optim_rounds * 5):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            h0 = time.perf_counter()
            fn()
            e1.record()
            e1.synchronize()
            spans[name][1].append((time.perf_counter() - h0) * 1e6)
            spans[name][0].append(e0.elapsed_time(e1) * 1e3)
    rep = {'floats': g.numel()}
    for name, (dev, host) in spans.items():
        dev, host = sorted(dev), sorted(host)
        rep[name] = {'event_us_median': round(dev[len(dev) // 2], 2), 'event_us_min': round(dev[0], 2), 'event_us_max': round(dev[-1], 2),
                     'host_us_median': round(host[len(host) // 2], 2), 'host_us_min': round(host[0], 2), 'host_us_max': round(host[-1], 2)}
    out['norm_alone'] = rep
if args.optimizer:
    from conformer_ocr_amd.engine import HipRecognizer

    def optim_engine(eng_kind=None):
        eng = HipRecognizer(hp, torch.device('cuda', 0), 'fp32')
        eng.load_state(state)
        eng.train_begin()
        eng.train_grad_buffer().copy_(tr.engine.train_grad_buffer())           # the gradients of the last real step
        if args.dec_steps:                                                      # the Adam kinds' per-tensor bias corrections, as after a frozen phase
            eng.train_optim_restore('AdamW' if eng_kind is None else eng_kind, 0, args.dec_steps)
        return eng

    kind = args.optimizer
    mom = args.momentum if kind in ('SGD', 'RMSprop') else 0.0
    old_eng, new_eng = optim_engine(), optim_engine(kind)
    n = new_eng.train_grad_buffer().numel()
    # vectors of n floats the step reads + writes: P twice, G once, every slot it uses twice
    slots = {'AdamW': 2, 'Adam': 2, 'SGD': 1 if mom > 0 else 0, 'RMSprop': 2 if mom > 0 else 1}[kind]
    calls = {'cocr_train_adamw': lambda: old_eng.train_adamw(args.lr, weight_decay=1e-2),
             f'cocr_train_optim_step[{kind}]': lambda: new_eng.train_optim_step(kind, args.lr, weight_decay=1e-2, momentum=mom)}
    times = {k: [] for k in calls}
    for fn in calls.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.optim_rounds):
        for name, fn in calls.items():                                         # alternating: both see the same neighbours on the machine
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.optim_reps):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.optim_reps)
    rep = {'params': n, 'momentum': mom}
    for name, ts in times.items():
        ts = sorted(ts)
        nbytes = 4 * n * (3 + 2 * (2 if name == 'cocr_train_adamw' else slots))
        rep[name] = {'us_median': round(ts[len(ts) // 2], 2), 'us_min': round(ts[0], 2), 'us_max': round(ts[-1], 2), 'bytes': nbytes,
                     'GB_per_s': round(nbytes / ts[len(ts) // 2] / 1e3, 1)}
    out['optimizer_step'] = rep
if args.fit:
    hist = []
    for step in range(args.fit):
        loss = tr.training_step(batch)
        if step % max(1, args.fit // 8) == 0 or step == args.fit - 1:
            tr.sync_module()
            pred = net.predict_labels(batch['image'], batch['seq_lens'])
            cer = ErrorRate()
            cer.update([[r[0] for r in line] for line in pred], texts)
            hist.append({'step': step, 'loss': round(loss, 2), 'cer': round(cer.compute(), 4)})
    out['fit'] = hist
print(json.dumps(out))
