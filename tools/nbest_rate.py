#!/usr/bin/env python3
"""Rate of n-best decoding.

    python tools/nbest_rate.py [--iters 100] [--legs text_nbest16,text_ctc_beam]

ms per call on cfg2-shaped logits (32 x 300 x 128), beam 16: `cocr_ctc_beam_nbest` for nbest 1, 4 and 16 next to `cocr_ctc_beam`, and
the same with an order-3 n-gram model (8 classes) next to `cocr_ctc_beam_lm` -- HIP-event medians after warm-up, legs alternating in
one process.  Two kinds of logits: "random" (normal x 2.5, blank + 1.5: tools/lm_rate.py's; nearly every frame appends a label, so the
hypotheses exceed 255 labels and carry no score: the search, the trace and the records alone) and "text" (a label every four frames,
held for two, + 6 over normal noise: about 75 labels per hypothesis, every one scored).  The n-best call is the 1-best call's launches with the walk kernel's back-pointers in
global memory, plus one memset and ctc_nbest_kernel: nbest 1 against the 1-best call shows what the global back-pointer path and the
new kernel's fixed part cost together.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conformer_ocr_amd import synth  # noqa: E402
from conformer_ocr_amd.lm import build_lm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=100)
ap.add_argument('--legs', default='', help='comma-separated leg names to run alone (under a profiler: one kernel mix per run)')
args = ap.parse_args()

import torch  # noqa: E402
from conformer_ocr_amd.engine import HipRecognizer  # noqa: E402

N, T, C, BEAM = 32, 300, 128, 16
g = np.random.default_rng(7)
eng = HipRecognizer(synth.hparams('tiny'), torch.device('cuda:0'), 'fp32')
lens = np.full(N, T, dtype=np.int32)
x = (g.standard_normal((N, T, C)) * 2.5).astype(np.float32)
x[:, :, 0] += 1.5
y = g.standard_normal((N, T, C)).astype(np.float32)
path = np.zeros((N, T), dtype=np.int64)
path[:, 0::4] = path[:, 1::4] = g.integers(1, C, (N, T // 4))
np.put_along_axis(y, path[:, :, None], 6.0 + np.take_along_axis(y, path[:, :, None], 2), 2)
kinds = {'random': torch.from_numpy(x).cuda(), 'text': torch.from_numpy(y).cuda()}
P = g.dirichlet(np.full(C - 1, 0.3), size=C - 1)
corpus = []
for _ in range(2000):
    s = [int(g.integers(1, C))]
    for _ in range(49):
        s.append(1 + int(g.choice(C - 1, p=P[s[-1] - 1])))
    corpus.append(s)
lm = build_lm(corpus, 3, C)


def timed(fn, collect):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    h = fn()
    e1.record()
    e1.synchronize()
    collect(h)
    return e0.elapsed_time(e1)                                           # ms


legs = {}
for kind, logits in kinds.items():
    legs[f'{kind}_ctc_beam'] = (lambda logits=logits: eng.ctc_beam_async(logits, lens, BEAM), eng.collect)
    legs[f'{kind}_ctc_beam_lm'] = (lambda logits=logits: eng.ctc_beam_lm_async(logits, lens, lm, BEAM, 8, 0.5, 0.0), eng.collect)
    for k in (1, 4, 16):
        legs[f'{kind}_nbest{k}'] = (lambda k=k, logits=logits: eng.ctc_beam_nbest_async(logits, lens, BEAM, k), eng.collect_nbest)
        legs[f'{kind}_nbest{k}_lm'] = (lambda k=k, logits=logits: eng.ctc_beam_nbest_async(logits, lens, BEAM, k, lm, 8, 0.5, 0.0), eng.collect_nbest)
if args.legs:
    legs = {k: legs[k] for k in args.legs.split(',')}
for fn, collect in legs.values():
    for _ in range(3):
        timed(fn, collect)
ts = {k: [] for k in legs}
for _ in range(args.iters):
    for k, (fn, collect) in legs.items():
        ts[k].append(timed(fn, collect))
out = {k + '_ms_median': round(float(np.median(v)), 4) for k, v in ts.items()}
out.update({k + '_ms_p10_p90': [round(float(np.percentile(v, q)), 4) for q in (10, 90)] for k, v in ts.items()})
for kind, logits in kinds.items():
    out[kind + '_labels_per_hypothesis_mean'] = round(float(np.mean([len(h[0]) for hs in eng.ctc_beam_nbest(logits, lens, BEAM, 16) for h in hs])), 1)
print(json.dumps(dict(out, shape=[N, T, C], beam=BEAM, lm_order=3, classes=8, iters=args.iters)))
