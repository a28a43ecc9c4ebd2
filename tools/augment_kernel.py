#!/usr/bin/env python3
"""The augmentation kernel alone at a batch shape, for `rocprofv3 --kernel-trace --stats`:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/augment_kernel.py [--n 32] [--h 96] [--w 1200] [--calls 50]

Runs `--calls` launches with the default parameter draw (half the lines untouched) and `--calls` with every stage on for every line,
on a text-line batch; prints the host-side time per call."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_ocr_amd import synth  # noqa: E402
from conformer_ocr_amd.augment import AugmentConfig, draw, line_keys  # noqa: E402
from conformer_ocr_amd.engine import HipRecognizer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--n', type=int, default=32)
ap.add_argument('--h', type=int, default=96)
ap.add_argument('--w', type=int, default=1200)
ap.add_argument('--calls', type=int, default=50)
args = ap.parse_args()
eng = HipRecognizer(synth.hparams('tiny'), torch.device('cuda:0'), 'fp32')
image, lens, _, _ = synth.make_text_lines(args.n, args.h, args.w, seed=3)
x = torch.from_numpy(synth.lines_u8(image)[:, 0].copy()).cuda()
out = torch.empty_like(x)
sl = lens.astype(np.int32)
res = {'shape': [args.n, args.h, args.w]}
for name, cfg in (('default', AugmentConfig()), ('all_stages', AugmentConfig(p=1.0, p_geometry=1.0, p_elastic=1.0, p_blur=1.0, p_dropout=1.0))):
    tables = [draw(line_keys(0, e, np.arange(args.n)), sl, args.h, args.w, cfg) for e in range(args.calls)]
    eng.augment(x, sl, *tables[0], out=out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p, g in tables:
        eng.augment(x, sl, p, g, out=out)
    torch.cuda.synchronize()
    res[name + '_ms_per_call'] = round((time.perf_counter() - t0) / args.calls * 1e3, 4)
print(json.dumps(res))
