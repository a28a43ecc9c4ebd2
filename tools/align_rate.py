#!/usr/bin/env python3
"""Rate of forced alignment.

    python tools/align_rate.py [--iters 200] [--host-sample 4] [--pages 16] [--reps 3] [--skip-pages]

(a) `cocr_ctc_align` on 32 x 300 x 128 random logits with 25 - 60 labels per line: HIP-event medians per call (label upload + kernel),
    next to `cocr_ctc_loss` called for the loss only on the same logits and targets, and next to the host definition
    `align.viterbi_align` on a SAMPLE of the lines, scaled to lines/s.
(b) lines/s of `align.align_pages` next to `page.recognize_pages` on tools/page_rate.py's synthetic pages (cfg2 text model, bf16), every
    line aligned to the string it was read as.
Legs alternate in one process; medians.  Kernel time alone: run under `rocprofv3 --kernel-trace --stats` and read ctc_align_kernel.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from conformer_ocr_amd import synth  # noqa: E402
from conformer_ocr_amd.align import align_pages, viterbi_align  # noqa: E402
from conformer_ocr_amd.engine import HipRecognizer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=200, help='timed calls per leg of (a)')
ap.add_argument('--host-sample', type=int, default=4, help='lines the host leg of (a) aligns (scaled)')
ap.add_argument('--pages', type=int, default=16)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--skip-pages', action='store_true', help='leg (a) only')
args = ap.parse_args()


def med(xs):
    return float(np.median(xs))


# ---- (a) the kernel
N, T, C = 32, 300, 128
g = np.random.default_rng(7)
logits_h = (g.standard_normal((N, T, C)) * 2.0).astype(np.float32)
label_lens = g.integers(25, 61, N)
targets = np.concatenate([g.integers(1, C, l) for l in label_lens])
out_lens = np.full(N, T, dtype=np.int32)
eng = HipRecognizer(synth.hparams('tiny'), torch.device('cuda:0'), 'fp32')
logits = torch.from_numpy(logits_h).cuda()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, r                                 # us


def leg_align():
    return eng.collect_align(eng.ctc_align_async(logits, out_lens, targets, label_lens))


def leg_loss():
    return eng.ctc_loss(logits, out_lens, targets, label_lens, with_grad=False)


for _ in range(5):                                                      # warm-up: rings, code objects
    leg_align(), leg_loss()
torch.cuda.synchronize()
t_align, t_loss = [], []
for _ in range(args.iters):
    t_align.append(timed(lambda: eng.ctc_align_async(logits, out_lens, targets, label_lens))[0])
    t_loss.append(timed(leg_loss)[0])
t0 = time.perf_counter()
off = np.concatenate([[0], np.cumsum(label_lens)])
for n in range(args.host_sample):
    viterbi_align(logits_h[n].T, targets[off[n]:off[n + 1]])
host_rate = args.host_sample / (time.perf_counter() - t0)
out = {'a': {'shape': [N, T, C], 'labels_per_line': [int(label_lens.min()), int(label_lens.max())], 'iters': args.iters,
             'ctc_align_us_median': round(med(t_align), 1), 'ctc_loss_nograd_us_median': round(med(t_loss), 1),
             'ctc_align_us_p10_p90': [round(float(np.percentile(t_align, q)), 1) for q in (10, 90)],
             'ctc_loss_nograd_us_p10_p90': [round(float(np.percentile(t_loss, q)), 1) for q in (10, 90)],
             'align_time_over_loss': round(med(t_align) / med(t_loss), 3),
             'device_lines_per_s': round(N / (med(t_align) * 1e-6), 1),
             'host_viterbi_lines_per_s_scaled_from_sample': round(host_rate, 1)}}

# ---- (b) pages
if not args.skip_pages:
    import bench
    from page_rate import make_page
    from conformer_ocr_amd.codec import ascii_codec
    from conformer_ocr_amd.page import Line, recognize_pages
    from conformer_ocr_amd.pred import PytorchRecognitionModel
    fix = bench.load_text_fixture('cfg2_text')
    hp = fix['hp']
    net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1,
                                  codec=ascii_codec(hp.num_classes), compute_dtype='bf16')
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fix['state'].items()})
    net = net.to('cuda:0').eval()
    lines_u8 = [np.rint(np.asarray(ln, dtype=np.float32)[::2, :1100:2].repeat(2, axis=1) * 255.0).astype(np.uint8) for ln in fix['lines']]
    distinct = [make_page(lines_u8, s) for s in range(4)]
    pages = [distinct[i % 4] for i in range(args.pages)]
    read = recognize_pages(net, pages)                                  # warm-up; the strings the lines are aligned to
    with_text = [(img, [Line(l.id, l.baseline, l.boundary, r['text']) for l, r in zip(lines, recs)]) for (img, lines), recs in zip(pages, read)]
    got = align_pages(net, with_text)
    nlines = sum(len(l) for _, l in pages)
    same = sum([(c, q) for c, q, _ in a['cuts'] or ()] == [(c, q) for c, q, _ in r['cuts']] for ap_, rp in zip(got, read) for a, r in zip(ap_, rp))

    def leg(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return nlines / (time.perf_counter() - t0)
    rates = {'recognize_pages': [], 'align_pages': []}
    for _ in range(args.reps):
        rates['recognize_pages'].append(leg(lambda: recognize_pages(net, pages)))
        rates['align_pages'].append(leg(lambda: align_pages(net, with_text)))
    m = {k: med(v) for k, v in rates.items()}
    out['b'] = {'pages': args.pages, 'lines': nlines, 'lines_with_the_cuts_of_recognize_pages': int(same),
                'recognize_pages_lines_per_s': round(m['recognize_pages'], 1), 'align_pages_lines_per_s': round(m['align_pages'], 1),
                'align_rate_over_recognize_rate': round(m['align_pages'] / m['recognize_pages'], 3),
                'raw': {k: [round(x, 1) for x in v] for k, v in rates.items()}}
print(json.dumps(out))
