#!/usr/bin/env python3
"""Rate of text-to-page alignment.

    python tools/page_align_rate.py [--iters 50] [--pages 16] [--reps 3] [--skip-pages] [--skip-host]

(a) `cocr_ctc_align_page` on one page of 40 lines x 300 frames x 128 classes with 2 000 labels (a planted page as the tests plant it: the
    text cut into the lines at spaces that are then not shown): HIP-event medians per call (table upload + kernel), next to ONE
    `cocr_ctc_align` call on the same 40 lines with the labels the page puts on each (the per-line problem, were the breaks known),
    and next to the host definition `align.viterbi_align_page` (one run).
(b) lines/s of `align.align_text_pages` next to `align.align_pages` on tools/page_rate.py's synthetic pages cut into halves of 20 lines
    (cfg2 text model, bf16), every half page aligned to the space-joined strings its lines were read as.
Legs alternate in one process; medians.  Kernel time alone: run under `rocprofv3 --kernel-trace --stats` and read
ctc_align_page_kernel.  Prints one JSON line."""
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
from conformer_ocr_amd.align import align_pages, align_text_pages, viterbi_align_page  # noqa: E402
from conformer_ocr_amd.engine import HipRecognizer  # noqa: E402
from tests.test_hip_align_page import _planted_page  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=50, help='timed calls per leg of (a)')
ap.add_argument('--pages', type=int, default=16)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--skip-pages', action='store_true', help='leg (a) only')
ap.add_argument('--skip-host', action='store_true', help='leg (a) without the host definition')
args = ap.parse_args()


def med(xs):
    return float(np.median(xs))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, r                                 # us


# ---- (a) the kernel
K, T, C, L = 40, 300, 128, 2000
logits_h, lens, labels, optional, want = _planted_page(K, T, C, L, np.random.default_rng(7))
eng = HipRecognizer(synth.hparams('tiny'), torch.device('cuda:0'), 'fp32')
logits = torch.from_numpy(logits_h).cuda()
rows = [list(range(K))]
per_line = [[int(labels[i]) for i in range(L) if want[i][0] == k] for k in range(K)]
flat, flat_lens = [l for ln in per_line for l in ln], [len(ln) for ln in per_line]


def leg_page():
    return eng.ctc_align_page_async(logits, lens, rows, [labels], [optional])


def leg_lines():
    return eng.ctc_align_async(logits, lens, flat, flat_lens)


for _ in range(3):                                                      # warm-up: rings, workspace, code objects
    got = eng.collect_align_page(leg_page())
    eng.collect_align(leg_lines())
torch.cuda.synchronize()
t_page, t_lines = [], []
for _ in range(args.iters):
    t, h = timed(leg_page)
    t_page.append(t)
    eng.collect_align_page(h)
    t, h = timed(leg_lines)
    t_lines.append(t)
    eng.collect_align(h)
out = {'a': {'shape': [K, T, C], 'labels': L, 'spaces_dropped_at_breaks': sum(1 for w in want if w[0] < 0), 'iters': args.iters,
             'path_is_the_planted_one': [r[1:4] for r in got[0][0]] == want,
             'ctc_align_page_us_median': round(med(t_page), 1), 'ctc_align_40_lines_us_median': round(med(t_lines), 1),
             'ctc_align_page_us_p10_p90': [round(float(np.percentile(t_page, q)), 1) for q in (10, 90)],
             'ctc_align_40_lines_us_p10_p90': [round(float(np.percentile(t_lines, q)), 1) for q in (10, 90)],
             'page_time_over_lines_time': round(med(t_page) / med(t_lines), 2),
             'us_per_frame': round(med(t_page) / (K * T), 4)}}
if not args.skip_host:
    t0 = time.perf_counter()
    viterbi_align_page([logits_h[k, :lens[k]].T for k in range(K)], labels, optional)
    out['a']['host_viterbi_align_page_s'] = round(time.perf_counter() - t0, 3)

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
    # half pages of 20 lines (about 2 200 labels): a whole one of these pages has more labels than the kernel holds (4 095) and would
    # go through the host definition
    pages = [(img, lines[h:h + 20]) for i in range(args.pages) for img, lines in [distinct[i % 4]] for h in range(0, len(lines), 20)]
    read = recognize_pages(net, pages)                                  # warm-up; the strings the pages are aligned to
    with_text = [(img, [Line(l.id, l.baseline, l.boundary, r['text']) for l, r in zip(lines, recs)]) for (img, lines), recs in zip(pages, read)]
    texts = [' '.join(r['text'] for r in recs) for recs in read]
    got = align_text_pages(net, pages, texts)
    from conformer_ocr_amd.align import MAX_PAGE_LABELS, encode_text
    labels_per_page = [len(encode_text(net.codec, t)[0]) for t in texts]
    nlines = sum(len(l) for _, l in pages)
    same = sum(a['text'] == r['text'] for res, recs in zip(got, read) if res['lines'] is not None for a, r in zip(res['lines'], recs))

    def leg(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return nlines / (time.perf_counter() - t0)
    rates = {'align_pages': [], 'align_text_pages': []}
    for _ in range(args.reps):
        rates['align_pages'].append(leg(lambda: align_pages(net, with_text)))
        rates['align_text_pages'].append(leg(lambda: align_text_pages(net, pages, texts)))
    m = {k: med(v) for k, v in rates.items()}
    out['b'] = {'pages': len(pages), 'lines': nlines, 'labels_per_page_max': max(labels_per_page),
                'pages_through_the_host_definition': sum(n > MAX_PAGE_LABELS for n in labels_per_page), 'lines_with_the_string_they_were_read_as': int(same),
                'align_pages_lines_per_s': round(m['align_pages'], 1), 'align_text_pages_lines_per_s': round(m['align_text_pages'], 1),
                'text_rate_over_line_rate': round(m['align_text_pages'] / m['align_pages'], 3),
                'raw': {k: [round(x, 1) for x in v] for k, v in rates.items()}}
print(json.dumps(out))
