#!/usr/bin/env python3
"""Rate of keyword spotting.

    python tools/search_rate.py [--iters 200] [--host-sample 2] [--pages 16] [--reps 3] [--skip-pages]

(a) `cocr_ctc_spot` on 32 x 300 x 128 random logits with Q = 16 queries of 4 - 12 labels, 4 hits each: HIP-event medians per call (table
    upload + kernel), next to 16 `cocr_ctc_align` calls on the same logits (one per query, the query as every line's labels: the nearest
    thing the library offered before), and next to the host definition `search.spot_host` on a SAMPLE of the lines, scaled to
    (line, query) pairs/s.
(b) lines/s of `search.search_pages` (16 queries cut from the pages' own reading) next to `page.recognize_pages` on tools/page_rate.py's
    synthetic pages (cfg2 text model, bf16).
Legs alternate in one process; medians.  Kernel time alone: run under `rocprofv3 --kernel-trace --stats` and read ctc_spot_kernel.
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
from conformer_ocr_amd.engine import HipRecognizer  # noqa: E402
from conformer_ocr_amd.search import search_pages, spot_host  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=200, help='timed calls per leg of (a)')
ap.add_argument('--host-sample', type=int, default=2, help='lines the host leg of (a) searches (scaled)')
ap.add_argument('--pages', type=int, default=16)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--skip-pages', action='store_true', help='leg (a) only')
args = ap.parse_args()


def med(xs):
    return float(np.median(xs))


# ---- (a) the kernel
N, T, C, Q, K = 32, 300, 128, 16, 4
g = np.random.default_rng(7)
logits_h = (g.standard_normal((N, T, C)) * 2.0).astype(np.float32)
queries = [g.integers(1, C, int(l)).tolist() for l in g.integers(4, 13, Q)]
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


def leg_spot():
    return eng.ctc_spot_async(logits, out_lens, queries, K)


def leg_align():
    return [eng.ctc_align_async(logits, out_lens, q * N, [len(q)] * N) for q in queries]


for _ in range(5):                                                      # warm-up: rings, code objects
    eng.collect_spot(leg_spot())
    for h in leg_align():
        eng.collect_align(h)
torch.cuda.synchronize()
t_spot, t_align = [], []
for _ in range(args.iters):
    us, h = timed(leg_spot)
    t_spot.append(us)
    eng.collect_spot(h)
    us, hs = timed(leg_align)
    t_align.append(us)
    for h in hs:
        eng.collect_align(h)
t0 = time.perf_counter()
for n in range(args.host_sample):
    for q in queries:
        spot_host(logits_h[n].T, q, K)
host_rate = args.host_sample * Q / (time.perf_counter() - t0)
out = {'a': {'shape': [N, T, C], 'queries': Q, 'hits': K, 'labels_per_query': [min(map(len, queries)), max(map(len, queries))], 'iters': args.iters,
             'ctc_spot_us_median': round(med(t_spot), 1), 'ctc_align_x16_us_median': round(med(t_align), 1),
             'ctc_spot_us_p10_p90': [round(float(np.percentile(t_spot, q)), 1) for q in (10, 90)],
             'ctc_align_x16_us_p10_p90': [round(float(np.percentile(t_align, q)), 1) for q in (10, 90)],
             'spot_time_over_16_aligns': round(med(t_spot) / med(t_align), 3),
             'device_pairs_per_s': round(N * Q / (med(t_spot) * 1e-6), 1),
             'host_spot_pairs_per_s_scaled_from_sample': round(host_rate, 1)}}

# ---- (b) pages
if not args.skip_pages:
    import bench
    from page_rate import make_page
    from conformer_ocr_amd.codec import ascii_codec
    from conformer_ocr_amd.page import recognize_pages
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
    read = recognize_pages(net, pages)                                  # warm-up; the strings the queries are cut from
    words = []
    for r in (r for recs in read for r in recs):
        for w in r['text'].split():
            if len(w) >= 4 and w not in words:
                words.append(w)
    words = words[:Q]
    found = search_pages(net, pages, words, hits=K)
    nlines = sum(len(l) for _, l in pages)

    def leg(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return nlines / (time.perf_counter() - t0)
    rates = {'recognize_pages': [], 'search_pages': []}
    for _ in range(args.reps):
        rates['recognize_pages'].append(leg(lambda: recognize_pages(net, pages)))
        rates['search_pages'].append(leg(lambda: search_pages(net, pages, words, hits=K)))
    m = {k: med(v) for k, v in rates.items()}
    out['b'] = {'pages': args.pages, 'lines': nlines, 'queries': len(words), 'hits_found': len(found),
                'hits_at_score_0': sum(1 for h in found if h['score'] == 0.0),
                'recognize_pages_lines_per_s': round(m['recognize_pages'], 1), 'search_pages_lines_per_s': round(m['search_pages'], 1),
                'search_rate_over_recognize_rate': round(m['search_pages'] / m['recognize_pages'], 3),
                'raw': {k: [round(x, 1) for x in v] for k, v in rates.items()}}
print(json.dumps(out))
