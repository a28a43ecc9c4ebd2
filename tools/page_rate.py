#!/usr/bin/env python3
"""Whole-page recognition rate: synthetic 2480 x 3508 pages (A4 at 300 dpi) of 40 lines each -- two columns of 20,
straight, rotated by +-3 / +-7 degrees and bent along circular arcs -- through `recognize_pages` with the cfg2 text model in bf16.

    python tools/page_rate.py [--pages 16] [--quick]

Prints pages/s and lines/s through `recognize_pages`, the host geometry's share, the extraction call's device time per page (HIP events
around `extract_lines`: table upload + both kernels), `recognize_crops` lines/s on the same strips, and the numpy restatement's
(tests/page_ref.py) host time per page -- this project's own CPU baseline, not kraken's.  Kernel times: run under
`rocprofv3 --kernel-trace --stats` (with --quick) and read page_spans_kernel / page_sample_kernel."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (load_text_fixture)
from conformer_ocr_amd.codec import ascii_codec  # noqa: E402
from conformer_ocr_amd.evaluate import recognize_crops  # noqa: E402
from conformer_ocr_amd.page import Line, line_geometry, recognize_pages  # noqa: E402
from conformer_ocr_amd.pred import PytorchRecognitionModel  # noqa: E402
from tests import page_ref, page_synth  # noqa: E402

KINDS = [('line', 0.0)] * 5 + [('line', 3.0), ('line', -3.0), ('line', 7.0), ('line', -7.0), ('arc', 2500.0, 1)]


def make_page(lines_u8, seed):
    """(page (3508, 2480) uint8, [Line]) : two columns of 20 lines."""
    rng = np.random.default_rng(seed)
    page = np.zeros((3508, 2480), dtype=np.uint8)
    out = []
    for col in range(2):
        pick = rng.choice(len(lines_u8), 20)
        kinds = [KINDS[int(k)] for k in rng.integers(0, len(KINDS), 20)]
        sub, placed = page_synth.text_page([lines_u8[i] for i in pick], kinds, margin=30, gap=40)
        assert sub.shape[0] <= 3508 and sub.shape[1] <= 1240, sub.shape
        x0 = 1240 * col
        page[:sub.shape[0], x0:x0 + sub.shape[1]] = np.maximum(page[:sub.shape[0], x0:x0 + sub.shape[1]], sub)
        for k, (_, P, B) in enumerate(placed):
            out.append(Line(f'c{col}l{k}', P + [x0, 0], B + [x0, 0]))
    return page, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pages', type=int, default=16)
    ap.add_argument('--distinct', type=int, default=4, help='distinct synthetic pages (repeated to --pages)')
    ap.add_argument('--quick', action='store_true', help='one warm pass and one timed pass (for a profiler run)')
    args = ap.parse_args()
    fix = bench.load_text_fixture('cfg2_text')
    hp = fix['hp']
    net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1,
                                  codec=ascii_codec(hp.num_classes), compute_dtype='bf16')
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fix['state'].items()})
    net = net.to('cuda:0').eval()
    # 48-row lines (the fixture's 96 x 1200 lines halved): 40 of them fit an A4 page at 300 dpi
    lines_u8 = [np.rint(np.asarray(ln, dtype=np.float32)[::2, :1100:2].repeat(2, axis=1) * 255.0).astype(np.uint8) for ln in fix['lines']]
    t0 = time.perf_counter()
    distinct = [make_page(lines_u8, s) for s in range(args.distinct)]
    print(f'{args.distinct} synthetic pages of {len(distinct[0][1])} lines rendered in {time.perf_counter() - t0:.1f} s', flush=True)
    pages = [distinct[i % args.distinct] for i in range(args.pages)]
    nlines = sum(len(l) for _, l in pages)

    reps = 1 if args.quick else 3
    recognize_pages(net, pages)                                          # warm: engine, code objects, batch shapes
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        recognize_pages(net, pages)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    print(f'recognize_pages: {args.pages / best:8.2f} pages/s  {nlines / best:9.0f} lines/s  ({best * 1e3:.0f} ms for {args.pages} pages, '
          f'{nlines} lines; best of {reps})', flush=True)
    t0 = time.perf_counter()
    geoms = [[line_geometry(l.id, l.baseline, l.boundary) for l in lines] for _, lines in pages]
    tg = (time.perf_counter() - t0) / args.pages
    print(f'host geometry (line_geometry): {tg * 1e3:.2f} ms per page = {tg / best * args.pages * 100:.0f} % of the recognize_pages time', flush=True)

    eng = net.engine(torch.device('cuda:0'))
    d_pages = [torch.from_numpy(p).cuda() for p, _ in distinct]
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times, strips_bytes = [], 0
    for it in range(1 if args.quick else 5):
        for p in range(args.distinct):
            ev0.record()
            buf, offs, hs, ws = eng.extract_lines(d_pages, [(p, g) for g in geoms[p]])
            ev1.record()
            ev1.synchronize()
            if it:
                times.append(ev0.elapsed_time(ev1))
            strips_bytes = int(buf.numel())
    if times:
        print(f'extract_lines per page (device events: table upload + span + sample kernels): median {np.median(times) * 1e3:.0f} us, '
              f'{strips_bytes / 1e6:.2f} MB of strips written', flush=True)
    strips = []
    for p, (page, lines) in enumerate(pages):
        buf, offs, hs, ws = eng.extract_lines([d_pages[p % args.distinct]], [(0, g) for g in geoms[p]])
        flat = buf.cpu().numpy()
        strips += [flat[o:o + h * w].reshape(h, w) for o, h, w in zip(offs, hs, ws)]
    recognize_crops(net, strips)
    torch.cuda.synchronize()
    best_c = None
    for _ in range(reps):
        t0 = time.perf_counter()
        recognize_crops(net, strips)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best_c = dt if best_c is None else min(best_c, dt)
    print(f'recognize_crops on the same strips: {len(strips) / best_c:9.0f} lines/s  (page path = {best_c / best * 100:.0f} % of it)', flush=True)

    page, lines = distinct[0]
    t0 = time.perf_counter()
    for l in lines:
        page_ref.strip(page, page_ref.geometry(l.baseline, l.boundary))
    print(f'numpy restatement (tests/page_ref.py, this project\'s CPU baseline, 1 thread): {(time.perf_counter() - t0) * 1e3:.0f} ms per page',
          flush=True)


if __name__ == '__main__':
    main()
