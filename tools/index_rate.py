#!/usr/bin/env python3
"""Rates of the search index.

    python tools/index_rate.py [--iters 200] [--pages 16] [--reps 3] [--skip-pages]

(a) `cocr_posterior_pack` on 32 x 300 x 128 random logits, keep 8, next to `cocr_ctc_greedy` on the same logits (from the values: the
    forward's argmax shortcut does not apply to foreign logits): HIP-event medians per call (length upload + kernels).
(b) 256 x 300 x 128, Q = 16 queries of 4 - 12 labels, 4 hits: `cocr_posterior_unpack` + `cocr_ctc_spot` on resident packed entries,
    next to `cocr_ctc_spot` on resident dense logits and to the unpack alone -- its share of the pair decides whether a spot kernel
    that reads the packed rows directly is worth building.
(c) tools/search_rate.py's synthetic pages (cfg2 text model, bf16; 16 pages, 640 lines): `index.search_index` (16 queries cut from the
    pages' own reading, 4 hits; the file is loaded once, as a search service would) in lines/s and queries/s, next to
    `search.search_pages` on the same pages and queries (search.py and its kernel are the parent commit's, unchanged) and next to
    `index.build_index`; bytes per line of the file next to the dense float32 logits.
Legs alternate in one process; medians with p10 / p90.  Prints one JSON line."""
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from conformer_ocr_amd import synth  # noqa: E402
from conformer_ocr_amd.engine import HipRecognizer  # noqa: E402
from conformer_ocr_amd.index import build_index, index_info, load_index, search_index  # noqa: E402
from conformer_ocr_amd.search import search_pages  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=200, help='timed calls per leg of (a) and (b)')
ap.add_argument('--pages', type=int, default=16)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--skip-pages', action='store_true', help='legs (a) and (b) only')
args = ap.parse_args()
KEEP, STEP, Q, K = 8, 0.125, 16, 4


def stats(xs):
    return {'median': round(float(np.median(xs)), 1), 'p10_p90': [round(float(np.percentile(xs, q)), 1) for q in (10, 90)]}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, r                                 # us


def alternate(legs, iters):
    """legs: {name: (enqueue, collect or None)}; per-call times in us, the legs taking turns."""
    for _ in range(5):                                                  # warm-up: rings, code objects, pinned pools
        for fn, done in legs.values():
            r = fn()
            if done:
                done(r)
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(iters):
        for k, (fn, done) in legs.items():
            us, r = timed(fn)
            times[k].append(us)
            if done:
                done(r)
    return times


g = np.random.default_rng(7)
eng = HipRecognizer(synth.hparams('tiny'), torch.device('cuda:0'), 'fp32')

# ---- (a) pack next to greedy
N, T, C = 32, 300, 128
logits = torch.from_numpy((g.standard_normal((N, T, C)) * 2.0).astype(np.float32)).cuda()
out_lens = np.full(N, T, dtype=np.int32)
t = alternate({'pack': (lambda: eng.posterior_pack(logits, out_lens, KEEP, STEP), None),
               'greedy': (lambda: eng.ctc_greedy_async(logits, out_lens), eng.collect)}, args.iters)
out = {'a': {'shape': [N, T, C], 'keep': KEEP, 'iters': args.iters, 'posterior_pack_us': stats(t['pack']), 'ctc_greedy_us': stats(t['greedy']),
             'pack_time_over_greedy': round(float(np.median(t['pack']) / np.median(t['greedy'])), 3),
             'pack_logits_GB_per_s': round(N * T * C * 4 / (float(np.median(t['pack'])) * 1e-6) / 1e9, 1)}}

# ---- (b) unpack + spot next to spot on dense logits
N = 256
dense = torch.from_numpy((g.standard_normal((N, T, C)) * 2.0).astype(np.float32)).cuda()
queries = [g.integers(1, C, int(l)).tolist() for l in g.integers(4, 13, Q)]
out_lens = np.full(N, T, dtype=np.int32)
classes, codes = eng.posterior_pack(dense, out_lens, KEEP, STEP)
t = alternate({'spot_dense': (lambda: eng.ctc_spot_async(dense, out_lens, queries, K), eng.collect_spot),
               'unpack_spot': (lambda: eng.ctc_spot_async(eng.posterior_unpack(classes, codes, C, STEP), out_lens, queries, K), eng.collect_spot),
               'unpack': (lambda: eng.posterior_unpack(classes, codes, C, STEP), None)}, args.iters)
m = {k: float(np.median(v)) for k, v in t.items()}
out['b'] = {'shape': [N, T, C], 'keep': KEEP, 'queries': Q, 'hits': K, 'iters': args.iters, 'ctc_spot_dense_us': stats(t['spot_dense']),
            'unpack_plus_spot_us': stats(t['unpack_spot']), 'unpack_us': stats(t['unpack']),
            'unpack_share_of_pair': round(m['unpack'] / m['unpack_spot'], 3), 'pair_over_dense_spot': round(m['unpack_spot'] / m['spot_dense'], 3),
            'dense_pairs_per_s': round(N * Q / (m['spot_dense'] * 1e-6), 1), 'indexed_pairs_per_s': round(N * Q / (m['unpack_spot'] * 1e-6), 1)}

# ---- (c) pages
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
    nlines = sum(len(l) for _, l in pages)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'corpus.cidx')
        build_index(net, pages, path, keep=KEEP, step=STEP)             # warm-up
        index = load_index(path)
        info = index_info(index)
        found = search_index(index, words, hits=K)
        direct = search_pages(net, pages, words, hits=K)

        def leg(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return nlines / (time.perf_counter() - t0)
        rates = {'search_index': [], 'search_index_from_file': [], 'search_pages': [], 'build_index': []}
        for _ in range(args.reps):
            rates['search_index'].append(leg(lambda: search_index(index, words, hits=K)))
            rates['search_index_from_file'].append(leg(lambda: search_index(path, words, hits=K)))
            rates['search_pages'].append(leg(lambda: search_pages(net, pages, words, hits=K)))
            rates['build_index'].append(leg(lambda: build_index(net, pages, path, keep=KEEP, step=STEP)))
    m = {k: float(np.median(v)) for k, v in rates.items()}
    zero = lambda hs: sum(1 for h in hs if h['score'] == 0.0)
    out['c'] = {'pages': args.pages, 'lines': nlines, 'queries': len(words), 'hits': K, 'keep': KEEP, 'step': STEP,
                'search_index_lines_per_s': round(m['search_index'], 1), 'search_index_queries_per_s': round(m['search_index'] / nlines * len(words), 2),
                'search_index_from_file_lines_per_s': round(m['search_index_from_file'], 1),
                'search_pages_lines_per_s': round(m['search_pages'], 1), 'build_index_lines_per_s': round(m['build_index'], 1),
                'search_index_over_search_pages': round(m['search_index'] / m['search_pages'], 2),
                'hits_found': {'index': len(found), 'pages': len(direct)}, 'hits_at_score_0': {'index': zero(found), 'pages': zero(direct)},
                'file_bytes_per_line': round(info['file_bytes_per_line'], 1), 'packed_bytes_per_line': round(info['packed_bytes_per_line'], 1),
                'dense_float32_bytes_per_line': round(info['dense_bytes_per_line'], 1), 'frames_per_line': round(info['frames'] / max(info['lines'], 1), 1),
                'raw': {k: [round(x, 1) for x in v] for k, v in rates.items()}}
print(json.dumps(out))
