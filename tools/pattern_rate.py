#!/usr/bin/env python3
"""Rate of pattern spotting.

    python tools/pattern_rate.py [--iters 200] [--match-sample 200] [--pages 16] [--reps 3] [--skip-pages]

On 32 x 300 x 128 random logits with 16 patterns, 4 hits each, HIP-event medians per call (table upload + kernel), legs alternating:
(a) `cocr_ctc_spot_pattern` on 16 literal chains of 4 - 12 labels FORCED through the graph kernel, next to `cocr_ctc_spot` on the same
    strings: the price of the graph form (in production a chain takes `cocr_ctc_spot`);
(b) `cocr_ctc_spot_pattern` on a mix of real patterns: 13 case-folded words of 4 - 12 letters, two `[0-9]{4}`-shaped year patterns and
    one alternation;
(c) the host `pattern.match_host` time per hit, on a sample of (b)'s hits;
(d) lines/s of `search.search_pages` with 16 case-folded patterns next to `search_pages` with the same 16 words as strings, on
    tools/page_rate.py's synthetic pages (cfg2 text model, bf16; its alphabet read through a codec with two cases).
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
from conformer_ocr_amd import pattern as PT, synth  # noqa: E402
from conformer_ocr_amd.codec import PytorchCodec, ascii_codec  # noqa: E402
from conformer_ocr_amd.engine import HipRecognizer  # noqa: E402
from conformer_ocr_amd.search import search_pages  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=200, help='timed calls per leg')
ap.add_argument('--match-sample', type=int, default=200, help='hits `match_host` is timed on')
ap.add_argument('--pages', type=int, default=16)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--skip-pages', action='store_true', help='the kernel legs only')
args = ap.parse_args()


def med(xs):
    return float(np.median(xs))


def spread(xs):
    return [round(float(np.percentile(xs, q)), 1) for q in (10, 90)]


N, T, C, Q, K = 32, 300, 128, 16, 4
g = np.random.default_rng(7)                                            # tools/search_rate.py's logits and strings
logits_h = (g.standard_normal((N, T, C)) * 2.0).astype(np.float32)
queries = [g.integers(1, C, int(l)).tolist() for l in g.integers(4, 13, Q)]
out_lens = np.full(N, T, dtype=np.int32)
eng = HipRecognizer(synth.hparams('tiny'), torch.device('cuda:0'), 'fp32')
logits = torch.from_numpy(logits_h).cuda()
codec = ascii_codec(C)
chains = [PT.chain_graph(q) for q in queries]
letters = [c for c in 'abcdefghijklmnopqrstuvwxyz']
words = [''.join(g.choice(letters, int(l))) for l in g.integers(4, 13, 13)]
mix = [PT.compile_pattern(w, codec, ignore_case=True) for w in words]
mix += [PT.compile_pattern(t, codec) for t in ('1[5-7][0-9][0-9]', '[0-9]{4}', '(anno|ano|a\\.d\\.)_?(domini|dni)')]
assert len(mix) == Q and not any(m.is_chain or m.skipped for m in mix)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, r                                 # us


legs = {'ctc_spot_strings': (lambda: eng.ctc_spot_async(logits, out_lens, queries, K), eng.collect_spot),
        'ctc_spot_pattern_chains': (lambda: eng.ctc_spot_pattern_async(logits, out_lens, chains, K), eng.collect_spot_pattern),
        'ctc_spot_pattern_mix': (lambda: eng.ctc_spot_pattern_async(logits, out_lens, mix, K), eng.collect_spot_pattern)}
for _ in range(5):                                                      # warm-up: rings, code objects
    for fn, collect in legs.values():
        collect(fn())
torch.cuda.synchronize()
times = {k: [] for k in legs}
for _ in range(args.iters):
    for k, (fn, collect) in legs.items():
        us, h = timed(fn)
        times[k].append(us)
        last = collect(h)
hits = [(n, qi, h) for n, per in enumerate(last) for qi, spots in enumerate(per) for h in spots][:args.match_sample]
t0 = time.perf_counter()
for n, qi, (st, en, _, fin) in hits:
    PT.match_host(logits_h[n].T, mix[qi], st, en, fin)
match_us = (time.perf_counter() - t0) / max(len(hits), 1) * 1e6
out = {'kernel': {'shape': [N, T, C], 'patterns': Q, 'hits': K, 'iters': args.iters,
                  'mix_states': [int(min(m.P for m in mix)), int(max(m.P for m in mix))], 'mix_edges': [int(min(m.edges for m in mix)), int(max(m.edges for m in mix))],
                  **{f'{k}_us_median': round(med(v), 1) for k, v in times.items()}, **{f'{k}_us_p10_p90': spread(v) for k, v in times.items()},
                  'graph_chains_over_strings': round(med(times['ctc_spot_pattern_chains']) / med(times['ctc_spot_strings']), 3),
                  'mix_over_strings': round(med(times['ctc_spot_pattern_mix']) / med(times['ctc_spot_strings']), 3)},
       'match_host': {'hits': len(hits), 'us_per_hit': round(match_us, 1)}}

if not args.skip_pages:
    import bench
    from page_rate import make_page
    from conformer_ocr_amd.pred import PytorchRecognitionModel
    fix = bench.load_text_fixture('cfg2_text')
    hp = fix['hp']
    h = min(26, (hp.num_classes - 1) // 2)                                  # the fixture's alphabet, read as letters of two cases
    c2l = {chr(0x61 + i): [1 + i] for i in range(h)}
    c2l.update({chr(0x41 + i): [1 + h + i] for i in range(h)})
    c2l.update({chr(0x2460 + k): [1 + 2 * h + k] for k in range(hp.num_classes - 1 - 2 * h)})
    net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1,
                                  codec=PytorchCodec(c2l), compute_dtype='bf16')
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fix['state'].items()})
    net = net.to('cuda:0').eval()
    lines_u8 = [np.rint(np.asarray(ln, dtype=np.float32)[::2, :1100:2].repeat(2, axis=1) * 255.0).astype(np.uint8) for ln in fix['lines']]
    distinct = [make_page(lines_u8, s) for s in range(4)]
    pages = [distinct[i % 4] for i in range(args.pages)]
    from conformer_ocr_amd.page import recognize_pages
    read = recognize_pages(net, pages)                                  # warm-up; the strings the queries are cut from
    cut = []
    for r in (r for recs in read for r in recs):
        for at in range(0, max(len(r['text']) - 5, 0), 7):
            w = r['text'][at:at + 6]
            if len(w) == 6 and w not in cut:
                cut.append(w)
    cut = cut[:Q]
    folded = [PT.escape(w.swapcase()) for w in cut]
    found = search_pages(net, pages, patterns=folded, ignore_case=True, hits=K)
    search_pages(net, pages, cut, hits=K)
    nlines = sum(len(l) for _, l in pages)

    def leg(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return nlines / (time.perf_counter() - t0)
    rates = {'search_pages_strings': [], 'search_pages_patterns': []}
    for _ in range(args.reps):
        rates['search_pages_strings'].append(leg(lambda: search_pages(net, pages, cut, hits=K)))
        rates['search_pages_patterns'].append(leg(lambda: search_pages(net, pages, patterns=folded, ignore_case=True, hits=K)))
    m = {k: med(v) for k, v in rates.items()}
    out['pages'] = {'pages': args.pages, 'lines': nlines, 'patterns': len(cut), 'hits_found': len(found),
                    'hits_at_score_0': sum(1 for x in found if x['score'] == 0.0),
                    **{f'{k}_lines_per_s': round(v, 1) for k, v in m.items()},
                    'patterns_rate_over_strings_rate': round(m['search_pages_patterns'] / m['search_pages_strings'], 3),
                    'raw': {k: [round(x, 1) for x in v] for k, v in rates.items()}}
print(json.dumps(out))
