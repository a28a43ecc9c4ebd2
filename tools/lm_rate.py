#!/usr/bin/env python3
"""Rate of the beam search with an n-gram model.

    python tools/lm_rate.py [--iters 100] [--beam 16] [--build-only] [--skip-build]

(a) ms per call on cfg2-shaped logits (32 x 300 x 128, random normal x 2.5, blank + 1.5), beam 16: `cocr_ctc_beam` next to
    `cocr_ctc_beam_lm` with 8 classes at orders 3 and 5 (models of 2000 lines of a random first-order chain) -- HIP-event medians,
    legs alternating in one process; then with `cocr_profile` on, the launches of one LM call one by one.
(b) line decodes/s of `lm.tune_grid` over a 5 x 5 grid on four such batches (logits resident, one forward's worth each).
(c) host only: table sizes and build time of an order-5 model of 50 000 lines of 50 labels (first-order chain over 127 labels).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conformer_ocr_amd import synth  # noqa: E402
from conformer_ocr_amd.lm import build_lm, tune_grid  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--iters', type=int, default=100)
ap.add_argument('--beam', type=int, default=16, help='beam of leg (a): above 16 the plain search runs ctc_beam_walk_kernel<3>')
ap.add_argument('--build-only', action='store_true', help='leg (c) only: no GPU needed')
ap.add_argument('--skip-build', action='store_true')
args = ap.parse_args()


def chain_corpus(lines, length, C, seed):
    g = synth._rng(seed, f'lm_rate:{lines}:{length}:{C}')
    P = np.cumsum(g.dirichlet(np.full(C - 1, 0.3), size=C - 1), axis=1)
    u = g.random((lines, length))
    out = np.zeros((lines, length), dtype=np.int64)
    out[:, 0] = g.integers(1, C, lines)
    for j in range(1, length):
        rows = P[out[:, j - 1] - 1]
        out[:, j] = 1 + np.minimum((rows < u[:, j:j + 1]).sum(axis=1), C - 2)
    return out


out = {}
if not args.skip_build:
    corpus = chain_corpus(50000, 50, 128, 1)
    t0 = time.perf_counter()
    big = build_lm(list(corpus), 5, 128)
    dt = time.perf_counter() - t0
    nbytes = sum(a.nbytes for a in (big.unigram, big.ngram_keys, big.ngram_logp, big.ctx_keys, big.ctx_bow))
    out['c'] = {'lines': 50000, 'labels_per_line': 50, 'order': 5, 'build_s': round(dt, 1), 'ngrams': int((big.ngram_keys != 0).sum()),
                'ngram_slots': int(big.ngram_keys.shape[0]), 'contexts': int((big.ctx_keys != 0).sum()), 'ctx_slots': int(big.ctx_keys.shape[0]),
                'table_MB': round(nbytes / 1e6, 1)}
if not args.build_only:
    import torch
    from conformer_ocr_amd.engine import HipRecognizer
    N, T, C = 32, 300, 128
    g = np.random.default_rng(7)
    eng = HipRecognizer(synth.hparams('tiny'), torch.device('cuda:0'), 'fp32')
    lens = np.full(N, T, dtype=np.int32)

    def batch():
        x = (g.standard_normal((N, T, C)) * 2.5).astype(np.float32)
        x[:, :, 0] += 1.5
        return torch.from_numpy(x).cuda()
    logits = batch()
    lms = {o: build_lm(list(chain_corpus(2000, 50, C, o)), o, C) for o in (3, 5)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h = fn()
        e1.record()
        e1.synchronize()
        eng.collect(h)
        return e0.elapsed_time(e1)                                       # ms
    legs = {'ctc_beam': lambda: eng.ctc_beam_async(logits, lens, args.beam),
            'ctc_beam_lm_order3': lambda: eng.ctc_beam_lm_async(logits, lens, lms[3], args.beam, 8, 0.5, 0.0),
            'ctc_beam_lm_order5': lambda: eng.ctc_beam_lm_async(logits, lens, lms[5], args.beam, 8, 0.5, 0.0),
            'ctc_beam_lm_order5_alpha0': lambda: eng.ctc_beam_lm_async(logits, lens, lms[5], args.beam, 8, 0.0, 0.0)}
    for fn in legs.values():
        for _ in range(3):
            timed(fn)
    ts = {k: [] for k in legs}
    for _ in range(args.iters):
        for k, fn in legs.items():
            ts[k].append(timed(fn))
    a = {k + '_ms_median': round(float(np.median(v)), 4) for k, v in ts.items()}
    a.update({k + '_ms_p10_p90': [round(float(np.percentile(v, q)), 4) for q in (10, 90)] for k, v in ts.items()})
    a['lm_order5_over_plain'] = round(float(np.median(ts['ctc_beam_lm_order5']) / np.median(ts['ctc_beam'])), 2)
    out['a'] = dict(a, shape=[N, T, C], beam=args.beam, classes=8, iters=args.iters)
    # (b) the grid
    batches = [(batch(), lens) for _ in range(4)]
    truths = [''.join(chr(33 + int(l)) for l in row) for row in chain_corpus(4 * N, 60, C, 9)]
    to_text = lambda rec: ''.join(chr(33 + r[0]) for r in rec)
    grid = [0.0, 0.25, 0.5, 0.75, 1.0], [0.0, 0.5, 1.0, 1.5, 2.0]
    tune_grid(eng, lms[5], batches[:1], truths[:N], to_text, grid[0][:1], grid[1][:1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tune_grid(eng, lms[5], batches, truths, to_text, *grid)
    dt = time.perf_counter() - t0
    out['b'] = {'lines': 4 * N, 'cells': 25, 'seconds': round(dt, 3), 'line_decodes_per_s': round(4 * N * 25 / dt, 1),
                'lines_per_s_through_the_whole_grid': round(4 * N / dt, 1)}
print(json.dumps(out))
