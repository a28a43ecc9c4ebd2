#!/usr/bin/env python3
"""Rate of the scoring behind CER / WER and the confusion report, device scorer against host scorer.

    python tools/score_rate.py [--pairs 50000] [--host-sample 200] [--lines 4096] [--reps 3] [--skip-evaluate]

(a) pairs/s of `score.score(report=True)` on synthetic text (lines of 24 / 60 / 120 characters over letters and spaces, predictions with
    5 % edits): the device leg is repeated until its timed window is a second or more and split into packing (host), upload + kernel +
    read-back of the two alignment calls (HIP events) and the tallies (host); the host leg (`ErrorRate` twice, `global_align`,
    `compute_confusions`) runs on a SAMPLE of the pairs and is scaled to pairs/s.
(b) lines/s of `evaluate.evaluate(report=True)` with each scorer next to `evaluate.recognize` alone on the same lines: the `cfg2_text`
    fixture's 32 lines repeated to `--lines`, truths perturbed so that errors exist.
Legs alternate in one process; medians over `--reps`.  Kernel time alone: run under `rocprofv3 --kernel-trace --stats` and read
edit_align_kernel.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conformer_ocr_amd import score, synth  # noqa: E402
from conformer_ocr_amd.engine import HipRecognizer  # noqa: E402
from conformer_ocr_amd.evaluate import ErrorRate, compute_confusions, evaluate, global_align, recognize  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--pairs', type=int, default=50000, help='pairs per device call of leg (a)')
ap.add_argument('--host-sample', type=int, default=200, help='pairs the host leg of (a) scores (scaled)')
ap.add_argument('--lines', type=int, default=4096, help='lines of leg (b)')
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--skip-evaluate', action='store_true', help='leg (a) only')
args = ap.parse_args()

ALPHABET = 'abcdefghijklmnopqrstuvwxyz    '


def synthetic(n: int, length: int, seed: int):
    g = np.random.default_rng(seed)
    letters = np.array(list(ALPHABET))
    sym = letters[g.integers(0, len(letters), (n, length))]
    truths = [''.join(r) for r in sym]
    r = g.random((n, length))
    sub = letters[g.integers(0, len(letters), (n, length))]
    preds = []
    for i in range(n):                                       # 5 % edits: a third each deletions, substitutions, insertions
        row, ri, si = sym[i], r[i], sub[i]
        out = np.where(ri < 0.0167, '', np.where(ri < 0.0333, si, np.where(ri > 0.9833, np.char.add(row, si), row)))
        preds.append(''.join(out.tolist()))
    return truths, preds


def device_parts(eng, preds, truths):
    """`score.score(report=True)` step by step: seconds of packing, of the two alignment calls (HIP events), of the tallies."""
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t0 = time.perf_counter()
    a, a_offs = score.pack(truths)
    b, b_offs = score.pack(preds)
    wa, wa_offs, wb, wb_offs, _ = score.pack_words(preds, truths)
    t1 = time.perf_counter()
    e[0].record()
    counts, ops, _ = score.align_pairs(eng, a, a_offs, b, b_offs, want_ops=True)
    e[1].record()
    t2 = time.perf_counter()
    e[2].record()
    score.align_pairs(eng, wa, wa_offs, wb, wb_offs)
    e[3].record()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    score.tally(a, b, ops)
    t4 = time.perf_counter()
    return {'pack_s': t1 - t0, 'align_chars_wall_s': t2 - t1, 'align_chars_event_s': e[0].elapsed_time(e[1]) * 1e-3,
            'align_words_wall_s': t3 - t2, 'align_words_event_s': e[2].elapsed_time(e[3]) * 1e-3, 'tally_s': t4 - t3}


def device_leg(eng, preds, truths):
    calls, t0 = 0, time.perf_counter()
    while True:
        score.score(eng, preds, truths, report=True)
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= 1.0:
            return calls * len(preds) / dt, calls, dt


def host_leg(preds, truths):
    t0 = time.perf_counter()
    cer, wer = ErrorRate(False), ErrorRate(True)
    cer.update(preds, truths)
    wer.update(preds, truths)
    gt, pr = [], []
    for t, p in zip(truths, preds):
        _, a1, a2 = global_align(t, p)
        gt.extend(a1)
        pr.extend(a2)
    compute_confusions(gt, pr)
    return len(preds) / (time.perf_counter() - t0)


def med(xs):
    return float(np.median(xs))


eng = HipRecognizer(synth.hparams('tiny'), torch.device('cuda:0'), 'fp32')
out = {'pairs_per_call': args.pairs, 'host_sample': args.host_sample, 'reps': args.reps, 'a': {}}
for length in (24, 60, 120):
    truths, preds = synthetic(args.pairs, length, seed=length)
    hs_t, hs_p = truths[:args.host_sample], preds[:args.host_sample]
    score.score(eng, preds, truths, report=True)            # warm-up: pinned staging, rings, the kernel's code object
    host_leg(hs_p[:20], hs_t[:20])
    dev, host, parts, windows = [], [], [], []
    for _ in range(args.reps):
        rate, calls, dt = device_leg(eng, preds, truths)
        dev.append(rate)
        windows.append((calls, round(dt, 3)))
        host.append(host_leg(hs_p, hs_t))
        parts.append(device_parts(eng, preds, truths))
    out['a'][str(length)] = {
        'device_pairs_per_s': round(med(dev), 1), 'host_pairs_per_s_scaled_from_sample': round(med(host), 1),
        'device_windows_calls_seconds': windows,
        'device_parts_ms_per_call': {k[:-2] + '_ms': round(med([p[k] for p in parts]) * 1e3, 2) for k in parts[0]}}

if not args.skip_evaluate:
    with open(os.path.join(ROOT, 'tests', 'golden', 'meta.json')) as fp:
        meta = json.load(fp)
    from conformer_ocr_amd.codec import ascii_codec
    from conformer_ocr_amd.pred import PytorchRecognitionModel
    from tests.conftest import TextCase
    tc = TextCase(meta, 'cfg2_text')
    codec = ascii_codec(tc.hp.num_classes)
    net = PytorchRecognitionModel(**tc.hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1,
                                  conv_dropout_p=0.1, codec=codec, compute_dtype='bf16', chain_rows=0)
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    net = net.to('cuda:0').eval()
    g = np.random.default_rng(1)
    lines, truths = [], []
    for i in range(args.lines):
        lines.append(np.rint(tc.lines[i % tc.n] * 255.0).astype(np.uint8))
        t = [codec.l2c[(l,)] for l in tc.texts[i % tc.n]]
        for _ in range(int(g.integers(0, 4))):
            k = int(g.integers(0, len(t)))
            t[k] = ALPHABET[int(g.integers(0, len(ALPHABET)))]
        truths.append(''.join(t))
    kw = dict(batch_size=32, streams=4)

    def leg(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return len(lines) / (time.perf_counter() - t0), r
    legs = {'recognize': lambda: recognize(net, lines, **kw),
            'evaluate_device': lambda: evaluate(net, lines, truths, report=True, scorer='device', **kw),
            'evaluate_host': lambda: evaluate(net, lines, truths, report=True, scorer='host', **kw)}
    leg(legs['recognize'])                                   # warm-up
    _, warm = leg(legs['evaluate_device'])
    rates = {k: [] for k in legs}
    reports = {}
    for _ in range(args.reps):
        for k, fn in legs.items():
            r, res = leg(fn)
            rates[k].append(r)
            if k != 'recognize':
                reports[k] = res
    assert reports['evaluate_device'] == reports['evaluate_host']
    m = {k: med(v) for k, v in rates.items()}
    out['b'] = {'lines': len(lines), 'chars': reports['evaluate_host']['chars'], 'errors': reports['evaluate_host']['errors'],
                'recognize_lines_per_s': round(m['recognize'], 1), 'evaluate_device_lines_per_s': round(m['evaluate_device'], 1),
                'evaluate_host_lines_per_s': round(m['evaluate_host'], 1),
                'evaluate_device_time_over_recognize': round(m['recognize'] / m['evaluate_device'], 3),
                'evaluate_host_time_over_recognize': round(m['recognize'] / m['evaluate_host'], 3),
                'raw': {k: [round(x, 1) for x in v] for k, v in rates.items()}}
print(json.dumps(out))
