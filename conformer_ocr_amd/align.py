"""Forced alignment: where each character of a KNOWN transcription sits on its line.

    python -m conformer_ocr_amd.align -m MODEL [-f page|alto|xml] [-u NFD|NFC|NFKD|NFKC] [--no-normalize-whitespace] [--worst K]
                                      [--device cuda:0] [--batch-size 32] [--pad 16] [--edge 200] -i IN.xml OUT.json [-i IN2.xml OUT2.json ...]

IN is a PAGE XML or ALTO file whose lines carry text; the image it names is resolved relative to it.  OUT.json receives, per line in
document order, {'id', 'text', 'cuts': [(char, quad, conf)] or null, 'words': [(word, quad, conf)], 'score', 'frames', 'skipped'}
(`align_pages`).  One summary line per file goes to stderr; `--worst K` also lists the K lines of lowest score per frame, the usual
filter for ground truth whose text does not belong to its line.

`viterbi_align` is the definition (host, float64): the best path of the label sequence through the CTC lattice of a line's
log-softmax.  The device form is `cocr_ctc_align` (csrc/ctc_align.hip.h); kraken offers the operation as `kraken.align.forced_align`,
against which nothing here is pinned (kraken is not installed).

Not built: writing Word / Glyph / String elements back into PAGE or ALTO, a `--min-align-score` filter inside `GroundTruthDataset`,
bidi reordering (text is aligned in logical order), n-best alignments."""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_DEVICE_LABELS = 255          # labels per line the kernel holds (512 states of the blank-extended sequence); longer lines: `viterbi_align`


def log_softmax64(outputs) -> np.ndarray:
    """float64 log-softmax over the classes of a (C, T) matrix."""
    x = np.asarray(outputs, dtype=np.float64)
    if x.shape[1] == 0:
        return x
    m = x.max(axis=0, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=0, keepdims=True)))


def viterbi_path(lp: np.ndarray, labels: Sequence[int]) -> Tuple[Optional[np.ndarray], float]:
    """The best path of `labels` through the (C, T) log-probabilities `lp`: (state per frame or None, its score).  States s in
    [0, 2 L + 1): even = blank (class 0), odd = labels[(s - 1) / 2].  A candidate replaces the running best only if it is strictly
    greater, tried in the order stay, s - 1, s - 2; the path ends in state S - 1, or S - 2 when that scores strictly higher."""
    T = lp.shape[1]
    lab = [int(l) for l in labels]
    L = len(lab)
    S = 2 * L + 1
    if T == 0:
        return (np.zeros(0, dtype=np.int64), 0.0) if L == 0 else (None, -np.inf)
    ext = np.zeros(S, dtype=np.int64)
    ext[1::2] = lab
    skip = np.zeros(S, dtype=bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    delta = np.full(S, -np.inf)
    delta[0] = lp[0, 0]
    if S > 1:
        delta[1] = lp[ext[1], 0]
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        best = delta.copy()
        code = np.zeros(S, dtype=np.int8)
        prev = np.concatenate([[-np.inf, -np.inf], delta])
        c1, c2 = prev[1:S + 1], prev[:S]
        take = c1 > best
        best[take], code[take] = c1[take], 1
        take = skip & (c2 > best)
        best[take], code[take] = c2[take], 2
        delta = best + lp[ext, t]
        back[t] = code
    end = S - 1
    if S > 1 and delta[S - 2] > delta[S - 1]:
        end = S - 2
    score = float(delta[end])
    if score == -np.inf:
        return None, -np.inf
    states = np.empty(T, dtype=np.int64)
    s = end
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(back[t, s])
    return states, score


def viterbi_align(outputs, labels: Sequence[int]):
    """Forced alignment of `labels` (ints in [1, C)) to the (C, T) logits `outputs` (the decoders' orientation), in float64: returns
    ([(label, start, end, conf)] -- one record per label, first and last frame of its run on the best path, conf the largest softmax
    probability of the label over the run --, the path's log-probability), or (None, -inf) when no alignment fits (T = 0 with labels, or
    fewer frames than labels plus repeats).  No labels: ([], the log-probability of the all-blank path)."""
    lp = log_softmax64(outputs)
    lab = [int(l) for l in labels]
    if any(l < 1 or l >= lp.shape[0] for l in lab):
        raise ValueError(f'labels must lie in [1, {lp.shape[0]})')
    states, score = viterbi_path(lp, lab)
    if states is None:
        return None, score
    records = []
    for k, l in enumerate(lab):
        frames = np.nonzero(states == 2 * k + 1)[0]
        st, en = int(frames[0]), int(frames[-1])
        records.append((l, st, en, float(np.exp(lp[l, st:en + 1].max()))))
    return records, score


# ---- text <-> labels ----------------------------------------------------------------------------------------------------------------
def encode_text(codec, text: str) -> Tuple[List[int], str]:
    """`codec.encode(text)` and the characters it could not encode (a non-strict codec drops them; a strict one raises)."""
    labels = [int(l) for l in codec.encode(text)]
    graphemes = sorted(codec.c2l.keys(), key=len, reverse=True)
    skipped, idx = [], 0
    while idx < len(text):
        for g in graphemes:
            if text.startswith(g, idx):
                idx += len(g)
                break
        else:
            skipped.append(text[idx])
            idx += 1
    return labels, ''.join(skipped)


def line_result(codec, records, score: float, frames: int, skipped: str) -> Dict:
    """One line of `PytorchRecognitionModel.align`: label records -> characters through `codec.decode`."""
    return {'chars': None if records is None else codec.decode(records), 'score': float(score), 'frames': int(frames), 'skipped': skipped}


def align_text(codec, outputs, text: str) -> Dict:
    """`PytorchRecognitionModel.align` for one line on the host: `text` against the (C, T) logits `outputs`."""
    labels, skipped = encode_text(codec, text)
    records, score = viterbi_align(outputs, labels)
    return line_result(codec, records, score, np.asarray(outputs).shape[1], skipped)


def word_records(cuts: Optional[Sequence[Tuple]]) -> List[Tuple]:
    """(char, quad, conf) cuts of a line -> [(word, quad, conf)] for the runs between whitespace: the quad spans from the first
    character's left edge to the last character's right edge, conf is the smallest of its characters'."""
    words, run = [], []

    def close():
        if run:
            first, last = run[0][1], run[-1][1]
            words.append((''.join(c[0] for c in run), [first[0], last[1], last[2], first[3]], min(c[2] for c in run)))
            run.clear()
    for cut in cuts or ():
        if cut[0].isspace():
            close()
        else:
            run.append(cut)
    close()
    return words


# ---- pages --------------------------------------------------------------------------------------------------------------------------
def align_pages(net, pages, batch_size: int = 32, edge: int = 200, pad: int = 16, fill: int = 0, device: str = 'cuda:0') -> List[List[Dict]]:
    """The counterpart of `page.recognize_pages` for `Line`s that carry `text`: per page, in the order of its lines, {'id', 'text',
    'cuts': [(char, quad, conf)] or None, 'words': [(word, quad, conf)], 'score', 'frames', 'skipped'} with quads in page pixels.
    `cuts` is None and `score` -inf where the text does not fit the line's frames; a line without text (`text` None) is returned with
    `cuts` None and `score` None and costs no forward.

    Same bucketing and the same extraction, pre-processing and forward as `recognize_pages`, so a line's frames are the ones it is
    recognized on; then `cocr_ctc_align` on the batch, the previous batch's records being collected while it runs."""
    import torch
    from . import _lib
    from .evaluate import make_batches
    from .page import _check_image, cut_quads, line_geometry
    lib = _lib.load()
    imgs = [_check_image(img) for img, _ in pages]
    results: List[List[Dict]] = [[None] * len(lines) for _, lines in pages]
    flat = []                                    # (page, line within page, geometry, text)
    for p, (_, lines) in enumerate(pages):
        for j, ln in enumerate(lines):
            if ln.text is None:
                results[p][j] = {'id': str(ln.id), 'text': None, 'cuts': None, 'words': [], 'score': None, 'frames': None, 'skipped': ''}
            else:
                flat.append((p, j, line_geometry(ln.id, ln.baseline, ln.boundary), ln.text))
    if not flat:
        return results
    dev = torch.device(device)
    eng = net.engine(dev)
    d_pages = [torch.from_numpy(a).to(dev) for a in imgs]
    height = int(net.height)
    widths = [int(lib.cocr_preproc_width(g.H_s, g.W_s, height, int(pad))) for _, _, g, _ in flat]
    batches = make_batches(widths, batch_size, edge)

    def finish(pend):
        idx, handle, lens = pend
        for n, (i, rec) in enumerate(zip(idx, net.collect_align(handle))):
            p, j, g, text = flat[i]
            W_in = int(lens[n])
            cuts = None if rec['chars'] is None else cut_quads(g, rec['chars'], W_in, rec['frames'], pad)
            results[p][j] = {'id': g.id, 'text': text, 'cuts': cuts, 'words': word_records(cuts), 'score': rec['score'],
                             'frames': rec['frames'], 'skipped': rec['skipped']}

    pending = None
    for width, idx in batches:
        strips, offs, hs, ws = eng.extract_lines(d_pages, [(flat[i][0], flat[i][2]) for i in idx], fill=fill)
        im, lens = eng.preprocess_device(strips, offs, hs, ws, height=height, pad=pad, width=width)
        handle = net.align_async(im.unsqueeze(1), torch.from_numpy(lens), [flat[i][3] for i in idx])
        if pending is not None:
            finish(pending)
        pending = (idx, handle, lens)
    finish(pending)
    return results


# ---- command ------------------------------------------------------------------------------------------------------------------------
def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog='python -m conformer_ocr_amd.align', description='Places the transcription of every line on its line.',
                                 epilog='Not built: writing Word / Glyph / String elements back into the documents, bidi reordering, '
                                        'n-best alignments.')
    ap.add_argument('-m', '--model', default=None, help='safetensors archive or checkpoint')
    ap.add_argument('-f', '--format-type', choices=('page', 'alto', 'xml'), default='xml', help='format of the inputs (xml: told apart by the root element)')
    ap.add_argument('-i', '--input', nargs=2, action='append', metavar=('IN', 'OUT'), default=[],
                    help='document with transcribed lines and the JSON file to write (repeatable)')
    ap.add_argument('-u', '--normalization', choices=('NFD', 'NFKD', 'NFC', 'NFKC'), default=None, help='text normalization')
    ap.add_argument('-n', '--normalize-whitespace', dest='normalize_whitespace', action='store_true', default=True,
                    help='normalizes unicode whitespace (default)')
    ap.add_argument('--no-normalize-whitespace', dest='normalize_whitespace', action='store_false')
    ap.add_argument('--worst', type=int, default=0, metavar='K', help='also list the K lines of lowest score per frame')
    ap.add_argument('-d', '--device', default='cuda:0')
    ap.add_argument('-B', '--batch-size', type=int, default=32)
    ap.add_argument('--pad', type=int, default=16, help='zero columns left and right of every scaled line (the model\'s training form)')
    ap.add_argument('--edge', type=int, default=200, help='width bucket edge: lines are padded to a multiple of it')
    return ap


def main(argv=None) -> int:
    ap = parser()
    args = ap.parse_args(argv)

    def usage(msg: str) -> int:
        ap.print_usage(sys.stderr)
        print(f'{ap.prog}: error: {msg}', file=sys.stderr)
        return 1
    if not args.model:
        return usage('No model given.')
    if not args.input:
        return usage('No input given. Use `-i IN.xml OUT.json`.')
    missing = [f for f in [args.model] + [src for src, _ in args.input] if not os.path.exists(f)]
    if missing:
        return usage(f'no such file: {", ".join(missing)}')
    from .dataset import normalize_text
    from .page import READERS, Line
    docs = []
    for src, dst in args.input:
        page = READERS[args.format_type](src)
        lines = []
        for ln in page.lines:
            text = None if ln.text is None else normalize_text(ln.text, args.normalization, args.normalize_whitespace)
            lines.append(Line(ln.id, ln.baseline, ln.boundary, text or None))
        docs.append((src, dst, page.image, lines))
    if not any(ln.text is not None for _, _, _, lines in docs for ln in lines):
        return usage('no line with text in the inputs')
    from .ocr import load_image, load_model
    pages = []
    for src, _, image, lines in docs:
        if not image:
            return usage(f'{src}: names no image file')
        pages.append((load_image(os.path.join(os.path.dirname(os.path.abspath(src)), image)), lines))
    net = load_model(args.model, device=args.device)
    results = align_pages(net, pages, batch_size=args.batch_size, edge=args.edge, pad=args.pad, device=args.device)
    worst = []
    for (src, dst, _, _), recs in zip(docs, results):
        with open(dst, 'w', encoding='utf-8') as fp:
            json.dump(recs, fp, ensure_ascii=False)
        aligned = sum(1 for r in recs if r['cuts'] is not None)
        unfit = sum(1 for r in recs if r['cuts'] is None and r['score'] is not None)
        print(f'{dst}: {aligned} lines aligned, {unfit} do not fit, {sum(1 for r in recs if r["skipped"])} with skipped characters',
              file=sys.stderr)
        worst.extend((r['score'] / max(r['frames'], 1), src, r) for r in recs if r['cuts'] is not None)
    if args.worst > 0:
        worst.sort(key=lambda w: w[0])
        for per_frame, src, r in worst[:args.worst]:
            print(f'{per_frame:9.4f}  {src}  {r["id"]}  {r["text"]}', file=sys.stderr)
    return 0


if __name__ == '__main__':
    sys.exit(main())
