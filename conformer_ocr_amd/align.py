"""Forced alignment: where each character of a KNOWN transcription sits on its line.

    python -m conformer_ocr_amd.align -m MODEL [-f page|alto|xml] [-u NFD|NFC|NFKD|NFKC] [--no-normalize-whitespace] [--worst K]
                                      [--device cuda:0] [--batch-size 32] [--pad 16] [--edge 200] -i IN.xml OUT.json [-i IN2.xml OUT2.json ...]
    python -m conformer_ocr_amd.align -m MODEL --text-input IN.xml TEXT.txt OUT.json [--gt-dir DIR] [--min-line-score X] [--worst K]

The second form places the running text of a PAGE (TEXT.txt: no line breaks, or breaks that are not the scan's)
on the segmented lines of IN.xml: OUT.json receives `align_text_pages`' record of the page; `--gt-dir` writes every line that took
text as DIR/<page stem>_<line id>.png + .gt.txt, which `train -f path` reads.

IN is a PAGE XML or ALTO file whose lines carry text; the image it names is resolved relative to it.  OUT.json receives, per line in
document order, {'id', 'text', 'cuts': [(char, quad, conf)] or null, 'words': [(word, quad, conf)], 'score', 'frames', 'skipped'}
(`align_pages`).  One summary line per file goes to stderr; `--worst K` also lists the K lines of lowest score per frame, the usual
filter for ground truth whose text does not belong to its line.

`viterbi_align` is the definition (host, float64): the best path of the label sequence through the CTC lattice of a line's
log-softmax.  The device form is `cocr_ctc_align` (csrc/ctc_align.hip.h); kraken offers the operation as `kraken.align.forced_align`,
against which nothing here is pinned (kraken is not installed).

`viterbi_align_page` is the definition of the second form: the page's text as one label sequence over the frames of its lines in
reading order, where a character never spans a line break and a space may be absent at one; the device form is
`cocr_ctc_align_page` (csrc/ctc_align_page.hip.h).

Not built: writing Word / Glyph / String elements back into PAGE or ALTO, a `--min-align-score` filter inside `GroundTruthDataset`,
bidi reordering (text is aligned in logical order), n-best alignments; for page texts also hyphens the typesetter added at line
ends, passages missing from the page or from the text (beyond whole lines left empty), reading order other than document order."""
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


# ---- a page's running text on its lines ------------------------------------------------------------------------
def page_frames(lens: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """(first frame of every line in the page's concatenated frames, K + 1 entries; is-break-frame per frame): a break frame is the
    first frame of a line k >= 1 that has frames."""
    first = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)
    brk = np.zeros(int(first[-1]), dtype=bool)
    for k in range(1, len(lens)):
        if lens[k] > 0:
            brk[first[k]] = True
    return first, brk


def check_optional(optional, L: int) -> np.ndarray:
    opt = np.asarray(optional, dtype=bool).reshape(-1)
    if opt.shape[0] != L:
        raise ValueError('optional needs one entry per label')
    if L and (opt[0] or opt[-1]):
        raise ValueError('the first and the last label cannot be optional')
    if np.any(opt[1:] & opt[:-1]):
        raise ValueError('two adjacent labels cannot both be optional')
    return opt


def viterbi_page_path(lp: np.ndarray, brk: np.ndarray, labels: Sequence[int], optional) -> Tuple[Optional[np.ndarray], float]:
    """`viterbi_path` over the concatenated (C, sum T) log-probabilities of a page's lines with the two rules of a line break: an odd
    state does not stay over a break frame (`brk`), and an optional label may be stepped over (from s - 3, the blank before it, or
    from s - 4).  Candidates in the order stay, s - 1, s - 2, s - 3, s - 4, a later one winning only if strictly greater; the edges
    from s - 2 and s - 4 between equal classes exist at break frames only."""
    T = lp.shape[1]
    lab = [int(l) for l in labels]
    L = len(lab)
    S = 2 * L + 1
    opt = check_optional(optional, L)
    if T == 0:
        return (np.zeros(0, dtype=np.int64), 0.0) if L == 0 else (None, -np.inf)
    ext = np.zeros(S, dtype=np.int64)
    ext[1::2] = lab
    odd = (np.arange(S) & 1) == 1
    odd3 = odd & (np.arange(S) >= 3)
    diff2 = np.zeros(S, dtype=bool)
    diff2[3::2] = ext[3::2] != ext[1:-2:2]
    over = np.zeros(S, dtype=bool)                  # odd s >= 5 whose label s - 2 is optional
    over[5::2] = opt[1:-1] if L >= 3 else False
    diff4 = np.zeros(S, dtype=bool)
    diff4[5::2] = ext[5::2] != ext[1:-4:2]
    delta = np.full(S, -np.inf)
    delta[0] = lp[0, 0]
    if S > 1:
        delta[1] = lp[ext[1], 0]
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        b = bool(brk[t])
        best = delta.copy()
        if b:
            best[odd] = -np.inf
        code = np.zeros(S, dtype=np.int8)
        prev = np.concatenate([np.full(4, -np.inf), delta])
        for d, allowed in ((1, np.ones(S, dtype=bool)), (2, diff2 | odd3 if b else diff2), (3, over), (4, over if b else over & diff4)):
            cand = prev[4 - d:4 - d + S]
            take = allowed & (cand > best)
            best[take], code[take] = cand[take], d
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


def viterbi_align_page(outputs, labels: Sequence[int], optional=None):
    """Places the labels of a page's running text on its lines, in float64.  `outputs`: the K lines' (C, T_k) logits in reading order;
    `labels`: ints in [1, C); `optional`: one bool per label (no two adjacent, neither the first nor the last) -- a label that may be
    absent, as a space of the text is where the line breaks.  Returns ([(label, line, start, end, conf)] -- `line` the index in
    `outputs`, start / end frames within it, a skipped optional label (label, -1, -1, -1, 0.0) --, the page's score, the (K,) sums of
    the path's log-probabilities over each line's frames), or (None, -inf, None) when the text does not fit."""
    lps = [log_softmax64(o) for o in outputs]
    lab = [int(l) for l in labels]
    opt = check_optional(np.zeros(len(lab), dtype=bool) if optional is None else optional, len(lab))
    C = lps[0].shape[0] if lps else 0
    if any(p.ndim != 2 or p.shape[0] != C for p in lps):
        raise ValueError('every line needs (C, T) logits over the same classes')
    if any(l < 1 or l >= C for l in lab):
        raise ValueError(f'labels must lie in [1, {C})')
    lens = [p.shape[1] for p in lps]
    first, brk = page_frames(lens)
    lp = np.concatenate(lps, axis=1) if lps else np.zeros((0, 0))
    states, score = viterbi_page_path(lp, brk, lab, opt)
    if states is None:
        return None, score, None
    line_of = np.repeat(np.arange(len(lens)), lens)
    records = []
    for k, l in enumerate(lab):
        frames = np.nonzero(states == 2 * k + 1)[0]
        if frames.shape[0] == 0:
            records.append((l, -1, -1, -1, 0.0))
            continue
        st, en = int(frames[0]), int(frames[-1])
        ln = int(line_of[st])
        records.append((l, ln, st - int(first[ln]), en - int(first[ln]), float(np.exp(lp[l, st:en + 1].max()))))
    ext = np.zeros(2 * len(lab) + 1, dtype=np.int64)
    ext[1::2] = lab
    emitted = lp[ext[states], np.arange(lp.shape[1])]
    line_scores = np.array([emitted[first[k]:first[k + 1]].sum() for k in range(len(lens))], dtype=np.float64)
    return records, score, line_scores


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


# ---- a page's running text on its lines ----------------------------------------------------------------------------
MAX_PAGE_LABELS, MAX_PAGE_FRAMES, MAX_PAGE_LINES = 4095, 65535, 4096          # the bounds of `cocr_ctc_align_page`; beyond: `viterbi_align_page`
MAX_PAGE_TABLE_BYTES = 1 << 31                                               # ... and of one call's tables


def optional_labels(codec, labels: Sequence[int]) -> np.ndarray:
    """One bool per label: the label is a character of its own with `str.isspace()`, is neither the first nor the last label and
    does not follow another optional one -- a space of the text that the page may not show where its lines break."""
    opt = np.zeros(len(labels), dtype=bool)
    for k in range(1, len(labels) - 1):
        ch = codec.l2c.get((int(labels[k]),))
        opt[k] = bool(ch) and len(ch) == 1 and ch.isspace() and not opt[k - 1]
    return opt


def page_table_words(frames: int, labels: int, max_labels: int) -> int:
    """Words of one page's region in the workspace of `cocr_ctc_align_page` when the call's longest text has `max_labels` labels."""
    S = 2 * max_labels + 1
    sj = 1
    while sj < 8 and 1024 * sj < S:
        sj *= 2
    sp = 64 * sj * max(1, -(-S // (64 * sj)))
    return -(-((frames + 7) // 8 * sp + 2 * frames + 2 * labels) // 4) * 4


def page_result(codec, geoms, aligned, frames: Sequence[int], widths: Sequence[int], pad: int, skipped: str) -> Dict:
    """One page of `align_text_pages` from the returns of `viterbi_align_page` / `collect_align_page` (`aligned`): the records sorted
    onto the page's lines (`geoms`: their `LineGeometry`, `frames` / `widths`: output length and pre-processed width per line), the
    skipped optional labels as `dropped`."""
    from .page import cut_quads
    records, score, line_scores = aligned
    if records is None:
        return {'lines': None, 'score': float(score), 'skipped': skipped, 'dropped': ''}
    per_line = [[] for _ in geoms]
    for l, ln, st, en, cf in records:
        if ln >= 0:
            per_line[ln].append((l, st, en, cf))
    dropped = ''.join(codec.l2c[(int(r[0]),)] for r in records if r[1] < 0)
    lines = []
    for k, g in enumerate(geoms):
        chars = codec.decode(per_line[k])
        cuts = cut_quads(g, chars, widths[k], frames[k], pad) if chars else []
        lines.append({'id': g.id, 'text': ''.join(c[0] for c in chars), 'cuts': cuts, 'words': word_records(cuts),
                      'score': float(line_scores[k]), 'frames': frames[k]})
    return {'lines': lines, 'score': float(score), 'skipped': skipped, 'dropped': dropped}


def align_text_pages(net, pages, texts: Sequence[str], batch_size: int = 32, edge: int = 200, pad: int = 16, fill: int = 0, device: str = 'cuda:0',
                     normalization: Optional[str] = None, normalize_whitespace: bool = True, group_lines: int = 256) -> List[Dict]:
    """`align_pages` with one string per PAGE: places `texts[p]` (through `dataset.normalize_text`; with whitespace normalisation line
    feeds are whitespace) on the lines of `pages[p]` = (image, lines) in their order, whatever text the lines carry.  Per page
    {'lines': [{'id', 'text', 'cuts': [(char, quad, conf)], 'words': [(word, quad, conf)], 'score', 'frames'}] or None where the text
    does not fit the page's frames, 'score', 'skipped': the characters the codec cannot encode, 'dropped': the spaces of the text that
    the path stepped over}.  A line's `score` is the sum of the path's log-probabilities over its `frames`; a line may take no text.

    The forward runs bucketed as in `align_pages`, over groups of whole pages of about `group_lines` lines; a group's logits are
    gathered into one tensor at its widest bucket's frame count by device copies, and `cocr_ctc_align_page` is enqueued behind it on
    the same stream; a group's results are collected after the next group has been enqueued, so the host's share of the next group
    (geometry, extraction tables, launches) runs beside the device's work on this one.  On the device forward and aligner follow one
    another.  A page beyond the kernel's bounds goes through `viterbi_align_page`."""
    import torch
    from . import _lib
    from .dataset import normalize_text
    from .evaluate import make_batches
    from .page import _check_image, line_geometry
    if len(texts) != len(pages):
        raise ValueError('one text per page')
    lib = _lib.load()
    codec = net.codec
    imgs = [_check_image(img) for img, _ in pages]
    enc = [encode_text(codec, normalize_text(t, normalization, normalize_whitespace)) for t in texts]
    opts = [optional_labels(codec, lab) for lab, _ in enc]
    geoms = [[line_geometry(ln.id, ln.baseline, ln.boundary) for ln in lines] for _, lines in pages]
    results: List[Dict] = [None] * len(pages)
    dev = torch.device(device)
    eng = net.engine(dev)
    d_pages = [torch.from_numpy(a).to(dev) for a in imgs]
    height = int(net.height)

    groups, cur, n = [], [], 0                       # whole pages, about `group_lines` lines each
    for p in range(len(pages)):
        if cur and n + len(geoms[p]) > group_lines:
            groups.append(cur)
            cur, n = [], 0
        cur.append(p)
        n += len(geoms[p])
    if cur:
        groups.append(cur)

    def enqueue(group):
        flat = [(p, g) for p in group for g in geoms[p]]
        rows, at = {}, 0
        for p in group:
            rows[p] = list(range(at, at + len(geoms[p])))
            at += len(geoms[p])
        if not flat:
            return group, rows, None, None, None, [], []
        widths = [int(lib.cocr_preproc_width(g.H_s, g.W_s, height, int(pad))) for _, g in flat]
        gathered, frames, w_in = None, np.zeros(len(flat), dtype=np.int64), np.zeros(len(flat), dtype=np.int64)
        for width, idx in make_batches(widths, batch_size, edge):               # widest bucket first
            strips, offs, hs, ws = eng.extract_lines(d_pages, [flat[i] for i in idx], fill=fill)
            im, lens = eng.preprocess_device(strips, offs, hs, ws, height=height, pad=pad, width=width)
            o, olens = net.forward(im.unsqueeze(1), torch.from_numpy(lens))
            if gathered is None:
                gathered = torch.zeros((len(flat), o.shape[1], o.shape[2]), dtype=torch.float32, device=o.device)
            gathered[torch.as_tensor(idx, device=o.device), :o.shape[1]] = o
            frames[idx], w_in[idx] = olens.numpy(), lens
        # calls: the pages the kernel holds, split so that each call's tables stay below the bound
        on_host = [p for p in group if len(enc[p][0]) > MAX_PAGE_LABELS or len(rows[p]) > MAX_PAGE_LINES
                   or int(frames[rows[p]].sum()) > MAX_PAGE_FRAMES]
        calls, call, words, longest = [], [], 0, 0
        for p in group:
            if p in on_host:
                continue
            big = max(longest, len(enc[p][0]))
            need = sum(page_table_words(int(frames[rows[q]].sum()), len(enc[q][0]), big) for q in call + [p])
            if call and need * 4 > MAX_PAGE_TABLE_BYTES:
                calls.append(call)
                call, big = [], len(enc[p][0])
            call.append(p)
            longest = big
        if call:
            calls.append(call)
        handles = [(c, eng.ctc_align_page_async(gathered, frames, [rows[p] for p in c], [enc[p][0] for p in c], [opts[p] for p in c]))
                   for c in calls]
        return group, rows, gathered, frames, w_in, handles, on_host

    def finish(pend):
        group, rows, gathered, frames, w_in, handles, on_host = pend
        aligned = {}
        for c, h in handles:
            for p, res in zip(c, eng.collect_align_page(h)):
                aligned[p] = res
        for p in on_host:
            outs = [gathered[r, :int(frames[r])].transpose(0, 1).cpu().numpy() for r in rows[p]]
            aligned[p] = viterbi_align_page(outs, enc[p][0], opts[p])
        for p in group:
            labels, skipped = enc[p]
            if p not in aligned:                                                  # a page without lines
                fits = not labels
                results[p] = {'lines': [] if fits else None, 'score': 0.0 if fits else -np.inf, 'skipped': skipped, 'dropped': ''}
                continue
            results[p] = page_result(codec, geoms[p], aligned[p], [int(frames[r]) for r in rows[p]], [int(w_in[r]) for r in rows[p]], pad, skipped)

    pending = None
    for group in groups:
        nxt = enqueue(group)
        if pending is not None:
            finish(pending)
        pending = nxt
    if pending is not None:
        finish(pending)
    return results


def gt_file_id(line_id) -> str:
    """A line id as part of a file name: everything but letters, digits, '.', '-' and '_' becomes '_' (an id may hold '/' or ':')."""
    import re
    return re.sub(r'[^\w.-]', '_', str(line_id))


def write_ground_truth(net, image, lines, page_result: Dict, gt_dir: str, stem: str, min_line_score: float = -np.inf, fill: int = 0,
                       device: str = 'cuda:0') -> int:
    """`path`-format ground truth of one aligned page: DIR/<stem>_<line id>.png (the line's straightened strip, `extract_lines`) and
    .gt.txt for every line that took at least one character and whose score per frame is at least `min_line_score`.  Returns the
    number of lines written."""
    import torch
    from PIL import Image
    from .dataset import gt_text_path
    from .page import _check_image, line_geometry
    if page_result['lines'] is None:
        return 0
    keep = [(ln, r) for ln, r in zip(lines, page_result['lines']) if r['text'] and r['score'] / max(r['frames'], 1) >= min_line_score]
    if not keep:
        return 0
    os.makedirs(gt_dir, exist_ok=True)
    img = _check_image(image)
    eng = net.engine(torch.device(device))
    strips, offs, hs, ws = eng.extract_lines([img], [(0, line_geometry(ln.id, ln.baseline, ln.boundary)) for ln, _ in keep], fill=fill)
    host = strips.cpu().numpy()
    ch = 1 if img.ndim == 2 else 3
    for (ln, r), off, h, w in zip(keep, offs, hs, ws):
        strip = host[int(off):int(off) + int(h) * int(w) * ch].reshape((int(h), int(w)) if ch == 1 else (int(h), int(w), 3))
        path = os.path.join(gt_dir, f'{stem}_{gt_file_id(ln.id)}.png')
        Image.fromarray(strip).save(path)
        with open(gt_text_path(path), 'w', encoding='utf-8') as fp:
            fp.write(r['text'] + '\n')
    return len(keep)


# ---- command ------------------------------------------------------------------------------------------------------------------------
def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog='python -m conformer_ocr_amd.align', description='Places the transcription of every line on its line.',
                                 epilog='Not built: writing Word / Glyph / String elements back into the documents, bidi reordering, '
                                        'n-best alignments.')
    ap.add_argument('-m', '--model', default=None, help='safetensors archive or checkpoint')
    ap.add_argument('-f', '--format-type', choices=('page', 'alto', 'xml'), default='xml', help='format of the inputs (xml: told apart by the root element)')
    ap.add_argument('-i', '--input', nargs=2, action='append', metavar=('IN', 'OUT'), default=[],
                    help='document with transcribed lines and the JSON file to write (repeatable)')
    ap.add_argument('--text-input', nargs=3, action='append', metavar=('IN', 'TEXT', 'OUT'), default=[],
                    help='document with segmented lines, the file holding the running text of its page and the JSON file to write (repeatable)')
    ap.add_argument('--gt-dir', default=None, metavar='DIR',
                    help='with --text-input: also write DIR/<page stem>_<line id>.png and .gt.txt for every line that took text (the `-f path` training format)')
    ap.add_argument('--min-line-score', type=float, default=-np.inf, metavar='X',
                    help='with --gt-dir: only lines whose score per frame is at least X (default: all)')
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
    if not args.input and not args.text_input:
        return usage('No input given. Use `-i IN.xml OUT.json` or `--text-input IN.xml TEXT.txt OUT.json`.')
    missing = [f for f in [args.model] + [src for src, _ in args.input] + [f for src, txt, _ in args.text_input for f in (src, txt)]
               if not os.path.exists(f)]
    if missing:
        return usage(f'no such file: {", ".join(missing)}')
    net = None
    if args.text_input:
        rc, net = main_text_pages(args, usage)
        if rc or not args.input:
            return rc
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
    net = net or load_model(args.model, device=args.device)
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


def main_text_pages(args, usage):
    """The `--text-input` half of the command: `align_text_pages` on every (document, text) pair, JSON out, ground truth with --gt-dir.
    Returns (exit status, the loaded model)."""
    from .ocr import load_image, load_model
    from .page import READERS
    docs, pages, texts = [], [], []
    for src, txt, dst in args.text_input:
        page = READERS[args.format_type](src)
        if not page.image:
            return usage(f'{src}: names no image file'), None
        with open(txt, encoding='utf-8') as fp:
            texts.append(fp.read())
        docs.append((src, dst, page.lines))
        pages.append((load_image(os.path.join(os.path.dirname(os.path.abspath(src)), page.image)), page.lines))
    net = load_model(args.model, device=args.device)
    results = align_text_pages(net, pages, texts, batch_size=args.batch_size, edge=args.edge, pad=args.pad, device=args.device,
                               normalization=args.normalization, normalize_whitespace=args.normalize_whitespace)
    worst = []
    for (src, dst, lines), (image, _), res in zip(docs, pages, results):
        with open(dst, 'w', encoding='utf-8') as fp:
            json.dump(res, fp, ensure_ascii=False)
        if res['lines'] is None:
            print(f'{dst}: the text does not fit the page', file=sys.stderr)
            continue
        took = [r for r in res['lines'] if r['text']]
        wrote = ''
        if args.gt_dir:
            n = write_ground_truth(net, image, lines, res, args.gt_dir, os.path.splitext(os.path.basename(src))[0], args.min_line_score,
                                   device=args.device)
            wrote = f', {n} written to {args.gt_dir}'
        print(f'{dst}: {len(took)} of {len(res["lines"])} lines took text, {len(res["dropped"])} spaces dropped at line breaks, '
              f'{len(res["skipped"])} characters skipped{wrote}', file=sys.stderr)
        worst.extend((r['score'] / max(r['frames'], 1), src, r) for r in took)
    if args.worst > 0:
        worst.sort(key=lambda w: w[0])
        for per_frame, src, r in worst[:args.worst]:
            print(f'{per_frame:9.4f}  {src}  {r["id"]}  {r["text"]}', file=sys.stderr)
    return 0, net


if __name__ == '__main__':
    sys.exit(main())
