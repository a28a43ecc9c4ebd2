"""Search: where query strings occur on lines, from the frame posteriors instead of the 1-best reading.

    python -m conformer_ocr_amd.search -m MODEL [-q WORD ...] [-Q FILE] [-e REGEX ...] [-E FILE] [--ignore-case] [--hits K] [--min-conf X]
                                       [-f page|alto|xml] [-u NFD|NFC|NFKD|NFKC] [--no-normalize-whitespace] [--device cuda:0]
                                       [--batch-size 32] [--pad 16] [--edge 200] -i IN.xml [IN.xml ...] OUT.json

IN is a PAGE XML or ALTO file; the image it names is resolved relative to it.  `-Q FILE` reads one query per line.  `-e REGEX` searches
a regular expression (`conformer_ocr_amd.pattern`: syntax and limits), `-E FILE` reads one per line (taken as
written: no normalization); `--ignore-case` folds the case of the patterns' literals and of the `-q` words, which are then compiled as
patterns too.  OUT.json receives the hits of all inputs, {'page', 'line', 'query', 'start', 'end', 'score', 'conf', 'quad'}, a
pattern's hit with 'pattern' and 'match' (the text it matched) in place of 'query' (`search_pages`; 'page' is the input file).
One summary line per file goes to stderr.  No confidence threshold is set by default: none has been measured on real material.

`spot_host` is the definition (host, float64); the device form is `cocr_ctc_spot` (csrc/ctc_spot.hip.h).  Kraken and the reference have
no such operation: the definition is this build's own.

Not built: whole-word matching (a query also matches inside a longer word), anchors, lexicon tries that share prefixes, bidi
reordering (queries are matched in logical order), queries by example.  An on-disk index of posteriors: `conformer_ocr_amd.index`."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
from typing import Dict, List, Sequence, Tuple

import numpy as np

MAX_DEVICE_LABELS = 255          # labels per query the kernel holds (511 states); longer queries: `spot_host`
MAX_DEVICE_HITS = 8


def spot_host(outputs, labels: Sequence[int], hits: int, min_score: float = -np.inf, dtype=np.float64) -> List[Tuple[int, int, float]]:
    """Occurrences of `labels` (ints in [1, C)) in the (C, T) logits `outputs` (the decoders' orientation): up to `hits`
    non-overlapping (start, end, score), best first.

    r_t(c) = logits[t, c] - max_c' logits[t, c'] (<= 0).  States s in [0, 2 L - 1): even = labels[s / 2], odd = blank -- no outer
    blanks, so a hit starts on the first label's first frame and ends on the last label's last frame.  Per frame
        delta_t(s) = best + r_t(class(s)),
    best over the candidates stay, delta_{t-1}(s-1), delta_{t-1}(s-2) (s even, s >= 2, the two labels differ) and, for s = 0, the fresh
    start 0, tried in this order, a candidate replacing the running best only if strictly greater; sigma_t(s) is the frame at which
    the state's path entered state 0 (a fresh start sets it to t).  The candidate of frame t is e_t = delta_t(S-1) with start
    sigma_t(S-1): the log-ratio between the best path spelling the query over [sigma, t] and the unconstrained best path there, 0
    exactly when the query's path is the frame-wise argmax.  Selection, up to `hits` times: the largest live e_t > -inf (ties: the
    largest t); stop if it is < min_score; record it; every live candidate whose [sigma_u, u] intersects it dies.

    `dtype`: the type the recursion runs in (float32: what the device computes)."""
    e, st = spot_candidates(outputs, labels, dtype)
    T = e.shape[0]
    out: List[Tuple[int, int, float]] = []
    alive = e > -np.inf
    frames = np.arange(T)
    while len(out) < int(hits) and alive.any():
        m = e[alive].max()
        if m < min_score:
            break
        t = int(frames[alive & (e == m)][-1])
        s0 = int(st[t])
        out.append((s0, t, float(m)))
        alive &= (frames < s0) | (st > t)
    return out


def spot_candidates(outputs, labels: Sequence[int], dtype=np.float64) -> Tuple[np.ndarray, np.ndarray]:
    """The recursion of `spot_host`: (e (T), sigma (T)) -- per frame the score of the best occurrence ending there (-inf: none) and
    its first frame (-1: none)."""
    dt = np.dtype(dtype).type
    x = np.asarray(outputs)
    if x.ndim != 2:
        raise ValueError('outputs must be a (C, T) matrix')
    C, T = x.shape
    lab = np.asarray([int(l) for l in labels], dtype=np.int64)
    L = lab.shape[0]
    if L == 0:
        raise ValueError('an empty query')
    if ((lab < 1) | (lab >= C)).any():
        raise ValueError(f'labels must lie in [1, {C})')
    S = 2 * L - 1
    cls = np.zeros(S, dtype=np.int64)
    cls[0::2] = lab
    skip = np.zeros(S, dtype=bool)
    skip[2::2] = lab[1:] != lab[:-1]
    e, st = np.full(T, -np.inf, dtype=dt), np.full(T, -1, dtype=np.int64)
    if T == 0:
        return e, st
    xs = x.astype(dt)
    r = (xs - xs.max(axis=0, keepdims=True)).astype(dt)[cls]            # (S, T)
    NEG = dt(-np.inf)
    delta, sigma = np.full(S + 2, NEG, dtype=dt), np.full(S + 2, -1, dtype=np.int64)      # two cells of padding in front
    for t in range(T):
        best, src = delta[2:].copy(), sigma[2:].copy()
        take = delta[1:S + 1] > best
        best[take], src[take] = delta[1:S + 1][take], sigma[1:S + 1][take]
        take = skip & (delta[:S] > best)
        best[take], src[take] = delta[:S][take], sigma[:S][take]
        if dt(0) > best[0]:
            best[0], src[0] = dt(0), t
        reached = best > NEG
        delta[2:] = np.where(reached, best + r[:, t], NEG)
        sigma[2:] = np.where(reached, src, -1)
        e[t], st[t] = delta[-1], sigma[-1]
    return e, st


# ---- pages --------------------------------------------------------------------------------------------------------------------------
def search_pages(net, pages, queries: Sequence[str] = (), hits: int = 1, min_conf: float = None, batch_size: int = 32, edge: int = 200,
                 pad: int = 16, fill: int = 0, device: str = 'cuda:0', patterns=(), ignore_case: bool = False) -> List[Dict]:
    """`page.recognize_pages` with `cocr_ctc_spot` in the decoder's place: every query string on every line of `pages` ((image, lines)
    pairs).  Returns the hits, ordered by page, line, query and then best first: {'page': index into `pages`, 'line': the line's id,
    'query', 'start', 'end' (frames), 'score', 'conf' = exp(score / labels of the query), 'quad': 4 (x, y) page points from the first
    label's left edge to the last label's right edge (`page.cut_quads` on the record (0, start, end, conf))}.  `min_conf`: hits of
    lower `conf` are dropped (None: no threshold).  A query the codec cannot encode completely raises ValueError.

    `patterns`: regular expressions (`pattern.compile_pattern` over the model's codec, with `ignore_case`) or `pattern.PatternGraph`s,
    searched beside the queries.  Their hits follow a line's query hits, in the patterns' order, and carry
    'pattern' (the pattern's text) in place of 'query' and 'match', the text the hit matched; `conf` = exp(score / labels matched) and
    `quad` come from the matched span.  A pattern whose graph is a plain chain goes through `cocr_ctc_spot`; the queries themselves are
    untouched by `ignore_case`.  A pattern the codec cannot express, or one the compiler refuses, raises ValueError.

    Same bucketing and the same extraction, pre-processing and forward as `recognize_pages`, so a line's frames are the ones it is
    recognized on; the previous batch's hits are collected while the next one runs."""
    import torch
    from . import _lib
    from .align import encode_text
    from .evaluate import make_batches
    from .page import _check_image, cut_quads, line_geometry
    lib = _lib.load()
    from .pattern import PatternGraph, chain_graph, compile_pattern, labels_text
    queries = list(queries)
    enc = [encode_text(net.codec, q) for q in queries]
    bad = [q for q, (lab, sk) in zip(queries, enc) if sk or not lab]
    graphs = [p if isinstance(p, PatternGraph) else compile_pattern(p, net.codec, ignore_case) for p in patterns]
    bad += [g.text for g in graphs if g.skipped or not g.P]
    if bad or not (queries or graphs):
        raise ValueError(f'queries the codec cannot encode: {bad}' if bad else 'no query')
    labels = [lab for lab, _ in enc]
    if graphs and any(len(l) > MAX_DEVICE_LABELS for l in labels):
        raise ValueError(f'a query of more than {MAX_DEVICE_LABELS} labels cannot share a call with patterns')
    min_score = -np.inf
    if min_conf is not None and not 0.0 < min_conf <= 1.0:
        raise ValueError('min_conf must lie in (0, 1]')
    if min_conf is not None and not graphs:          # (with patterns the matched length is not known in advance: `conf` alone decides)
        # one bound for the whole call, the loosest any query needs (rounded away from zero); `conf` itself is held to min_conf below
        min_score = max(len(l) for l in labels) * math.log(min_conf) * (1.0 + 1e-6) - 1e-6
    imgs = [_check_image(img) for img, _ in pages]
    flat = []                                    # (page, line within page, geometry)
    for p, (_, lines) in enumerate(pages):
        for j, ln in enumerate(lines):
            flat.append((p, j, line_geometry(ln.id, ln.baseline, ln.boundary)))
    found: List[Tuple[int, int, List[Dict]]] = []
    if not flat:
        return []
    dev = torch.device(device)
    eng = net.engine(dev)
    d_pages = [torch.from_numpy(a).to(dev) for a in imgs]
    height = int(net.height)
    widths = [int(lib.cocr_preproc_width(g.H_s, g.W_s, height, int(pad))) for _, _, g in flat]
    batches = make_batches(widths, batch_size, edge)

    # with patterns, one forward serves both: the queries ride along as chains (which `spot_patterns_async` sends through cocr_ctc_spot)
    everything = [chain_graph(l, q) for l, q in zip(labels, queries)] + graphs

    def finish(pend):
        idx, handle, lens = pend
        if graphs:
            per_line, olens, _ = net.collect_spot_patterns(handle)
        else:
            per_line, olens = net.collect_spot_labels(handle)
        for n, i in enumerate(idx):
            p, j, g = flat[i]
            W_in = int(lens[n])
            recs = []
            for qi, spots in enumerate(per_line[n]):
                for start, end, score, *matched in spots:
                    n_labels = len(matched[0]) if qi >= len(queries) else len(labels[qi])
                    conf = math.exp(score / max(n_labels, 1))
                    if min_conf is not None and conf < min_conf:
                        if qi < len(queries):
                            break
                        continue                             # (a pattern's matches differ in length: a later one may pass)
                    quad = cut_quads(g, [(0, start, end, conf)], W_in, int(olens[n]), pad)[0][1]
                    rec = {'page': p, 'line': g.id, 'query': queries[qi]} if qi < len(queries) else \
                        {'page': p, 'line': g.id, 'pattern': everything[qi].text, 'match': labels_text(net.codec, matched[0])}
                    rec.update({'start': start, 'end': end, 'score': score, 'conf': conf, 'quad': quad})
                    recs.append(rec)
            found.append((p, j, recs))

    pending = None
    for width, idx in batches:
        strips, offs, hs, ws = eng.extract_lines(d_pages, [(flat[i][0], flat[i][2]) for i in idx], fill=fill)
        im, lens = eng.preprocess_device(strips, offs, hs, ws, height=height, pad=pad, width=width)
        if graphs:
            handle = net.spot_patterns_async(im.unsqueeze(1), torch.from_numpy(lens), everything, hits=hits, min_score=min_score)
        else:
            handle = net.spot_labels_async(im.unsqueeze(1), torch.from_numpy(lens), labels, hits=hits, min_score=min_score)
        if pending is not None:
            finish(pending)
        pending = (idx, handle, lens)
    finish(pending)
    found.sort(key=lambda f: f[:2])
    return [r for _, _, recs in found for r in recs]


# ---- command ------------------------------------------------------------------------------------------------------------------------
def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog='python -m conformer_ocr_amd.search', description='Finds query strings on the lines of pages.',
                                 epilog='Not built: whole-word matching, anchors, lexicon tries that share prefixes, bidi '
                                        'reordering, queries by example.  Many queries of the same pages: python -m conformer_ocr_amd.index.')
    ap.add_argument('-m', '--model', default=None, help='safetensors archive or checkpoint')
    ap.add_argument('-q', '--query', action='append', default=[], metavar='WORD', help='string to search for (repeatable)')
    ap.add_argument('-Q', '--query-file', default=None, metavar='FILE', help='file with one query per line')
    add_pattern_arguments(ap)
    ap.add_argument('-f', '--format-type', choices=('page', 'alto', 'xml'), default='xml', help='format of the inputs (xml: told apart by the root element)')
    ap.add_argument('-i', '--input', nargs='+', action='extend', metavar='IN', default=[], help='documents to search; the JSON file to write follows them')
    ap.add_argument('output', nargs='?', default=None, metavar='OUT.json')
    ap.add_argument('--hits', type=int, default=1, metavar='K', help=f'hits per line and query (1..{MAX_DEVICE_HITS})')
    ap.add_argument('--min-conf', type=float, default=None, metavar='X', help='drops hits below this per-label confidence (default: none)')
    ap.add_argument('-u', '--normalization', choices=('NFD', 'NFKD', 'NFC', 'NFKC'), default=None, help='text normalization of the queries')
    ap.add_argument('-n', '--normalize-whitespace', dest='normalize_whitespace', action='store_true', default=True,
                    help='normalizes unicode whitespace (default)')
    ap.add_argument('--no-normalize-whitespace', dest='normalize_whitespace', action='store_false')
    ap.add_argument('-d', '--device', default='cuda:0')
    ap.add_argument('-B', '--batch-size', type=int, default=32)
    ap.add_argument('--pad', type=int, default=16, help='zero columns left and right of every scaled line (the model\'s training form)')
    ap.add_argument('--edge', type=int, default=200, help='width bucket edge: lines are padded to a multiple of it')
    return ap


def add_pattern_arguments(ap: argparse.ArgumentParser) -> None:
    """The pattern options the search and index commands share."""
    ap.add_argument('-e', '--pattern', action='append', default=[], metavar='REGEX', help='regular expression to search for (repeatable)')
    ap.add_argument('-E', '--pattern-file', default=None, metavar='FILE', help='file with one regular expression per line')
    ap.add_argument('--ignore-case', action='store_true', help='folds the case of the patterns\' literals and of the -q words')


def read_patterns(args) -> List[str]:
    """The pattern texts of a command line, each once, in order."""
    raw = list(args.pattern)
    if args.pattern_file:
        with open(args.pattern_file, encoding='utf-8') as fp:
            raw.extend(l.rstrip('\n') for l in fp)
    return [t for t in dict.fromkeys(raw) if t]


def compile_for_command(prog: str, codec, queries: Sequence[str], patterns: Sequence[str], ignore_case: bool, whose: str = 'model'):
    """What a command searches: (the queries kept as strings, the graphs).  With `ignore_case` the queries become graphs too (their
    text is the query).  Whatever the codec cannot express, or the compiler refuses, is reported on stderr and left out."""
    from .align import encode_text
    from .pattern import compile_pattern, escape
    kept, graphs = [], []
    for q in queries:
        lab, skipped = encode_text(codec, q)
        if skipped or not lab:
            print(f'{prog}: query {q!r} skipped: the {whose} cannot encode {skipped!r}', file=sys.stderr)
        elif ignore_case:
            g = compile_pattern(escape(q), codec, True)
            g.text = q
            graphs.append(g)
        else:
            kept.append(q)
    for t in patterns:
        try:
            g = compile_pattern(t, codec, ignore_case)
        except ValueError as e:
            print(f'{prog}: pattern {t!r} skipped: {e}', file=sys.stderr)
            continue
        if g.skipped or not g.P:
            print(f'{prog}: pattern {t!r} skipped: the {whose} cannot encode {g.skipped!r}', file=sys.stderr)
        else:
            graphs.append(g)
    return kept, graphs


def main(argv=None) -> int:
    ap = parser()
    args = ap.parse_args(argv)

    def usage(msg: str) -> int:
        ap.print_usage(sys.stderr)
        print(f'{ap.prog}: error: {msg}', file=sys.stderr)
        return 1
    inputs, output = list(args.input), args.output
    if output is None and len(inputs) >= 2:                   # `-i A.xml B.xml OUT.json`: the list took the output with it
        output = inputs.pop()
    if not args.model:
        return usage('No model given.')
    if not inputs or output is None:
        return usage('No input given. Use `-i IN.xml [IN.xml ...] OUT.json`.')
    if not 1 <= args.hits <= MAX_DEVICE_HITS:
        return usage(f'--hits must lie in 1..{MAX_DEVICE_HITS}')
    if args.min_conf is not None and not 0.0 < args.min_conf <= 1.0:
        return usage('--min-conf must lie in (0, 1]')
    missing = [f for f in [args.model, args.query_file, args.pattern_file] + inputs if f and not os.path.exists(f)]
    if missing:
        return usage(f'no such file: {", ".join(missing)}')
    from .dataset import normalize_text
    raw = list(args.query)
    if args.query_file:
        with open(args.query_file, encoding='utf-8') as fp:
            raw.extend(l.rstrip('\n') for l in fp)
    queries = []
    for q in raw:
        q = normalize_text(q, args.normalization, args.normalize_whitespace)
        if q and q not in queries:
            queries.append(q)
    regexes = read_patterns(args)
    if not queries and not regexes:
        return usage('No query given. Use `-q WORD`, `-Q FILE`, `-e REGEX` or `-E FILE`.')
    from .page import READERS
    docs = [(src, READERS[args.format_type](src)) for src in inputs]
    from .ocr import load_image, load_model
    pages = []
    for src, page in docs:
        if not page.image:
            return usage(f'{src}: names no image file')
        pages.append((load_image(os.path.join(os.path.dirname(os.path.abspath(src)), page.image)), page.lines))
    net = load_model(args.model, device=args.device)
    searchable, graphs = compile_for_command(ap.prog, net.codec, queries, regexes, args.ignore_case)
    if not searchable and not graphs:
        return usage('no query the model can encode')
    found = search_pages(net, pages, searchable, hits=args.hits, min_conf=args.min_conf, batch_size=args.batch_size, edge=args.edge,
                         pad=args.pad, device=args.device, patterns=graphs)
    for h in found:
        h['page'] = docs[h['page']][0]
    with open(output, 'w', encoding='utf-8') as fp:
        json.dump(found, fp, ensure_ascii=False)
    for src, page in docs:
        mine = [h for h in found if h['page'] == src]
        print(f'{src}: {len(mine)} hits of {len({h.get("query", h.get("pattern")) for h in mine})} of {len(searchable) + len(graphs)} queries on '
              f'{len({h["line"] for h in mine})} of {len(page.lines)} lines', file=sys.stderr)
    return 0


if __name__ == '__main__':
    sys.exit(main())
