"""Search index: pruned, quantised frame posteriors packed once, query strings spotted in them without a forward.

    python -m conformer_ocr_amd.index build  -m MODEL -i IN.xml [IN.xml ...] -o CORPUS.cidx [--keep 8] [--step 0.125] [-f page|alto|xml]
                                             [--device cuda:0] [--batch-size 32] [--pad 16] [--edge 200]
    python -m conformer_ocr_amd.index search --index CORPUS.cidx [-q WORD ...] [-Q FILE] [-e REGEX ...] [-E FILE] [--ignore-case] [--hits K]
                                             [--min-conf X] [-u NFD|NFC|NFKD|NFKC] [--no-normalize-whitespace] [--device cuda:0]
                                             [--batch-size 256] OUT.json
    python -m conformer_ocr_amd.index info   --index CORPUS.cidx

`build` runs extraction, pre-processing and the forward of `search` once and keeps, per frame, the `keep` classes of the largest logit
with r_t(c) = logits[t, c] - max_c' logits[t, c'] quantised to steps of `step` (`pack_host` is the definition, `cocr_posterior_pack`
the device form).  `search` needs no model and no images: the file's lines are expanded on the GPU (`cocr_posterior_unpack`) and
handed to the unchanged `cocr_ctc_spot` (regular expressions, `-e` / `-E` / `--ignore-case` as in `search`: `cocr_ctc_spot_pattern`,
DESIGN.md section 7m); OUT.json receives the records of `search.search_pages`, 'page' being the input file the line
came from.  `info` prints what the file holds.

keep = 8 and step = 1/8 (a floor of -31.875 for every class not kept) are placeholders, not tuned: recall against keep / step has not
been measured on real material.

Not built: recall measurements, whole-word matching, anchors, lexicon tries that share prefixes, incremental append to an existing index,
sharded indexes and multi-GPU search, a spot kernel that reads the packed rows directly."""
from __future__ import annotations

import argparse
import json
import math
import os
import struct
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

import numpy as np

FORMAT = 1
MAX_KEEP = 32
MAX_CLASSES = 65535
MAX_CODE = 255
META_KEY = 'posterior_index'


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def inv_step(step: float) -> np.float32:
    """float32(1 / float32(step)), what `pack_host` and `cocr_posterior_pack` multiply by; ValueError unless both are finite and > 0."""
    try:
        with np.errstate(over='ignore'):
            s32 = np.float32(step)
    except (TypeError, ValueError):
        raise ValueError(f'step must be a number, not {step!r}')
    if not (np.isfinite(s32) and s32 > 0):
        raise ValueError(f'step must be finite and positive, not {step!r}')
    with np.errstate(over='ignore'):
        inv = np.float32(1.0 / float(s32))
    if not (np.isfinite(inv) and inv > 0):
        raise ValueError(f'step {step!r} has no finite float32 reciprocal')
    return inv


def _check_keep(keep, C: int) -> int:
    if C > MAX_CLASSES:
        raise ValueError(f'{C} classes: the index holds class ids of 16 bits')
    if int(keep) != keep or not 1 <= int(keep) <= min(C, MAX_KEEP):
        raise ValueError(f'keep must lie in 1..{min(C, MAX_KEEP)}, not {keep!r}')
    return int(keep)


def pack_host(outputs, keep: int = 8, step: float = 0.125) -> Tuple[np.ndarray, np.ndarray]:
    """The (C, T) float32 logits `outputs` (the decoders' orientation) -> (classes (T, keep) uint16, codes (T, keep) uint8).

    Per frame t, with m = max_c x[t, c]: the kept classes are the `keep` classes of the largest logit, ties to the lower class, stored
    in that order (entry 0 is np.argmax's class); code_c = min(255, ceil(float32(float32(m - x[t, c]) * inv_step))) with
    inv_step = `inv_step(step)`: one float32 subtraction, one float32 multiply, ceil -- so code == 0 exactly where x[t, c] == m.
    A difference of +inf (a logit of -inf beside a finite maximum) codes as 255.  NaN is outside the contract."""
    x = np.asarray(outputs, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError('outputs must be a (C, T) matrix')
    C, T = x.shape
    K = _check_keep(keep, C)
    inv = inv_step(step)
    xt = x.T
    order = np.argsort(-xt, axis=1, kind='stable')[:, :K]                      # descending; equal logits keep their class order
    kept = np.take_along_axis(xt, order, axis=1)
    with np.errstate(invalid='ignore', over='ignore'):
        d = (xt.max(axis=1, keepdims=True) - kept).astype(np.float32) if T else kept
        q = np.ceil((d * inv).astype(np.float32))
    codes = np.where(q < MAX_CODE, q, MAX_CODE).astype(np.uint8)
    return np.ascontiguousarray(order.astype(np.uint16)), np.ascontiguousarray(codes)


def expand_host(classes, codes, C: int, step: float = 0.125) -> np.ndarray:
    """The (C, T) float32 table a packed line stands for: -(float32(code) * float32(step)) for the stored classes, -(255 * step) for
    every other class.  Each row's maximum is exactly 0 when entry 0 has code 0 (as `pack_host` writes it), so
    `search.spot_host(expand_host(...), labels, hits, min_score)` IS searching the index.  An entry whose class is >= C is ignored,
    of two entries of one class the later one wins (the device form's rule)."""
    cls = np.asarray(classes)
    cod = np.asarray(codes)
    if cls.ndim != 2 or cls.shape != cod.shape:
        raise ValueError('classes and codes must be (T, keep) matrices of one shape')
    T, K = cls.shape
    C = int(C)
    if C < 1 or C > MAX_CLASSES:
        raise ValueError(f'C must lie in 1..{MAX_CLASSES}')
    if not 1 <= K <= min(C, MAX_KEEP):
        raise ValueError(f'keep must lie in 1..{min(C, MAX_KEEP)}, not {K}')
    inv_step(step)
    s32 = np.float32(step)
    out = np.full((T, C), -(np.float32(MAX_CODE) * s32), dtype=np.float32)
    vals = -(cod.astype(np.float32) * s32)
    rows = np.arange(T)
    for e in range(K):
        ok = cls[:, e] < C
        out[rows[ok], cls[ok, e].astype(np.int64)] = vals[ok, e]
    return np.ascontiguousarray(out.T)


# ---- the file -----------------------------------------------------------------------------------------------------------------------
@dataclass
class Index:
    """A loaded index: `header` (the file's JSON record), classes (sum T, keep) uint16, codes (sum T, keep) uint8 -- the lines' valid
    frames concatenated -- and line_offsets (L + 1) int64."""
    header: Dict
    classes: np.ndarray
    codes: np.ndarray
    line_offsets: np.ndarray
    path: str = None
    _geometry: Dict = field(default_factory=dict, repr=False, compare=False)      # line -> page.LineGeometry, made on first use

    @property
    def keep(self) -> int:
        return int(self.header['keep'])

    @property
    def step(self) -> float:
        return float(self.header['step'])

    @property
    def ncls(self) -> int:
        return int(self.header['ncls'])

    def __len__(self) -> int:
        return int(self.line_offsets.shape[0]) - 1

    def frames(self, line: int) -> int:
        return int(self.line_offsets[line + 1] - self.line_offsets[line])

    def line(self, line: int) -> Tuple[np.ndarray, np.ndarray]:
        a, b = int(self.line_offsets[line]), int(self.line_offsets[line + 1])
        return self.classes[a:b], self.codes[a:b]

    def codec(self):
        from .codec import PytorchCodec
        return PytorchCodec(self.header['codec'])

    def geometry(self, line: int):
        """`page.line_geometry` of the stored baseline and boundary: what `page.cut_quads` places a hit with."""
        if line not in self._geometry:
            from .page import line_geometry
            ln = self.header['lines'][line]
            self._geometry[line] = line_geometry(ln['id'], np.asarray(ln['baseline'], dtype=np.float64), np.asarray(ln['boundary'], dtype=np.float64))
        return self._geometry[line]


def _check_index(header, classes, codes, offsets, name: str) -> None:
    if not isinstance(header, dict) or header.get('format') != FORMAT:
        raise ValueError(f'{name}: index format {header.get("format") if isinstance(header, dict) else header!r}; this build reads format {FORMAT}')
    try:
        keep, ncls, lines = int(header['keep']), int(header['ncls']), header['lines']
        inv_step(header['step'])
        pages = header['pages']
        for k in ('codec', 'height', 'pad', 'subsampling_factor', 'model'):
            header[k]
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError(f'{name}: incomplete index header ({e})')
    if classes.dtype != np.uint16 or codes.dtype != np.uint8 or offsets.dtype != np.int64:
        raise ValueError(f'{name}: tensors of the wrong type')
    if not (1 <= ncls <= MAX_CLASSES and 1 <= keep <= min(ncls, MAX_KEEP)):
        raise ValueError(f'{name}: keep {keep} / {ncls} classes outside the format')
    if classes.ndim != 2 or classes.shape != codes.shape or classes.shape[1] != keep:
        raise ValueError(f'{name}: classes {classes.shape} and codes {codes.shape} disagree with keep {keep}')
    if offsets.ndim != 1 or offsets.shape[0] != len(lines) + 1 or offsets[0] != 0 or offsets[-1] != classes.shape[0] or (np.diff(offsets) < 0).any():
        raise ValueError(f'{name}: line_offsets disagree with {len(lines)} lines of {classes.shape[0]} frames')
    for ln in lines:
        if not 0 <= int(ln['page']) < len(pages):
            raise ValueError(f'{name}: line {ln.get("id")!r} names page {ln["page"]} of {len(pages)}')


def write_index(path, header: Dict, classes: np.ndarray, codes: np.ndarray, line_offsets: np.ndarray) -> None:
    """One safetensors file, written beside `path` and moved over it (as `train.write_state_file` does)."""
    import safetensors.numpy
    header = dict(header, format=FORMAT)
    classes, codes = np.ascontiguousarray(classes, dtype=np.uint16), np.ascontiguousarray(codes, dtype=np.uint8)
    offsets = np.ascontiguousarray(line_offsets, dtype=np.int64)
    _check_index(header, classes, codes, offsets, str(path))
    blob = safetensors.numpy.save({'classes': classes, 'codes': codes, 'line_offsets': offsets}, metadata={META_KEY: json.dumps(header)})
    tmp = f'{path}.tmp'
    with open(tmp, 'wb') as fp:
        fp.write(blob)
    os.replace(tmp, path)


def read_header(path) -> Dict:
    """The JSON record of an index file, without its tensors."""
    with open(path, 'rb') as fp:
        head = fp.read(8)
        try:
            meta = (json.loads(fp.read(struct.unpack('<Q', head)[0])).get('__metadata__') or {}).get(META_KEY)
        except (struct.error, ValueError, MemoryError, OverflowError, AttributeError):
            raise ValueError(f'{path}: not a safetensors file')
    if meta is None:
        raise ValueError(f'{path} is not a search index (no {META_KEY} record)')
    header = json.loads(meta)
    if not isinstance(header, dict) or header.get('format') != FORMAT:
        raise ValueError(f'{path}: index format {header.get("format") if isinstance(header, dict) else header!r}; this build reads format {FORMAT}')
    return header


def load_index(path) -> Index:
    """Reads an index file; ValueError, naming the file, for an unknown version, a cut file or tensors that disagree with the header."""
    import safetensors.numpy
    header = read_header(path)
    with open(path, 'rb') as fp:
        data = fp.read()
    try:
        t = safetensors.numpy.load(data)
        classes, codes, offsets = t['classes'], t['codes'], t['line_offsets']
    except KeyError as e:
        raise ValueError(f'{path}: no tensor {e}')
    except Exception as e:                                  # (the reader's own error type for a cut or damaged file)
        raise ValueError(f'{path}: {e}')
    _check_index(header, classes, codes, offsets, str(path))
    return Index(header, classes, codes, offsets, str(path))


def _loaded(index) -> Index:
    return index if isinstance(index, Index) else load_index(index)


def greedy_records(index: Index, line: int) -> List[Tuple[int, int, int]]:
    """(label, first frame, last frame) of the line's greedy reading, from entry 0 of each frame: the frame's argmax under np.argmax's
    tie rule, so these are the greedy decoder's records on the original logits."""
    lab = index.line(line)[0][:, 0].astype(np.int64)
    T = lab.shape[0]
    if T == 0:
        return []
    cut = np.concatenate([[0], np.nonzero(lab[1:] != lab[:-1])[0] + 1, [T]])
    return [(int(lab[a]), int(a), int(b) - 1) for a, b in zip(cut[:-1], cut[1:]) if lab[a] != 0]


def greedy_text(index: Index, line: int) -> str:
    """The line's 1-best reading, without the model."""
    return ''.join(c[0] for c in index.codec().decode([(l, s, e, 1.0) for l, s, e in greedy_records(index, line)]))


# ---- building -----------------------------------------------------------------------------------------------------------------------
def build_index(net, pages, path, keep: int = 8, step: float = 0.125, batch_size: int = 32, edge: int = 200, pad: int = 16, fill: int = 0,
                device: str = 'cuda:0', names: Sequence[str] = None) -> Index:
    """`page.recognize_pages` / `search.search_pages` with `cocr_posterior_pack` in the decoder's place: every line of `pages`
    ((image, lines) pairs; `names`: what the file calls them, default their indices) packed into the index file `path`.  Same
    bucketing, extraction, pre-processing and forward, so a line's frames are the ones it is recognized and searched on; the previous
    batch is collected while the next one runs.  Lines are stored in page and line order, whatever the batches were.  Returns the
    index as `load_index(path)` reads it."""
    import torch
    from . import _lib
    from .evaluate import make_batches
    from .page import _check_image, line_geometry
    from .train import _model_record
    lib = _lib.load()
    ncls = int(net.hparams_record.num_classes)
    keep = _check_keep(keep, ncls)
    inv_step(step)
    names = [str(i) for i in range(len(pages))] if names is None else [str(n) for n in names]
    if len(names) != len(pages):
        raise ValueError('one name per page')
    imgs = [_check_image(img) for img, _ in pages]
    flat = []                                    # (page, line, geometry)
    for p, (_, lines) in enumerate(pages):
        for ln in lines:
            flat.append((p, ln, line_geometry(ln.id, ln.baseline, ln.boundary)))
    packed: List = [None] * len(flat)
    seq_lens = [0] * len(flat)
    if flat:
        dev = torch.device(device)
        eng = net.engine(dev)
        d_pages = [torch.from_numpy(a).to(dev) for a in imgs]
        height = int(net.height)
        widths = [int(lib.cocr_preproc_width(g.H_s, g.W_s, height, int(pad))) for _, _, g in flat]

        def finish(pend):
            idx, handle, lens = pend
            for n, (i, rec) in enumerate(zip(idx, net.collect_packed(handle))):
                packed[i], seq_lens[i] = rec, int(lens[n])

        pending = None
        for width, idx in make_batches(widths, batch_size, edge):
            strips, offs, hs, ws = eng.extract_lines(d_pages, [(flat[i][0], flat[i][2]) for i in idx], fill=fill)
            im, lens = eng.preprocess_device(strips, offs, hs, ws, height=height, pad=pad, width=width)
            handle = net.pack_posteriors_async(im.unsqueeze(1), torch.from_numpy(lens), keep, step)
            if pending is not None:
                finish(pending)
            pending = (idx, handle, lens)
        finish(pending)
    record = _model_record(net)
    header = {'format': FORMAT, 'keep': keep, 'step': float(np.float32(step)), 'ncls': ncls, 'codec': record['codec'], 'height': int(net.height),
              'pad': int(pad), 'subsampling_factor': int(net.hparams_record.subsampling_factor), 'model': record, 'pages': names,
              'lines': [{'page': p, 'id': str(ln.id), 'seq_len': seq_lens[i],
                         'baseline': np.asarray(ln.baseline, dtype=np.float64).reshape(-1, 2).tolist(),
                         'boundary': np.asarray(ln.boundary, dtype=np.float64).reshape(-1, 2).tolist()} for i, (p, ln, _) in enumerate(flat)]}
    classes = np.concatenate([c for c, _ in packed] + [np.zeros((0, keep), dtype=np.uint16)])
    codes = np.concatenate([c for _, c in packed] + [np.zeros((0, keep), dtype=np.uint8)])
    offsets = np.concatenate([[0], np.cumsum([c.shape[0] for c, _ in packed])]).astype(np.int64)
    write_index(path, header, classes, codes, offsets)
    return load_index(path)


# ---- searching ----------------------------------------------------------------------------------------------------------------------
def _batch_arrays(index: Index, lines: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The lines' packed frames padded to the longest of them: frames past a line's end are class 0 / code 255, as the pack writes them."""
    lens = np.asarray([index.frames(i) for i in lines], dtype=np.int32)
    T = max(int(lens.max()), 1)
    classes = np.zeros((len(lines), T, index.keep), dtype=np.uint16)
    codes = np.full((len(lines), T, index.keep), MAX_CODE, dtype=np.uint8)
    for n, i in enumerate(lines):
        classes[n, :lens[n]], codes[n, :lens[n]] = index.line(i)
    return classes, codes, lens


def search_index(index, queries: Sequence[str] = (), hits: int = 1, min_conf: float = None, batch_size: int = 256, device: str = 'cuda:0',
                 patterns=(), ignore_case: bool = False) -> List[Dict]:
    """`search.search_pages` on an index file (or a loaded `Index`): every query string on every stored line, without model, images or
    forward.  Returns the same records in the same order -- by page, line, query, then best first: {'page': index into the file's
    pages, 'line', 'query', 'start', 'end', 'score', 'conf', 'quad'}, the quad from the stored line geometry -- with the same handling
    of `min_conf`.  A query the stored codec cannot encode completely raises ValueError.

    The scores are those of `search.spot_host` on `expand_host` of the stored entries: at most the scores of the original logits, and
    the same (start, end) for every leading hit of score 0.  Lines are sorted by frame count and batched to the
    batch's longest line: uploaded, expanded by `cocr_posterior_unpack` and searched by `cocr_ctc_spot` on a model-less engine;
    frames past a line's end do not exist for the spotter, so the result does not depend on `batch_size`.  Queries of more than 255
    labels, and everything with device='cpu', go through `spot_host` (float32, the type the device computes in) on `expand_host`.

    `patterns` (regular expressions over the stored codec, compiled with `ignore_case`, or `pattern.PatternGraph`s) are searched as
    `search_pages` searches them: records with 'pattern' and 'match' in place of 'query', after the line's
    query hits.  Chains go through `cocr_ctc_spot`, every other graph through `cocr_ctc_spot_pattern`, with device='cpu' through
    `pattern.spot_pattern_host` (float32); the matched text is `pattern.match_host` on `expand_host` of the line either way."""
    from .align import encode_text
    from .page import cut_quads
    from .pattern import PatternGraph, compile_pattern, labels_text, match_host, spot_pattern_host
    from .search import MAX_DEVICE_HITS, MAX_DEVICE_LABELS, spot_host
    index = _loaded(index)
    codec = index.codec()
    queries = list(queries)
    enc = [encode_text(codec, q) for q in queries]
    bad = [q for q, (lab, sk) in zip(queries, enc) if sk or not lab]
    graphs = [p if isinstance(p, PatternGraph) else compile_pattern(p, codec, ignore_case) for p in patterns]
    bad += [g.text for g in graphs if g.skipped or not g.P]
    if bad or not (queries or graphs):
        raise ValueError(f'queries the codec cannot encode: {bad}' if bad else 'no query')
    nq = len(queries)
    # what is searched: the queries' label strings, then the patterns -- a chain as its label string, any other graph as itself
    labels = [lab for lab, _ in enc] + [g.labels if g.is_chain else None for g in graphs]
    if any(int(c) >= index.ncls for g in graphs for c in g.cls):
        raise ValueError(f'the stored codec uses labels beyond the index\'s {index.ncls} classes')
    if any(l >= index.ncls for lab in labels[:nq] for l in lab):
        raise ValueError(f'the stored codec uses labels beyond the index\'s {index.ncls} classes')
    if not 1 <= int(hits) <= MAX_DEVICE_HITS:
        raise ValueError(f'hits must lie in 1..{MAX_DEVICE_HITS}')
    if int(batch_size) < 1:
        raise ValueError('batch_size must be positive')
    hits = int(hits)
    min_score = -np.inf
    if min_conf is not None and not 0.0 < min_conf <= 1.0:
        raise ValueError('min_conf must lie in (0, 1]')
    if min_conf is not None and not graphs:
        # (search_pages' bound: the loosest any query needs, rounded away from zero; `conf` itself is held to min_conf below.  With
        # patterns the matched length is not known in advance: `conf` alone decides)
        min_score = max(len(l) for l in labels) * math.log(min_conf) * (1.0 + 1e-6) - 1e-6
    L = len(index)
    spots: List[List[List[Tuple]]] = [[[] for _ in labels] for _ in range(L)]           # (start, end, score[, final state])
    on_host = str(device) == 'cpu'
    short = [] if on_host else [i for i, lab in enumerate(labels) if lab is not None and len(lab) <= MAX_DEVICE_LABELS]
    wide = [] if on_host else [i for i, lab in enumerate(labels) if lab is None]             # the graph kernel's
    slow = [i for i in range(len(labels)) if i not in short and i not in wide]
    order = sorted((i for i in range(L) if index.frames(i) > 0), key=lambda i: (index.frames(i), i))
    if (short or wide) and order:
        import torch
        from .ctc_decoder import _scratch_engine
        dev = torch.device(device)
        eng = _scratch_engine(torch.device('cuda', dev.index if dev.index is not None else torch.cuda.current_device()))

        def finish(pend):
            lines, handle, handle_wide = pend
            if handle is not None:
                for i, per_query in zip(lines, eng.collect_spot(handle)):
                    for qi, found in zip(short, per_query):
                        spots[i][qi] = found
            if handle_wide is not None:
                for i, per_pattern in zip(lines, eng.collect_spot_pattern(handle_wide)):
                    for qi, found in zip(wide, per_pattern):
                        spots[i][qi] = found

        pending = None
        with torch.cuda.device(eng.device):
            for at in range(0, len(order), int(batch_size)):
                lines = order[at:at + int(batch_size)]
                classes, codes, lens = _batch_arrays(index, lines)
                table = eng.posterior_unpack(torch.from_numpy(classes).to(eng.device), torch.from_numpy(codes).to(eng.device), index.ncls, index.step)
                handle = eng.ctc_spot_async(table, lens, [labels[qi] for qi in short], hits, min_score) if short else None
                handle_wide = eng.ctc_spot_pattern_async(table, lens, [graphs[qi - nq] for qi in wide], hits, min_score) if wide else None
                if pending is not None:
                    finish(pending)
                pending = (lines, handle, handle_wide)
            finish(pending)
    if slow:
        for i in order:
            table = expand_host(*index.line(i), index.ncls, index.step)
            for qi in slow:
                if labels[qi] is not None:
                    spots[i][qi] = spot_host(table, labels[qi], hits, min_score, dtype=np.float32)
                else:
                    spots[i][qi] = spot_pattern_host(table, graphs[qi - nq], hits, min_score, dtype=np.float32)
    out: List[Dict] = []
    by_page = sorted(range(L), key=lambda i: int(index.header['lines'][i]['page']))          # (stable: the stored order within a page)
    for i in by_page:
        ln = index.header['lines'][i]
        recs = []                                            # (query, start, end, score, conf, matched labels) of the line's hits
        table = None
        for qi, found in enumerate(spots[i]):
            for start, end, score, *final in found:
                matched = labels[qi]
                if matched is None:
                    if table is None:
                        table = expand_host(*index.line(i), index.ncls, index.step)
                    matched = match_host(table, graphs[qi - nq], start, end, final[0])
                conf = math.exp(score / max(len(matched), 1))
                if min_conf is not None and conf < min_conf:
                    if qi < nq:
                        break
                    continue                                 # (a pattern's matches differ in length: a later one may pass)
                recs.append((qi, start, end, score, conf, matched))
        # one call places all of the line's hits (`cut_quads` works element by element: the quads are those of one call per hit)
        quads = cut_quads(index.geometry(i), [(0, r[1], r[2], r[4]) for r in recs], int(ln['seq_len']), index.frames(i), int(index.header['pad']))
        for (qi, start, end, score, conf, matched), (_, quad, _) in zip(recs, quads):
            rec = {'page': int(ln['page']), 'line': ln['id'], 'query': queries[qi]} if qi < nq else \
                {'page': int(ln['page']), 'line': ln['id'], 'pattern': graphs[qi - nq].text, 'match': labels_text(codec, matched)}
            rec.update({'start': start, 'end': end, 'score': score, 'conf': conf, 'quad': quad})
            out.append(rec)
    return out


def index_info(index) -> Dict:
    """What `info` prints: lines, frames, bytes per line of the file's tensors next to the dense float32 logits, keep, step, the model."""
    index = _loaded(index)
    L, frames = len(index), int(index.classes.shape[0])
    packed = index.classes.nbytes + index.codes.nbytes + index.line_offsets.nbytes
    info = {'format': int(index.header['format']), 'pages': len(index.header['pages']), 'lines': L, 'frames': frames, 'keep': index.keep,
            'step': index.step, 'ncls': index.ncls, 'floor': -MAX_CODE * index.step, 'packed_bytes': packed,
            'packed_bytes_per_line': packed / max(L, 1), 'dense_bytes_per_line': frames * index.ncls * 4 / max(L, 1),
            'height': index.header['height'], 'pad': index.header['pad'], 'subsampling_factor': index.header['subsampling_factor'],
            'model': {k: v for k, v in index.header['model'].items() if k != 'codec'}}
    if index.path and os.path.exists(index.path):
        info['file_bytes'] = os.path.getsize(index.path)
        info['file_bytes_per_line'] = info['file_bytes'] / max(L, 1)
    return info


# ---- command ------------------------------------------------------------------------------------------------------------------------
NOT_BUILT = ('Not built: recall measurements against keep / step, whole-word matching, anchors, lexicon tries that share prefixes, incremental '
             'append, sharded indexes and multi-GPU search, a spot kernel that reads the packed rows directly.')


def parser() -> argparse.ArgumentParser:
    from .search import MAX_DEVICE_HITS
    ap = argparse.ArgumentParser(prog='python -m conformer_ocr_amd.index', description='Builds and searches an on-disk index of line posteriors.',
                                 epilog=NOT_BUILT)
    sub = ap.add_subparsers(dest='command', metavar='build|search|info')
    b = sub.add_parser('build', help='pack the posteriors of pages into an index file', epilog=NOT_BUILT)
    b.add_argument('-m', '--model', default=None, help='safetensors archive or checkpoint')
    b.add_argument('-i', '--input', nargs='+', action='extend', metavar='IN', default=[], help='PAGE XML / ALTO documents')
    b.add_argument('-o', '--output', default=None, metavar='CORPUS.cidx')
    b.add_argument('-f', '--format-type', choices=('page', 'alto', 'xml'), default='xml', help='format of the inputs (xml: told apart by the root element)')
    b.add_argument('--keep', type=int, default=8, help=f'classes kept per frame, 1..{MAX_KEEP} (default 8: a placeholder, not tuned on real material)')
    b.add_argument('--step', type=float, default=0.125, help='quantisation step of the log-ratios; classes not kept sit at -255 * step '
                                                             '(default 0.125: a placeholder, not tuned on real material)')
    b.add_argument('-d', '--device', default='cuda:0')
    b.add_argument('-B', '--batch-size', type=int, default=32)
    b.add_argument('--pad', type=int, default=16, help='zero columns left and right of every scaled line (the model\'s training form)')
    b.add_argument('--edge', type=int, default=200, help='width bucket edge: lines are padded to a multiple of it')
    s = sub.add_parser('search', help='find query strings on the lines of an index file', epilog=NOT_BUILT)
    s.add_argument('--index', default=None, metavar='CORPUS.cidx')
    s.add_argument('-q', '--query', action='append', default=[], metavar='WORD', help='string to search for (repeatable)')
    s.add_argument('-Q', '--query-file', default=None, metavar='FILE', help='file with one query per line')
    from .search import add_pattern_arguments
    add_pattern_arguments(s)
    s.add_argument('output', nargs='?', default=None, metavar='OUT.json')
    s.add_argument('--hits', type=int, default=1, metavar='K', help=f'hits per line and query (1..{MAX_DEVICE_HITS})')
    s.add_argument('--min-conf', type=float, default=None, metavar='X', help='drops hits below this per-label confidence (default: none)')
    s.add_argument('-u', '--normalization', choices=('NFD', 'NFKD', 'NFC', 'NFKC'), default=None, help='text normalization of the queries')
    s.add_argument('-n', '--normalize-whitespace', dest='normalize_whitespace', action='store_true', default=True,
                   help='normalizes unicode whitespace (default)')
    s.add_argument('--no-normalize-whitespace', dest='normalize_whitespace', action='store_false')
    s.add_argument('-d', '--device', default='cuda:0', help='cpu: the host definition instead of the kernels')
    s.add_argument('-B', '--batch-size', type=int, default=256)
    i = sub.add_parser('info', help='print what an index file holds')
    i.add_argument('--index', default=None, metavar='CORPUS.cidx')
    return ap


def _build_command(ap, args, usage) -> int:
    if not args.model:
        return usage('No model given.')
    if not args.input or not args.output:
        return usage('No input given. Use `-i IN.xml [IN.xml ...] -o CORPUS.cidx`.')
    missing = [f for f in [args.model] + args.input if not os.path.exists(f)]
    if missing:
        return usage(f'no such file: {", ".join(missing)}')
    try:
        inv_step(args.step)
    except ValueError as e:
        return usage(str(e))
    if not 1 <= args.keep <= MAX_KEEP:
        return usage(f'--keep must lie in 1..{MAX_KEEP}')
    from .ocr import load_image, load_model
    from .page import READERS
    docs = [(src, READERS[args.format_type](src)) for src in args.input]
    pages = []
    for src, page in docs:
        if not page.image:
            return usage(f'{src}: names no image file')
        pages.append((load_image(os.path.join(os.path.dirname(os.path.abspath(src)), page.image)), page.lines))
    net = load_model(args.model, device=args.device)
    if args.keep > net.hparams_record.num_classes:
        return usage(f'--keep {args.keep} exceeds the model\'s {net.hparams_record.num_classes} classes')
    index = build_index(net, pages, args.output, keep=args.keep, step=args.step, batch_size=args.batch_size, edge=args.edge, pad=args.pad,
                        device=args.device, names=[src for src, _ in docs])
    info = index_info(index)
    print(f'{args.output}: {info["lines"]} lines of {info["pages"]} pages, {info["frames"]} frames, keep {info["keep"]}, step {info["step"]:g}, '
          f'{info["packed_bytes_per_line"]:.0f} bytes per line (dense float32: {info["dense_bytes_per_line"]:.0f})', file=sys.stderr)
    return 0


def _search_command(ap, args, usage) -> int:
    from .search import MAX_DEVICE_HITS
    if not args.index:
        return usage('No index given. Use `--index CORPUS.cidx`.')
    if args.output is None:
        return usage('No output given. Name the JSON file to write.')
    if not 1 <= args.hits <= MAX_DEVICE_HITS:
        return usage(f'--hits must lie in 1..{MAX_DEVICE_HITS}')
    if args.min_conf is not None and not 0.0 < args.min_conf <= 1.0:
        return usage('--min-conf must lie in (0, 1]')
    missing = [f for f in [args.index, args.query_file, args.pattern_file] if f and not os.path.exists(f)]
    if missing:
        return usage(f'no such file: {", ".join(missing)}')
    from .dataset import normalize_text
    from .search import compile_for_command, read_patterns
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
    index = load_index(args.index)
    searchable, graphs = compile_for_command(ap.prog, index.codec(), queries, regexes, args.ignore_case, whose='index\'s codec')
    if not searchable and not graphs:
        return usage('no query the index\'s codec can encode')
    found = search_index(index, searchable, hits=args.hits, min_conf=args.min_conf, batch_size=args.batch_size, device=args.device, patterns=graphs)
    names = index.header['pages']
    per_page = [sum(1 for ln in index.header['lines'] if ln['page'] == p) for p in range(len(names))]
    for p, src in enumerate(names):
        mine = [h for h in found if h['page'] == p]
        print(f'{src}: {len(mine)} hits of {len({h.get("query", h.get("pattern")) for h in mine})} of {len(searchable) + len(graphs)} queries on '
              f'{len({h["line"] for h in mine})} of {per_page[p]} lines', file=sys.stderr)
    for h in found:
        h['page'] = names[h['page']]
    with open(args.output, 'w', encoding='utf-8') as fp:
        json.dump(found, fp, ensure_ascii=False)
    return 0


def main(argv=None) -> int:
    ap = parser()
    args = ap.parse_args(argv)

    def usage(msg: str) -> int:
        ap.print_usage(sys.stderr)
        print(f'{ap.prog}: error: {msg}', file=sys.stderr)
        return 1
    if args.command == 'build':
        return _build_command(ap, args, usage)
    try:
        if args.command == 'search':
            return _search_command(ap, args, usage)
        if args.command == 'info':
            if not args.index or not os.path.exists(args.index):
                return usage('No index given. Use `--index CORPUS.cidx`.' if not args.index else f'no such file: {args.index}')
            print(json.dumps(index_info(args.index), ensure_ascii=False, indent=1))
            return 0
    except ValueError as e:                                  # (a file that is no index of this format)
        return usage(str(e))
    return usage('No command given. Use `build`, `search` or `info`.')


if __name__ == '__main__':
    sys.exit(main())
