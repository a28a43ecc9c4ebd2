"""Whole-page recognition: a page image plus a baseline segmentation (PAGE XML or ALTO, as kraken's segmenter writes them) -> the
text of every line, with per-character positions in page coordinates.

The reference's `cocr ocr` (README.rst:32-39) hands this step to kraken (`rpred` -> `extract_polygons`: a host-side piecewise-affine
warp per line).  Here each line's baseline and boundary polygon become a per-column frame on the host (`line_geometry`, float64,
DESIGN.md section 7), the GPU cuts and straightens every line of a batch in one launch (`cocr_extract_lines`, csrc/page.hip.h), and
the strips go on to the existing pre-processing (`cocr_preproc_lines`) and recognizer without a host round trip.  The semantics are
this project's own and are not pinned against kraken (not installed)."""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_STRIP_HEIGHT = 4096
MAX_STRIP_WIDTH = 65535
MAX_VERTICES = 4096
MAX_COORD = float(1 << 24)       # |coordinate| bound of the device path (int64 fixed-point products)
FIX = 65536.0                    # column frames are int64 in 1/65536 px


@dataclass
class Line:
    """One text line of a segmentation: `baseline` (n, 2) polyline in reading order, `boundary` (V, 2) closed polygon, page pixels;
    `text` its ground truth as the document gives it (None if it has none)."""
    id: str
    baseline: np.ndarray
    boundary: np.ndarray
    text: Optional[str] = None


@dataclass
class Page:
    """A parsed PAGE / ALTO document: the image file name as written in it (relative to the XML) and its lines in document order."""
    image: str
    lines: List[Line] = field(default_factory=list)


@dataclass
class LineGeometry:
    """DESIGN.md section 7 for one line: the deduplicated baseline `points` (m+1, 2), segment lengths `seg_len` (m,), cumulative arc
    length `arc` (m+1,), unit directions `dirs` / normals `normals` (m, 2), vertex normals `vnormals` (m+1, 2), the integer boundary
    `verts` (V, 2) int32, the strip's `T` rows above and `Bt` below the baseline row, `H_s` x `W_s`, and `cols` (W_s, 4) int64: per
    strip column (Bx, By, Nx, Ny) in 1/65536 px."""
    id: str
    points: np.ndarray
    seg_len: np.ndarray
    arc: np.ndarray
    dirs: np.ndarray
    normals: np.ndarray
    vnormals: np.ndarray
    verts: np.ndarray
    top: float
    bottom: float
    T: int
    Bt: int
    H_s: int
    W_s: int
    cols: np.ndarray

    @property
    def length(self) -> float:
        return float(self.arc[-1])

    def frame(self, s) -> Tuple[np.ndarray, np.ndarray]:
        """Baseline point B(s) and unit normal N(s), float64 (..., 2), at arc lengths `s` (fractional allowed)."""
        return _frame(self.points, self.seg_len, self.arc, self.vnormals, self.normals, np.asarray(s, dtype=np.float64))


def _frame(P, L, A, nu, n, s):
    m = L.shape[0]
    k = np.clip(np.searchsorted(A[:m], s, side='right') - 1, 0, m - 1)
    t = (s - A[k]) / L[k]
    bx = P[k, 0] + t * (P[k + 1, 0] - P[k, 0])
    by = P[k, 1] + t * (P[k + 1, 1] - P[k, 1])
    vx = (1.0 - t) * nu[k, 0] + t * nu[k + 1, 0]
    vy = (1.0 - t) * nu[k, 1] + t * nu[k + 1, 1]
    nn = np.sqrt(vx * vx + vy * vy)
    zero = nn == 0.0                       # opposite vertex normals (a baseline that doubles back): the segment's own normal
    nn = np.where(zero, 1.0, nn)
    nx = np.where(zero, n[k, 0], vx / nn)
    ny = np.where(zero, n[k, 1], vy / nn)
    return np.stack([bx, by], -1), np.stack([nx, ny], -1)


def line_geometry(line_id: str, baseline, boundary) -> LineGeometry:
    """Host geometry of one line.  Raises ValueError, naming the line, for a baseline of fewer than 2 distinct
    points, a boundary of fewer than 3 or more than 4096 vertices, a strip over 4096 x 65535, or coordinates beyond +-2^24 px."""
    P = np.asarray(baseline, dtype=np.float64).reshape(-1, 2)
    Q = np.asarray(boundary, dtype=np.float64).reshape(-1, 2)
    if not (np.isfinite(P).all() and np.isfinite(Q).all()):
        raise ValueError(f'line {line_id!r}: non-finite coordinates')
    if P.shape[0]:
        keep = np.concatenate([[True], np.any(P[1:] != P[:-1], axis=1)])
        P = P[keep]
    if P.shape[0] < 2:
        raise ValueError(f'line {line_id!r}: the baseline has fewer than 2 distinct points')
    if not 3 <= Q.shape[0] <= MAX_VERTICES:
        raise ValueError(f'line {line_id!r}: {Q.shape[0]} boundary vertices (3 .. {MAX_VERTICES})')
    if np.abs(P).max() > MAX_COORD or np.abs(Q).max() > MAX_COORD:
        raise ValueError(f'line {line_id!r}: coordinates beyond +-2^24 px')
    V = np.rint(Q)
    m = P.shape[0] - 1
    dx, dy = P[1:, 0] - P[:-1, 0], P[1:, 1] - P[:-1, 1]
    L2 = dx * dx + dy * dy
    L = np.sqrt(L2)
    A = np.concatenate([[0.0], np.cumsum(L)])
    d = np.stack([dx / L, dy / L], -1)
    n = np.stack([-d[:, 1], d[:, 0]], -1)
    nu = np.empty((m + 1, 2))
    nu[0], nu[m] = n[0], n[m - 1]
    if m > 1:
        sx, sy = n[:-1, 0] + n[1:, 0], n[:-1, 1] + n[1:, 1]
        sn = np.sqrt(sx * sx + sy * sy)
        zero = sn == 0.0
        sn1 = np.where(zero, 1.0, sn)
        nu[1:m, 0] = np.where(zero, n[1:, 0], sx / sn1)
        nu[1:m, 1] = np.where(zero, n[1:, 1], sy / sn1)
    # nearest segment of every boundary vertex (point-to-segment distance, ties to the lowest k), signed distance along its normal
    qx, qy = V[:, 0:1], V[:, 1:2]
    u = np.clip(((qx - P[:-1, 0]) * dx + (qy - P[:-1, 1]) * dy) / L2, 0.0, 1.0)
    cx, cy = P[:-1, 0] + u * dx, P[:-1, 1] + u * dy
    dist2 = (qx - cx) * (qx - cx) + (qy - cy) * (qy - cy)
    ks = np.argmin(dist2, axis=1)
    delta = (V[:, 0] - P[ks, 0]) * n[ks, 0] + (V[:, 1] - P[ks, 1]) * n[ks, 1]
    top = max(0.0, float(np.max(-delta)))
    bottom = max(0.0, float(np.max(delta)))
    T, Bt = int(math.ceil(top)), int(math.ceil(bottom))
    H_s, W_s = T + Bt + 1, int(math.floor(A[-1])) + 1
    if H_s > MAX_STRIP_HEIGHT or W_s > MAX_STRIP_WIDTH:
        raise ValueError(f'line {line_id!r}: strip of {H_s} x {W_s} px exceeds {MAX_STRIP_HEIGHT} x {MAX_STRIP_WIDTH}')
    B, N = _frame(P, L, A, nu, n, np.arange(W_s, dtype=np.float64))
    cols = np.rint(np.concatenate([B, N], axis=1) * FIX).astype(np.int64)
    return LineGeometry(str(line_id), P, L, A, d, n, nu, V.astype(np.int32), top, bottom, T, Bt, H_s, W_s, np.ascontiguousarray(cols))


def cut_quads(geom: LineGeometry, records: Sequence[Tuple], seq_len: int, out_len: int, pad: int):
    """Greedy records (label or char, start, end, conf) of a line -> [(label, quad, conf)], quad = 4 (x, y) page points (DESIGN.md
    section 7, cuts): frames -> strip columns through the scaling and padding of the pre-processing, the strip's top and bottom
    edges at those columns."""
    if not records:
        return []
    w_sc = seq_len - 2 * pad
    f = np.array([[r[1], r[2] + 1] for r in records], dtype=np.float64)
    s = np.clip((f * seq_len / out_len - pad) * geom.W_s / w_sc, 0.0, geom.length)          # (n, 2): s0, s1 per record
    B, N = geom.frame(s)
    top, bot = (B - geom.T * N).tolist(), (B + geom.Bt * N).tolist()
    return [(r[0], [tuple(top[i][0]), tuple(top[i][1]), tuple(bot[i][1]), tuple(bot[i][0])], r[3]) for i, r in enumerate(records)]


# ---- readers ----------------------------------------------------------------------------------------------------------------
def _local(tag) -> str:
    return tag.rsplit('}', 1)[-1] if isinstance(tag, str) else ''


def _points(text: Optional[str]) -> Optional[np.ndarray]:
    """'x,y x,y ...' or 'x y x y ...' -> (n, 2) float64; None if empty or odd."""
    if not text or not text.strip():
        return None
    vals = text.replace(',', ' ').split()
    if len(vals) % 2:
        return None
    try:
        return np.array([float(v) for v in vals], dtype=np.float64).reshape(-1, 2)
    except ValueError:
        return None


def _child(el, name):
    for c in el:
        if _local(c.tag) == name:
            return c
    return None


def _warn_skipped(path, skipped):
    if skipped:
        warnings.warn(f'{path}: skipped {len(skipped)} line(s) without a baseline or boundary polygon: {", ".join(skipped)}')


def _page_text(line_el) -> Optional[str]:
    """TextLine/TextEquiv/Unicode of the line's DIRECT TextEquiv children (Word / Glyph level ones are not read): the one of smallest
    `index` if any carries an index, else the first; None without a TextEquiv or Unicode element."""
    eqs = [c for c in line_el if _local(c.tag) == 'TextEquiv']
    if not eqs:
        return None

    def index(e):
        try:
            return int(e.get('index'))
        except (TypeError, ValueError):
            return None
    indexed = [e for e in eqs if index(e) is not None]
    eq = min(indexed, key=index) if indexed else eqs[0]
    uni = _child(eq, 'Unicode')
    return None if uni is None else (uni.text or '')


def _alto_text(line_el) -> Optional[str]:
    """The TextLine's String@CONTENT, SP (one space) and HYP@CONTENT children in document order; None if it has none."""
    parts = []
    for c in line_el:
        tag = _local(c.tag)
        if tag in ('String', 'HYP'):
            parts.append(c.get('CONTENT', ''))
        elif tag == 'SP':
            parts.append(' ')
    return ''.join(parts) if parts else None


def read_page_xml(path) -> Page:
    """PAGE XML (any schema version: namespaces are ignored): Page@imageFilename, TextLine@id, TextLine/Coords@points,
    TextLine/Baseline@points, TextLine/TextEquiv/Unicode (`_page_text`).  Lines without a baseline or polygon are skipped with a
    warning naming them."""
    import xml.etree.ElementTree as ET
    root = ET.parse(path).getroot()
    image = ''
    for el in root.iter():
        if _local(el.tag) == 'Page':
            image = el.get('imageFilename', '')
            break
    lines, skipped = [], []
    for el in root.iter():
        if _local(el.tag) != 'TextLine':
            continue
        lid = el.get('id', f'line_{len(lines) + len(skipped)}')
        coords, base = _child(el, 'Coords'), _child(el, 'Baseline')
        bl = _points(base.get('points')) if base is not None else None
        bd = _points(coords.get('points')) if coords is not None else None
        if bl is None or bd is None:
            skipped.append(lid)
            continue
        lines.append(Line(lid, bl, bd, _page_text(el)))
    _warn_skipped(path, skipped)
    return Page(image, lines)


def read_alto(path) -> Page:
    """ALTO (any version: namespaces are ignored): sourceImageInformation/fileName, TextLine@ID, TextLine@BASELINE ('x,y x,y' or
    'x y x y'), TextLine/Shape/Polygon@POINTS, the line's text (`_alto_text`).  Lines without a baseline or polygon are skipped with
    a warning naming them."""
    import xml.etree.ElementTree as ET
    root = ET.parse(path).getroot()
    image = ''
    for el in root.iter():
        if _local(el.tag) == 'sourceImageInformation':
            fn = _child(el, 'fileName')
            image = (fn.text or '').strip() if fn is not None else ''
            break
    lines, skipped = [], []
    for el in root.iter():
        if _local(el.tag) != 'TextLine':
            continue
        lid = el.get('ID', f'line_{len(lines) + len(skipped)}')
        bl = _points(el.get('BASELINE'))
        shape = _child(el, 'Shape')
        poly = _child(shape, 'Polygon') if shape is not None else None
        bd = _points(poly.get('POINTS')) if poly is not None else None
        if bl is None or bd is None:
            skipped.append(lid)
            continue
        lines.append(Line(lid, bl, bd, _alto_text(el)))
    _warn_skipped(path, skipped)
    return Page(image, lines)


def read_xml(path) -> Page:
    """PAGE or ALTO, told apart by the root element (PcGts / alto, namespaces ignored)."""
    import xml.etree.ElementTree as ET
    for _, el in ET.iterparse(path, events=('start',)):
        root = _local(el.tag)
        break
    else:
        root = ''
    if root == 'PcGts':
        return read_page_xml(path)
    if root.lower() == 'alto':
        return read_alto(path)
    raise ValueError(f'{path}: root element <{root}> is neither PAGE (PcGts) nor ALTO (alto)')


READERS = {'page': read_page_xml, 'alto': read_alto, 'xml': read_xml}


# ---- recognition ------------------------------------------------------------------------------------------------------------
def _check_image(image) -> np.ndarray:
    a = np.asarray(image)
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
        raise ValueError('a page is an (H, W) or (H, W, 3) uint8 image')
    if a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f'empty page image of shape {a.shape}')
    return np.ascontiguousarray(a)


def recognize_pages(net, pages: Sequence[Tuple[np.ndarray, Sequence[Line]]], batch_size: int = 32, edge: int = 200, pad: int = 16,
                    fill: int = 0, device: str = 'cuda:0', nbest: int = 0) -> List[List[Dict]]:
    """Text of every line of `pages` ((image, lines) pairs: (H, W) gray or (H, W, 3) RGB uint8 images, `Line`s).  Returns per page, in
    the order of its lines, {'id', 'text', 'cuts': [(char, quad, conf)]} with quads in page pixels.  nbest > 0 (a beam decoder is
    required): every record also has 'nbest', `net.predict_nbest`'s [(text, logp, lm_logp, label records)]; 'text' and 'cuts' are
    those of its first entry, which is the 1-best reading.

    All lines of all pages are bucketed together by the widths they have after scaling (`make_batches`, like `recognize_crops`), so a
    line's string is the one `recognize_crops` gives for its strip.  Per batch: `cocr_extract_lines` cuts the strips out of the pages
    (which stay in device memory for the whole call), `cocr_preproc_lines` scales them, the forward and `net.ctc_decoder`'s device decode
    are enqueued, and the previous batch's records are collected while it runs.  Errors (bad or oversize lines, empty page images)
    raise ValueError before anything is launched."""
    import torch
    from . import _lib
    from .evaluate import make_batches
    lib = _lib.load()
    imgs = [_check_image(img) for img, _ in pages]
    flat: List[Tuple[int, int, LineGeometry]] = []          # (page, line within page, geometry)
    for p, (_, lines) in enumerate(pages):
        for j, ln in enumerate(lines):
            flat.append((p, j, line_geometry(ln.id, ln.baseline, ln.boundary)))
    results: List[List[Dict]] = [[None] * len(lines) for _, lines in pages]
    if not flat:
        return results
    dev = torch.device(device)
    eng = net.engine(dev)
    d_pages = [torch.from_numpy(a).to(dev) for a in imgs]
    height = int(net.height)
    widths = [int(lib.cocr_preproc_width(g.H_s, g.W_s, height, int(pad))) for _, _, g in flat]
    batches = make_batches(widths, batch_size, edge)
    codec = net.codec

    def finish(pend):
        idx, handle, lens = pend
        kind, h, e = handle
        hyps = h if kind == 'nbest' else None
        records = [hs[0][3] for hs in hyps] if hyps else e.collect(h) if kind == 'device' else h
        for n, (i, recs) in enumerate(zip(idx, records)):
            p, j, g = flat[i]
            chars = codec.decode(recs)
            W_in = int(lens[n])
            cuts = cut_quads(g, chars, W_in, int(lib.cocr_out_len(W_in, net.hparams_record.subsampling_factor)), pad)
            results[p][j] = {'id': g.id, 'text': ''.join(c[0] for c in chars), 'cuts': cuts}
            if hyps:
                results[p][j]['nbest'] = hyps[n]

    pending = None
    for width, idx in batches:
        strips, offs, hs, ws = eng.extract_lines(d_pages, [(flat[i][0], flat[i][2]) for i in idx], fill=fill)
        im, lens = eng.preprocess_device(strips, offs, hs, ws, height=height, pad=pad, width=width)
        if nbest > 0:
            handle = ('nbest', net.predict_nbest(im.unsqueeze(1), torch.from_numpy(lens), nbest), None)
        else:
            handle = net.predict_string_async(im.unsqueeze(1), torch.from_numpy(lens))
        if pending is not None:
            finish(pending)
        pending = (idx, handle, lens)
    finish(pending)
    return results
