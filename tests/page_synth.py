"""Synthetic pages for the page-recognition tests and tools/page_rate.py: known text lines pasted into a page along straight, rotated
and circular-arc baselines.  Rendering is an analytic inverse map (page pixel -> line coordinates, bilinear in the line image), not
the code under test.  Every line gets its baseline on its last row and a boundary polygon of integer vertices chosen so that the
strip holds all of its rows at the line's own height (T = 95 on a 96-row line, Bt = 0: H_s = 96, no rescaling by the pre-processing).
Lines are offset by half a row (not by a fraction of a column): the metric's fixture model, fitted on its own 32 lines, misreads some
of them after a 97 -> 96 row rescale or a horizontal half-pixel blur (checked against the CPU oracle), which says nothing about the
extraction."""
import math

import numpy as np


class Placement:
    """Line coordinates (u along the line, v down its rows; v = h - 1 on the baseline) <-> page coordinates.
    kind 'line': origin `o` = page position of (0, h - 1), angle `deg` (clockwise on screen, y down).
    kind 'arc': circle centre `c`, radius `R` of the baseline, start angle `phi0`; sigma = +1 bends the line's ends down (centre below),
    -1 bends them up (centre above)."""

    def __init__(self, kind, h, w, o=None, deg=0.0, c=None, R=None, phi0=0.0, sigma=1):
        self.kind, self.h, self.w = kind, h, w
        self.o, self.deg, self.c, self.R, self.phi0, self.sigma = o, deg, c, R, phi0, sigma

    def _dn(self, u):
        if self.kind == 'line':
            a = math.radians(self.deg)
            d = np.array([math.cos(a), math.sin(a)])
            return np.broadcast_to(d, np.shape(u) + (2,)), np.broadcast_to(np.array([-d[1], d[0]]), np.shape(u) + (2,))
        phi = self.phi0 + np.asarray(u, dtype=np.float64) / self.R
        d = np.stack([np.cos(phi), self.sigma * np.sin(phi)], -1)
        return d, np.stack([-d[..., 1], d[..., 0]], -1)

    def base(self, u):
        """Baseline point at line column u."""
        u = np.asarray(u, dtype=np.float64)
        if self.kind == 'line':
            d, _ = self._dn(u)
            return np.asarray(self.o, dtype=np.float64) + u[..., None] * d
        phi = self.phi0 + u / self.R
        return np.asarray(self.c, dtype=np.float64) + self.R * np.stack([np.sin(phi), -self.sigma * np.cos(phi)], -1)

    def forward(self, u, v):
        """Page position of line point (u, v)."""
        _, n = self._dn(u)
        return self.base(u) + (np.asarray(v, dtype=np.float64) - (self.h - 1))[..., None] * n

    def inverse(self, x, y):
        """(u, v) of page points."""
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        if self.kind == 'line':
            a = math.radians(self.deg)
            dx, dy = x - self.o[0], y - self.o[1]
            u = dx * math.cos(a) + dy * math.sin(a)
            off = -dx * math.sin(a) + dy * math.cos(a)
            return u, off + (self.h - 1)
        dx, dy = x - self.c[0], y - self.c[1]
        r = np.sqrt(dx * dx + dy * dy)
        phi = np.arctan2(dx, -self.sigma * dy)
        off = self.sigma * (self.R - r)
        return (phi - self.phi0) * self.R, off + (self.h - 1)

    def baseline(self, npts=None):
        if self.kind == 'line':
            return self.base(np.array([0.0, self.w - 1.0]))
        return self.base(np.linspace(0.0, self.w - 1.0, npts or 24))


def _delta(P, q):
    """Signed distance of q from the polyline P along the normal of its nearest segment."""
    best, out = None, 0.0
    for k in range(len(P) - 1):
        px, py = P[k]
        dx, dy = P[k + 1][0] - px, P[k + 1][1] - py
        u = min(max(((q[0] - px) * dx + (q[1] - py) * dy) / (dx * dx + dy * dy), 0.0), 1.0)
        dd = (q[0] - px - u * dx) ** 2 + (q[1] - py - u * dy) ** 2
        if best is None or dd < best:
            l = math.sqrt(dx * dx + dy * dy)
            best, out = dd, (q[0] - px) * (-dy / l) + (q[1] - py) * (dx / l)
    return out


def boundary(pl: Placement, P, nside=None):
    """Integer polygon around the line: top vertices with -delta in (h - 2, h - 1] (as close to h - 1 as the grid allows), bottom
    vertices with delta in (-1, 0]: T = h - 1, Bt = 0, H_s = h; ends one column beyond the line."""
    h = pl.h
    us = np.array([-1.0, pl.w]) if pl.kind == 'line' else np.linspace(-1.0, pl.w, nside or 30)
    top, bot = [], []
    for u in us:
        for want, lo, hi, out in ((-(h - 1), h - 2, h - 1, top), (-0.5, -1.0, 0.0, bot)):
            cx, cy = pl.forward(u, (h - 1) + want)
            best = None
            for ix in range(int(math.floor(cx)) - 1, int(math.floor(cx)) + 3):
                for iy in range(int(math.floor(cy)) - 1, int(math.floor(cy)) + 3):
                    d = _delta(P, (float(ix), float(iy)))
                    val = -d if out is top else d
                    if lo < val <= hi and (best is None or val > best[0]):
                        best = (val, ix, iy)
            assert best is not None
            out.append((best[1], best[2]))
    return np.array(top + bot[::-1], dtype=np.float64)


def render(page, line_u8, pl: Placement):
    """Pastes `line_u8` (h, w) into `page` (2-D uint8, in place) along `pl`: every page pixel whose inverse image lies within the line
    takes the bilinear sample of the zero-bordered line there."""
    h, w = line_u8.shape
    pad = np.zeros((h + 2, w + 2), dtype=np.float64)
    pad[1:-1, 1:-1] = line_u8
    corners = pl.forward(np.array([0, w - 1, 0, w - 1] + list(np.linspace(0, w - 1, 16))), np.array([0, 0, h - 1, h - 1] + [0] * 8 + [h - 1] * 8))
    x0, y0 = np.floor(corners.min(0)).astype(int) - 2
    x1, y1 = np.ceil(corners.max(0)).astype(int) + 3
    x0, y0 = max(x0, 0), max(y0, 0)
    x1, y1 = min(x1, page.shape[1]), min(y1, page.shape[0])
    ys, xs = np.mgrid[y0:y1, x0:x1]
    u, v = pl.inverse(xs, ys)
    ok = (u > -1) & (u < w) & (v > -1) & (v < h)
    uu, vv = u[ok] + 1, v[ok] + 1
    iu, iv = np.floor(uu).astype(int), np.floor(vv).astype(int)
    fu, fv = uu - iu, vv - iv
    val = ((1 - fu) * (1 - fv) * pad[iv, iu] + fu * (1 - fv) * pad[iv, iu + 1] + (1 - fu) * fv * pad[iv + 1, iu]
           + fu * fv * pad[iv + 1, iu + 1])
    sub = page[y0:y1, x0:x1]
    sub[ok] = np.maximum(sub[ok], np.clip(np.rint(val), 0, 255).astype(np.uint8))


def text_page(lines_u8, kinds, margin=40, gap=30):
    """A page holding `lines_u8` ((h, w) uint8 each), one per row band, placed by `kinds` entries: ('line', deg) or ('arc', R, sigma).
    Returns (page (H, W) uint8, [(Placement, baseline (n, 2), boundary (V, 2))])."""
    out, y = [], margin
    pls = []
    for img, kind in zip(lines_u8, kinds):
        h, w = img.shape
        if kind[0] == 'line':
            pl = Placement('line', h, w, o=(0.0, 0.0), deg=kind[1])
        else:
            R, sigma = kind[1], kind[2]
            half = (w - 1) / 2.0 / R
            pl = Placement('arc', h, w, c=(0.0, 0.0), R=R, phi0=-half, sigma=sigma)
        # shift to the band: bounding box of the line (+ 3 px) starts at (margin, y)
        pts = pl.forward(np.concatenate([np.linspace(-2, w + 1, 64)] * 2), np.concatenate([np.full(64, -2.0), np.full(64, h + 1.0)]))
        lo, hi = pts.min(0), pts.max(0)
        shift = np.array([margin - lo[0], y - lo[1]]) + np.array([0.0, 0.5])          # rows between page rows
        if pl.kind == 'line':
            pl.o = tuple(np.asarray(pl.o) + shift)
        else:
            pl.c = tuple(np.asarray(pl.c) + shift)
        pls.append(pl)
        y = int(math.ceil(y + hi[1] - lo[1])) + gap
    width = int(max(max(p.forward(np.array([p.w + 2.0]), np.array([0.0]))[0, 0] for p in pls),
                    max(p.forward(np.array([p.w + 2.0]), np.array([p.h * 1.0]))[0, 0] for p in pls))) + margin
    width = max(width, max(img.shape[1] for img in lines_u8) + 2 * margin)
    page = np.zeros((y + margin, width), dtype=np.uint8)
    for img, pl in zip(lines_u8, pls):
        render(page, img, pl)
        P = pl.baseline()
        out.append((pl, P, boundary(pl, P)))
    return page, out
