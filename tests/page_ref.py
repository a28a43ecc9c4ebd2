"""CPU restatement of the line extraction's semantics, written from the definition alone: the checker of
conformer_ocr_amd.page (geometry tables) and of the device kernels (strips).  It does not import conformer_ocr_amd.page.

Geometry is scalar float64 Python, one operation at a time as the definition states it; the mask and the sampler are exact integer
numpy."""
import math

import numpy as np


def geometry(baseline, boundary):
    """dict with the deduplicated points, T, Bt, H_s, W_s, S, the integer boundary and the column table (W_s, 4) int64."""
    pts = [(float(x), float(y)) for x, y in np.asarray(baseline, dtype=np.float64).reshape(-1, 2)]
    P = []
    for p in pts:
        if not P or p != P[-1]:
            P.append(p)
    if len(P) < 2:
        raise ValueError('fewer than 2 distinct baseline points')
    Q = [(float(np.rint(x)), float(np.rint(y))) for x, y in np.asarray(boundary, dtype=np.float64).reshape(-1, 2)]
    if not 3 <= len(Q) <= 4096:
        raise ValueError('boundary vertex count')
    m = len(P) - 1
    seg, A, d, n = [], [0.0], [], []
    for k in range(m):
        dx, dy = P[k + 1][0] - P[k][0], P[k + 1][1] - P[k][1]
        l = math.sqrt(dx * dx + dy * dy)
        seg.append(l)
        A.append(A[-1] + l)
        d.append((dx / l, dy / l))
        n.append((-(dy / l), dx / l))
    nu = [n[0]] + [None] * (m - 1) + [n[m - 1]]
    for k in range(1, m):
        sx, sy = n[k - 1][0] + n[k][0], n[k - 1][1] + n[k][1]
        s = math.sqrt(sx * sx + sy * sy)
        nu[k] = n[k] if s == 0.0 else (sx / s, sy / s)
    top = bottom = 0.0
    for qx, qy in Q:
        best, bk = None, 0
        for k in range(m):
            px, py = P[k]
            dx, dy = P[k + 1][0] - px, P[k + 1][1] - py
            u = ((qx - px) * dx + (qy - py) * dy) / (dx * dx + dy * dy)
            u = min(max(u, 0.0), 1.0)
            cx, cy = px + u * dx, py + u * dy
            dd = (qx - cx) * (qx - cx) + (qy - cy) * (qy - cy)
            if best is None or dd < best:
                best, bk = dd, k
        delta = (qx - P[bk][0]) * n[bk][0] + (qy - P[bk][1]) * n[bk][1]
        top, bottom = max(top, -delta), max(bottom, delta)
    T, Bt = int(math.ceil(top)), int(math.ceil(bottom))
    S = A[m]
    W_s = int(math.floor(S)) + 1
    H_s = T + Bt + 1
    if H_s > 4096 or W_s > 65535:
        raise ValueError('strip too large')
    cols = np.zeros((W_s, 4), dtype=np.int64)
    for c in range(W_s):
        (bx, by), (nx, ny) = frame(P, seg, A, nu, n, float(c))
        cols[c] = [int(np.rint(v * 65536.0)) for v in (bx, by, nx, ny)]
    return dict(points=np.array(P), T=T, Bt=Bt, H_s=H_s, W_s=W_s, S=S, top=top, bottom=bottom,
                verts=np.array(Q, dtype=np.int64), cols=cols, seg=seg, A=A, nu=nu, n=n)


def frame(P, seg, A, nu, n, s):
    m = len(seg)
    k = 0
    for j in range(m):
        if A[j] <= s:
            k = j
    t = (s - A[k]) / seg[k]
    bx = P[k][0] + t * (P[k + 1][0] - P[k][0])
    by = P[k][1] + t * (P[k + 1][1] - P[k][1])
    vx = (1.0 - t) * nu[k][0] + t * nu[k + 1][0]
    vy = (1.0 - t) * nu[k][1] + t * nu[k + 1][1]
    l = math.sqrt(vx * vx + vy * vy)
    if l == 0.0:
        return (bx, by), n[k]
    return (bx, by), (vx / l, vy / l)


def frame_of(g, s):
    return frame([tuple(p) for p in g['points']], g['seg'], g['A'], g['nu'], g['n'], float(s))


def mask(verts, xs, ys):
    """Even-odd inside test of integer pixels (xs, ys) (same-shape int arrays) against the integer polygon `verts`."""
    xs, ys = np.asarray(xs, dtype=np.int64), np.asarray(ys, dtype=np.int64)
    odd = np.zeros(xs.shape, dtype=bool)
    V = len(verts)
    for e in range(V):
        ax, ay = int(verts[e][0]), int(verts[e][1])
        bx, by = int(verts[(e + 1) % V][0]), int(verts[(e + 1) % V][1])
        cross = (ay > ys) != (by > ys)
        if not cross.any() or ay == by:
            continue
        num = (ys - ay) * (bx - ax)
        den = by - ay
        if den < 0:
            num, den = -num, -den
        t = ax + (-((-num) // den))                # ceil(num / den), exact
        odd ^= cross & (t > xs)
    return odd


def gray(page):
    page = np.asarray(page)
    if page.ndim == 2:
        return page.astype(np.int64)
    p = page.astype(np.int64)
    return (p[..., 0] * 19595 + p[..., 1] * 38470 + p[..., 2] * 7471 + 0x8000) >> 16


def strip(page, g, fill=0):
    """The (H_s, W_s) uint8 strip of geometry `g` (from `geometry`) cut out of `page`."""
    G = gray(page)
    H, W = G.shape
    cols = g['cols']
    r = np.arange(g['H_s'], dtype=np.int64)[:, None] - g['T']
    X = cols[None, :, 0] + r * cols[None, :, 2]
    Y = cols[None, :, 1] + r * cols[None, :, 3]
    Xq, Yq = (X + 128) // 256, (Y + 128) // 256
    x0, y0 = Xq // 256, Yq // 256
    fx, fy = Xq - 256 * x0, Yq - 256 * y0

    def px(x, y):
        ok = (x >= 0) & (y >= 0) & (x < W) & (y < H)
        ok &= mask(g['verts'], x, y)
        v = np.full(x.shape, int(fill), dtype=np.int64)
        v[ok] = G[y[ok], x[ok]]
        return v
    v = ((256 - fx) * (256 - fy) * px(x0, y0) + fx * (256 - fy) * px(x0 + 1, y0) + (256 - fx) * fy * px(x0, y0 + 1)
         + fx * fy * px(x0 + 1, y0 + 1) + 32768) >> 16
    return v.astype(np.uint8)
