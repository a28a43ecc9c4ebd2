"""numpy restatement of DESIGN.md section 7b (the augmentation's device half), written from that text alone: the parameter table and
control grid -> the augmented (N, H, W) uint8 batch.  Integer arithmetic only; the device must equal it bit for bit."""
import numpy as np

FIELDS = 16
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def _mix64(z):
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _hash(key, x):
    with np.errstate(over='ignore'):
        return _mix64(np.uint64(key) + (x.astype(np.uint64) + np.uint64(1)) * GOLDEN)


def _warp(src, sl, H, p, g):
    """Warped values of the line's [0, H) x [0, sl) region (zeros elsewhere are the caller's)."""
    r = np.arange(H, dtype=np.int64)[:, None]
    c = np.arange(sl, dtype=np.int64)[None, :]
    flags = int(p[1])
    if flags & 1:
        a0, a1, a2, a3, a4, a5 = (int(v) for v in p[2:8])
        X = a0 * c + a1 * r + a2
        Y = a3 * c + a4 * r + a5
    else:
        X = np.broadcast_to(c << 16, (H, sl)).copy()
        Y = np.broadcast_to(r << 16, (H, sl)).copy()
    if flags & 2:
        j, t = c >> 5, c & 31
        gg = g.astype(np.int64)
        dx = (gg[j, 0] * (32 - t) + gg[j + 1, 0] * t) >> 5
        dy = (gg[j, 1] * (32 - t) + gg[j + 1, 1] * t) >> 5
        sh = (gg[j, 2] * (32 - t) + gg[j + 1, 2] * t) >> 5
        X = X + dx + (sh * (2 * r - H + 1)) // H
        Y = Y + dy
    Xq, Yq = (X + 128) >> 8, (Y + 128) >> 8
    x0, y0 = Xq >> 8, Yq >> 8
    fx, fy = Xq & 255, Yq & 255
    pad = src[:, :sl].astype(np.int64)

    def px(x, y):
        ok = (x >= 0) & (x < sl) & (y >= 0) & (y < H)
        return np.where(ok, pad[np.clip(y, 0, H - 1), np.clip(x, 0, max(sl - 1, 0))], 0)
    v = ((256 - fx) * (256 - fy) * px(x0, y0) + fx * (256 - fy) * px(x0 + 1, y0) + (256 - fx) * fy * px(x0, y0 + 1)
         + fx * fy * px(x0 + 1, y0 + 1) + 32768) >> 16
    return v


def augment_line(src, sl, p, g):
    """One line: src (H, W) uint8, seq_len sl, table row p (16,) int64, grid g (G, 3) int32 -> (H, W) uint8."""
    H, W = src.shape
    out = src.copy()
    flags = int(p[1])
    if flags == 0 or sl == 0:
        return out
    v = _warp(src, sl, H, p, g) if flags & 3 else src[:, :sl].astype(np.int64)
    if flags & 4:
        kind = int(p[8])
        z = np.zeros((H + 6, sl + 6), dtype=np.int64)
        z[3:3 + H, 3:3 + sl] = v

        def nb(dy, dx):
            return z[3 + dy:3 + dy + H, 3 + dx:3 + dx + sl]
        if kind == 1:
            v = (sum(nb(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) + 4) // 9
        elif kind == 2:
            v = np.sort(np.stack([nb(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]), axis=0)[4]
        elif kind == 3:
            L, d = int(p[9]), int(p[10])
            ddx, ddy = {0: (1, 0), 1: (0, 1), 2: (1, 1), 3: (1, -1)}[d]
            h = L // 2
            v = (sum(nb(k * ddy, k * ddx) for k in range(-h, h + 1)) + h) // L
    if flags & 8:
        r = np.arange(H, dtype=np.int64)[:, None]
        c = np.arange(sl, dtype=np.int64)[None, :]
        u = (_hash(np.int64(p[12]).view(np.uint64), (r << 16) + c) >> np.uint64(48)).astype(np.int64)
        v = np.where(u < int(p[11]), 0, v)
    out[:, :sl] = v.astype(np.uint8)
    return out


def augment_batch(batch, seq_lens, params, grid):
    """batch (N, H, W) uint8 -> augmented copy."""
    batch = np.asarray(batch)
    return np.stack([augment_line(batch[i], int(seq_lens[i]), params[i], grid[i]) for i in range(batch.shape[0])])
