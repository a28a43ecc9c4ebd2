"""Training-time augmentation: the host half.  Every random number is drawn here, per line, from a counter-based
hash of the line's 64-bit key, vectorised in numpy over a batch; the device (`cocr_augment_lines`, csrc/augment.hip.h) only applies the
resulting integer tables to the pre-processed u8 batch.

    keys = line_keys(seed, epoch, uids)                              # splitmix64 chain of (seed, epoch, line uid)
    params, grid = draw(keys, seq_lens, H, W, AugmentConfig())       # int64 (N, 16), int32 (N, G, 3)
    out = engine.augment(batch, seq_lens, params, grid)

A line's augmentation depends only on its key: not on its batch, its position in it or the batch width.  The model is kraken's default
augmenter (albumentations: pixel dropout, one of three blurs, shift / scale / rotate, an elastic distortion, all behind a p = 0.5 gate);
neither package is installed, so the definition is this project's own and unpinned."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import numpy as np

FIELDS = 16
F_SEQ, F_FLAGS, F_A, F_BLUR, F_MLEN, F_MDIR, F_DROP, F_KEY = 0, 1, 2, 8, 9, 10, 11, 12
GEOM, ELASTIC, BLUR, DROPOUT = 1, 2, 4, 8
GRID_STEP = 32
FIX = 65536
MAX_H, MAX_W = 4096, 65535
BOX, MEDIAN, MOTION = 1, 2, 3

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)

# hash fields of a line's parameters
H_GATE, H_GEOM, H_ELASTIC, H_BLUR, H_DROP = 0, 1, 2, 3, 4
H_ANGLE, H_SCALE, H_TX, H_TY = 5, 6, 7, 8
H_KIND, H_MLEN, H_MDIR, H_DKEY = 9, 10, 11, 12
H_GRID = 1024                       # control column j, component k: field 1024 + 3 j + k


def mix64(z):
    """splitmix64's output function on uint64 arrays (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
    return z ^ (z >> np.uint64(31))


def hash64(key, x):
    """mix64(key + (x + 1) * golden): element-wise, broadcasting, uint64."""
    key = np.asarray(key, dtype=np.uint64)
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        return mix64(key + (x + np.uint64(1)) * GOLDEN)


def line_keys(seed: int, epoch: int, uids) -> np.ndarray:
    """The 64-bit key of each line: hash64(hash64(hash64(0, seed), epoch), uid)."""
    k = hash64(hash64(np.uint64(0), np.uint64(int(seed) & (2 ** 64 - 1))), np.uint64(int(epoch) & (2 ** 64 - 1)))
    return hash64(k, np.asarray(uids, dtype=np.int64).astype(np.uint64))


def _u16(h):
    """Top 16 bits: a uniform integer in [0, 65536)."""
    return (h >> np.uint64(48)).astype(np.int64)


def _unit(h):
    """Top 53 bits as a float64 in [0, 1)."""
    return (h >> np.uint64(11)).astype(np.float64) * (2.0 ** -53)


def _below(h, n: int):
    """Bits 32..63 reduced mod n: a (near-)uniform integer in [0, n)."""
    return ((h >> np.uint64(32)) % np.uint64(n)).astype(np.int64)


def _threshold(p: float) -> int:
    return int(round(float(p) * 65536))


@dataclass
class AugmentConfig:
    """All probabilities and ranges of the augmentation in one place.  Probabilities are applied as 16-bit
    thresholds round(p * 65536)."""
    p: float = 0.5                  # a line is augmented at all with this probability (kraken's Compose(..., p=0.5))
    p_geometry: float = 0.2
    max_rotation_deg: float = 3.0
    min_scale: float = 0.8
    max_scale: float = 1.2
    max_shift: float = 1.0 / 16     # of the line height (vertical) and of seq_len (horizontal)
    p_elastic: float = 0.2
    max_displacement: int = 2 * FIX  # |dx|, |dy|, |shear| of a control column, 1/65536 px
    p_blur: float = 0.2
    p_dropout: float = 0.2
    dropout_pixel: int = 655          # per-pixel probability, of 65536

    def __post_init__(self):
        for name in ('p', 'p_geometry', 'p_elastic', 'p_blur', 'p_dropout'):
            if not 0.0 <= getattr(self, name) <= 1.0:
                raise ValueError(f'{name} must be a probability')
        if not 0 < self.min_scale <= self.max_scale or not 0 <= self.max_rotation_deg <= 45 or not 0 <= self.max_shift <= 1:
            raise ValueError('scale, rotation or shift range out of bounds')
        if not 0 <= self.max_displacement <= 64 * FIX or not 0 <= self.dropout_pixel <= 65536:
            raise ValueError('displacement or dropout range out of bounds')


def grid_cols(width: int) -> int:
    """Control columns a batch `width` px wide needs: 0, 32, ... up to one beyond the last column."""
    return (int(width) - 1) // GRID_STEP + 2


def draw(keys, seq_lens, height: int, width: int, cfg: AugmentConfig = None) -> Tuple[np.ndarray, np.ndarray]:
    """Per-line parameter table (N, 16) int64 and control grid (N, grid_cols(width), 3) int32 for lines of `seq_lens` in an
    (N, height, width) batch.  Pure function of (key, seq_len, height, cfg): the grid's column j does not depend on the width."""
    cfg = cfg or AugmentConfig()
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    sl = np.asarray(seq_lens, dtype=np.int64).reshape(-1)
    n, H, G = keys.shape[0], int(height), grid_cols(width)
    if sl.shape[0] != n:
        raise ValueError('one seq_len per key')

    def h(field):
        return hash64(keys, np.uint64(field))
    on = _u16(h(H_GATE)) < _threshold(cfg.p)
    flags = np.zeros(n, dtype=np.int64)
    for bit, field, p in ((GEOM, H_GEOM, cfg.p_geometry), (ELASTIC, H_ELASTIC, cfg.p_elastic), (BLUR, H_BLUR, cfg.p_blur),
                          (DROPOUT, H_DROP, cfg.p_dropout)):
        flags |= np.where(on & (_u16(h(field)) < _threshold(p)), bit, 0)
    t = np.zeros((n, FIELDS), dtype=np.int64)
    t[:, F_SEQ] = sl
    t[:, F_FLAGS] = flags
    # inverse of p' = C + s R(theta) (p - C) + shift, about the line centre C = ((seq_len - 1) / 2, (H - 1) / 2)
    theta = np.radians((2.0 * _unit(h(H_ANGLE)) - 1.0) * cfg.max_rotation_deg)
    s = cfg.min_scale + (cfg.max_scale - cfg.min_scale) * _unit(h(H_SCALE))
    tx = (2.0 * _unit(h(H_TX)) - 1.0) * cfg.max_shift * sl
    ty = (2.0 * _unit(h(H_TY)) - 1.0) * cfg.max_shift * H
    cx, cy = (sl - 1) / 2.0, (H - 1) / 2.0
    a0, a1 = np.cos(theta) / s, np.sin(theta) / s
    a3, a4 = -a1, a0
    ox, oy = cx + tx, cy + ty
    a2 = cx - a0 * ox - a1 * oy
    a5 = cy - a3 * ox - a4 * oy
    geo = (flags & GEOM) != 0
    ident = np.array([FIX, 0, 0, 0, FIX, 0], dtype=np.int64)
    A = np.rint(np.stack([a0, a1, a2, a3, a4, a5], -1) * FIX).astype(np.int64)
    t[:, F_A:F_A + 6] = np.where(geo[:, None], A, ident[None, :])
    blur = (flags & BLUR) != 0
    t[:, F_BLUR] = np.where(blur, 1 + _below(h(H_KIND), 3), 0)
    t[:, F_MLEN] = np.where(blur, 3 + 2 * _below(h(H_MLEN), 3), 0)
    t[:, F_MDIR] = np.where(blur, _below(h(H_MDIR), 4), 0)
    t[:, F_DROP] = np.where((flags & DROPOUT) != 0, int(cfg.dropout_pixel), 0)
    t[:, F_KEY] = h(H_DKEY).view(np.int64)
    grid = np.zeros((n, G, 3), dtype=np.int32)
    el = (flags & ELASTIC) != 0
    if el.any():
        f = H_GRID + 3 * np.arange(G, dtype=np.uint64)[:, None] + np.arange(3, dtype=np.uint64)[None, :]
        hh = hash64(keys[el][:, None, None], f[None])
        span = 2 * int(cfg.max_displacement) + 1
        grid[el] = (_below(hh, span) - int(cfg.max_displacement)).astype(np.int32)
    return t, grid


def check_tables(params: np.ndarray, grid: np.ndarray, seq_lens, height: int, width: int) -> None:
    """ValueError for a table the device would not apply as DESIGN.md section 7b defines it (called before anything is launched)."""
    n = np.asarray(seq_lens).reshape(-1).shape[0]
    if params.dtype != np.int64 or params.shape != (n, FIELDS):
        raise ValueError(f'params must be int64 ({n}, {FIELDS}), got {params.dtype} {params.shape}')
    if grid.dtype != np.int32 or grid.ndim != 3 or grid.shape[0] != n or grid.shape[2] != 3 or grid.shape[1] < grid_cols(width):
        raise ValueError(f'grid must be int32 ({n}, >= {grid_cols(width)}, 3), got {grid.dtype} {grid.shape}')
    sl = np.asarray(seq_lens, dtype=np.int64).reshape(-1)
    if (params[:, F_SEQ] != sl).any():
        raise ValueError('the table\'s seq_len column differs from seq_lens')
    fl = params[:, F_FLAGS]
    if ((fl < 0) | (fl > 15)).any():
        raise ValueError('stage flags outside 0..15')
    blur = (fl & BLUR) != 0
    kind = params[:, F_BLUR]
    if (blur & ((kind < BOX) | (kind > MOTION))).any():
        raise ValueError('blur kind outside 1..3')
    mot = blur & (kind == MOTION)
    if (mot & ~np.isin(params[:, F_MLEN], (3, 5, 7))).any() or (mot & ((params[:, F_MDIR] < 0) | (params[:, F_MDIR] > 3))).any():
        raise ValueError('motion blur length must be 3, 5 or 7 and its direction 0..3')
    if ((params[:, F_DROP] < 0) | (params[:, F_DROP] > 65536)).any():
        raise ValueError('dropout threshold outside 0..65536')
    lim = np.array([4, 4, 1 << 24, 4, 4, 1 << 24], dtype=np.int64) * FIX
    if (np.abs(params[:, F_A:F_A + 6]) > lim).any():
        raise ValueError('affine map out of range (|a0|, |a1|, |a3|, |a4| <= 4, offsets <= 2^24 px)')
    if (np.abs(grid.astype(np.int64)) > 64 * FIX).any():
        raise ValueError('control-grid displacement beyond 64 px')
