"""Character n-gram language model for the CTC beam search (shallow fusion) -- DESIGN.md section 7g.  The definition is this
build's own (kraken has no language model): UNPINNED.

    python -m conformer_ocr_amd.lm build -m MODEL -o lm.safetensors --order 5 [-f path|page|alto|xml|text] [-u NFD] FILES...
    python -m conformer_ocr_amd.lm tune -m MODEL --lm lm.safetensors -f xml [--alphas 0,0.25,..] [--betas ..] [--classes 8] EVAL...

`build` counts the n-grams of the transcriptions (ground truth through `dataset.read_ground_truth`, or plain UTF-8 text with
`-f text`, one line per line), encoded with the model's codec, and writes the back-off tables.  `tune` runs the forward once per
batch, keeps the logits on the device and decodes them for every (alpha, beta) of a grid; it prints the CER per cell and the best
cell.  The decoder's defaults (alpha 0.5, beta 0, 8 classes) are placeholders: no real material was at hand to tune them on.

The model is over codec labels 1..C-1 (blank 0 never occurs), order n in 1..8, interpolated Witten-Bell smoothing in float64,
stored in back-off form as float32 natural logs in two open-addressing hash tables that the host lookup below and the device
kernel (csrc/ctc_lm.hip.h) both read, byte for byte."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_ORDER = 8
HASH_SCHEME = 'fnv-chain/splitmix64-v1'
_M64 = (1 << 64) - 1
_FNV_OFFSET, _FNV_PRIME = 1469598103934665603, 1099511628211
_GOLD, _LEVEL = 0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93
_MIX1, _MIX2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


# ---------------------------------------------------------------------------------------------- keys
def _mix(h: int, c: int, k: int) -> int:
    """The key of (context hash h of length k, class c; c = 0: the context itself): splitmix64's finalizer, 0 -> 1 (0 = empty slot)."""
    z = (h ^ (c * _GOLD) ^ (k * _LEVEL)) & _M64
    z = ((z ^ (z >> 30)) * _MIX1) & _M64
    z = ((z ^ (z >> 27)) * _MIX2) & _M64
    z ^= z >> 31
    return z or 1


def _mix_np(h: np.ndarray, c, k: int) -> np.ndarray:
    """`_mix` on uint64 arrays (wrapping arithmetic)."""
    z = h ^ (np.asarray(c, dtype=np.uint64) * np.uint64(_GOLD)) ^ np.uint64((k * _LEVEL) & _M64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(_MIX1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(_MIX2)
    z = z ^ (z >> np.uint64(31))
    return np.where(z == 0, np.uint64(1), z)


def _chain_np(ctx_rows: np.ndarray) -> np.ndarray:
    """Context hashes of the rows of a (M, k) label array (oldest label first): the multiply-add chain runs from the NEWEST label
    backwards, so the hashes of the shorter contexts of one lookup are its running values."""
    h = np.full(ctx_rows.shape[0], _FNV_OFFSET, dtype=np.uint64)
    for j in range(ctx_rows.shape[1] - 1, -1, -1):
        h = h * np.uint64(_FNV_PRIME) + (ctx_rows[:, j].astype(np.uint64) + np.uint64(1))
    return h


def _fill_table(keys: np.ndarray, vals: np.ndarray, what: str) -> Tuple[np.ndarray, np.ndarray]:
    """Open addressing, linear probing, key 0 = empty, a power-of-two slot count >= 2 x entries.  Refuses two entries with one key."""
    keys = np.asarray(keys, dtype=np.uint64)
    n = keys.shape[0]
    if np.unique(keys).shape[0] != n:
        raise ValueError(f'{what}: two different entries share a 64-bit key (hash scheme {HASH_SCHEME}); not writing such a table')
    slots = 2
    while slots < 2 * n:
        slots *= 2
    mask = np.uint64(slots - 1)
    tk, tv = np.zeros(slots, dtype=np.uint64), np.zeros(slots, dtype=np.float32)
    pos = keys & mask
    pending = np.arange(n)
    while pending.size:                                   # per round the first entry that reaches an empty slot takes it, the others move on
        p = pos[pending]
        free = tk[p] == 0
        us, first = np.unique(p[free], return_index=True)
        win = pending[free][first]
        tk[us.astype(np.int64)] = keys[win]
        tv[us.astype(np.int64)] = vals[win]
        placed = np.zeros(n, dtype=bool)
        placed[win] = True
        pending = pending[~placed[pending]]
        pos[pending] = (pos[pending] + np.uint64(1)) & mask
    return tk.view(np.int64), tv


def _find(keys_u64: np.ndarray, vals: np.ndarray, key: int) -> Optional[np.float32]:
    """One probe sequence: stops at the key, at an empty slot, or after `slots` probes."""
    mask = keys_u64.shape[0] - 1
    slot = key & mask
    for _ in range(mask + 1):
        g = int(keys_u64[slot])
        if g == key:
            return vals[slot]
        if g == 0:
            return None
        slot = (slot + 1) & mask
    return None


# ---------------------------------------------------------------------------------------------- the model
class NGramLM:
    def __init__(self, order: int, num_classes: int, unigram, ngram_keys, ngram_logp, ctx_keys, ctx_bow, meta: Optional[Dict] = None):
        self.order, self.num_classes = int(order), int(num_classes)
        self.unigram = np.ascontiguousarray(unigram, dtype=np.float32)
        self.ngram_keys = np.ascontiguousarray(ngram_keys, dtype=np.int64)
        self.ngram_logp = np.ascontiguousarray(ngram_logp, dtype=np.float32)
        self.ctx_keys = np.ascontiguousarray(ctx_keys, dtype=np.int64)
        self.ctx_bow = np.ascontiguousarray(ctx_bow, dtype=np.float32)
        self.meta = dict(meta or {})
        if not 1 <= self.order <= MAX_ORDER:
            raise ValueError(f'order must be in 1..{MAX_ORDER}')
        if self.unigram.shape != (self.num_classes,):
            raise ValueError('unigram must hold one entry per class')
        for k, v in ((self.ngram_keys, self.ngram_logp), (self.ctx_keys, self.ctx_bow)):
            if k.shape != v.shape or k.ndim != 1 or k.shape[0] < 2 or k.shape[0] & (k.shape[0] - 1):
                raise ValueError('a table needs a power-of-two slot count and one value per key')
        self._memo: Dict = {}
        self._dev: Dict = {}

    # -- lookup (the device kernel reads the same bytes in the same order)
    def logp(self, ctx: Sequence[int], c: int) -> np.float32:
        """lm(ctx, c): natural log of P(c | the last min(order - 1, len(ctx)) labels of ctx); first hit wins, float32 sums."""
        ctx = tuple(int(x) for x in ctx[len(ctx) - min(self.order - 1, len(ctx)):]) if self.order > 1 else ()
        c = int(c)
        hit = self._memo.get((ctx, c))
        if hit is not None:
            return hit
        nk, ck = self.ngram_keys.view(np.uint64), self.ctx_keys.view(np.uint64)
        hashes, h = [], _FNV_OFFSET
        for lab in reversed(ctx):                          # newest label first
            h = (h * _FNV_PRIME + lab + 1) & _M64
            hashes.append(h)
        acc = np.float32(0.0)
        out = None
        for k in range(len(ctx), 0, -1):
            v = _find(nk, self.ngram_logp, _mix(hashes[k - 1], c, k))
            if v is not None:
                out = np.float32(acc + v)
                break
            b = _find(ck, self.ctx_bow, _mix(hashes[k - 1], 0, k))
            if b is not None:
                acc = np.float32(acc + b)
        if out is None:
            out = np.float32(acc + self.unigram[c])
        if len(self._memo) > (1 << 20):
            self._memo.clear()
        self._memo[(ctx, c)] = out
        return out

    # -- file
    def save(self, path: str) -> None:
        import safetensors.numpy
        meta = {'format': 'cocr-ngram-lm', 'order': str(self.order), 'num_classes': str(self.num_classes), 'hash_scheme': HASH_SCHEME}
        meta.update({k: v if isinstance(v, str) else json.dumps(v) for k, v in self.meta.items()})
        safetensors.numpy.save_file({'unigram': self.unigram, 'ngram_keys': self.ngram_keys, 'ngram_logp': self.ngram_logp,
                                     'ctx_keys': self.ctx_keys, 'ctx_bow': self.ctx_bow}, path, metadata=meta)

    @classmethod
    def load(cls, path: str) -> 'NGramLM':
        from safetensors import safe_open
        with safe_open(path, framework='np') as f:
            meta = dict(f.metadata() or {})
            t = {k: f.get_tensor(k) for k in ('unigram', 'ngram_keys', 'ngram_logp', 'ctx_keys', 'ctx_bow')}
        if meta.get('format') != 'cocr-ngram-lm':
            raise ValueError(f'{path}: not a language model file')
        if meta.get('hash_scheme') != HASH_SCHEME:
            raise ValueError(f'{path}: hash scheme {meta.get("hash_scheme")!r}, this build reads {HASH_SCHEME!r}')
        order, ncls = int(meta.pop('order')), int(meta.pop('num_classes'))
        for k in ('format', 'hash_scheme'):
            meta.pop(k)
        for k in ('codec', 'tokens', 'lines', 'skipped_lines'):
            if k in meta:
                meta[k] = json.loads(meta[k])
        return cls(order, ncls, t['unigram'], t['ngram_keys'], t['ngram_logp'], t['ctx_keys'], t['ctx_bow'], meta)

    def check_codec(self, codec, num_classes: int) -> None:
        """ValueError naming the first difference between the model's output layer / codec and what this file was built for."""
        if int(num_classes) != self.num_classes:
            raise ValueError(f'the language model was built for {self.num_classes} classes, the model has {int(num_classes)}')
        mine = self.meta.get('codec')
        if mine is None:
            return
        theirs = {k: [int(x) for x in v] for k, v in codec.c2l.items()}
        for g in sorted(set(mine) | set(theirs)):
            if mine.get(g) != theirs.get(g):
                raise ValueError(f'the language model\'s codec differs from the model\'s: grapheme {g!r} has labels {mine.get(g)} in the '
                                 f'language model and {theirs.get(g)} in the model')

    # -- device
    def to_device(self, engine) -> 'DeviceLM':
        """The tables on `engine`'s device (copied once per device; freed with this object)."""
        key = engine.dev_index
        if key not in self._dev:
            self._dev[key] = DeviceLM(self, engine)
        return self._dev[key]


class DeviceLM:
    def __init__(self, lm: NGramLM, engine):
        from . import _lib
        self.lib = engine.lib
        h = C.c_void_p()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(self.lib.cocr_lm_create(engine._h, lm.order, lm.num_classes, vp(lm.unigram), vp(lm.ngram_keys), vp(lm.ngram_logp),
                                           lm.ngram_keys.shape[0], vp(lm.ctx_keys), vp(lm.ctx_bow), lm.ctx_keys.shape[0], C.byref(h)))
        self.handle = h

    def __del__(self):
        h, self.handle = getattr(self, 'handle', None), None
        if h:
            try:
                self.lib.cocr_lm_destroy(h)
            except Exception:
                pass


# ---------------------------------------------------------------------------------------------- builder
def _windows(flat: np.ndarray, remaining: np.ndarray, k: int) -> np.ndarray:
    """Every (k + 1)-gram that lies inside one line: (M, k + 1) uint16."""
    if flat.shape[0] <= k:
        return np.zeros((0, k + 1), dtype=np.uint16)
    win = np.lib.stride_tricks.sliding_window_view(flat, k + 1)
    return np.ascontiguousarray(win[remaining[:win.shape[0]] > k])


def build_lm(label_sequences: Sequence[Sequence[int]], order: int, num_classes: int, meta: Optional[Dict] = None) -> NGramLM:
    """Interpolated Witten-Bell over the label sequences (one per line; no start / end symbols), float64, stored as float32 logs:
    level -1 is uniform 1/(C-1); P_k(c|h) = (count(h,c) + D(h) P_{k-1}(c|h')) / (N(h) + D(h)) for a seen context h of k labels
    (N(h) occurrences with a successor, D(h) distinct successors, h' = h without its oldest label), P_{k-1}(c|h') for an unseen one.
    Back-off form: logp(h,c) for every seen n-gram of order >= 2, bow(h) = log(D(h) / (N(h) + D(h))) for every seen context."""
    order, Cn = int(order), int(num_classes)
    if not 1 <= order <= MAX_ORDER:
        raise ValueError(f'order must be in 1..{MAX_ORDER}')
    if not 2 <= Cn <= 65535:
        raise ValueError('num_classes must be in 2..65535')
    seqs = [np.asarray(s, dtype=np.int64).reshape(-1) for s in label_sequences]
    seqs = [s for s in seqs if s.shape[0]]
    flat = np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.int64)
    if flat.shape[0] and (flat.min() < 1 or flat.max() >= Cn):
        raise ValueError(f'labels must lie in 1..{Cn - 1} (0 is the blank)')
    remaining = np.concatenate([np.arange(s.shape[0], 0, -1) for s in seqs]) if seqs else np.zeros(0, dtype=np.int64)
    flat16 = flat.astype(np.uint16)

    cnt0 = np.bincount(flat, minlength=Cn).astype(np.float64)
    n0, d0 = cnt0.sum(), float((cnt0 > 0).sum())
    p0 = np.full(Cn, 1.0 / (Cn - 1))
    if n0 > 0:
        p0 = (cnt0 + d0 * p0) / (n0 + d0)
    unigram = np.log(p0).astype(np.float32)
    unigram[0] = 0.0

    nk, nv, ck, cv = [], [], [], []
    prev_rows, prev_p = None, None                        # level k - 1: its sorted distinct n-grams and their probabilities
    for k in range(1, order):
        rows, cnt = np.unique(_windows(flat16, remaining, k), axis=0, return_counts=True)
        if rows.shape[0] == 0:
            break
        ctx = rows[:, :k]
        first = np.ones(rows.shape[0], dtype=bool)
        first[1:] = (ctx[1:] != ctx[:-1]).any(axis=1)     # rows are sorted: one context's n-grams are adjacent
        starts = np.nonzero(first)[0]
        group = np.cumsum(first) - 1
        n_h = np.add.reduceat(cnt.astype(np.float64), starts)
        d_h = np.diff(np.append(starts, rows.shape[0])).astype(np.float64)
        if k == 1:
            lower = p0[rows[:, 1].astype(np.int64)]
        else:                                             # the n-gram without its oldest label is a seen n-gram of the level below
            both = np.concatenate([prev_rows, rows[:, 1:]])
            uniq, inv = np.unique(both, axis=0, return_inverse=True)
            assert uniq.shape[0] == prev_rows.shape[0]
            lower = prev_p[inv.reshape(-1)[prev_rows.shape[0]:]]
        p = (cnt + d_h[group] * lower) / (n_h[group] + d_h[group])
        h_rows = _chain_np(ctx)
        nk.append(_mix_np(h_rows, rows[:, k], k))
        nv.append(np.log(p).astype(np.float32))
        ck.append(_mix_np(h_rows[starts], 0, k))
        cv.append(np.log(d_h / (n_h + d_h)).astype(np.float32))
        prev_rows, prev_p = rows, p
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dtype=dt)
    ngram_keys, ngram_logp = _fill_table(cat(nk, np.uint64), cat(nv, np.float32), 'n-gram table')
    ctx_keys, ctx_bow = _fill_table(cat(ck, np.uint64), cat(cv, np.float32), 'context table')
    info = {'tokens': int(flat.shape[0]), 'lines': len(seqs)}
    info.update(meta or {})
    return NGramLM(order, Cn, unigram, ngram_keys, ngram_logp, ctx_keys, ctx_bow, info)


# ---------------------------------------------------------------------------------------------- the decoder's definition
def _log_softmax(outputs: np.ndarray) -> np.ndarray:
    x = np.asarray(outputs, dtype=np.float32)
    m = x.max(axis=0, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(axis=0, keepdims=True, dtype=np.float32))


def _lse(a: np.float32, b: np.float32) -> np.float32:
    """logaddexp in float32 in the fixed form max + log1p(exp(-|a - b|))."""
    if a == -np.inf:
        return np.float32(b)
    if b == -np.inf:
        return np.float32(a)
    m = a if a > b else b
    d = np.float32(-abs(np.float32(a - b)))
    return np.float32(m + np.log1p(np.exp(d, dtype=np.float32), dtype=np.float32))


def records_host(lp: np.ndarray, labels: Sequence[int], starts: Sequence[int]) -> List[Tuple[int, int, int, float]]:
    """The post-pass of every beam decoder on (C, T) log-softmax scores: label k appended at frame starts[k] -> (label, start, end,
    conf); end = start extended while the next frame (before the next label's start, or the line's end) scores the label above
    blank; conf = max softmax(label) over [start, end]."""
    T = lp.shape[1]
    res = []
    for i, (c, s) in enumerate(zip(labels, starts)):
        limit = starts[i + 1] if i + 1 < len(starts) else T
        e = s
        while e + 1 < limit and lp[c, e + 1] > lp[0, e + 1]:
            e += 1
        res.append((int(c), int(s), int(e), float(np.exp(lp[c, s:e + 1].max()))))
    return res


def beam_decode_host(outputs: np.ndarray, lm: NGramLM, beam_size: int = 16, classes: int = 8, alpha: float = 0.5, beta: float = 0.0,
                     return_scores: bool = False, return_gap: bool = False):
    """THE DEFINITION of the LM beam search on one line's (C, T) logits: the CTC prefix beam search this build fixes
    (p_b / p_nb recurrences, folding, creation order, starts, ends, conf) with three changes: (1) a frame's candidate classes are
    blank + its K = min(classes, C - 1) non-blank classes of largest lp (ties: smaller class) -- a prefix is extended only by those,
    its stay term p_nb + lp[last] is unchanged; (2) a prefix first created as parent + (s,) carries
    lmv = f32(lmv(parent) + f32(f32(alpha lm(parent, s)) + beta)), the empty prefix 0; (3) candidates rank by
    f32(logaddexp(p_b, p_nb) + lmv), ties keep creation order.  Returns [(label, start, end, conf)] of the best prefix after the last
    frame; with return_scores also (its CTC log-probability logaddexp(p_b, p_nb), its lmv); with return_gap also the smallest
    decision gap met: the beam-th against the (beam+1)-th candidate of any frame, and the final top two."""
    lp = _log_softmax(outputs)
    Cn, T = lp.shape
    K = min(int(classes), Cn - 1)
    al, be = np.float32(alpha), np.float32(beta)
    NEG = np.float32(-np.inf)
    beam = [((), np.float32(0.0), NEG, (), np.float32(0.0))]          # (labels, p_b, p_nb, start frames, lmv)
    gap = np.inf
    final = [np.float32(0.0)]
    for t in range(T):
        col = lp[1:, t]
        top = sorted((np.argsort(-col, kind='stable')[:K] + 1).tolist())          # the K best non-blank classes, ascending
        cand = {}                                                      # insertion-ordered: creation order
        for key, p_b, p_nb, starts, lmv in beam:
            tot = _lse(p_b, p_nb)
            last = key[-1] if key else None
            c = cand.setdefault(key, [NEG, NEG, starts, lmv])
            c[0] = _lse(c[0], np.float32(tot + lp[0, t]))
            if last is not None:
                c[1] = _lse(c[1], np.float32(p_nb + lp[last, t]))
            for s in top:
                add = np.float32((p_b if s == last else tot) + lp[s, t])
                if add == NEG:
                    continue
                q = key + (s,)
                c = cand.get(q)
                if c is None:
                    c = cand[q] = [NEG, NEG, starts + (t,), np.float32(lmv + np.float32(np.float32(al * lm.logp(key, s)) + be))]
                c[1] = _lse(c[1], add)
        scored = [(np.float32(_lse(v[0], v[1]) + v[3]), i, k, v) for i, (k, v) in enumerate(cand.items())]
        scored.sort(key=lambda x: (-float(x[0]), x[1]))
        if len(scored) > beam_size:
            gap = min(gap, float(scored[beam_size - 1][0]) - float(scored[beam_size][0]))
        beam = [(k, v[0], v[1], v[2], v[3]) for _, _, k, v in scored[:beam_size]]
        final = [s for s, _, _, _ in scored[:2]]
    if len(final) > 1:
        gap = min(gap, float(final[0]) - float(final[1]))
    labels, p_b, p_nb, starts, lmv = beam[0]
    out = (records_host(lp, labels, starts),)
    if return_scores:
        out += ((float(_lse(p_b, p_nb)), float(lmv)),)
    if return_gap:
        out += (gap,)
    return out[0] if len(out) == 1 else out


# ---------------------------------------------------------------------------------------------- commands
def _floats(s: str) -> List[float]:
    return [float(x) for x in s.split(',') if x.strip()]


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog='python -m conformer_ocr_amd.lm', description='Character n-gram language models for the beam search.')
    sub = ap.add_subparsers(dest='command', required=True)
    b = sub.add_parser('build', help='count n-grams of transcriptions and write the tables')
    b.add_argument('files', nargs='+', help='ground-truth files, or plain text files with -f text (globs allowed)')
    b.add_argument('-m', '--model', required=True, help='the model whose codec encodes the text: safetensors archive or checkpoint')
    b.add_argument('-o', '--output', required=True, help='the language model file to write')
    b.add_argument('--order', type=int, default=5, help=f'n-gram order, 1..{MAX_ORDER}')
    b.add_argument('-f', '--format-type', choices=('path', 'page', 'alto', 'xml', 'text'), default='path')
    b.add_argument('-u', '--normalization', choices=('NFD', 'NFKD', 'NFC', 'NFKC'), default=None)
    b.add_argument('--no-normalize-whitespace', dest='normalize_whitespace', action='store_false', default=True)
    t = sub.add_parser('tune', help='CER over a grid of (alpha, beta): one forward per batch, the logits stay on the device',
                       epilog='The decoder\'s defaults (0.5 / 0 / 8) are placeholders; this command finds the values for your material.')
    t.add_argument('files', nargs='+', help='evaluation ground truth (globs allowed)')
    t.add_argument('-m', '--model', required=True)
    t.add_argument('--lm', required=True, help='language model file written by `build`')
    t.add_argument('-f', '--format-type', choices=('path', 'page', 'alto', 'xml'), default='path')
    t.add_argument('-u', '--normalization', choices=('NFD', 'NFKD', 'NFC', 'NFKC'), default=None)
    t.add_argument('--no-normalize-whitespace', dest='normalize_whitespace', action='store_false', default=True)
    t.add_argument('--alphas', type=_floats, default=[0.0, 0.25, 0.5, 0.75, 1.0], help='comma-separated LM weights')
    t.add_argument('--betas', type=_floats, default=[0.0, 0.5, 1.0, 1.5, 2.0], help='comma-separated per-label bonuses')
    t.add_argument('--classes', type=int, default=8, help='candidate classes per frame, 1..64')
    t.add_argument('--beam', type=int, default=16)
    t.add_argument('-B', '--batch-size', type=int, default=32)
    t.add_argument('--pad', type=int, default=16)
    t.add_argument('--edge', type=int, default=200)
    t.add_argument('-d', '--device', default='cuda:0')
    return ap


def read_lines(files: Sequence[str], format_type: str, normalization: Optional[str], normalize_whitespace: bool) -> List[Tuple[str, str]]:
    """(file, text) per line of the inputs, normalized like ground truth."""
    from .dataset import normalize_text, read_ground_truth
    if format_type != 'text':
        return [(ln.image, ln.text) for ln in read_ground_truth(files, format_type, normalization, normalize_whitespace)]
    out = []
    for f in files:
        with open(f, encoding='utf-8') as fp:
            for raw in fp:
                text = normalize_text(raw.rstrip('\n'), normalization, normalize_whitespace)
                if text:
                    out.append((f, text))
    return out


def encode_lines(codec, lines: Sequence[Tuple[str, str]]) -> Tuple[List[List[int]], Dict[str, int]]:
    """Label sequences of the lines the codec encodes completely; the others are skipped and counted per file."""
    from .align import encode_text
    seqs, skipped = [], {}
    for f, text in lines:
        labels, missing = encode_text(codec, text)
        if missing or not labels:
            skipped[f] = skipped.get(f, 0) + 1
            continue
        seqs.append(labels)
    return seqs, skipped


def _load_host(path):
    """The model on the host: its codec and class count are all `build` needs."""
    import tarfile
    from .pred import PytorchRecognitionModel
    return PytorchRecognitionModel.load_safetensors(path) if tarfile.is_tarfile(path) else PytorchRecognitionModel.load_checkpoint(path)


def build_main(args) -> int:
    from .test import expand_globs
    if not 1 <= args.order <= MAX_ORDER:
        print(f'error: --order must be in 1..{MAX_ORDER}', file=sys.stderr)
        return 1
    net = _load_host(args.model)
    lines = read_lines(expand_globs(args.files), args.format_type, args.normalization, args.normalize_whitespace)
    seqs, skipped = encode_lines(net.codec, lines)
    for f, n in skipped.items():
        print(f'warning: {f}: {n} line(s) skipped: the model\'s codec cannot encode them', file=sys.stderr)
    t0 = time.time()
    lm = build_lm(seqs, args.order, net.hparams_record.num_classes,
                  {'codec': {k: list(v) for k, v in net.codec.c2l.items()}, 'normalization': args.normalization or '',
                   'skipped_lines': int(sum(skipped.values()))})
    lm.save(args.output)
    used = int((lm.ngram_keys != 0).sum())
    print(f'{args.output}: order {lm.order}, {lm.num_classes} classes, {lm.meta["lines"]} lines, {lm.meta["tokens"]} labels, {used} n-grams of '
          f'order >= 2 in {lm.ngram_keys.shape[0]} slots, {int((lm.ctx_keys != 0).sum())} contexts in {lm.ctx_keys.shape[0]} slots, '
          f'built in {time.time() - t0:.1f} s')
    return 0


def tune_grid(eng, lm: NGramLM, batches, truths: Sequence[str], to_text, alphas, betas, classes: int = 8, beam: int = 16):
    """CER per (alpha, beta) over `batches` = [(logits (N,T,C) on `eng`'s device, out_lens)] (the forward ran once), line order =
    `truths`; `to_text` turns one line's label records into its string.  Returns (cer[len(alphas)][len(betas)], (best alpha, best beta))."""
    from .score import align_pairs, pack
    ta, ta_offs = pack(truths)
    total = max(1, int(ta_offs[-1]))
    cer = np.zeros((len(alphas), len(betas)))
    for ia, a in enumerate(alphas):
        for ib, b in enumerate(betas):
            preds, inflight = [], []
            for logits, olens in batches:                             # a few decodes enqueued ahead of the one being read
                inflight.append(eng.ctc_beam_lm_async(logits, olens, lm, beam, classes, a, b))
                if len(inflight) > 4:
                    preds.extend(to_text(rec) for rec in eng.collect(inflight.pop(0)))
            for h in inflight:
                preds.extend(to_text(rec) for rec in eng.collect(h))
            pb, pb_offs = pack(preds)
            counts, _, _ = align_pairs(eng, ta, ta_offs, pb, pb_offs)          # the cell's edit distances in one call (section 7c)
            cer[ia, ib] = int(counts[:, 0].sum()) / total
    ia, ib = np.unravel_index(int(np.argmin(cer)), cer.shape)
    return cer, (alphas[ia], betas[ib])


def line_logits(net, gt: Sequence, batch_size: int = 32, edge: int = 200, pad: int = 16, device: str = 'cuda:0'):
    """The forward of every `dataset.GTLine`, once: ([(logits (N,T,C) on the device, out_lens)], the gt index of every line in batch
    order).  Page lines are cut and scaled like `page.recognize_pages` does, line images like `evaluate.recognize_crops`."""
    import torch
    from . import _lib
    from .evaluate import make_batches
    from .ocr import load_image
    from .page import _check_image
    from .test import PAGE_GROUP
    lib = _lib.load()
    dev = torch.device(device)
    eng = net.engine(dev)
    height = int(net.height)
    batches, order = [], []
    by_page: Dict[str, List[int]] = {}
    crops: List[int] = []
    for i, ln in enumerate(gt):
        if ln.geom is None:
            crops.append(i)
        else:
            by_page.setdefault(ln.image, []).append(i)
    images = list(by_page)
    for k in range(0, len(images), PAGE_GROUP):
        group = images[k:k + PAGE_GROUP]
        d_pages = [torch.from_numpy(_check_image(load_image(image))).to(dev) for image in group]
        flat = [(p, gt[i].geom, i) for p, image in enumerate(group) for i in by_page[image]]
        widths = [int(lib.cocr_preproc_width(g.H_s, g.W_s, height, int(pad))) for _, g, _ in flat]
        for width, idx in make_batches(widths, batch_size, edge):
            strips, offs, hs, ws = eng.extract_lines(d_pages, [(flat[j][0], flat[j][1]) for j in idx])
            im, lens = eng.preprocess_device(strips, offs, hs, ws, height=height, pad=pad, width=width)
            o, olens = net.forward(im.unsqueeze(1), torch.from_numpy(lens))
            batches.append((o, olens.numpy()))
            order.extend(flat[j][2] for j in idx)
    if crops:
        imgs = [load_image(gt[i].image) for i in crops]
        widths = [int(lib.cocr_preproc_width(int(c.shape[0]), int(c.shape[1]), height, int(pad))) for c in imgs]
        for width, idx in make_batches(widths, batch_size, edge):
            im, lens = net.transform_lines([imgs[j] for j in idx], pad=pad, bucket_edge=edge, device=device)
            o, olens = net.forward(im, lens)
            batches.append((o, olens.numpy()))
            order.extend(crops[j] for j in idx)
    return batches, order


def tune_main(args) -> int:
    import torch
    from .dataset import read_ground_truth
    from .ocr import load_model
    from .test import expand_globs
    lm = NGramLM.load(args.lm)
    net = load_model(args.model, device=args.device)
    lm.check_codec(net.codec, net.hparams_record.num_classes)
    gt = read_ground_truth(expand_globs(args.files), args.format_type, args.normalization, args.normalize_whitespace)
    if not gt:
        print('error: no usable line in the evaluation data', file=sys.stderr)
        return 1
    t0 = time.time()
    batches, order = line_logits(net, gt, args.batch_size, args.edge, args.pad, args.device)
    truths = [gt[i].text for i in order]
    codec = net.codec
    cer, best = tune_grid(net._engine, lm, batches, truths, lambda rec: ''.join(x[0] for x in codec.decode(rec)), args.alphas, args.betas,
                          args.classes, args.beam)
    torch.cuda.synchronize()
    dt = time.time() - t0
    print('CER (%) by alpha (rows) and beta (columns)')
    print('alpha\\beta ' + ' '.join(f'{b:7.2f}' for b in args.betas))
    for a, row in zip(args.alphas, cer):
        print(f'{a:10.2f} ' + ' '.join(f'{100 * v:7.2f}' for v in row))
    print(f'best: alpha {best[0]:g}, beta {best[1]:g}, CER {100 * cer.min():.2f}% ({len(truths)} lines, {cer.size} cells, '
          f'{len(truths) * cer.size / dt:.0f} line decodes/s)')
    return 0


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    return build_main(args) if args.command == 'build' else tune_main(args)


if __name__ == '__main__':
    sys.exit(main())
