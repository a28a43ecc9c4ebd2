"""CER / WER scoring and the confusion tallies of the report on the GPU.

`evaluate.edit_distance`, `ErrorRate`, `global_align` and `compute_confusions` are the definition; this module computes the same
integers in bulk: the strings are packed into code points (or word ids) with one encode, `HipRecognizer.edit_align` aligns every
(ground truth, prediction) pair in one call, and the tallies are built from the alignment ops with numpy.  A pair with a sequence
over the kernel's limit is aligned by `global_align` and merged in, so no caller sees the limit."""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_LEN = 4096                      # symbols per sequence the kernel takes (include/cocr.h: cocr_edit_align)
EQUAL, SUB, DEL, INS = 0, 1, 2, 3   # alignment ops, one byte per column


def use_device(scorer: Optional[str], engine) -> bool:
    """Which scorer a caller's `scorer` argument means: 'host' (or COCR_HOST_SCORE=1) the Python functions, 'device' the GPU kernel
    (an engine is required), None the kernel whenever the model has an engine."""
    if scorer not in (None, 'device', 'host'):
        raise ValueError("scorer must be 'device' or 'host'")
    if scorer == 'host' or (scorer is None and os.environ.get('COCR_HOST_SCORE') == '1'):
        return False
    if engine is None:
        if scorer == 'device':
            raise RuntimeError('the device scorer needs the model\'s engine on a GPU')
        return False
    return True


def pack(strings: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """(code points int32, offsets int64 (len + 1)) of `strings`: one UTF-32 encode of the joined text."""
    offs = np.zeros(len(strings) + 1, dtype=np.int64)
    if len(strings):
        np.cumsum(np.fromiter(map(len, strings), dtype=np.int64, count=len(strings)), out=offs[1:])
    cps = np.frombuffer(''.join(strings).encode('utf-32-le', 'surrogatepass'), dtype='<u4').astype(np.int32)
    assert cps.shape[0] == offs[-1]
    return cps, offs


def unpack(cps: np.ndarray, offs: np.ndarray) -> List[str]:
    """Inverse of `pack`."""
    text = np.asarray(cps, dtype='<u4').tobytes().decode('utf-32-le', 'surrogatepass')
    return [text[int(s):int(e)] for s, e in zip(offs[:-1], offs[1:])]


def pack_words(preds: Sequence[str], truths: Sequence[str]) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, List[str]]:
    """`str.split()` of every string (what `ErrorRate(words=True)` compares), words as ids of one shared table: (truth ids, truth
    offsets, prediction ids, prediction offsets, the table)."""
    table: Dict[str, int] = {}
    intern = table.setdefault

    def ids(strings):
        offs = np.zeros(len(strings) + 1, dtype=np.int64)
        out: List[int] = []
        for k, s in enumerate(strings):
            out.extend([intern(w, len(table)) for w in s.split()])
            offs[k + 1] = len(out)
        return np.asarray(out, dtype=np.int32), offs
    a, a_offs = ids(truths)
    b, b_offs = ids(preds)
    return a, a_offs, b, b_offs, list(table)


def ops_from_alignment(al1: Sequence, al2: Sequence) -> np.ndarray:
    """The op bytes of one `evaluate.global_align` result ('' marks a gap)."""
    return np.fromiter((DEL if p == '' else INS if g == '' else int(g != p) for g, p in zip(al1, al2)), dtype=np.uint8, count=len(al1))


def _host_pair(sa: np.ndarray, sb: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    from .evaluate import global_align
    cost, al1, al2 = global_align(sa.tolist(), sb.tolist())
    ops = ops_from_alignment(al1, al2)
    c = np.array([cost, int((ops == INS).sum()), int((ops == DEL).sum()), int((ops == SUB).sum())], dtype=np.int32)
    return c, ops


def align_pairs(engine, a: np.ndarray, a_offs: np.ndarray, b: np.ndarray, b_offs: np.ndarray, want_ops: bool = False
                ) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:
    """Alignment of P packed pairs: counts (P, 4) int32 = (distance, insertions, deletions, substitutions) and, with `want_ops`, the ops
    of all pairs one after the other (forward order) with their offsets (P + 1).  `engine`: a `HipRecognizer`, or None for the host
    functions alone."""
    a_offs, b_offs = np.asarray(a_offs, dtype=np.int64), np.asarray(b_offs, dtype=np.int64)
    a, b = np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.int32)
    P = a_offs.shape[0] - 1
    la, lb = np.diff(a_offs), np.diff(b_offs)
    host = (la > MAX_LEN) | (lb > MAX_LEN) if engine is not None else np.ones(P, dtype=bool)
    counts = np.zeros((P, 4), dtype=np.int32)
    lens = np.zeros(P, dtype=np.int64)
    dev_ops = dev_start = None
    dev = np.flatnonzero(~host)
    if dev.size:
        if dev.size == P:
            da, dao, db, dbo = a, a_offs, b, b_offs
        else:                                       # the pairs the kernel takes, packed again
            dao, dbo = np.concatenate([[0], np.cumsum(la[dev])]), np.concatenate([[0], np.cumsum(lb[dev])])
            da = np.concatenate([a[a_offs[p]:a_offs[p + 1]] for p in dev]) if dao[-1] else a[:0]
            db = np.concatenate([b[b_offs[p]:b_offs[p + 1]] for p in dev]) if dbo[-1] else b[:0]
        c, raw, used = engine.edit_align(da, dao, db, dbo, want_ops)
        counts[dev] = c
        if want_ops:
            lens[dev] = used
            dev_ops, dev_start = raw, (dao + dbo)[1:] - used          # a pair's ops are the last `used` bytes of its slot
    host_ops: Dict[int, np.ndarray] = {}
    for p in np.flatnonzero(host):
        counts[p], ops = _host_pair(a[a_offs[p]:a_offs[p + 1]], b[b_offs[p]:b_offs[p + 1]])
        if want_ops:
            host_ops[int(p)] = ops
            lens[p] = ops.shape[0]
    if not want_ops:
        return counts, None, None
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out = np.empty(int(offs[-1]), dtype=np.uint8)
    if dev.size:
        # gather: output byte t of device pair k comes from raw[dev_start[k] + t]
        dl = lens[dev]
        src = np.repeat(dev_start - (np.cumsum(dl) - dl), dl) + np.arange(int(dl.sum()), dtype=np.int64)
        if dev.size == P:
            out[:] = dev_ops[src]
        else:
            dst = np.repeat(offs[dev] - (np.cumsum(dl) - dl), dl) + np.arange(int(dl.sum()), dtype=np.int64)
            out[dst] = dev_ops[src]
    for p, ops in host_ops.items():
        out[offs[p]:offs[p + 1]] = ops
    return counts, out, offs


def _by_script(chars: np.ndarray) -> Dict[str, int]:
    """{script: count} of the code points `chars`, scripts in order of first occurrence; `_script` once per distinct character."""
    from .evaluate import _script
    if chars.size == 0:
        return {}
    uniq, first, cnt = np.unique(chars, return_index=True, return_counts=True)
    agg: Dict[str, List[int]] = {}
    for u, f, c in zip(uniq.tolist(), first.tolist(), cnt.tolist()):
        e = agg.setdefault(_script(chr(u)), [0, f])
        e[0] += c
        e[1] = min(e[1], f)
    return {s: e[0] for s, e in sorted(agg.items(), key=lambda kv: kv[1][1])}


def tally(a: np.ndarray, b: np.ndarray, ops: np.ndarray):
    """`evaluate.compute_confusions` of the concatenated alignments, from their ops: `a` / `b` the packed code points of all ground
    truths / predictions, `ops` the alignments of all pairs in order.  An op consumes a symbol of `a` unless it is an insertion and
    one of `b` unless it is a deletion, so cumulative sums of the op kinds index both.  Returns (confusions, scripts, ins, dels, subs)
    with the host's ordering: confusions by falling count, ties by first occurrence; the script tables by first occurrence."""
    a, b, ops = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(ops)
    diff = np.flatnonzero(ops != EQUAL)
    kinds = ops[diff]
    ia = np.cumsum(ops != INS)[diff] - 1                       # index into a of the symbol a non-insertion consumes
    ib = np.cumsum(ops != DEL)[diff] - 1
    g = np.where(kinds != INS, a[np.maximum(ia, 0)] if a.size else 0, -1)
    p = np.where(kinds != DEL, b[np.maximum(ib, 0)] if b.size else 0, -1)
    confusions = {}
    if diff.size:
        keys = ((g + 1) << 22) | (p + 1)                       # code points need 21 bits; 0 is the gap
        uniq, first, cnt = np.unique(keys, return_index=True, return_counts=True)
        for k in np.lexsort((first, -cnt)):
            ug, up = int(uniq[k] >> 22) - 1, int(uniq[k] & ((1 << 22) - 1)) - 1
            confusions[('' if ug < 0 else chr(ug), '' if up < 0 else chr(up))] = int(cnt[k])
    scripts = _by_script(a)
    ins = _by_script(p[kinds == INS])
    subs = _by_script(g[kinds == SUB])
    return confusions, scripts, ins, int((kinds == DEL).sum()), subs


def score(engine, preds: Sequence[str], truths: Sequence[str], report: bool = False) -> Dict:
    """What `evaluate.evaluate` needs of (predictions, ground truths): `char_errors`, `chars`, `word_errors`, `words`, and with
    `report` the `tallies` = the five values of `compute_confusions` over the lines in order."""
    if len(preds) != len(truths):
        raise ValueError('one prediction per ground truth')
    a, a_offs = pack(truths)
    b, b_offs = pack(preds)
    counts, ops, _ = align_pairs(engine, a, a_offs, b, b_offs, want_ops=report)
    wa, wa_offs, wb, wb_offs, _ = pack_words(preds, truths)
    wcounts, _, _ = align_pairs(engine, wa, wa_offs, wb, wb_offs)
    out = {'char_errors': int(counts[:, 0].sum()), 'chars': int(a_offs[-1]), 'word_errors': int(wcounts[:, 0].sum()),
           'words': int(wa_offs[-1])}
    if report:
        out['tallies'] = tally(a, b, ops)
    return out
