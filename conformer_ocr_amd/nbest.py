"""N-best decoding: the top hypotheses of the beam with exact CTC scores, and what is built on them --
rescoring without a new search, the oracle error rate of a beam, a sequence posterior per line.

`nbest_host` is THE DEFINITION of `cocr_ctc_beam_nbest` (include/cocr.h; kernel: csrc/ctc_nbest.hip.h).  A hypothesis holds at most
255 labels with a score (COCR_LATTICE_MAX_LABELS, the criterion's limit): a longer one keeps its records and has logp = NaN."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .lm import _log_softmax, _lse, records_host

MAX_LABELS = 255                    # csrc/ctc_lattice.hip.h COCR_LATTICE_MAX_LABELS

Records = List[Tuple[int, int, int, float]]


def ctc_logp(outputs: np.ndarray, labels: Sequence[int]) -> float:
    """log P(labels | outputs) over ALL alignments: the CTC forward recursion on the blank-extended sequence over log_softmax(outputs),
    (C, T) logits, float64 throughout.  T = 0: 0 for the empty sequence, -inf otherwise."""
    x = np.asarray(outputs, dtype=np.float64)
    T = x.shape[1]
    L = len(labels)
    if T == 0:
        return 0.0 if L == 0 else -math.inf
    m = x.max(axis=0, keepdims=True)
    lp = x - m - np.log(np.exp(x - m).sum(axis=0, keepdims=True))
    ext = np.zeros(2 * L + 1, dtype=np.int64)
    ext[1::2] = np.asarray(labels, dtype=np.int64)
    S = ext.shape[0]
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != 0) & (ext[2:] != ext[:-2])
    alpha = np.full(S, -np.inf)
    alpha[0] = lp[0, 0]
    if S > 1:
        alpha[1] = lp[ext[1], 0]
    ninf = np.full(2, -np.inf)
    with np.errstate(invalid='ignore'):
        for t in range(1, T):
            p = np.concatenate([ninf, alpha])
            acc = np.logaddexp(p[2:], p[1:-1])
            acc = np.where(skip, np.logaddexp(acc, p[:-2]), acc)
            alpha = acc + lp[ext, t]
        return float(np.logaddexp(alpha[S - 1], alpha[S - 2] if S > 1 else -np.inf))


def lm_sum(lm, labels: Sequence[int]) -> float:
    """The float32 sum, in label order, of lm.logp(labels before k, label k): raw, without alpha or beta."""
    acc = np.float32(0.0)
    labels = tuple(int(c) for c in labels)
    for k, c in enumerate(labels):
        acc = np.float32(acc + lm.logp(labels[:k], c))
    return float(acc)


def nbest_host(outputs: np.ndarray, beam_size: int, nbest: int, lm=None, classes: int = 8, alpha: float = 0.5, beta: float = 0.0,
               return_gap: bool = False):
    """One line's (C, T) logits -> the first min(nbest, live) prefixes of the final beam, in beam order, live = the prefixes alive after
    the last frame; each as (records, logp, lm_logp).  The search is exactly `oracle.ctc_ref.beam_decoder`'s (restated here: the product
    path does not import the oracle) or, with `lm`, exactly `lm.beam_decode_host`'s, which differs in three points: a frame's candidate
    classes are its min(classes, C - 1) best non-blank ones, a prefix carries lmv, and candidates rank by f32(logaddexp(p_b, p_nb) +
    lmv) (lmv = 0 without lm: the same number).
      records   [(label, start, end, conf)] by the post-pass of the 1-best decoders;
      logp      `ctc_logp`: the exact CTC log-probability of the label sequence -- not the beam's pruned logaddexp(p_b, p_nb); NaN for
                more than 255 labels (MAX_LABELS: the kernel's limit, kept here so that both sides say the same);
      lm_logp   `lm_sum`; 0.0 without lm.
    T = 0: exactly one hypothesis, the empty one, with logp 0.  return_gap: also (the smallest frame decision gap as
    `lm.beam_decode_host` defines it -- the beam-th against the (beam+1)-th candidate of any frame --, the smallest gap between adjacent
    final scores among the first min(nbest, live) + 1 candidates of the last frame); inf where there is no such pair."""
    lp = _log_softmax(outputs)
    Cn, T = lp.shape
    beam_size, nbest = int(beam_size), int(nbest)
    if not 1 <= nbest <= beam_size:
        raise ValueError('nbest must be in 1..beam_size')
    K = min(int(classes), Cn - 1) if lm is not None else Cn - 1
    al, be = np.float32(alpha), np.float32(beta)
    NEG = np.float32(-np.inf)
    ZERO = np.float32(0.0)
    beam = [((), ZERO, NEG, (), ZERO)]                                # (labels, p_b, p_nb, start frames, lmv)
    frame_gap = math.inf
    final: List[np.float32] = []
    for t in range(T):
        if lm is not None:
            top = sorted((np.argsort(-lp[1:, t], kind='stable')[:K] + 1).tolist())
        else:
            top = range(1, Cn)
        cand: Dict = {}                                                # insertion-ordered: creation order
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
                    nlmv = ZERO if lm is None else np.float32(lmv + np.float32(np.float32(al * lm.logp(key, s)) + be))
                    c = cand[q] = [NEG, NEG, starts + (t,), nlmv]
                c[1] = _lse(c[1], add)
        scored = [(np.float32(_lse(v[0], v[1]) + v[3]), i, k, v) for i, (k, v) in enumerate(cand.items())]
        scored.sort(key=lambda x: (-float(x[0]), x[1]))
        if len(scored) > beam_size:
            frame_gap = min(frame_gap, float(scored[beam_size - 1][0]) - float(scored[beam_size][0]))
        beam = [(k, v[0], v[1], v[2], v[3]) for _, _, k, v in scored[:beam_size]]
        final = [s for s, _, _, _ in scored]
    take = min(nbest, len(beam))
    hyps = []
    for labels, _, _, starts, _ in beam[:take]:
        res: Records = records_host(lp, labels, starts)
        logp = ctc_logp(outputs, labels) if len(labels) <= MAX_LABELS else math.nan
        hyps.append((res, logp, lm_sum(lm, labels) if lm is not None else 0.0))
    if not return_gap:
        return hyps
    head = [float(s) for s in final[:take + 1]]
    final_gap = min((a - b for a, b in zip(head[:-1], head[1:])), default=math.inf)
    return hyps, (frame_gap, final_gap)


# ---------------------------------------------------------------------------------------------- on the hypotheses
def rescore(hyps: Sequence, alpha: float, beta: float) -> List:
    """One line's hypotheses reordered by logp + alpha * lm_logp + beta * len, largest first; ties keep beam order; a NaN logp sorts
    last (those keep beam order among themselves).  A hypothesis is (records, logp, lm_logp) or (text, logp, lm_logp, records): the
    length is that of its records."""
    def key(item):
        i, h = item
        recs = h[0] if len(h) == 3 else h[3]
        logp, lmv = float(h[1]), float(h[2])
        if math.isnan(logp):
            return (1, 0.0, i)
        return (0, -(logp + alpha * lmv + beta * len(recs)), i)
    return [h for _, h in sorted(enumerate(hyps), key=key)]


def oracle_errors(hyps: Sequence[Sequence[str]], truths: Sequence[str], engine=None, scorer: Optional[str] = None) -> List[int]:
    """Per line the smallest edit distance between its truth and any of its hypothesis strings (a line without hypotheses: the length
    of its truth).  All K pairs of every line go through `cocr_edit_align` in one call on `engine` (a `HipRecognizer`); scorer 'host'
    (or no engine): the Python functions, same integers."""
    from . import score as _score
    if len(hyps) != len(truths):
        raise ValueError('one list of hypotheses per truth')
    owner = [n for n, hs in enumerate(hyps) for _ in hs]
    a, a_offs = _score.pack([truths[n] for n in owner])
    b, b_offs = _score.pack([h for hs in hyps for h in hs])
    counts, _, _ = _score.align_pairs(engine if _score.use_device(scorer, engine) else None, a, a_offs, b, b_offs)
    best = [len(t) for t in truths]
    seen = [False] * len(truths)
    for n, d in zip(owner, counts[:, 0].tolist()):
        best[n] = d if not seen[n] else min(best[n], d)
        seen[n] = True
    return best


def recognize_nbest(net, lines: Sequence[np.ndarray], nbest: int, batch_size: int = 32, edge: int = 200, device: str = 'cuda:0') -> Dict[int, List]:
    """`evaluate.recognize` returning, per line index, `predict_nbest`'s [(text, logp, lm_logp, records)] (H x w float arrays in [0, 1],
    the same width buckets, so entry 0's text is `recognize`'s string)."""
    import torch
    from .evaluate import collate, make_batches
    out: Dict[int, List] = {}
    dev = torch.device(device)
    for width, idx in make_batches([l.shape[1] for l in lines], batch_size, edge):
        im, lens = collate(lines, idx, width)
        for i, h in zip(idx, net.predict_nbest(im.to(dev), lens, nbest)):
            out[i] = h
    return out
