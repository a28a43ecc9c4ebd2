"""Regular-expression patterns on the CTC lattice: a pattern is compiled to a graph of label states and spotted
in a line's frame posteriors like a query string (`search.spot_host`, section 7i), the recursion walking the graph instead of a chain.

Syntax (`compile_pattern`): literals (`\\` escapes), groups `( )`, alternation `|`, quantifiers `?` `*` `+` `{m}` `{m,n}` `{m,}`
(bounded repeats are expanded), sets `[abc]` `[a-z]` `[^...]` (a range is code-point order restricted to the codec's single-label
characters; a negated set is the codec's single-label characters minus the set), `.` (every single-label character of the codec),
`\\d` `\\w` `\\s` (the codec's single-label characters for which str.isdigit / str.isalnum or '_' / str.isspace hold).

Not built: anchors (`^`, `$`), `\\b`, back-references, look-around, non-greedy quantifiers (they change nothing for a search), named
groups.  They raise ValueError.

`spot_pattern_host` is the definition (host); the device form is `cocr_ctc_spot_pattern` (csrc/ctc_spot_graph.hip.h)."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

MAX_STATES = 256          # label states of one pattern (the kernel: 4 registers of a wave)
MAX_EDGES = 4096          # predecessor-list entries of one pattern


class PatternGraph:
    """Glushkov's position automaton of a pattern over labels: label state p in [0, P) has class `cls[p]` in [1, C), flags `first[p]`
    (a match may begin in it) and `last[p]` (a match may end in it) and the strictly ascending predecessor list `preds[p]` (a state
    may precede itself).  States are numbered in order of occurrence in the pattern text.  `skipped`: the characters the codec could
    not encode ('' for a usable graph; a graph with skipped characters has no states and is not searched)."""

    def __init__(self, text: str, cls, first, last, preds, skipped: str = '', ignore_case: bool = False):
        self.text = text
        self.cls = np.asarray(cls, dtype=np.int32).reshape(-1)
        self.first = np.asarray(first, dtype=bool).reshape(-1)
        self.last = np.asarray(last, dtype=bool).reshape(-1)
        self.preds = [[int(p) for p in ps] for ps in preds]
        self.skipped = skipped
        self.ignore_case = bool(ignore_case)

    @property
    def P(self) -> int:
        return int(self.cls.shape[0])

    @property
    def edges(self) -> int:
        return sum(len(ps) for ps in self.preds)

    @property
    def is_chain(self) -> bool:
        """A plain label string: state p follows state p - 1 and nothing else, one beginning, one end."""
        P = self.P
        return (P >= 1 and all(self.preds[p] == ([p - 1] if p else []) for p in range(P))
                and self.first.tolist() == [p == 0 for p in range(P)] and self.last.tolist() == [p == P - 1 for p in range(P)])

    @property
    def labels(self) -> List[int]:
        """The label string of a chain."""
        if not self.is_chain:
            raise ValueError('not a chain')
        return self.cls.tolist()

    def accepts(self, labels: Sequence[int]) -> bool:
        """Whether the label sequence is in the pattern's language."""
        labels = [int(l) for l in labels]
        if not labels or not self.P:
            return False
        cur = self.first & (self.cls == labels[0])
        for l in labels[1:]:
            nxt = np.zeros(self.P, dtype=bool)
            for q in np.nonzero(self.cls == l)[0]:
                nxt[q] = any(cur[p] for p in self.preds[q])
            cur = nxt
        return bool((cur & self.last).any())

    def tables(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """What `cocr_ctc_spot_pattern` takes: (classes (P), flags (P): 1 = first, 2 = last, pred_off (P + 1), preds (edges)), int32."""
        off = np.zeros(self.P + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(ps) for ps in self.preds])
        flat = np.asarray([p for ps in self.preds for p in ps], dtype=np.int32)
        return self.cls.copy(), (self.first.astype(np.int32) | (self.last.astype(np.int32) << 1)), off, flat


def chain_graph(labels: Sequence[int], text: str = '') -> PatternGraph:
    """The graph of a plain label string."""
    L = len(labels)
    return PatternGraph(text, labels, [p == 0 for p in range(L)], [p == L - 1 for p in range(L)], [[p - 1] if p else [] for p in range(L)])


# ---- the compiler -------------------------------------------------------------------------------------------------------------------
# AST: ('run', str) literal characters | ('set', [char]) | ('cat', [node]) | ('alt', [node]) | ('rep', node, lo, hi or None)
class _Parser:
    def __init__(self, text: str, singles: List[str]):
        self.s, self.i, self.singles = text, 0, singles

    def fail(self, msg: str):
        raise ValueError(f'pattern {self.s!r}: {msg} (at {self.i})')

    def peek(self) -> str:
        return self.s[self.i] if self.i < len(self.s) else ''

    def parse(self):
        node = self.alt()
        if self.i < len(self.s):
            self.fail('unbalanced )')
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == '|':
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ('alt', branches)

    def cat(self):
        items = []
        while self.peek() not in ('', '|', ')'):
            atom = self.atom()
            rep = self.quantifier()
            if rep is not None:
                atom = ('rep', atom, rep[0], rep[1])
            if atom[0] == 'run' and items and items[-1][0] == 'run':
                items[-1] = ('run', items[-1][1] + atom[1])       # adjacent literals: one run, encoded together
            else:
                items.append(atom)
        return ('cat', items)

    def quantifier(self):
        c = self.peek()
        rep = None
        if c == '?':
            rep = (0, 1)
        elif c == '*':
            rep = (0, None)
        elif c == '+':
            rep = (1, None)
        elif c == '{':
            j = self.s.find('}', self.i)
            body = self.s[self.i + 1:j] if j > 0 else ''
            parts = body.split(',')
            if j < 0 or len(parts) > 2 or not parts[0].isdigit() or (len(parts) == 2 and parts[1] and not parts[1].isdigit()):
                self.fail('malformed {m,n}')
            lo = int(parts[0])
            hi = lo if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
            if hi is not None and hi < lo:
                self.fail('{m,n} with n < m')
            if max(lo, hi or 0) > MAX_STATES:
                raise ValueError(f'pattern {self.s!r}: more than {MAX_STATES} label states')
            self.i = j
            rep = (lo, hi)
        if rep is None:
            return None
        self.i += 1
        if self.peek() in ('?', '+', '*', '{'):
            self.fail('a quantifier on a quantifier (non-greedy and possessive forms are not built)')
        return rep

    def shorthand(self, c: str):
        test = {'d': str.isdigit, 'w': lambda ch: ch.isalnum() or ch == '_', 's': str.isspace}.get(c)
        return None if test is None else [ch for ch in self.singles if test(ch)]

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == '(':
            if self.peek() == '?':
                self.fail('(?...) groups and look-around are not built')
            node = self.alt()
            if self.peek() != ')':
                self.fail('missing )')
            self.i += 1
            return ('cat', [node])
        if c == '[':
            return self.char_set()
        if c == '.':
            return ('set', list(self.singles), True)
        if c in ('^', '$'):
            self.fail('anchors are not built')
        if c in ('?', '*', '+', '{'):
            self.fail('nothing to repeat')
        if c == '\\':
            e = self.peek()
            if e == '':
                self.fail('a trailing backslash')
            self.i += 1
            sh = self.shorthand(e)
            if sh is not None:
                return ('set', sh, True)
            if e.isalnum():
                self.fail(f'\\{e} is not built')
            return ('run', e)
        return ('run', c)

    def char_set(self):
        negate = self.peek() == '^'
        if negate:
            self.i += 1
        members: List[str] = []            # explicit members, in order
        ranged: List[str] = []             # members that came from a range or a shorthand: the codec's own characters
        start = self.i
        while True:
            c = self.peek()
            if c == '':
                self.fail('missing ]')
            if c == ']' and self.i > start:
                self.i += 1
                break
            self.i += 1
            if c == '\\':
                e = self.peek()
                if e == '':
                    self.fail('a trailing backslash')
                self.i += 1
                sh = self.shorthand(e)
                if sh is not None:
                    ranged.extend(sh)
                    continue
                if e.isalnum():
                    self.fail(f'\\{e} is not built')
                c = e
            if self.peek() == '-' and self.i + 1 < len(self.s) and self.s[self.i + 1] != ']':
                hi = self.s[self.i + 1]
                self.i += 2
                if hi == '\\':
                    hi = self.peek()
                    self.i += 1
                if not hi or ord(hi) < ord(c):
                    self.fail('a range that runs backwards')
                ranged.extend(ch for ch in self.singles if ord(c) <= ord(ch) <= ord(hi))
            else:
                members.append(c)
        if negate:
            out = set(members) | set(ranged)
            return ('set', [ch for ch in self.singles if ch not in out], True)
        return ('set', members + ranged, False)


class _Builder:
    """Glushkov's construction; positions are allocated in the order the pattern text is walked."""

    def __init__(self, text: str, codec, ignore_case: bool):
        self.text, self.codec, self.ignore_case = text, codec, ignore_case
        self.cls: List[int] = []
        self.follow: List[set] = []
        self.skipped: List[str] = []

    def position(self, label: int) -> int:
        if len(self.cls) >= MAX_STATES:
            raise ValueError(f'pattern {self.text!r}: more than {MAX_STATES} label states')
        self.cls.append(int(label))
        self.follow.append(set())
        return len(self.cls) - 1

    def link(self, last, first):
        for p in last:
            self.follow[p].update(first)

    # every build returns (nullable, first positions, last positions)
    def labels(self, labels):
        prev, first = None, None
        for l in labels:
            p = self.position(l)
            if prev is None:
                first = p
            else:
                self.follow[prev].add(p)
            prev = p
        return (True, [], []) if prev is None else (False, [first], [prev])

    def encode(self, s: str):
        from .align import encode_text
        labels, skipped = encode_text(self.codec, s)
        self.skipped.extend(skipped)
        return labels

    def cat(self, parts):
        nullable, first, last = True, [], []
        for n2, f2, l2 in parts:
            self.link(last, f2)
            first = first + f2 if nullable else first
            last = last + l2 if n2 else l2
            nullable = nullable and n2
        return nullable, first, last

    def alt(self, parts):
        return any(p[0] for p in parts), [x for p in parts for x in p[1]], [x for p in parts for x in p[2]]

    def build(self, node):
        kind = node[0]
        if kind == 'run':
            if not self.ignore_case:
                return self.labels(self.encode(node[1]))
            parts = []
            for c in node[1]:
                variants = [v for v in dict.fromkeys((c, c.lower(), c.upper())) if v in self.codec.c2l]
                if not variants:
                    self.skipped.append(c)
                    continue
                parts.append(self.alt([self.labels(self.codec.c2l[v]) for v in variants]))
            return self.cat(parts)
        if kind == 'set':
            members = list(dict.fromkeys(node[1]))
            labels = []
            for c in members:
                lab = self.codec.c2l.get(c)
                if lab is None:
                    if not node[2]:
                        self.skipped.append(c)
                    continue
                if len(lab) != 1:
                    raise ValueError(f'pattern {self.text!r}: set member {c!r} has {len(lab)} labels; a set member must have exactly one')
                labels.append(lab[0])
            if not labels and not self.skipped:
                raise ValueError(f'pattern {self.text!r}: a set that holds no character of the codec')
            return self.alt([self.labels([l]) for l in labels]) if labels else (True, [], [])
        if kind == 'cat':
            return self.cat([self.build(n) for n in node[1]])
        if kind == 'alt':
            return self.alt([self.build(n) for n in node[1]])
        _, inner, lo, hi = node
        parts = [self.build(inner) for _ in range(lo)]
        if hi is None:
            if lo == 0:
                parts.append(self.build(inner))
            n2, f2, l2 = parts[-1]
            self.link(l2, f2)                          # the last copy loops
            if lo == 0:
                parts[-1] = (True, f2, l2)
        else:
            for _ in range(hi - lo):
                n2, f2, l2 = self.build(inner)
                parts.append((True, f2, l2))
        return self.cat(parts)


def escape(text: str) -> str:
    """`text` as a pattern that matches exactly it (usable inside a set too)."""
    return ''.join('\\' + c if c in '\\.[](){}|?*+^$-' else c for c in text)


def single_label_chars(codec) -> List[str]:
    """The codec's characters `.`, ranges, negated sets and the shorthands draw from: one code point, exactly one label; in code-point
    order."""
    return sorted(c for c, lab in codec.c2l.items() if len(c) == 1 and len(lab) == 1)


def compile_pattern(text: str, codec, ignore_case: bool = False) -> PatternGraph:
    """The graph of the regular expression `text` over `codec`'s labels (module docstring: syntax).  A run of literals is encoded with
    `codec.encode`; with `ignore_case` a literal character c stands for those of {c, c.lower(), c.upper()} the codec has.  A character
    the codec lacks is reported in `.skipped` (then the graph has no states).  ValueError: a syntax error, something not built, a
    pattern that matches the empty string, more than 256 label states or more than 4096 predecessor-list entries."""
    b = _Builder(text, codec, ignore_case)
    nullable, first, last = b.build(_Parser(text, single_label_chars(codec)).parse())
    if b.skipped:
        return PatternGraph(text, [], [], [], [], ''.join(dict.fromkeys(b.skipped)), ignore_case)
    if nullable:
        raise ValueError(f'pattern {text!r} matches the empty string')
    P = len(b.cls)
    preds: List[List[int]] = [[] for _ in range(P)]
    for p in range(P):
        for q in sorted(b.follow[p]):
            preds[q].append(p)
    if sum(len(ps) for ps in preds) > MAX_EDGES:
        raise ValueError(f'pattern {text!r}: more than {MAX_EDGES} edges between its label states')
    fs, ls = set(first), set(last)
    return PatternGraph(text, b.cls, [p in fs for p in range(P)], [p in ls for p in range(P)], preds, '', ignore_case)


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def _rounds(graph: PatternGraph):
    """The predecessor lists by position: round k holds (states with more than k predecessors, their k-th predecessor, whether the
    two classes differ) -- the candidates of one frame are tried round by round, which is list order for every state."""
    out = []
    for k in range(max((len(ps) for ps in graph.preds), default=0)):
        qs = np.asarray([q for q, ps in enumerate(graph.preds) if len(ps) > k], dtype=np.int64)
        ps = np.asarray([graph.preds[q][k] for q in qs], dtype=np.int64)
        out.append((qs, ps, graph.cls[ps] != graph.cls[qs]))
    return out


def _check(outputs, graph: PatternGraph):
    x = np.asarray(outputs)
    if x.ndim != 2:
        raise ValueError('outputs must be a (C, T) matrix')
    if graph.P == 0:
        raise ValueError('a pattern without states')
    if ((graph.cls < 1) | (graph.cls >= x.shape[0])).any():
        raise ValueError(f'classes must lie in [1, {x.shape[0]})')
    return x


def pattern_candidates(outputs, graph: PatternGraph, dtype=np.float64) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The recursion of `spot_pattern_host`: (e (T), sigma (T), final (T)) -- per frame the score of the best match ending there
    (-inf: none), its first frame and the label state it ends in (-1: none).

    r_t(c) as in `search.spot_host`.  Label state q has a blank state q' after it.  Per frame, a candidate replacing the running best
    only if strictly greater, tried in this order:
        delta_t(q)  = best + r_t(cls[q]) over: stay; for each p of preds[q], ascending: delta_{t-1}(p'), then delta_{t-1}(p) if
                      cls[p] != cls[q]; the fresh start 0 if first[q] (it sets sigma = t);
        delta_t(q') = best + r_t(0) over: stay, then delta_{t-1}(q);
    sigma is carried with delta.  e_t = max over last[q] of delta_t(q), ties to the lowest q."""
    dt = np.dtype(dtype).type
    x = _check(outputs, graph)
    C, T = x.shape
    P = graph.P
    e, st, fin = np.full(T, -np.inf, dtype=dt), np.full(T, -1, dtype=np.int64), np.full(T, -1, dtype=np.int64)
    if T == 0:
        return e, st, fin
    xs = x.astype(dt)
    rall = (xs - xs.max(axis=0, keepdims=True)).astype(dt)
    r, rb = rall[graph.cls], rall[0]
    rounds = _rounds(graph)
    NEG = dt(-np.inf)
    first, last_q = graph.first, np.nonzero(graph.last)[0]
    da, sa = np.full(P, NEG, dtype=dt), np.full(P, -1, dtype=np.int64)          # label states
    db, sb = da.copy(), sa.copy()                                              # their blank states
    for t in range(T):
        best, src = da.copy(), sa.copy()
        for qs, ps, differ in rounds:
            take = db[ps] > best[qs]
            best[qs[take]], src[qs[take]] = db[ps[take]], sb[ps[take]]
            take = differ & (da[ps] > best[qs])
            best[qs[take]], src[qs[take]] = da[ps[take]], sa[ps[take]]
        take = first & (dt(0) > best)
        best[take], src[take] = dt(0), t
        bb, bs = db.copy(), sb.copy()
        take = da > bb
        bb[take], bs[take] = da[take], sa[take]
        reached = best > NEG
        da, sa = np.where(reached, best + r[:, t], NEG).astype(dt), np.where(reached, src, -1)
        reached = bb > NEG
        db, sb = np.where(reached, bb + rb[t], NEG).astype(dt), np.where(reached, bs, -1)
        k = int(np.argmax(da[last_q]))                  # the first maximum: the lowest q
        if da[last_q[k]] > NEG:
            e[t], st[t], fin[t] = da[last_q[k]], sa[last_q[k]], last_q[k]
    return e, st, fin


def spot_pattern_host(outputs, graph: PatternGraph, hits: int, min_score: float = -np.inf, dtype=np.float64) -> List[Tuple[int, int, float, int]]:
    """Matches of the pattern in the (C, T) logits `outputs`: up to `hits` non-overlapping (start, end, score, final state), best
    first.  The candidates are `pattern_candidates`'; the selection is `search.spot_host`'s: the largest live e_t (ties: the largest
    t), stop below min_score, every live candidate whose [sigma_u, u] intersects the hit dies."""
    e, st, fin = pattern_candidates(outputs, graph, dtype)
    T = e.shape[0]
    out: List[Tuple[int, int, float, int]] = []
    alive = e > -np.inf
    frames = np.arange(T)
    while len(out) < int(hits) and alive.any():
        m = e[alive].max()
        if m < min_score:
            break
        t = int(frames[alive & (e == m)][-1])
        s0 = int(st[t])
        out.append((s0, t, float(m), int(fin[t])))
        alive &= (frames < s0) | (st > t)
    return out


def match_host(outputs, graph: PatternGraph, start: int, end: int, final: int, dtype=np.float64, with_score: bool = False):
    """What a hit (start, end, ., final) of `spot_pattern_host` matched: the recursion of `pattern_candidates` on frames
    [start, end] only, a fresh start allowed at `start` only, with back-pointers; the collapsed label sequence of the best path that
    ends in label state `final` at `end` ([] if there is none).  `with_score`: (labels, that path's score) -- in exact arithmetic the
    hit's score."""
    dt = np.dtype(dtype).type
    x = _check(outputs, graph)
    P = graph.P
    start, end, final = int(start), int(end), int(final)
    if not (0 <= start <= end < x.shape[1] and 0 <= final < P):
        raise ValueError('not a hit of this pattern on these frames')
    xs = x[:, start:end + 1].astype(dt)
    rall = (xs - xs.max(axis=0, keepdims=True)).astype(dt)
    # plain lists of scalars: Python floats for float64 (the same arithmetic), numpy scalars of the type otherwise
    scalars = (lambda a: a.tolist()) if dt is np.float64 else (lambda a: [list(row) for row in a] if a.ndim == 2 else list(a))
    r, rb = scalars(rall[graph.cls].T), scalars(rall[0])                      # r[t][q]
    NEG = -np.inf if dt is np.float64 else dt(-np.inf)
    ZERO = 0.0 if dt is np.float64 else dt(0)
    n = end - start + 1
    cls = graph.cls.tolist()
    edges = [[(p, cls[p] != cls[q]) for p in graph.preds[q]] for q in range(P)]
    first = graph.first.tolist()
    da, db = [NEG] * P, [NEG] * P
    # back-pointers: state ids are q for a label state, P + q for its blank; -1: the fresh start; -2: not reached
    bpa, bpb = [], []
    for t in range(n):
        na, nb, ba, bb = [NEG] * P, [NEG] * P, [-2] * P, [-2] * P
        rt, rbt = r[t], rb[t]
        for q in range(P):
            dq = da[q]
            best, frm = dq, q
            for p, differ in edges[q]:
                v = db[p]
                if v > best:
                    best, frm = v, P + p
                if differ:
                    v = da[p]
                    if v > best:
                        best, frm = v, p
            if t == 0 and first[q] and ZERO > best:
                best, frm = ZERO, -1
            if best > NEG:
                na[q], ba[q] = best + rt[q], frm
            best, frm = db[q], P + q
            if dq > best:
                best, frm = dq, q
            if best > NEG:
                nb[q], bb[q] = best + rbt, frm
        da, db = na, nb
        bpa.append(ba)
        bpb.append(bb)
    if not da[final] > NEG:
        return ([], float(NEG)) if with_score else []
    path, s = [], final
    for t in range(n - 1, -1, -1):
        if s < P and (not path or path[-1] != s or was_blank):
            path.append(s)
        was_blank = s >= P
        s = bpa[t][s] if s < P else bpb[t][s - P]
        if s == -1:
            break
    labels = [int(graph.cls[q]) for q in reversed(path)]
    return (labels, float(da[final])) if with_score else labels


def labels_text(codec, labels: Sequence[int]) -> str:
    """The text of a matched label sequence."""
    return ''.join(c for c, _, _, _ in codec.decode([(int(l), 0, 0, 1.0) for l in labels]))
