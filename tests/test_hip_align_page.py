"""GPU: text-to-page alignment (cocr_ctc_align_page) against the definition `align.viterbi_align_page`.

Paths are compared where the inputs decide them, as in tests/test_hip_align.py: planted pages whose runner-up lies above twice the
float32 error bound
    tol = 8 sumT 2^-23 max(1, |s*|)
(7d's bound with the page's frame count: each of the sumT steps adds one rounding of the running sum and the error of one
log-probability), single-path pages, and the hand-derived cases of tests/test_align_page_host.py, whose decisions are exact ties or
whole logit levels apart."""
import json

import numpy as np
import pytest
import torch

from conformer_ocr_amd import align as A
from tests import test_align_page_host as H

pytestmark = pytest.mark.gpu
NEG = -np.inf
# the kernel's layout constants (csrc/ctc_align_page.hip.h): at most 16 waves of 64 lanes, 1 / 2 / 4 / 8 registers per lane
WAVES, LANES = 16, 64


def _form(S):
    sj = 1
    while sj < 8 and WAVES * LANES * sj < S:
        sj *= 2
    return sj, max(1, -(-S // (LANES * sj)))


def _engine():
    from conformer_ocr_amd.ctc_decoder import _scratch_engine
    return _scratch_engine(torch.device('cuda', 0))


def _dev(logits):
    return torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).cuda()


def _run(logits, out_lens, pages, targets, optional=None):
    return _engine().ctc_align_page(_dev(logits), out_lens, pages, targets, optional)


def _outputs(logits, out_lens, rows):
    return [logits[r, :out_lens[r]].T for r in rows]


def _tol(frames, score):
    return 8 * frames * 2.0 ** -23 * max(1.0, abs(score))


def _runner_up_gap(outputs, labels, optional):
    """Best score minus the best score of any path that leaves the best path somewhere: max-plus forward and backward tables over the
    page's lattice (float64), with the edges of the definition."""
    lps = [A.log_softmax64(o) for o in outputs]
    brk = H.break_frames([p.shape[1] for p in lps])                  # the tests' own reading of the definition
    lp = np.concatenate(lps, axis=1)
    T, L = lp.shape[1], len(labels)
    S = 2 * L + 1
    opt = np.asarray(optional, dtype=bool)
    ext = np.zeros(S, dtype=np.int64)
    ext[1::2] = labels
    idx = np.arange(S)
    odd, odd3 = (idx & 1) == 1, ((idx & 1) == 1) & (idx >= 3)
    diff2 = np.zeros(S, dtype=bool)
    diff2[3::2] = ext[3::2] != ext[1:-2:2]
    over = np.zeros(S, dtype=bool)
    over[5::2] = opt[1:-1] if L >= 3 else False
    diff4 = np.zeros(S, dtype=bool)
    diff4[5::2] = ext[5::2] != ext[1:-4:2]
    every = np.ones(S, dtype=bool)
    edges = {False: (every, every, diff2, over, over & diff4), True: (~odd, every, odd3, over, over)}       # [break frame][d]: into state s from s - d
    e = lp[ext]                                                      # (S, T)
    f = np.full((T, S), NEG)
    f[0, :2] = e[:2, 0]
    for t in range(1, T):
        p = np.concatenate([np.full(4, NEG), f[t - 1]])
        best = np.full(S, NEG)
        for d, ok in enumerate(edges[bool(brk[t])]):
            best = np.maximum(best, np.where(ok, p[4 - d:4 - d + S], NEG))
        f[t] = best + e[:, t]
    g = np.full((T, S), NEG)
    g[T - 1, max(S - 2, 0):] = 0.0
    for t in range(T - 2, -1, -1):
        n = np.concatenate([g[t + 1] + e[:, t + 1], np.full(4, NEG)])
        best = np.full(S, NEG)
        for d, ok in enumerate(edges[bool(brk[t + 1])]):
            best = np.maximum(best, np.where(np.concatenate([ok, np.zeros(4, dtype=bool)])[d:d + S], n[d:d + S], NEG))
        g[t] = best
    through = f + g                                                  # the best score of any path through a cell
    states = through.argmax(axis=1)                                  # the best path's cells (a second best path makes the gap 0)
    best = through.max()
    through[np.arange(T), states] = NEG
    return float(best - through.max())


# ---- 1. planted pages: the path itself ------------------------------------------------------------------------------------------------
SPACE = 1


def _planted_page(K, T, C, L, rng, gain=12.0, lens=None):
    """A text of L labels with single spaces (class SPACE, optional) between words, cut into K lines at K - 1 of its spaces, which are
    then not shown; every line planted on its frames as tests/test_hip_align.py `_planted` plants a line.  Returns the lines' (T, C)
    logits, their valid lengths, the labels, the optional flags and the expected (line, start, end) per label."""
    lab = rng.integers(2, C, L)
    spaces = [i for i in range(2, L - 2, 4) if rng.random() < 0.6]
    if len(spaces) < K - 1:
        spaces = list(range(2, L - 2, 4))
    lab[spaces] = SPACE
    optional = lab == SPACE
    cuts = [len(spaces) * k // K for k in range(1, K)]                # lines of about L / K labels
    bounds = [0] + [spaces[c] for c in cuts] + [L]
    logits = np.empty((K, T, C), dtype=np.float32)
    lens = [T] * K if lens is None else lens
    want = [None] * L
    for k in range(K):
        a = bounds[k] + (1 if k else 0)                              # the space a line was cut at belongs to neither side
        piece = lab[a:bounds[k + 1]]
        if k:
            want[bounds[k]] = (-1, -1, -1)
        n, S = len(piece), 2 * len(piece) + 1
        runs = np.zeros(S, dtype=np.int64)
        runs[1::2] = 1
        runs[2:-1:2] = piece[1:] == piece[:-1]
        runs += rng.multinomial(lens[k] - int(runs.sum()), [1.0 / S] * S)
        ext = np.zeros(S, dtype=np.int64)
        ext[1::2] = piece
        x = rng.standard_normal((T, C)).astype(np.float32)
        x[np.arange(lens[k]), np.repeat(ext, runs)] += np.float32(gain)
        logits[k] = x
        first = np.concatenate([[0], np.cumsum(runs)])
        for i in range(n):
            want[a + i] = (k, int(first[2 * i + 1]), int(first[2 * i + 2]) - 1)
    return logits, lens, lab, optional, want


def _check_page(got, outputs, labels, optional, planted=None, need_gap=True):
    records, score, line_scores = got
    want, s_star, want_lines = A.viterbi_align_page(outputs, labels, optional)
    frames = sum(o.shape[1] for o in outputs)
    tol = _tol(frames, s_star)
    if need_gap:
        gap = _runner_up_gap(outputs, labels, optional)
        print(f'page: K {len(outputs)} frames {frames} L {len(labels)} score {s_star:.4f} tol {tol:.3g} runner-up gap {gap:.4g}')
        assert gap > 2 * tol
    if planted is not None:
        assert [r[1:4] for r in want] == planted
    assert records is not None
    assert [r[:4] for r in records] == [r[:4] for r in want]
    assert abs(score - s_star) <= tol, (score, s_star, tol)
    assert np.abs(line_scores - want_lines).max() <= tol
    np.testing.assert_allclose([r[4] for r in records], [r[4] for r in want], atol=1e-5, rtol=0)


@pytest.mark.parametrize('P,K,T,C,L,seed', [(3, 3, 37, 12, 20, 21), (2, 8, 300, 64, 600, 22), (1, 16, 300, 128, 2100, 23)])
def test_planted_pages(P, K, T, C, L, seed):
    """The smallest page (one wave), wave seams (2 registers on 10 waves), several registers per lane (8 on 9 waves)."""
    rng = np.random.default_rng(seed)
    pages = [_planted_page(K, T, C, L + p, rng) for p in range(P)]
    logits = np.concatenate([pg[0] for pg in pages])
    rows = [list(range(p * K, (p + 1) * K)) for p in range(P)]
    out_lens = [T] * (P * K)
    # the premise first: every page's runner-up gap, before the device is asked
    for (_, _, lab, opt, want), r in zip(pages, rows):
        outs = _outputs(logits, out_lens, r)
        s_star = A.viterbi_align_page(outs, lab, opt)[1]
        assert _runner_up_gap(outs, lab, opt) > 2 * _tol(K * T, s_star)
    got = _run(logits, out_lens, rows, [pg[2] for pg in pages], [pg[3] for pg in pages])
    for (_, _, lab, opt, want), r, g in zip(pages, rows, got):
        _check_page(g, _outputs(logits, out_lens, r), lab, opt, planted=want, need_gap=False)


@pytest.mark.parametrize('K,T', [(10, 1300), (20, 1300)])
def test_long_planted_pages(K, T):
    """13 000 frames: lz in more than 48 KB of dynamic LDS (the kernel's limit is raised first); 26 000 frames: above 24 576, lz in the
    page's workspace region."""
    rng = np.random.default_rng(60 + K)
    logits, lens, lab, opt, want = _planted_page(K, T, 8, 100, rng)
    assert (K * T * 4 > 48 * 1024) and ((K * T > 24576) == (K == 20))
    got, = _run(logits, lens, [list(range(K))], [lab], [opt])
    _check_page(got, _outputs(logits, lens, range(K)), lab, opt, planted=want)


def test_optional_spaces_through_the_page_layer():
    """The Python page layer on the device's records: a text with spaces (a codec that has one) on lines cut at two of them --
    `optional_labels` -> `cocr_ctc_align_page` -> `page_result`: the spaces at the breaks come back as `dropped`, the others stay."""
    from conformer_ocr_amd.codec import PytorchCodec
    from conformer_ocr_amd.page import line_geometry
    codec = PytorchCodec([' ', 'a', 'b', 'c'])
    text = 'ab ca bc ab ccb a'
    labels, skipped = A.encode_text(codec, text)
    optional = A.optional_labels(codec, labels)
    pieces = ['ab ca', 'bc ab', 'ccb a']
    T, C = 30, 5
    rng = np.random.default_rng(71)
    logits = rng.standard_normal((3, T, C)).astype(np.float32)
    for k, piece in enumerate(pieces):                                # every character on 3 frames, one blank frame between
        for i, ch in enumerate(piece):
            logits[k, 4 * i:4 * i + 3, codec.c2l[ch][0]] += 12.0
            logits[k, 4 * i + 3, 0] += 12.0
        logits[k, 4 * len(piece):, 0] += 12.0
    got, = _run(logits, [T] * 3, [[0, 1, 2]], [labels], [optional])
    want = A.viterbi_align_page(_outputs(logits, [T] * 3, range(3)), labels, optional)
    assert [r[:4] for r in got[0]] == [r[:4] for r in want[0]]
    geoms = [line_geometry(f'l{k}', [(10, 20 + 40 * k), (310, 20 + 40 * k)], [(10, 5 + 40 * k), (310, 5 + 40 * k), (310, 30 + 40 * k), (10, 30 + 40 * k)])
             for k in range(3)]
    res = A.page_result(codec, geoms, got, [T] * 3, [300] * 3, 0, skipped)
    assert [ln['text'] for ln in res['lines']] == pieces and res['dropped'] == '  ' and res['skipped'] == ''
    assert [[w[0] for w in ln['words']] for ln in res['lines']] == [p.split() for p in pieces]


def test_mixed_forms_in_one_call():
    """Pages of different K and S in one call (the form follows the largest S: 2 registers per lane; the small pages leave waves
    without a live state), rows in shuffled order, ragged lengths, a line of no frames and a planted all-blank line."""
    rng = np.random.default_rng(31)
    T, C = 120, 40
    big = _planted_page(6, T, C, 560, rng, lens=[T, 100, T, 117, T, 119])
    small = _planted_page(2, T, C, 9, rng, lens=[40, 33])
    blank = _planted_page(3, T, C, 30, rng, lens=[64, 50, 90])
    one = _planted_page(1, T, C, 0, rng, lens=[25])
    # page `blank`: an all-blank line and a line of no frames between its planted lines
    quiet = rng.standard_normal((1, T, C)).astype(np.float32)
    quiet[0, :, 0] += 12.0
    logits = np.concatenate([big[0], small[0], blank[0], one[0], quiet, rng.standard_normal((2, T, C)).astype(np.float32)])
    out_lens = big[1] + small[1] + blank[1] + one[1] + [70, 0, T]
    perm = rng.permutation(len(out_lens))                             # rows in another order than the pages name them
    inv = np.argsort(perm)
    logits, out_lens = logits[perm], [out_lens[i] for i in perm]
    rows = [[0, 1, 2, 3, 4, 5], [6, 7], [8, 12, 9, 13, 10], [11]]
    rows = [[int(inv[r]) for r in pg] for pg in rows]
    targets = [big[2], small[2], blank[2], one[2]]
    optional = [big[3], small[3], blank[3], one[3]]
    got = _run(logits, out_lens, rows, targets, optional)
    shift = {0: 0, 1: 2, 2: 4}
    wants = [big[4], small[4], [(shift[k], a, b) if k >= 0 else (k, a, b) for k, a, b in blank[4]], one[4]]
    for g, r, lab, opt, want in zip(got, rows, targets, optional, wants):
        _check_page(g, _outputs(logits, out_lens, r), lab, opt, planted=want)
    assert got[3][0] == []


# ---- 2. seams: single-path pages ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,K', [(100, 3), (300, 4), (600, 5), (1100, 6), (2100, 7), (4095, 9)])
def test_seams_on_the_single_path(L, K):
    """sumT = L frames for L labels without equal neighbours inside a line: one path, label k on frame k, every step two states up --
    through the lane rotations, and at every state index that is a multiple of 64 through a register seam (the previous register's
    rotation) or, at multiples of 64 SJ, a wave seam (the LDS slot).  S = 2 L + 1 selects (SJ, waves) = (1, 4), (1, 10), (2, 10),
    (4, 9), (8, 9), (8, 16) -- the largest text the entry takes --: label states lie on both sides of every seam of the form, since every state below S is a multiple of 64
    away from one."""
    sj, waves = _form(2 * L + 1)
    assert (sj, waves) == {100: (1, 4), 300: (1, 10), 600: (2, 10), 1100: (4, 9), 2100: (8, 9), 4095: (8, 16)}[L]
    wave_seams = [w * LANES * sj for w in range(1, waves)]
    register_seams = [r * LANES for r in range(1, sj * waves) if r % sj and r * LANES < 2 * L]
    assert wave_seams[-1] < 2 * L and (sj == 1 or len(register_seams) >= (sj - 1) * (waves - 1))
    rng = np.random.default_rng(7100 + L)
    C = 6
    lens = np.diff(np.concatenate([[0], np.sort(rng.choice(np.arange(1, L), K - 1, replace=False)), [L]])).tolist()
    T = max(lens)
    labels = np.empty(L, dtype=np.int64)
    labels[0] = rng.integers(1, C)
    breaks = set(np.cumsum(lens)[:-1].tolist())
    for k in range(1, L):                                             # equal neighbours over every break (two emissions, no blank), nowhere else
        labels[k] = labels[k - 1] if k in breaks else 1 + (labels[k - 1] - 1 + rng.integers(1, C - 1)) % (C - 1)
    logits = (rng.standard_normal((K, T, C)) * 2.0).astype(np.float32)
    (records, score, line_scores), = _run(logits, lens, [list(range(K))], [labels])
    lps = [A.log_softmax64(logits[k, :lens[k]].T) for k in range(K)]
    first = np.concatenate([[0], np.cumsum(lens)])
    own = np.concatenate(lps, axis=1)[labels, np.arange(L)]
    line_of = np.repeat(np.arange(K), lens)
    assert [r[:4] for r in records] == [(int(labels[k]), int(line_of[k]), int(k - first[line_of[k]]), int(k - first[line_of[k]])) for k in range(L)]
    tol = _tol(L, own.sum())
    assert abs(score - own.sum()) <= tol
    assert np.abs(line_scores - np.array([own[first[k]:first[k + 1]].sum() for k in range(K)])).max() <= tol
    np.testing.assert_allclose([r[4] for r in records], np.exp(own), atol=1e-5, rtol=0)


# ---- 3. the hand-derived cases of the host file, on the device ----------------------------------------------------------------------
HAND = [
    ('aa over two 1-frame lines', [H.line(H.col(1)), H.line(H.col(1))], [1, 1], None),
    ('aa on one 2-frame line', [H.line(H.col(1), H.col(1))], [1, 1], None),
    ('a label strong on both sides of a break', [H.line(H.col(0), H.col(1)), H.line(H.col(1), H.col(2))], [1, 2], None),
    ('a space inside a line', [H.line(H.col(1), H.col(3), H.col(2))], [1, 3, 2], [False, True, False]),
    ('space skipped from s-4', [H.line(H.col(1)), H.line(H.col(2))], [1, 3, 2], [False, True, False]),
    ('space skipped from s-3', [H.line(H.col(1), H.col(0)), H.line(H.col(2))], [1, 3, 2], [False, True, False]),
    ('equal-class s-4 inside a line', [H.line(H.col(1), H.col(1))], [1, 3, 1], [False, True, False]),
    ('equal-class s-4 at a break', [H.line(H.col(1)), H.line(H.col(1))], [1, 3, 1], [False, True, False]),
    ('equal-class with a blank inside a line', [H.line(H.col(1), H.col(0), H.col(1))], [1, 3, 1], [False, True, False]),
    ('tie stay / s-1', [H.line(H.col(0), H.both(0, 1), H.col(1))], [1], None),
    ('tie s-1 / s-2', [H.line(H.both(1, 0), H.both(1, 0), H.col(2))], [1, 2], None),
    ('tie s-2 / s-3 / s-4', [H.line(H.col(1), np.array([H.HI, H.HI, H.LO, H.HI]), H.col(2))], [1, 3, 2], [False, True, False]),
    ('tie s-3 / s-4', [H.line(H.col(1), H.both(0, 1), H.col(2))], [1, 3, 2], [False, True, False]),
    ('a line that takes no label', [H.line(H.col(1)), H.line(H.col(0), H.col(0)), H.line(H.col(2))], [1, 2], None),
    ('a line of no frames', [H.line(H.col(1), H.col(0)), H.line(), H.line(H.col(2))], [1, 2], None),
    ('an empty first line', [H.line(), H.line(H.col(1), H.col(0)), H.line(H.col(2))], [1, 2], None),
]


def test_hand_derived_cases_in_one_call():
    """Every case a page of one call.  The logits are whole levels (0 and 4), identical columns give bit-identical log-probabilities
    on the device too (one order of summation per frame), so the ties are ties there as well: the records are compared exactly."""
    T, C = 3, 4
    n_rows = sum(len(outs) for _, outs, _, _ in HAND)
    logits = np.zeros((n_rows, T, C), dtype=np.float32)
    out_lens, rows, at = [], [], 0
    for _, outs, _, _ in HAND:
        rows.append(list(range(at, at + len(outs))))
        for o in outs:
            logits[at, :o.shape[1]] = o.T
            out_lens.append(o.shape[1])
            at += 1
    targets = [lab for _, _, lab, _ in HAND]
    optional = [None if opt is None else opt for _, _, _, opt in HAND]
    got = _run(logits, out_lens, rows, targets, optional)
    for (name, outs, lab, opt), g in zip(HAND, got):
        want = A.viterbi_align_page(outs, lab, opt)
        if want[0] is None:
            assert g == (None, NEG, None), name
            continue
        assert g[0] is not None, name
        assert [r[:4] for r in g[0]] == [r[:4] for r in want[0]], name
        assert abs(g[1] - want[1]) <= 1e-5 and np.abs(g[2] - want[2]).max() <= 1e-5, name
        np.testing.assert_allclose([r[4] for r in g[0]], [r[4] for r in want[0]], atol=1e-5, rtol=0)


# ---- 4. one line against cocr_ctc_align -------------------------------------------------------------------------------------------------
def test_one_line_pages_against_ctc_align():
    """K = 1 and nothing optional on the planted lines of tests/test_hip_align.py: starts, ends and counts exactly."""
    from tests.test_hip_align import _planted
    N, T = 8, 300
    logits, labels, _ = _planted(N, T, 128, 25, 120, 11, 6)
    eng = _engine()
    d = _dev(logits)
    flat = eng.ctc_align(d, [T] * N, np.concatenate(labels), [len(l) for l in labels])
    paged = eng.ctc_align_page(d, [T] * N, [[n] for n in range(N)], labels)
    for (records, score), (page_records, page_score, line_scores) in zip(flat, paged):
        assert records is not None and page_records is not None and len(records) == len(page_records)
        assert [(l, st, en) for l, _, st, en, _ in page_records] == [r[:3] for r in records]
        assert all(r[1] == 0 for r in page_records)
        assert abs(page_score - score) <= _tol(T, score) and abs(line_scores[0] - score) <= _tol(T, score)


# ---- 5. edges, reproducibility, errors, the greedy shortcut ---------------------------------------------------------------------------
def test_no_labels_and_no_fit():
    rng = np.random.default_rng(41)
    logits = rng.standard_normal((5, 6, 5)).astype(np.float32)
    out_lens = [6, 3, 0, 2, 0]
    #        L = 0 over two lines   no fit: 4 labels in 2 frames   no frames, no labels   no frames with a label
    rows = [[0, 1], [3], [2], [4]]
    got = _run(logits, out_lens, rows, [[], [1, 2, 3, 1], [], [2]])
    lp = [A.log_softmax64(logits[r, :out_lens[r]].T) for r in range(5)]
    assert got[0][0] == [] and abs(got[0][1] - (lp[0][0].sum() + lp[1][0].sum())) < 1e-4
    np.testing.assert_allclose(got[0][2], [lp[0][0].sum(), lp[1][0].sum()], atol=1e-4)
    assert got[1] == (None, NEG, None) and got[3] == (None, NEG, None)
    assert got[2][0] == [] and got[2][1] == 0.0 and got[2][2].tolist() == [0.0]
    # the raw outputs of a page that does not fit
    eng = _engine()
    h = eng.ctc_align_page_async(_dev(logits), out_lens, rows, [[], [1, 2, 3, 1], [], [2]])
    eng.collect_align_page(h)
    ints, conf, score, counts, line_score = h[1]
    assert counts.numpy()[:4].tolist() == [0, -1, 0, -1]
    assert ints.numpy()[:, :5].tolist() == [[-1] * 5] * 3 and conf.numpy()[:5].tolist() == [0.0] * 5


def test_runs_are_bitwise_reproducible():
    rng = np.random.default_rng(51)
    logits = (rng.standard_normal((6, 90, 30)) * 2.0).astype(np.float32)
    labels = rng.integers(1, 30, 150)
    optional = np.zeros(150, dtype=bool)
    optional[5:145:7] = True
    args = (logits, [90, 80, 90, 70, 90, 85], [[0, 1, 2, 3, 4, 5]], [labels], [optional])
    a, b = _run(*args), _run(*args)
    assert a[0][0] is not None and a[0][0] == b[0][0] and a[0][1] == b[0][1] and a[0][2].tobytes() == b[0][2].tobytes()


def test_argument_errors():
    eng = _engine()
    p = torch.zeros((3, 4, 3), device='cuda')
    ok = dict(out_lens=[4, 4, 4], pages=[[0, 1]], targets=[[1, 2, 1]], optional=[[False, True, False]])

    def call(**kw):
        a = dict(ok, **kw)
        return eng.ctc_align_page(p, a['out_lens'], a['pages'], a['targets'], a['optional'])
    for bad in (dict(targets=[[1, 3, 1]]), dict(targets=[[1, 0, 1]]),                     # a label outside [1, ncls)
                dict(out_lens=[5, 4, 4]), dict(out_lens=[4, -1, 4]),                       # out_lens outside [0, T]
                dict(pages=[[0, 3]]), dict(pages=[[-1, 1]]), dict(pages=[[0, 0]]),        # a row outside [0, N) or used twice
                dict(pages=[[0, 1], [1]], targets=[[1], [1]], optional=[None, None]),     # ... over two pages
                dict(optional=[[True, False, False]]), dict(optional=[[False, False, True]]),
                dict(targets=[[1, 2, 2, 1]], optional=[[False, True, True, False]]),
                dict(pages=[], targets=[], optional=[])):                                  # P < 1
        with pytest.raises(ValueError):
            call(**bad)
    # descending offsets reach the C entry only directly
    import ctypes as C
    i32 = lambda a: np.asarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    lens, off, rows, tg, tl = (np.asarray(a, dtype=np.int32) for a in ([4, 4, 4], [0, 2, 1], [0, 1], [1], [1, 0]))
    opt = np.zeros(1, dtype=np.uint8)
    out = torch.zeros(16, dtype=torch.int32, device='cuda')
    ptr = C.c_void_p(out.data_ptr())
    rc = eng.lib.cocr_ctc_align_page(eng._h, C.c_void_p(p.data_ptr()), 3, 4, 3, lens.ctypes.data_as(C.POINTER(C.c_int32)), 2,
                                     off.ctypes.data_as(C.POINTER(C.c_int32)), rows.ctypes.data_as(C.POINTER(C.c_int32)),
                                     tg.ctypes.data_as(C.POINTER(C.c_int32)), tl.ctypes.data_as(C.POINTER(C.c_int32)),
                                     opt.ctypes.data_as(C.POINTER(C.c_uint8)), ptr, ptr, ptr, ptr, ptr, ptr, ptr, None)
    assert rc == -1 and b'descend' in eng.lib.cocr_last_error()                           # COCR_EINVAL
    # the limits (COCR_EUNSUPPORTED surfaces as NotImplementedError)
    long_text = [1, 2] * 2048                                                              # 4096 labels
    with pytest.raises(NotImplementedError):
        eng.ctc_align_page(p, [4, 4, 4], [[0]], [long_text])
    wide = torch.zeros((4097, 1, 3), device='cuda')
    with pytest.raises(NotImplementedError):
        eng.ctc_align_page(wide, [1] * 4097, [list(range(4097))], [[1]])                   # 4097 lines
    tall = torch.zeros((10, 7000, 3), device='cuda')
    with pytest.raises(NotImplementedError):
        eng.ctc_align_page(tall, [7000] * 10, [list(range(10))], [[1]])                    # 70000 frames
    # tables beyond 2 GiB: 9 pages of 65000 frames x 4095 labels ask for 8125 x 8192 words of back-pointers each (266 MB)
    many = torch.zeros((90, 6500, 3), device='cuda')
    with pytest.raises(NotImplementedError):
        eng.ctc_align_page(many, [6500] * 90, [list(range(10 * i, 10 * i + 10)) for i in range(9)], [long_text[:4095]] * 9)
    with pytest.raises(NotImplementedError):
        eng.ctc_align_page(torch.zeros((1, 1, (1 << 22) + 1), device='cuda'), [1], [[0]], [[1]])    # more than 2^22 classes
    got, = call()
    assert got[0] is not None                                                              # the engine is still usable


def test_greedy_shortcut_is_not_disturbed(text_case):
    """`ctc_align_page` between a forward and its `ctc_greedy`: the decoder epilogue's per-frame argmax still belongs to the logits."""
    from tests.test_hip_align import _net
    tc = text_case('cfg2_text')
    net = _net(tc, 'bf16')
    image, lens, idx = tc.batch(0)
    line = torch.from_numpy(image[:8]).cuda().squeeze(1)
    eng = net.engine(torch.device('cuda', 0))
    logits, out_lens = eng.forward(line, lens[:8])
    assert eng._argmax_is_fresh(logits)
    labels = [tc.ref_strings[i] for i in idx[:8]]
    got = eng.ctc_align_page(logits, out_lens, [[0, 1, 2, 3], [4, 5, 6, 7]], [sum(labels[:4], []), sum(labels[4:], [])])
    assert all(r is not None for r, _, _ in got)
    assert eng._argmax_is_fresh(logits)
    after = eng.ctc_greedy(logits, out_lens)
    logits2, out_lens2 = eng.forward(line, lens[:8])
    assert eng.ctc_greedy(logits2, out_lens2) == after
    assert eng.ctc_greedy(logits.clone(), out_lens) == after              # from the values, without the shortcut


# ---- 6. pages end to end --------------------------------------------------------------------------------------------------------------
def test_pages_aligned_to_the_strings_they_were_read_as(text_case, tmp_path, capsys):
    """`page_synth` pages aligned to the space-joined strings they were read as give `recognize_pages`' per-line strings and cuts: the
    greedy path of every line is the per-frame argmax, so their concatenation is the page's best path.  (The fixture's alphabet has
    no space: the joining spaces are reported as skipped, and the line breaks are found without them.)  Two groups of pages, so that
    the second forward is enqueued before the first alignment is collected."""
    from PIL import Image
    from conformer_ocr_amd.codec import ascii_codec
    from conformer_ocr_amd.dataset import GroundTruthDataset, gt_text_path
    from conformer_ocr_amd.page import Line, read_page_xml, recognize_pages
    from conformer_ocr_amd.pred import PytorchRecognitionModel, save_safetensors
    from tests import page_synth
    from tests.test_hip_align import DROPS, FIXTURE_FORM, KINDS, PICK, _net
    tc = text_case('cfg2_text')
    lines = [np.rint(tc.lines[i] * 255.0).astype(np.uint8) for i in PICK]
    page, placed = page_synth.text_page(lines, KINDS)
    page_lines = [Line(f'line{k}', P, B) for k, (_, P, B) in enumerate(placed)]
    net = _net(tc, 'bf16')
    read, = recognize_pages(net, [(page, page_lines)], batch_size=4, **FIXTURE_FORM)
    text = ' '.join(r['text'] for r in read)
    head = '\n'.join(r['text'] for r in read[:4])
    got, part = A.align_text_pages(net, [(page, page_lines), (page, page_lines[:4])], [text, head], batch_size=4, group_lines=10, **FIXTURE_FORM)
    for res, want in ((got, read), (part, read[:4])):
        assert res['lines'] is not None and res['skipped'] == ' ' * (len(want) - 1) and res['dropped'] == ''
        assert [g['id'] for g in res['lines']] == [f'line{k}' for k in range(len(want))]
        frames = sum(g['frames'] for g in res['lines'])
        assert abs(sum(g['score'] for g in res['lines']) - res['score']) <= _tol(frames, res['score'])
        for g, r in zip(res['lines'], want):
            assert g['text'] == r['text'] and g['frames'] > 0 and np.isfinite(g['score']) and g['score'] < 0
            assert [(c, q) for c, q, _ in g['cuts']] == [(c, q) for c, q, _ in r['cuts']]
            assert ''.join(w[0] for w in g['words']) == r['text'].replace(' ', '')
    # a page above the kernel's bound goes through the definition: the same lines (scores within the bound of the float32 kernel)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(A, 'MAX_PAGE_LABELS', 10)
        host, = A.align_text_pages(net, [(page, page_lines)], [text], batch_size=4, **FIXTURE_FORM)
    assert [(g['id'], g['text'], g['frames']) for g in host['lines']] == [(g['id'], g['text'], g['frames']) for g in got['lines']]
    assert [[(c, q) for c, q, _ in g['cuts']] for g in host['lines']] == [[(c, q) for c, q, _ in g['cuts']] for g in got['lines']]
    assert abs(host['score'] - got['score']) <= _tol(sum(g['frames'] for g in got['lines']), host['score'])
    # a text that does not fit: more characters than the page has frames
    none, = A.align_text_pages(net, [(page, page_lines[:1])], [text * 3], batch_size=4, **FIXTURE_FORM)
    assert none['lines'] is None and none['score'] == NEG

    # the command on the same page: JSON as the function returns, ground truth that `-f path` reads
    Image.fromarray(page).save(tmp_path / 'scan.png')
    pts = lambda a: ' '.join(f'{x:.3f},{y:.3f}' for x, y in a)
    body = ''.join(f'<TextLine id="{l.id}"><Coords points="{pts(l.boundary)}"/><Baseline points="{pts(l.baseline)}"/></TextLine>\n' for l in page_lines)
    (tmp_path / 'scan.xml').write_text('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2019-07-15">'
                                       f'<Page imageFilename="scan.png"><TextRegion id="r">{body}</TextRegion></Page></PcGts>\n', encoding='utf-8')
    (tmp_path / 'scan.txt').write_text(text + '\n', encoding='utf-8')
    src = PytorchRecognitionModel(**tc.hp.as_dict(), **DROPS, codec=ascii_codec(tc.hp.num_classes))
    src.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    save_safetensors(src, tmp_path / 'model.tar')
    capsys.readouterr()
    out, gt = tmp_path / 'out.json', tmp_path / 'gt'
    assert A.main(['-m', str(tmp_path / 'model.tar'), '-f', 'page', '--text-input', str(tmp_path / 'scan.xml'), str(tmp_path / 'scan.txt'), str(out),
                   '--gt-dir', str(gt), '--pad', '0', '--edge', '1200', '--batch-size', '4', '--worst', '2']) == 0
    err = capsys.readouterr().err
    assert f'{len(read)} of {len(read)} lines took text' in err and f'{len(read)} written' in err
    with open(out, encoding='utf-8') as fp:
        back = json.load(fp)
    # the file's coordinates are rounded to 3 decimals: the command is held to the function on the lines as the file gives them
    want, = A.align_text_pages(net, [(page, read_page_xml(tmp_path / 'scan.xml').lines)], [text], batch_size=4, **FIXTURE_FORM)
    assert back['skipped'] == want['skipped'] and back['dropped'] == want['dropped']
    assert abs(back['score'] - want['score']) <= _tol(sum(w['frames'] for w in want['lines']), want['score'])
    for b, w, r in zip(back['lines'], want['lines'], read):
        assert b['id'] == w['id'] and b['text'] == w['text'] == r['text'] and b['frames'] == w['frames']
        assert [(c, [list(p) for p in q]) for c, q, _ in w['cuts']] == [(c, q) for c, q, _ in b['cuts']]
    files = sorted(str(gt / f'scan_line{k}.png') for k in range(len(read)))
    assert sorted(str(p) for p in gt.glob('*.png')) == files
    for k, r in enumerate(read):
        with open(gt_text_path(str(gt / f'scan_line{k}.png')), encoding='utf-8') as fp:
            assert fp.read() == r['text'] + '\n'
    data = GroundTruthDataset(files, format_type='path', normalization=None, height=tc.hp.height, pad=0, batch_size=4, edge=1200, codec=net.codec,
                              codec_num_classes=tc.hp.num_classes)
    assert sorted(ln.text for ln in data.lines) == sorted(r['text'] for r in read)
    # a threshold above every line's score per frame writes nothing
    gt2 = tmp_path / 'gt2'
    assert A.main(['-m', str(tmp_path / 'model.tar'), '-f', 'page', '--text-input', str(tmp_path / 'scan.xml'), str(tmp_path / 'scan.txt'), str(out),
                   '--gt-dir', str(gt2), '--min-line-score', '0.5', '--pad', '0', '--edge', '1200', '--batch-size', '4']) == 0
    assert not gt2.exists()
