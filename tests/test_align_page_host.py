"""Host: the definition of text-to-page alignment, `align.viterbi_align_page`, against an enumeration of every
lattice path, against `align.viterbi_align` (P1: one line; P2: the best cut into lines) and against itself without optional labels
(P3), plus one hand-derived case per rule of a line break."""
import itertools

import numpy as np
import pytest

from conformer_ocr_amd import align as A

NEG = -np.inf


def _logits(rng, C, T, grid):
    if grid:
        return rng.integers(-24, 25, (C, T)).astype(np.float64) / 8.0
    return rng.standard_normal((C, T)) * 2.0


def _case(seed, grid=False, with_optional=True):
    """C = 4, K <= 3, T_k <= 4 (a line may have no frame), L <= 4."""
    rng = np.random.default_rng(seed)
    C, K = 4, int(rng.integers(1, 4))
    outputs = [_logits(rng, C, int(rng.integers(0, 5)), grid) for _ in range(K)]
    L = int(rng.integers(0, 5))
    labels = [int(l) for l in rng.integers(1, C, L)]
    optional = np.zeros(L, dtype=bool)
    if with_optional:
        for k in range(1, L - 1):
            if not optional[k - 1] and rng.random() < 0.5:
                optional[k] = True
    return outputs, labels, optional


def break_frames(lens):
    """The test's own reading of the definition: the first frame of every line but the first that has frames."""
    brk, at = [], 0
    for k, n in enumerate(lens):
        brk += [k >= 1 and t == 0 for t in range(n)]
        at += n
    return np.array(brk, dtype=bool)


def test_break_frames_of_the_module():
    for lens in ([3], [2, 2], [0, 2, 1], [2, 0, 0, 1], [0, 0], [1, 1, 1]):
        first, brk = A.page_frames(lens)
        assert brk.tolist() == break_frames(lens).tolist() and first.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()


def _enumerate(outputs, labels, optional):
    """The best score over every state sequence the definition admits, summed in frame order as the recursion sums it."""
    lps = [A.log_softmax64(o) for o in outputs]
    lp = np.concatenate(lps, axis=1)
    brk = break_frames([p.shape[1] for p in lps])
    T, L = lp.shape[1], len(labels)
    S = 2 * L + 1
    ext = [0] * S
    ext[1::2] = labels
    if T == 0:
        return 0.0 if L == 0 else NEG

    def allowed(s, d, t):
        if d == 0:
            return not (s & 1 and brk[t])
        if d == 1:
            return s >= 1
        if not s & 1 or s - d < 0:
            return False
        if d == 2:
            return ext[s] != ext[s - 2] or bool(brk[t])
        if not optional[(s - 3) // 2]:
            return False
        return d == 3 or ext[s] != ext[s - 4] or bool(brk[t])

    best = NEG

    def walk(t, s, score):
        nonlocal best
        if t == T - 1:
            if s >= S - 2:
                best = max(best, score)
            return
        for d in range(5):
            n = s + d
            if n < S and allowed(n, d, t + 1):
                walk(t + 1, n, score + lp[ext[n], t + 1])
    for s in range(min(2, S)):
        walk(0, s, lp[ext[s], 0])
    return best


def _path_ok(outputs, labels, records, line_scores, score):
    """The records describe one path: ascending, no label over two lines, and the line scores add up to the page score."""
    at = (-1, -1)
    for (l, ln, st, en, cf), want in zip(records, labels):
        assert l == want
        if ln < 0:
            assert (ln, st, en, cf) == (-1, -1, -1, 0.0)
            continue
        assert 0 <= st <= en < np.asarray(outputs[ln]).shape[1]
        assert (ln, st) > at
        at = (ln, en)
    assert abs(float(np.sum(line_scores)) - score) <= 1e-12 * max(1.0, abs(score))


@pytest.mark.parametrize('grid', [False, True])
def test_against_enumeration(grid):
    finite = 0
    for seed in range(150):
        outputs, labels, optional = _case(seed, grid)
        records, score, line_scores = A.viterbi_align_page(outputs, labels, optional)
        want = _enumerate(outputs, labels, optional)
        assert score == want, (seed, score, want)
        if records is None:
            assert score == NEG and line_scores is None
            continue
        finite += 1
        _path_ok(outputs, labels, records, line_scores, score)
    assert finite > 60


@pytest.mark.parametrize('grid', [False, True])
def test_p1_one_line_is_viterbi_align(grid):
    rng = np.random.default_rng(5)
    for _ in range(100):
        C, T, L = int(rng.integers(2, 7)), int(rng.integers(0, 12)), int(rng.integers(0, 6))
        out = _logits(rng, C, T, grid)
        labels = [int(l) for l in rng.integers(1, C, L)]
        want, s_want = A.viterbi_align(out, labels)
        got, s_got, line_scores = A.viterbi_align_page([out], labels, np.zeros(L, dtype=bool))
        assert s_got == s_want
        if want is None:
            assert got is None and line_scores is None
        else:
            assert [(l, st, en, cf) for l, _, st, en, cf in got] == want
            assert all(r[1] == 0 for r in got)


def _cuts(L, K):
    for c in itertools.combinations_with_replacement(range(L + 1), K - 1):
        yield (0,) + c + (L,)


def test_p2_best_cut_into_lines():
    finite = 0
    for seed in range(150):
        outputs, labels, _ = _case(seed, with_optional=False)
        _, score, _ = A.viterbi_align_page(outputs, labels, np.zeros(len(labels), dtype=bool))
        want = NEG
        for cut in _cuts(len(labels), len(outputs)):
            want = max(want, sum(A.viterbi_align(o, labels[a:b])[1] for o, a, b in zip(outputs, cut[:-1], cut[1:])))
        if want == NEG:
            assert score == NEG
        else:
            finite += 1
            assert abs(score - want) <= 1e-12, (seed, score, want)
    assert finite > 60


def test_p3_optional_is_best_deletion():
    finite = 0
    for seed in range(300):
        outputs, labels, optional = _case(1000 + seed)
        _, score, _ = A.viterbi_align_page(outputs, labels, optional)
        idx = [k for k in range(len(labels)) if optional[k]]
        want = NEG
        for r in range(len(idx) + 1):
            for gone in itertools.combinations(idx, r):
                kept = [l for k, l in enumerate(labels) if k not in gone]
                want = max(want, A.viterbi_align_page(outputs, kept, np.zeros(len(kept), dtype=bool))[1])
        assert score == want, (seed, score, want)
        finite += score != NEG
    assert finite > 100


# ---- hand-derived cases: columns are built from three logit levels, so that every comparison below is decided by counting them ----------
HI, LO = 4.0, 0.0


def col(c, C=4):
    """A frame that favours class c: HI there, LO elsewhere."""
    x = np.full(C, LO)
    x[c] = HI
    return x


def line(*cols):
    return np.stack(cols, axis=1) if cols else np.zeros((4, 0))


def both(c1, c2, C=4):
    x = np.full(C, LO)
    x[c1] = x[c2] = HI
    return x


def places(records):
    return [r[1:4] for r in records]


def test_equal_neighbours_over_a_break_need_no_blank():
    """'aa' over two 1-frame lines fits: two emissions; on one 2-frame line it does not."""
    records, score, _ = A.viterbi_align_page([line(col(1)), line(col(1))], [1, 1])
    assert places(records) == [(0, 0, 0), (1, 0, 0)] and np.isfinite(score)
    assert A.viterbi_align_page([line(col(1), col(1))], [1, 1]) == (None, NEG, None)


def test_label_does_not_span_a_break():
    """'ab' with a strong on the last frame of line 0 AND the first of line 1: on the concatenation a spans both frames; on the page
    it is placed on one side.  Three paths tie (blank a | b b, blank a | blank b, blank blank | a b: one frame off its class each);
    at the last frame b's state tries stay first and keeps it, so b began at the break frame, entered from a on line 0."""
    l0, l1 = line(col(0), col(1)), line(col(1), col(2))
    flat, _ = A.viterbi_align(np.concatenate([l0, l1], axis=1), [1, 2])
    assert [r[1:3] for r in flat] == [(1, 2), (3, 3)]
    records, _, _ = A.viterbi_align_page([l0, l1], [1, 2])
    assert places(records) == [(0, 1, 1), (1, 0, 1)]
    lp = A.log_softmax64(col(1).reshape(-1, 1))
    # the page's path pays one blank-for-a frame where the concatenation's pays none
    flat_score = A.viterbi_align(np.concatenate([l0, l1], axis=1), [1, 2])[1]
    assert abs((flat_score - A.viterbi_align_page([l0, l1], [1, 2])[1]) - (lp[1, 0] - lp[0, 0])) < 1e-12


def test_space_inside_a_line_is_kept():
    """'a b' (b = space class 3, optional) on one line that shows the space: it is placed, not skipped."""
    records, _, _ = A.viterbi_align_page([line(col(1), col(3), col(2))], [1, 3, 2], [False, True, False])
    assert places(records) == [(0, 0, 0), (0, 1, 1), (0, 2, 2)]


def test_space_absent_at_a_break_is_skipped_from_s4():
    """'a b' over lines 'a' | 'b' with no blank between: b's state is entered from a's, four states back."""
    records, _, line_scores = A.viterbi_align_page([line(col(1)), line(col(2))], [1, 3, 2], [False, True, False])
    assert records == [(1, 0, 0, 0, records[0][4]), (3, -1, -1, -1, 0.0), (2, 1, 0, 0, records[2][4])]
    states, _ = A.viterbi_page_path(A.log_softmax64(line(col(1), col(2))), np.array([False, True]), [1, 3, 2], [False, True, False])
    assert states.tolist() == [1, 5]
    assert line_scores.shape == (2,)


def test_space_absent_at_a_break_is_skipped_from_s3():
    """'a b' over lines 'a', blank | 'b': the trailing blank is the blank BEFORE the skipped space (state 2), b entered three back."""
    lp = A.log_softmax64(line(col(1), col(0), col(2)))
    states, _ = A.viterbi_page_path(lp, np.array([False, False, True]), [1, 3, 2], [False, True, False])
    assert states.tolist() == [1, 2, 5]
    records, _, _ = A.viterbi_align_page([line(col(1), col(0)), line(col(2))], [1, 3, 2], [False, True, False])
    assert places(records) == [(0, 0, 0), (-1, -1, -1), (1, 0, 0)]


def test_equal_class_s4_needs_the_blank_except_at_a_break():
    """'a a' with the space optional.  Inside one line of frames a, a the space cannot be stepped over without a blank (two equal
    emissions would collapse): no fit with two frames.  Over a break the same two frames are two emissions."""
    opt = [False, True, False]
    assert A.viterbi_align_page([line(col(1), col(1))], [1, 3, 1], opt)[0] is None
    records, _, _ = A.viterbi_align_page([line(col(1)), line(col(1))], [1, 3, 1], opt)
    assert places(records) == [(0, 0, 0), (-1, -1, -1), (1, 0, 0)]
    # inside a line, with a blank frame between them, the step is from s - 3
    states, _ = A.viterbi_page_path(A.log_softmax64(line(col(1), col(0), col(1))), np.zeros(3, dtype=bool), [1, 3, 1], opt)
    assert states.tolist() == [1, 2, 5]


def test_ties_go_to_the_earlier_candidate():
    # stay against s - 1: frame 1 favours blank and label alike -> the blank state 0 stays (label 1 begins at frame 1? no: at frame 2)
    lp = A.log_softmax64(line(col(0), both(0, 1), col(1)))
    states, _ = A.viterbi_page_path(lp, np.zeros(3, dtype=bool), [1], [False])
    # delta_1(1) = max(stay delta_0(1), delta_0(0)): delta_0(0) is greater, taken; at t = 2 state 1 is reached from 1 (stay) or from 0:
    # delta_1(1) = lp(0) + lp(1|both) equals delta_1(0) = lp(0) + lp(0|both) bit for bit -> stay
    assert states.tolist() == [0, 1, 1]
    # s - 1 against s - 2: 'ab', frame 0 favours a and blank alike, then b: state 3 at t = 1 from state 2? unreachable at t = 0; from 1
    lp = A.log_softmax64(line(both(1, 0), both(1, 0), col(2)))
    states, _ = A.viterbi_page_path(lp, np.zeros(3, dtype=bool), [1, 2], [False, False])
    # delta_1(2) = delta_0(1) + lp(0) and delta_1(1) = delta_0(1) + lp(1) tie; state 3 at t = 2 tries s - 1 (state 2) first
    assert states.tolist() == [1, 2, 3]
    # s - 2 against s - 3 and s - 3 against s - 4: 'a b' with the space optional, frames a, (space | blank | a alike), b
    three = np.full(4, LO)
    three[[0, 1, 3]] = HI
    lp = A.log_softmax64(line(col(1), three, col(2)))
    states, _ = A.viterbi_page_path(lp, np.zeros(3, dtype=bool), [1, 3, 2], [False, True, False])
    # at t = 1 states 1 (a stays), 2 (blank), 3 (space) tie; state 5 at t = 2 tries s - 1 = 4 (-inf), then s - 2 = 3: kept over 2 and 1
    assert states.tolist() == [1, 3, 5]
    two = np.full(4, LO)
    two[[0, 1]] = HI
    lp = A.log_softmax64(line(col(1), two, col(2)))
    states, _ = A.viterbi_page_path(lp, np.zeros(3, dtype=bool), [1, 3, 2], [False, True, False])
    # now the space state 3 is lower; states 2 and 1 tie: s - 3 is tried before s - 4
    assert states.tolist() == [1, 2, 5]


def test_a_line_that_takes_no_label():
    """Three lines, the middle one blank: it takes no label and its score is its blank sum."""
    mid = line(col(0), col(0))
    records, score, line_scores = A.viterbi_align_page([line(col(1)), mid, line(col(2))], [1, 2])
    assert places(records) == [(0, 0, 0), (2, 0, 0)]
    assert line_scores[1] == A.log_softmax64(mid)[0].sum()
    assert abs(line_scores.sum() - score) < 1e-12


def test_a_line_of_no_frames():
    """A line without frames takes part in nothing: the result is that of the page without it, line indices aside."""
    a, b = line(col(1), col(0)), line(col(2))
    with_empty = A.viterbi_align_page([a, line(), b], [1, 2])
    without = A.viterbi_align_page([a, b], [1, 2])
    assert with_empty[1] == without[1]
    assert places(with_empty[0]) == [(0, 0, 0), (2, 0, 0)] and places(without[0]) == [(0, 0, 0), (1, 0, 0)]
    assert with_empty[2].tolist() == [without[2][0], 0.0, without[2][1]]
    # an empty FIRST line: the first frame of the next line is the start frame, where no step is taken
    lead = A.viterbi_align_page([line(), a, b], [1, 2])
    assert lead[1] == without[1] and places(lead[0]) == [(1, 0, 0), (2, 0, 0)]


def test_no_labels_and_no_fit():
    outs = [line(col(1), col(0)), line(), line(col(2))]
    records, score, line_scores = A.viterbi_align_page(outs, [])
    lp = [A.log_softmax64(o) for o in outs]
    assert records == [] and line_scores.tolist() == [lp[0][0].sum(), 0.0, lp[2][0].sum()]
    assert score == A.viterbi_path(np.concatenate(lp, axis=1), [])[1]
    assert A.viterbi_align_page(outs, [1, 2, 3, 1]) == (None, NEG, None)
    assert A.viterbi_align_page([line(), line()], [1]) == (None, NEG, None)
    records, score, line_scores = A.viterbi_align_page([line(), line()], [])
    assert records == [] and score == 0.0 and line_scores.tolist() == [0.0, 0.0]


def test_arguments():
    out = [line(col(1), col(2), col(3))]
    for optional in ([True, False, False], [False, False, True], [False, True, True, False], [False, True]):
        with pytest.raises(ValueError):
            A.viterbi_align_page(out, [1, 2, 3, 1][:max(len(optional), 3)], optional)
    with pytest.raises(ValueError):
        A.viterbi_align_page(out, [4])
    with pytest.raises(ValueError):
        A.viterbi_align_page(out, [0])


def test_optional_labels_of_a_text():
    """The optional labels are the single whitespace characters, never the first or last label nor the second of two in a row (the
    kernel's rule), whatever normalisation left in the text."""
    from conformer_ocr_amd.codec import PytorchCodec
    codec = PytorchCodec([' ', 'a', 'b'])
    labels, skipped = A.encode_text(codec, ' ab  a b ?')
    assert skipped == '?' and ''.join(codec.l2c[(l,)] for l in labels) == ' ab  a b '
    opt = A.optional_labels(codec, labels)
    assert opt.tolist() == [False, False, False, True, False, False, True, False, False]
    A.check_optional(opt, len(labels))
    # with them the text fits three frames per word although no space is shown
    sp, a, b = (codec.c2l[c][0] for c in ' ab')
    labels, _ = A.encode_text(codec, 'ab a')
    outs = [line(col(a), col(b)), line(col(a))]
    records, _, _ = A.viterbi_align_page(outs, labels, A.optional_labels(codec, labels))
    assert places(records) == [(0, 0, 0), (0, 1, 1), (-1, -1, -1), (1, 0, 0)]


def test_page_table_words_follow_the_kernel_form():
    """One page's workspace region: back-pointer blocks of 8 frames x (64 lanes x registers x waves) words, lz, states, two run tables."""
    assert A.page_table_words(37, 20, 20) == (5 * 64 + 2 * 37 + 2 * 20 + 3) // 4 * 4                 # S = 41: one register, one wave
    assert A.page_table_words(2400, 600, 600) == 300 * 64 * 2 * 10 + 2 * 2400 + 2 * 600              # S = 1201: 2 registers x 10 waves
    assert A.page_table_words(12000, 2000, 4095) == 1500 * 8192 + 2 * 12000 + 2 * 2000               # the call's longest text sets the form


def test_page_result_sorts_records_onto_lines_and_reports_dropped_spaces():
    """The Python page layer behind the aligner: 'ab a' on lines 'ab' | 'a' -- the space is optional, not shown, and comes back as
    `dropped`; every line gets its characters, cuts and words."""
    from conformer_ocr_amd.codec import PytorchCodec
    from conformer_ocr_amd.page import line_geometry
    codec = PytorchCodec([' ', 'a', 'b'])
    sp, a, b = (codec.c2l[c][0] for c in ' ab')
    labels, skipped = A.encode_text(codec, 'ab a?')
    outs = [line(col(a), col(b)), line(col(0), col(a))]
    aligned = A.viterbi_align_page(outs, labels, A.optional_labels(codec, labels))
    geoms = [line_geometry(f'l{k}', [(10, 20 + 40 * k), (110, 20 + 40 * k)], [(10, 5 + 40 * k), (110, 5 + 40 * k), (110, 30 + 40 * k), (10, 30 + 40 * k)])
             for k in range(2)]
    res = A.page_result(codec, geoms, aligned, [2, 2], [100, 100], 0, skipped)
    assert res['dropped'] == ' ' and res['skipped'] == '?' and res['score'] == aligned[1]
    assert [(ln['id'], ln['text'], ln['frames']) for ln in res['lines']] == [('l0', 'ab', 2), ('l1', 'a', 2)]
    assert [w[0] for ln in res['lines'] for w in ln['words']] == ['ab', 'a']
    assert [len(ln['cuts']) for ln in res['lines']] == [2, 1] and [ln['score'] for ln in res['lines']] == aligned[2].tolist()
    none = A.page_result(codec, geoms, (None, NEG, None), [2, 2], [100, 100], 0, '')
    assert none == {'lines': None, 'score': NEG, 'skipped': '', 'dropped': ''}
    assert A.gt_file_id('r1/l:2 a') == 'r1_l_2_a'
