"""CPU: the definition of keyword spotting, `search.spot_host`, and the search command's usage errors."""
import itertools

import numpy as np
import pytest

from conformer_ocr_amd import search as S

NEG = -np.inf


def _brute(x, lab):
    """e_t by enumeration: the best sum of r over every window [a, t] and every legal state path from state 0 to state S - 1.  x (C, T)."""
    C, T = x.shape
    L = len(lab)
    n_states = 2 * L - 1
    r = x.astype(np.float64) - x.astype(np.float64).max(axis=0, keepdims=True)
    cls = [lab[s // 2] if s % 2 == 0 else 0 for s in range(n_states)]
    e = np.full(T, NEG)
    for a in range(T):
        for b in range(a, T):
            for p in itertools.product(range(n_states), repeat=b - a + 1):
                if p[0] != 0 or p[-1] != n_states - 1:
                    continue
                ok = True
                for i in range(1, len(p)):
                    d = p[i] - p[i - 1]
                    if d in (0, 1) or (d == 2 and p[i] % 2 == 0 and lab[p[i] // 2] != lab[p[i] // 2 - 1]):
                        continue
                    ok = False
                    break
                if ok:
                    e[b] = max(e[b], sum(r[cls[s], a + i] for i, s in enumerate(p)))
    return e


def test_candidates_equal_the_brute_force_maximum():
    rng = np.random.default_rng(0)
    reached = 0
    for _ in range(150):
        T, C, L = int(rng.integers(1, 7)), 4, int(rng.integers(1, 4))
        lab = [int(v) for v in rng.integers(1, C, L)]
        x = rng.integers(-16, 17, (C, T)) / 8.0
        e, st = S.spot_candidates(x, lab)
        assert np.array_equal(e, _brute(x, lab)), (x, lab)
        assert ((st >= 0) == (e > NEG)).all() and (st <= np.arange(T)).all()
        reached += int((e > NEG).sum())
    assert reached > 300


def _logits(T, C, frames):
    """-4 everywhere, 0 at the (frame, class) pairs given: those classes are the frame-wise argmax."""
    x = np.full((C, T), -4.0)
    for t, c in frames:
        x[c, t] = 0.0
    return x


def test_stay_beats_a_fresh_start_across_an_argmax_run():
    # label 1 is the argmax on frames 2..4: delta(0) = 0 there, and 0 > 0 is false, so the start stays at frame 2
    x = _logits(7, 3, [(0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 0), (6, 0)])
    e, st = S.spot_candidates(x, [1])
    assert e.tolist() == [-4.0, -4.0, 0.0, 0.0, 0.0, -4.0, -4.0]
    # frame 5 still continues the run (delta_4(0) = 0 is not beaten by a fresh start); frame 6 starts afresh, as frames 0 and 1 do
    assert st.tolist() == [0, 1, 2, 2, 2, 2, 6]
    assert S.spot_host(x, [1], 1) == [(2, 4, 0.0)]


def test_the_end_tie_goes_to_the_last_frame_of_the_last_labels_run():
    # 'ab': a on 1..2, b on 3..5; e = 0 at frames 3, 4 and 5, all with start 1: the hit takes the whole run
    x = _logits(8, 4, [(0, 0), (1, 1), (2, 1), (3, 2), (4, 2), (5, 2), (6, 0), (7, 0)])
    e, st = S.spot_candidates(x, [1, 2])
    assert e[3:6].tolist() == [0.0, 0.0, 0.0] and st[3:6].tolist() == [1, 1, 1]
    assert S.spot_host(x, [1, 2], 3)[0] == (1, 5, 0.0)


def test_a_repeated_label_needs_its_blank():
    # 'aa' on frames a a a: the middle frame must be the blank (-4); on a - a with a blank between it scores 0
    x = _logits(3, 3, [(0, 1), (1, 1), (2, 1)])
    assert S.spot_host(x, [1, 1], 1) == [(0, 2, -4.0)]
    assert S.spot_host(x[:, :2], [1, 1], 1) == []                   # two frames cannot hold a, blank, a
    x = _logits(5, 3, [(0, 1), (1, 1), (2, 0), (3, 1), (4, 1)])
    assert S.spot_host(x, [1, 1], 1) == [(0, 4, 0.0)]
    assert S.spot_host(x, [1, 2], 1)[0][2] < 0.0                    # different labels skip the blank, but 2 is nowhere the argmax


def _planted(rng, T, C, L, copies=3, grid=True):
    lab = [int(v) for v in rng.integers(1, C, L)]
    x = (rng.integers(-64, 65, (C, T)) / 8.0) if grid else rng.standard_normal((C, T)) * 2
    x = x.astype(np.float32)
    for pos in rng.choice(np.arange(0, T - 3 * L, 3 * L + 2), size=copies, replace=False):
        for k, l in enumerate(lab):
            x[l, pos + 3 * k:pos + 3 * k + 2] = 9.0
            x[0, pos + 3 * k + 2] = 9.0
    return x, lab


def test_selection_properties():
    rng = np.random.default_rng(3)
    for _ in range(20):
        L = int(rng.integers(1, 6))
        x, lab = _planted(rng, 120, 12, L)
        hits = S.spot_host(x, lab, 8)
        assert 3 <= len(hits) <= 8
        assert [h[2] for h in hits[:3]] == [0.0, 0.0, 0.0]
        assert all(a[2] >= b[2] for a, b in zip(hits, hits[1:]))
        spans = sorted((h[0], h[1]) for h in hits)
        assert all(0 <= s <= e < 120 for s, e in spans)
        assert all(a[1] < b[0] for a, b in zip(spans, spans[1:]))
        assert S.spot_host(x, lab, 1) == hits[:1]
        cut = S.spot_host(x, lab, 8, min_score=-0.5)
        assert cut == [h for h in hits if h[2] >= -0.5] and len(cut) >= 3
        assert S.spot_host(x, lab, 8, min_score=0.125) == []


def test_float32_recursion_is_exact_on_grid_logits():
    """Logits on the 1/8 grid in [-8, 8] (planted spots 9.0): every r and every partial sum is a multiple of 1/8 below 2^24 / 8 in
    magnitude, so the float32 recursion gives the float64 candidates bit for bit."""
    rng = np.random.default_rng(5)
    for _ in range(12):
        L = int(rng.integers(1, 20))
        x, lab = _planted(rng, 300, 64, L, copies=2)
        e64, s64 = S.spot_candidates(x, lab)
        e32, s32 = S.spot_candidates(x, lab, dtype=np.float32)
        assert e32.dtype == np.float32
        assert np.array_equal(e64, e32.astype(np.float64)) and np.array_equal(s64, s32)
        assert S.spot_host(x, lab, 4) == S.spot_host(x, lab, 4, dtype=np.float32)


def test_errors_and_short_lines():
    x = _logits(4, 3, [(0, 1), (1, 2), (2, 1), (3, 2)])
    with pytest.raises(ValueError):
        S.spot_host(x, [], 1)
    with pytest.raises(ValueError):
        S.spot_host(x, [3], 1)
    with pytest.raises(ValueError):
        S.spot_host(x, [0], 1)
    assert S.spot_host(x, [1, 2, 1, 2, 1], 2) == []                  # five labels in four frames
    assert S.spot_host(x[:, :0], [1], 2) == []
    assert S.spot_host(x, [1, 2, 1, 2], 2) == [(0, 3, 0.0)]


def test_parser_usage_errors(tmp_path, capsys):
    xml = tmp_path / 'a.xml'
    xml.write_text('<PcGts/>')
    model = tmp_path / 'model.tar'
    model.write_bytes(b'')
    out = str(tmp_path / 'out.json')
    assert S.main(['-q', 'word', '-i', str(xml), out]) == 1
    assert 'No model given' in capsys.readouterr().err
    assert S.main(['-m', str(model), '-i', str(xml), out]) == 1
    assert 'No query given' in capsys.readouterr().err
    assert S.main(['-m', str(model), '-q', '   ', '-i', str(xml), out]) == 1           # nothing is left of the query
    assert 'No query given' in capsys.readouterr().err
    assert S.main(['-m', str(model), '-q', 'word']) == 1
    assert 'No input given' in capsys.readouterr().err
    assert S.main(['-m', str(model), '-q', 'word', '-i', str(xml)]) == 1               # inputs but no output file
    assert 'No input given' in capsys.readouterr().err
    assert S.main(['-m', str(model), '-q', 'word', '--hits', '9', '-i', str(xml), out]) == 1
    assert '--hits' in capsys.readouterr().err
    assert S.main(['-m', str(tmp_path / 'none.tar'), '-q', 'word', '-i', str(xml), out]) == 1
    assert 'no such file' in capsys.readouterr().err
    args = S.parser().parse_args(['-m', 'm', '-q', 'a', '-q', 'b', '-i', 'x.xml', 'y.xml', 'o.json'])
    assert args.query == ['a', 'b'] and args.input == ['x.xml', 'y.xml', 'o.json'] and args.output is None and args.min_conf is None
    assert S.parser().parse_args(['-i', 'x.xml', '--hits', '2', 'o.json']).output == 'o.json'
