"""CPU: the pattern compiler and the definition of pattern spotting, `pattern.spot_pattern_host`."""
import itertools
import re

import numpy as np
import pytest

from conformer_ocr_amd import pattern as PT
from conformer_ocr_amd import search as S
from conformer_ocr_amd.codec import PytorchCodec, ascii_codec

NEG = -np.inf
ABCD = PytorchCodec('abcd')          # a..d = labels 1..4
ABC = PytorchCodec('abc')            # C = 4 with the blank

RE_PATTERNS = ['abc', 'a|b', 'ab|cd', '(a|b)c?a', 'a+b', '(ab)+', '[ab][ab]', 'ab?c', '(ab|ba)+', 'a*b', 'a{2}', 'a{1,3}b', '[a-c]d',
               '[^a]b', '.a', 'a.?b', '(a|bc)*d', '\\wd', 'a(b|c){2,}', '(a?b)+', 'a{0,2}b', '((a|b)(c|d))+', 'a\\|?b', '[a-bd]+c']


def _strings(alphabet, longest):
    for n in range(1, longest + 1):
        for w in itertools.product(alphabet, repeat=n):
            yield ''.join(w)


@pytest.mark.parametrize('text', RE_PATTERNS)
def test_graph_accepts_what_re_fullmatch_accepts(text):
    codec = PytorchCodec('abcd|') if '\\|' in text else ABCD
    g = PT.compile_pattern(text, codec)
    assert not g.skipped and 1 <= g.P <= PT.MAX_STATES
    for q, ps in enumerate(g.preds):
        assert ps == sorted(set(ps)) and all(0 <= p < g.P for p in ps)
    rx = re.compile(text)
    accepted = 0
    for w in _strings(sorted(codec.c2l), 5):
        want = rx.fullmatch(w) is not None
        assert g.accepts(codec.encode(w)) == want, (text, w)
        accepted += want
    assert accepted > 0
    assert not g.accepts([])


def test_a_literal_is_a_chain_numbered_in_text_order():
    g = PT.compile_pattern('dacb', ABCD)
    assert g.is_chain and g.labels == [4, 1, 3, 2] and g.preds == [[], [0], [1], [2]]
    assert g.first.tolist() == [True, False, False, False] and g.last.tolist() == [False, False, False, True]
    assert not PT.compile_pattern('da?cb', ABCD).is_chain and not PT.compile_pattern('a+', ABCD).is_chain
    g = PT.compile_pattern('a(b|c)d', ABCD)                   # states in order of occurrence
    assert g.cls.tolist() == [1, 2, 3, 4] and g.preds == [[], [0], [0], [1, 2]]
    g = PT.compile_pattern('a+', ABCD)
    assert g.preds == [[0]]                                   # a state may precede itself


def test_multi_label_graphemes_are_encoded_like_queries():
    codec = PytorchCodec({'a': [1], 'b': [2, 3], 'ch': [4]})
    g = PT.compile_pattern('achb', codec)
    assert g.is_chain and g.labels == codec.encode('achb') == [1, 4, 2, 3]
    with pytest.raises(ValueError, match='exactly one'):
        PT.compile_pattern('[ab]', codec)
    assert PT.compile_pattern('.', codec).cls.tolist() == [1]            # single code points of exactly one label


@pytest.mark.parametrize('text', ['a*', 'a?', '(a|)', '', 'a?b?', '(a*)+', 'a{0}'])
def test_nullable_patterns_are_refused(text):
    with pytest.raises(ValueError, match='empty string'):
        PT.compile_pattern(text, ABCD)


@pytest.mark.parametrize('text', ['^a', 'a$', 'a\\b', '(a)\\1', '(?=a)b', 'a+?', '(a', 'a)', '[a', 'a{2,1}', '*a', '[b-a]'])
def test_what_is_not_built_and_syntax_errors_are_refused(text):
    with pytest.raises(ValueError):
        PT.compile_pattern(text, ABCD)


def test_the_state_and_edge_limits():
    codec = ascii_codec(128)
    assert PT.compile_pattern('a{256}', codec).P == 256
    with pytest.raises(ValueError, match='256'):
        PT.compile_pattern('a{257}', codec)
    with pytest.raises(ValueError, match='256'):
        PT.compile_pattern('[a-c]{100}', codec)
    with pytest.raises(ValueError, match='4096'):
        PT.compile_pattern('..', codec)                         # 127 x 127 edges
    g = PT.compile_pattern('[a-j]{13}', codec)
    assert g.P == 130 and g.edges == 1200 and max(len(p) for p in g.preds) == 10
    g = PT.compile_pattern('.{2}', PytorchCodec('abcdefgh'))
    assert g.P == 16 and g.edges == 64


def test_ignore_case_and_the_shorthands_on_the_ascii_codec():
    codec = ascii_codec(128)
    g = PT.compile_pattern('anno', codec, ignore_case=True)
    assert g.P == 8 and not g.is_chain
    for w in ('anno', 'Anno', 'ANNO', 'aNnO'):
        assert g.accepts(codec.encode(w)), w
    for w in ('onna', 'ann', 'annoo'):
        assert not g.accepts(codec.encode(w)), w
    assert not PT.compile_pattern('anno', codec).accepts(codec.encode('Anno'))
    assert PT.compile_pattern('a1', codec, ignore_case=True).P == 3              # '1' has no other case
    singles = PT.single_label_chars(codec)
    for sh, test in (('\\d', str.isdigit), ('\\w', lambda c: c.isalnum() or c == '_'), ('\\s', str.isspace)):
        want = sorted(codec.c2l[c][0] for c in singles if test(c))
        if not want:
            with pytest.raises(ValueError):
                PT.compile_pattern(sh, codec)
            continue
        assert sorted(PT.compile_pattern(sh, codec).cls.tolist()) == want
    year = PT.compile_pattern('1[5-7][0-9][0-9]', codec)
    assert year.P == 24 and year.accepts(codec.encode('1648')) and not year.accepts(codec.encode('1848'))
    assert PT.compile_pattern('[^a]', PytorchCodec('abc')).cls.tolist() == [2, 3]
    assert len(PT.compile_pattern('.', codec).cls) == 127


def test_characters_the_codec_lacks_are_reported_as_skipped():
    g = PT.compile_pattern('aéb', ABCD)
    assert g.skipped == 'é' and g.P == 0
    assert PT.compile_pattern('a[bx]', ABCD).skipped == 'x'
    assert PT.compile_pattern('Xy', ABCD, ignore_case=True).skipped == 'Xy'
    assert PT.compile_pattern('[a-z]', ABCD).skipped == ''                        # a range is restricted to the codec


def _grid(rng, C, T):
    return rng.integers(-16, 17, (C, T)) / 8.0


def test_p1_a_literal_is_spot_candidates_bit_for_bit():
    rng = np.random.default_rng(1)
    reached = 0
    for i in range(300):
        C, T, L = int(rng.integers(2, 8)), int(rng.integers(1, 25)), int(rng.integers(1, 7))
        lab = [int(v) for v in rng.integers(1, C, L)]
        x = _grid(rng, C, T) if i % 2 else rng.standard_normal((C, T)) * 3
        g = PT.chain_graph(lab)
        assert g.is_chain
        for dt in (np.float32, np.float64):
            e, st, fin = PT.pattern_candidates(x, g, dt)
            e0, st0 = S.spot_candidates(x, lab, dt)
            assert e.dtype == e0.dtype and e.tobytes() == e0.tobytes() and np.array_equal(st, st0), (x, lab)
            assert np.array_equal(fin, np.where(e > NEG, L - 1, -1))
            assert PT.spot_pattern_host(x, g, 3, dtype=dt) == [h + (L - 1,) for h in S.spot_host(x, lab, 3, dtype=dt)]
        reached += int((e > NEG).sum())
    assert reached > 1000


@pytest.mark.parametrize('text', ['(a|b)c?a', 'a+b', '(ab)+', '[ab][ab]', 'ab?c', '(ab|ba)+'])
def test_p2_candidates_are_the_maximum_over_the_language(text):
    rng = np.random.default_rng(2)
    g = PT.compile_pattern(text, ABC)
    rx = re.compile(text)
    language = [ABC.encode(w) for w in _strings('abc', 6) if rx.fullmatch(w)]
    assert language
    reached = 0
    for _ in range(40):
        T = int(rng.integers(1, 7))
        x = _grid(rng, 4, T)
        e, st, fin = PT.pattern_candidates(x, g)
        want = np.full(T, NEG)
        for w in language:
            if len(w) <= T:
                want = np.maximum(want, S.spot_candidates(x, w)[0])
        assert np.array_equal(e, want), (text, x)
        assert ((st >= 0) == (e > NEG)).all() and ((fin >= 0) == (e > NEG)).all() and g.last[fin[fin >= 0]].all()
        reached += int((e > NEG).sum())
    assert reached > 40


@pytest.mark.parametrize('text', ['(a|b)c?a', 'a+b', '(ab)+', '[ab][ab]', 'ab?c', '(ab|ba)+', 'a+'])
def test_match_host_returns_a_string_of_the_language_with_the_hits_score(text):
    rng = np.random.default_rng(3)
    g = PT.compile_pattern(text, ABC)
    rx = re.compile(text)
    seen = 0
    for _ in range(40):
        T = int(rng.integers(2, 13))
        x = _grid(rng, 4, T)
        for start, end, score, final in PT.spot_pattern_host(x, g, 3):
            labels, best = PT.match_host(x, g, start, end, final, with_score=True)
            assert rx.fullmatch(''.join('abc'[l - 1] for l in labels)) and g.accepts(labels)
            assert best == score                                         # exact on the grid
            e, st = S.spot_candidates(x, labels)
            assert e[end] == score and st[end] == start, (text, x, labels)
            seen += 1
    assert seen > 40


@pytest.mark.parametrize('text', ['(a|b)c?a', 'a+b', '(ab|ba)+', '[a-c]{3}', 'a[bc]+a'])
def test_float32_equals_float64_bit_for_bit_on_grid_logits(text):
    rng = np.random.default_rng(4)
    g = PT.compile_pattern(text, ABC)
    for _ in range(20):
        x = _grid(rng, 4, int(rng.integers(1, 40)))
        e32, st32, f32 = PT.pattern_candidates(x, g, np.float32)
        e64, st64, f64 = PT.pattern_candidates(x, g, np.float64)
        assert e32.dtype == np.float32 and np.array_equal(e32.astype(np.float64), e64) and np.array_equal(st32, st64) and np.array_equal(f32, f64)
        assert PT.spot_pattern_host(x, g, 4, dtype=np.float32) == PT.spot_pattern_host(x, g, 4)


def _logits(T, C, frames):
    """-4 everywhere, 0 at the (frame, class) pairs given: those classes are the frame-wise argmax."""
    x = np.full((C, T), -4.0)
    for t, c in frames:
        x[c, t] = 0.0
    return x


def test_a_predecessor_of_equal_score_beats_the_fresh_start():
    # 'a?b': b is a first state and follows a.  a is the argmax at frame 0, b at frame 1: from a the score is 0, and the fresh start's
    # 0 > 0 is false, so the match begins at frame 0
    g = PT.compile_pattern('a?b', ABC)
    assert g.first.tolist() == [True, True] and g.preds == [[], [0]]
    e, st, fin = PT.pattern_candidates(_logits(2, 4, [(0, 1), (1, 2)]), g)
    assert e.tolist() == [-4.0, 0.0] and st.tolist() == [0, 0] and fin.tolist() == [1, 1]
    # without the a the fresh start is the only way in
    e, st, fin = PT.pattern_candidates(_logits(2, 4, [(0, 3), (1, 2)]), g)
    assert e.tolist() == [-4.0, 0.0] and st.tolist() == [0, 1]


def test_of_two_last_states_of_equal_score_the_lowest_wins():
    g = PT.compile_pattern('ab?', ABC)
    assert g.last.tolist() == [True, True]
    x = _logits(2, 4, [(0, 1), (1, 1), (1, 2)])              # frame 1: a and b are both the maximum
    e, st, fin = PT.pattern_candidates(x, g)
    assert e.tolist() == [0.0, 0.0] and st.tolist() == [0, 0] and fin.tolist() == [0, 0]
    x[1, 1] = -1.0                                            # now b is better: the higher state wins on score
    assert PT.pattern_candidates(x, g)[2].tolist() == [0, 1]
    g = PT.compile_pattern('a|a', ABC)
    assert PT.pattern_candidates(_logits(1, 4, [(0, 1)]), g)[2].tolist() == [0]


def test_a_plus_needs_its_blank_between_two_a():
    g = PT.compile_pattern('a+', ABC)
    x = _logits(3, 4, [(0, 1), (1, 1), (2, 1)])              # a a a: one a, held
    assert PT.spot_pattern_host(x, g, 1) == [(0, 2, 0.0, 0)]
    assert PT.match_host(x, g, 0, 2, 0) == [1]
    x = _logits(3, 4, [(0, 1), (1, 0), (2, 1)])              # a blank a: two
    assert PT.spot_pattern_host(x, g, 1) == [(0, 2, 0.0, 0)]
    assert PT.match_host(x, g, 0, 2, 0) == [1, 1]
    g = PT.compile_pattern('aa', ABC)                         # and 'aa' does not fit a a a without paying for a blank
    assert PT.pattern_candidates(_logits(3, 4, [(0, 1), (1, 1), (2, 1)]), g)[0].tolist() == [NEG, NEG, -4.0]


def test_selection_min_score_and_overlap():
    g = PT.compile_pattern('a[bc]', ABC)
    x = _logits(7, 4, [(0, 1), (1, 2), (2, 0), (3, 1), (4, 0), (5, 0), (6, 0)])
    x[3, 4] = -0.5                                            # frame 4: the blank is the maximum, c half a unit below
    hits = PT.spot_pattern_host(x, g, 8)
    assert hits[:2] == [(0, 1, 0.0, 1), (3, 4, -0.5, 2)]
    assert PT.spot_pattern_host(x, g, 8, min_score=-0.25) == hits[:1]
    assert PT.spot_pattern_host(x, g, 1) == hits[:1]
    assert PT.labels_text(ABC, PT.match_host(x, g, 0, 1, 1)) == 'ab'
    with pytest.raises(ValueError):
        PT.pattern_candidates(np.zeros((2, 3)), g)               # class 2 / 3 outside the logits


def test_search_index_with_patterns_on_the_host(tmp_path, capsys):
    import json
    import math
    from conformer_ocr_amd import index as I
    from tests.test_index_host import C_FILE, STEP, _corpus
    path, logits, queries = _corpus(tmp_path)
    idx = I.load_index(path)
    codec = idx.codec()
    ch = lambda c: PT.escape(c)
    # the three planted words: one with its middle position widened to a set, one with an optional extra, one as it is (a chain)
    q0, q1, q2 = queries
    other = next(c for c in PT.single_label_chars(codec) if c not in q0)
    texts = [f'{ch(q0[0])}[{ch(other)}{ch(q0[1])}]{ch(q0[2])}', f'{ch(q1[0])}{ch(other)}?{ch(q1[1])}', PT.escape(q2)]
    graphs = [PT.compile_pattern(t, codec) for t in texts]
    assert [g.is_chain for g in graphs] == [False, False, True]
    found = I.search_index(path, patterns=texts, hits=4, device='cpu')
    assert found == I.search_index(idx, patterns=graphs, hits=4, device='cpu')
    assert all(set(h) == {'page', 'line', 'pattern', 'match', 'start', 'end', 'score', 'conf', 'quad'} for h in found)
    zero = 0
    for i, x in enumerate(logits):
        if not x.shape[0]:
            continue
        table = I.expand_host(*idx.line(i), C_FILE, STEP)
        for t, g in zip(texts, graphs):
            mine = [h for h in found if h['line'] == f'l{i}' and h['pattern'] == t]
            want = PT.spot_pattern_host(table, g, 4, dtype=np.float32)
            assert [(h['start'], h['end'], h['score']) for h in mine] == [w[:3] for w in want]
            for h, w in zip(mine, want):
                labels = PT.match_host(table, g, *w[:2], w[3])
                assert h['match'] == PT.labels_text(codec, labels) and g.accepts(labels)
                assert h['conf'] == math.exp(h['score'] / len(labels))
                zero += h['score'] == 0.0
    assert zero >= 8
    # a chain is what the query string is; strings beside patterns are what they are alone
    plain = I.search_index(idx, [q2], hits=4, device='cpu')
    assert [(h['line'], h['start'], h['end'], h['score'], h['conf'], h['quad'], h['match']) for h in found if h['pattern'] == texts[2]] == \
        [(h['line'], h['start'], h['end'], h['score'], h['conf'], h['quad'], q2) for h in plain]
    both = I.search_index(idx, [q2], patterns=texts[:1], hits=4, device='cpu')
    assert [h for h in both if 'query' in h] == plain and [h for h in both if 'pattern' in h] == [h for h in found if h['pattern'] == texts[0]]
    kept = I.search_index(idx, patterns=texts, hits=4, min_conf=0.5, device='cpu')
    assert kept == [h for h in found if h['conf'] >= 0.5] and 0 < len(kept) < len(found)
    for bad in (['☃'], ['a*'], ['(']):
        with pytest.raises(ValueError):
            I.search_index(idx, patterns=bad, device='cpu')
    # the command
    (tmp_path / 'patterns.txt').write_text(texts[1] + '\n☃+\n', encoding='utf-8')
    capsys.readouterr()
    out = tmp_path / 'hits.json'
    assert I.main(['search', '--index', str(path), '-e', texts[0], '-e', '(', '-E', str(tmp_path / 'patterns.txt'), '-q', q2, '--ignore-case', '--hits', '4',
                   '-d', 'cpu', str(out)]) == 0
    err = capsys.readouterr().err
    assert err.count('skipped') == 2 and 'of 3 queries' in err
    back = json.loads(out.read_text(encoding='utf-8'))
    want = [h for h in found if h['pattern'] == texts[2]] + [h for h in found if h['pattern'] in texts[:2]]
    key = lambda h: (h['line'], h['pattern'].replace('\\', ''), h['start'], h['end'], h['score'], h['match'])
    assert sorted(key(h) for h in back) == sorted(key(h) for h in want) and len(back) > 0
    assert I.main(['search', '--index', str(path), '-e', 'a*', '-d', 'cpu', str(out)]) == 1
    assert 'codec can encode' in capsys.readouterr().err


def test_the_search_command_takes_patterns_in_place_of_queries(capsys):
    args = S.parser().parse_args(['-e', 'a+', '-e', 'b', '-E', 'f.txt', '--ignore-case', '-i', 'x.xml', 'o.json'])
    assert args.pattern == ['a+', 'b'] and args.pattern_file == 'f.txt' and args.ignore_case and args.query == []
    assert S.main(['-m', 'nowhere.tar', '-e', 'a+', '-E', 'nowhere.txt', '-i', 'x.xml', 'o.json']) == 1
    assert 'nowhere.txt' in capsys.readouterr().err
    assert PT.escape('a.b-c') == 'a\\.b\\-c' and PT.compile_pattern(PT.escape('(a|b)'), PytorchCodec('ab()|')).is_chain
