"""GPU: pattern spotting (cocr_ctc_spot_pattern) against keyword spotting on chains and against the definition
`pattern.spot_pattern_host`.

Exact where the arithmetic is exact (tests/test_hip_search.py): on logits that are multiples of 1/8 in [-8, 8] (planted spots 9.0)
every partial sum is a multiple of 1/8 of magnitude <= 17 T, exactly representable in float32 while 17 * 8 * T < 2^24, so the device
must give the definition's counts, starts, ends, scores and final states bit for bit, ties included (and the float32 definition equals
the float64 one there: tests/test_pattern_host.py).  A chain does the additions of `cocr_ctc_spot` in the same order, so it must give
that kernel's raw outputs on real-valued logits too.  On real-valued logits a real pattern's score is held to section 7i's bound
    tol = 8 T 2^-23 max(1, |s*|)."""
import json

import numpy as np
import pytest
import torch

from conformer_ocr_amd import index as I
from conformer_ocr_amd import pattern as PT
from conformer_ocr_amd import search as S
from conformer_ocr_amd.codec import PytorchCodec, ascii_codec
from conformer_ocr_amd.page import Line, recognize_pages
from conformer_ocr_amd.pred import PytorchRecognitionModel, save_safetensors
from tests import page_synth
from tests.test_hip_search import DROPS, FIXTURE_FORM, KINDS, PICK, _grid_case, _net, _plant, _planted_lines, _tol

pytestmark = pytest.mark.gpu
NEG = -np.inf


def _engine():
    from conformer_ocr_amd.ctc_decoder import _scratch_engine
    return _scratch_engine(torch.device('cuda', 0))


def _dev(logits):
    return torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).cuda()


def _raw(logits, out_lens, graphs, hits=1, min_score=NEG):
    """(starts, ends, scores, finals (N,Q,K), counts (N,Q)) of cocr_ctc_spot_pattern."""
    eng = _engine()
    return eng.collect_spot_pattern(eng.ctc_spot_pattern_async(_dev(logits), out_lens, graphs, hits, min_score), raw=True)


def _run(logits, out_lens, graphs, hits=1, min_score=NEG):
    return _engine().ctc_spot_pattern(_dev(logits), out_lens, graphs, hits, min_score)


def _want(logits, out_lens, graphs, hits=1, min_score=NEG):
    return [[PT.spot_pattern_host(logits[n, :int(out_lens[n])].T, g, hits, min_score, dtype=np.float32) for g in graphs]
            for n in range(logits.shape[0])]


def _letters(C):
    """label i = the i-th character from 'a' on."""
    return PytorchCodec({chr(0x61 + i): [i + 1] for i in range(C - 1)})


# ---- 1. chains: the graph kernel gives cocr_ctc_spot's raw outputs ---------------------------------------------------------------------
@pytest.mark.parametrize('N,T,C,lens_q,K,out_lens,width', [
    (3, 37, 5, [2, 3, 2, 1, 4], 3, [37, 0, 30], 2),                               # SJ 1; Q = 5 is no multiple of 4; a line without frames
    (4, 300, 64, [7, 12, 8, 40, 1, 3, 25, 5, 9], 4, [300, 0, 251, 64], 2),        # Q 9, chains of up to 40 labels
    (2, 600, 40, [3, 6, 200, 2, 4, 1], 8, [600, 555], 1),                        # SJ 4: the 200-label chain (planted in line 1) crosses the seams 63/64, 127/128, 191/192
])
def test_literal_chains_equal_the_string_kernel(N, T, C, lens_q, K, out_lens, width):
    grid, queries = _grid_case(N, T, C, lens_q, 100 + T, out_lens, width)
    real = grid + np.random.default_rng(T).standard_normal(grid.shape).astype(np.float32)
    graphs = [PT.chain_graph(q) for q in queries]
    eng = _engine()
    Q = len(queries)
    planted_long = None
    for logits in (grid, real):
        h = eng.ctc_spot_async(_dev(logits), out_lens, queries, K)
        eng.collect_spot(h)
        st0, en0 = h[1][0].numpy()[:, :N * Q * K].reshape(2, N, Q, K).copy()
        sc0 = h[1][1].numpy()[:N * Q * K].reshape(N, Q, K).copy()
        cnt0 = h[1][2].numpy()[:N * Q].reshape(N, Q).copy()
        st, en, sc, fin, cnt = _raw(logits, out_lens, graphs, K)
        assert np.array_equal(cnt, cnt0) and np.array_equal(st, st0) and np.array_equal(en, en0)
        assert sc.tobytes() == sc0.tobytes()
        want_fin = np.where(st0 >= 0, np.asarray([len(q) - 1 for q in queries])[None, :, None], -1)
        assert np.array_equal(fin, want_fin)
        assert cnt0.sum() > N
        if planted_long is None:
            planted_long = (float(sc0[1, 2, 0]), int(en0[1, 2, 0] - st0[1, 2, 0]))
    if 200 in lens_q:
        assert planted_long == (0.0, 2 * 200 - 2)              # the long chain where it was planted, on the grid


# ---- 2. grid logits: the definition, exactly ---------------------------------------------------------------------------------------------
PATTERNS = ['a[bc]d', '(ab|cd)e', 'ab?c', 'a+b', '(ab)+', '[a-e]{3}', '[a-j]{13}']
# strings of the languages, planted in turn; the first one, 13 letters for '[a-j]{13}', holds a match of every other pattern too
PLANTS = ['acdeabcabjihg', 'acd', 'cde', 'abc', 'aab', 'abab', 'eca', 'ac']


def _pattern_case(N, T, C, out_lens, seed, width):
    rng = np.random.default_rng(seed)
    codec = _letters(C)
    logits = (rng.integers(-64, 65, (N, T, C)) / 8.0).astype(np.float32)
    for n in range(N):
        at = int(rng.integers(0, 3))
        for k, w in enumerate(PLANTS):
            span = (width + 1) * len(w)
            if (k + n) % 3 != 1 and at + span <= out_lens[n]:
                _plant(logits[n], codec.encode(w), at, width)
                at += span + int(rng.integers(0, 3))
    return logits, [PT.compile_pattern(t, codec) for t in PATTERNS]


def _check_exact(logits, out_lens, graphs, K, min_score=NEG):
    N, Q = logits.shape[0], len(graphs)
    want = _want(logits, out_lens, graphs, K, min_score)
    assert _run(logits, out_lens, graphs, K, min_score) == want
    st, en, sc, fin, cnt = _raw(logits, out_lens, graphs, K, min_score)
    for n in range(N):
        for qi in range(Q):
            c = len(want[n][qi])
            assert cnt[n, qi] == c
            assert (st[n, qi, c:] == -1).all() and (en[n, qi, c:] == -1).all() and (fin[n, qi, c:] == -1).all() and (sc[n, qi, c:] == NEG).all()
    return want


GRID_SHAPES = [(3, 37, 12, [37, 0, 30], 1), (4, 300, 64, [300, 0, 251, 64], 2)]          # N, T, C, out_lens, frames per planted label


@pytest.mark.parametrize('N,T,C,out_lens,width', GRID_SHAPES)
@pytest.mark.parametrize('K', [1, 3])
def test_grid_logits_give_the_definition_exactly(N, T, C, out_lens, width, K):
    assert 17 * 8 * T < 2 ** 24
    logits, graphs = _pattern_case(N, T, C, out_lens, 300 + T, width)
    big = graphs[-1]
    assert big.P == 130 and max(len(p) for p in big.preds) == 10 and any(p < 64 <= q for q in range(big.P) for p in big.preds[q])
    want = _check_exact(logits, out_lens, graphs, K)
    zero = [sum(1 for line in want for h in line[qi] if h[2] == 0.0) for qi in range(len(graphs))]
    below = sum(1 for line in want for spots in line for h in spots if h[2] < 0.0)
    print(f'T {T} K {K}: hits at score 0 per pattern {zero}, {below} below')
    assert all(z >= 1 for z in zero) and (K == 1 or below > 0)
    assert any(len({h[3] for line in want for h in line[qi]}) > 1 for qi in range(len(graphs)))       # more than one final state is reported
    assert all(line == [[]] * len(graphs) for line, l in zip(want, out_lens) if l == 0)


def test_the_workspace_form_of_the_candidate_tables():
    T = 5150
    assert 17 * 8 * T < 2 ** 24
    rng = np.random.default_rng(77)
    codec = _letters(40)
    logits = (rng.integers(-64, 65, (1, T, 40)) / 8.0).astype(np.float32)
    for pos, w in ((5, 'acd'), (700, 'aab'), (2600, 'abab'), (5100, 'abd'), (5138, 'abab')):
        _plant(logits[0], codec.encode(w), pos, 2)
    graphs = [PT.compile_pattern(t, codec) for t in ('a[bc]d', 'a+b', '(ab)+')]
    want = _check_exact(logits, [T], graphs, 8)
    assert all(len(spots) == 8 for spots in want[0]) and all(spots[0][2] == 0.0 for spots in want[0])


# ---- 3. real-valued logits: the planted span, the score within the bound -----------------------------------------------------------------
def test_planted_pieces_in_real_valued_logits():
    """Pattern n: labels k..k+5 of line n's planted sequence, position 2 widened to a set of 3 classes and an optional label that is
    not there in front of position 4."""
    N, T, C = 8, 300, 128
    logits, labels, firsts = _planted_lines(N, T, C, 25, 60, 21, 8)
    codec = ascii_codec(C)
    ch = lambda l: PT.escape(codec.l2c[(int(l),)])
    graphs, spans, pieces = [], [], []
    for n in range(N):
        k = (7 * n + 3) % (len(labels[n]) - 5)
        lab = [int(l) for l in labels[n][k:k + 6]]
        others = [l for l in (lab[2] % (C - 1) + 1, (lab[2] + 40) % (C - 1) + 1)]
        extra = (lab[3] + 17) % (C - 1) + 1
        text = f'{ch(lab[0])}{ch(lab[1])}[{ch(others[0])}{ch(lab[2])}{ch(others[1])}]{ch(lab[3])}{ch(extra)}?{ch(lab[4])}{ch(lab[5])}'
        g = PT.compile_pattern(text, codec)
        assert g.P == 9 and not g.is_chain and g.accepts(lab)
        graphs.append(g)
        pieces.append(lab)
        spans.append((int(firsts[n][2 * k + 1]), int(firsts[n][2 * (k + 5) + 2]) - 1))
    got = _run(logits, [T] * N, graphs, 2)
    worst = 0.0
    for n in range(N):
        want = PT.spot_pattern_host(logits[n].T, graphs[n], 2)
        assert want and want[0][:2] == spans[n], (n, want, spans[n])                  # the definition first
        assert PT.match_host(logits[n].T, graphs[n], *want[0][:2], want[0][3]) == pieces[n]
        assert got[n][n] and got[n][n][0][:2] == spans[n] and got[n][n][0][3] == want[0][3], (n, got[n][n], spans[n])
        s_star, tol = want[0][2], _tol(T, want[0][2])
        gap = abs(got[n][n][0][2] - s_star)
        print(f'line {n}: span {spans[n]} s* {s_star:.6g} device {got[n][n][0][2]:.6g} tol {tol:.3g}')
        assert gap <= tol, (n, gap, tol)
        worst = max(worst, gap / tol)
        # another line's pattern: found somewhere at a score well below 0, where the float32 sums do round
        m = (n + 1) % N
        other = PT.spot_pattern_host(logits[n].T, graphs[m], 1)
        assert other[0][2] < -1.0 and got[n][m]
        assert abs(got[n][m][0][2] - other[0][2]) <= _tol(T, other[0][2])
    print(f'worst gap / tol {worst:.3g}')


# ---- 4. the model: a piece of the greedy string, one position widened ------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_own_greedy_piece_with_a_widened_position(text_case, dtype):
    tc = text_case('cfg2_text')
    net = _net(tc, dtype)
    codec = net.codec
    image, lens, idx = tc.batch(0)
    line, lens = torch.from_numpy(image).cuda(), torch.from_numpy(lens)
    greedy = net.predict_labels(line, lens)
    ch = lambda l: PT.escape(codec.l2c[(int(l),)])
    per_line, where, texts = [], [], []
    C = tc.hp.num_classes
    for n, recs in enumerate(greedy):
        assert len(recs) >= 6
        k = (5 * n + 1) % (len(recs) - 5)
        lab = [r[0] for r in recs[k:k + 6]]
        other = lab[3] % (C - 1) + 1
        per_line.append(f'{ch(lab[0])}{ch(lab[1])}{ch(lab[2])}[{ch(other)}{ch(lab[3])}]{ch(lab[4])}{ch(lab[5])}')
        where.append((recs[k][1], recs[k + 5][2]))
        texts.append(''.join(codec.l2c[(l,)] for l in lab))
    patterns = list(dict.fromkeys(per_line))
    found = net.spot_patterns(line, lens, patterns, hits=8)
    logits, out_lens = net.forward(line, lens)
    assert found['frames'] == [int(l) for l in out_lens]
    for n in range(len(greedy)):
        mine = found['hits'][n][patterns.index(per_line[n])]
        zero = [h for h in mine if h[2] == 0.0]
        assert zero, (n, mine)
        assert (where[n] + (0.0, texts[n])) in zero, (n, where[n], texts[n], zero)
        for per_pattern in found['hits'][n]:
            assert all(h[2] <= 0.0 for h in per_pattern)
    with pytest.raises(ValueError):
        net.spot_patterns(line, lens, ['☃+'])
    with pytest.raises(ValueError):
        net.spot_patterns(line, lens, ['a*'])


def _cased_codec(C):
    """The fixture's alphabet has no letters: labels 1..h read as 'a'.., labels h+1..2h as the same letters in upper case, so that every
    piece of a reading has another spelling that only case folding finds (labels left over read as caseless signs)."""
    h = min(26, (C - 1) // 2)
    c2l = {chr(0x61 + i): [1 + i] for i in range(h)}
    c2l.update({chr(0x41 + i): [1 + h + i] for i in range(h)})
    c2l.update({chr(0x2460 + k): [1 + 2 * h + k] for k in range(C - 1 - 2 * h)})
    return PytorchCodec(c2l)


def _cased_net(tc, dtype):
    net = PytorchRecognitionModel(**tc.hp.as_dict(), **DROPS, codec=_cased_codec(tc.hp.num_classes), compute_dtype=dtype)
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    return net.to('cuda:0').eval()


# ---- 5. pages and the index ----------------------------------------------------------------------------------------------------------------
M = 4


def test_pages_and_the_index_are_searched_for_patterns(text_case, tmp_path, capsys):
    from PIL import Image
    tc = text_case('cfg2_text')
    lines = [np.rint(tc.lines[i] * 255.0).astype(np.uint8) for i in PICK]
    page, placed = page_synth.text_page(lines, KINDS)
    page_lines = [Line(f'line{k}', P, B) for k, (_, P, B) in enumerate(placed)]
    pages = [(page, page_lines)]
    net = _cased_net(tc, 'bf16')
    read, = recognize_pages(net, pages, batch_size=4, **FIXTURE_FORM)
    def swap(text):
        """The other case of every character that has one in the codec."""
        return ''.join(c.swapcase() if c.swapcase() in net.codec.c2l and c.swapcase().swapcase() == c else c for c in text)

    queries = []
    for j, r in enumerate(read):
        k = (3 * j + 1) % (len(r['cuts']) - M)
        q = r['text'][k:k + M + 1]
        if q in queries or swap(q) in queries:
            q = r['text'][:M + 1]
        assert q not in queries
        queries.append(q)
    # the pieces in the other case, folded back by ignore_case; one real pattern beside them
    folded = [PT.escape(swap(q)) for q in queries]
    assert any(f != PT.escape(q) for f, q in zip(folded, queries)) and len(set(folded)) == len(folded)
    first = queries[0]
    alt = f'({PT.escape(first[:2])}|{PT.escape(queries[1][:2])})?{PT.escape(first[2:])}'
    literal = S.search_pages(net, pages, queries, hits=8, batch_size=4, **FIXTURE_FORM)
    hits = S.search_pages(net, pages, patterns=folded + [alt], ignore_case=True, hits=8, batch_size=4, **FIXTURE_FORM)
    assert all(set(h) == {'page', 'line', 'pattern', 'match', 'start', 'end', 'score', 'conf', 'quad'} for h in hits)
    for j, (q, f) in enumerate(zip(queries, folded)):
        want = [h for h in literal if h['line'] == f'line{j}' and h['query'] == q and h['score'] == 0.0]
        mine = [h for h in hits if h['line'] == f'line{j}' and h['pattern'] == f and h['score'] == 0.0]
        assert want and mine, (j, q)
        for w in want:
            same = [h for h in mine if (h['start'], h['end']) == (w['start'], w['end'])]
            assert same and same[0]['quad'] == w['quad'] and same[0]['match'] == q and same[0]['conf'] == 1.0, (j, q, w, mine)
    zero_alt = [h for h in hits if h['pattern'] == alt and h['line'] == 'line0' and h['score'] == 0.0]
    assert zero_alt and zero_alt[0]['match'] == first
    for h in hits:
        assert h['conf'] == pytest.approx(np.exp(h['score'] / len(net.codec.encode(h['match'])))) and 0 <= h['start'] <= h['end']
    # strings and patterns in one call: the strings' records are what they are alone
    both = S.search_pages(net, pages, queries[:3], patterns=folded[:2], ignore_case=True, hits=8, batch_size=4, **FIXTURE_FORM)
    assert [h for h in both if 'query' in h] == S.search_pages(net, pages, queries[:3], hits=8, batch_size=4, **FIXTURE_FORM)
    assert [h for h in both if 'pattern' in h] == [h for h in hits if h['pattern'] in folded[:2]]
    with pytest.raises(ValueError):
        S.search_pages(net, pages, patterns=['☃'], **FIXTURE_FORM)
    with pytest.raises(ValueError):
        S.search_pages(net, pages, patterns=['a*'], **FIXTURE_FORM)

    # the index built from those pages: the same lines, and device='cpu' gives the same records
    path = tmp_path / 'corpus.cidx'
    I.build_index(net, pages, path, batch_size=4, names=['scan'], **FIXTURE_FORM)
    found = I.search_index(path, patterns=folded + [alt], ignore_case=True, hits=8)
    assert all(set(h) == {'page', 'line', 'pattern', 'match', 'start', 'end', 'score', 'conf', 'quad'} for h in found)
    for j, (q, f) in enumerate(zip(queries, folded)):
        want = [h for h in hits if h['line'] == f'line{j}' and h['pattern'] == f and h['score'] == 0.0]
        mine = [h for h in found if h['line'] == f'line{j}' and h['pattern'] == f and h['score'] == 0.0]
        assert [(h['start'], h['end'], h['match']) for h in mine[:1]] == [(h['start'], h['end'], h['match']) for h in want[:1]], (j, q)
    assert {h['line'] for h in found if h['score'] == 0.0} == {h['line'] for h in hits if h['score'] == 0.0}
    assert found == I.search_index(path, patterns=folded + [alt], ignore_case=True, hits=8, device='cpu')
    mixed = I.search_index(path, queries[:2], patterns=[alt], hits=2)
    assert [h for h in mixed if 'query' in h] == I.search_index(path, queries[:2], hits=2)

    # the commands on the same page
    Image.fromarray(page).save(tmp_path / 'scan.png')
    pts = lambda a: ' '.join(f'{x:.3f},{y:.3f}' for x, y in a)
    body = ''.join(f'<TextLine id="{l.id}"><Coords points="{pts(l.boundary)}"/><Baseline points="{pts(l.baseline)}"/></TextLine>\n' for l in page_lines)
    (tmp_path / 'scan.xml').write_text('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2019-07-15">'
                                       f'<Page imageFilename="scan.png"><TextRegion id="r">{body}</TextRegion></Page></PcGts>\n', encoding='utf-8')
    src = PytorchRecognitionModel(**tc.hp.as_dict(), **DROPS, codec=_cased_codec(tc.hp.num_classes))
    src.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    save_safetensors(src, tmp_path / 'model.tar')
    (tmp_path / 'patterns.txt').write_text(folded[1] + '\n☃+\na*\n', encoding='utf-8')
    capsys.readouterr()
    out = tmp_path / 'out.json'
    xml = str(tmp_path / 'scan.xml')
    word = queries[2].strip()
    asked = swap(word)
    assert S.main(['-m', str(tmp_path / 'model.tar'), '-f', 'page', '-q', asked, '-e', alt, '-E', str(tmp_path / 'patterns.txt'), '--ignore-case',
                   '--hits', '2', '--pad', '0', '--edge', '1200', '--batch-size', '4', '-i', xml, str(out)]) == 0
    err = capsys.readouterr().err
    assert err.count('skipped') == 2 and 'empty string' in err and f'{xml}: ' in err and 'of 3 queries' in err
    from conformer_ocr_amd.page import read_page_xml
    file_lines = read_page_xml(tmp_path / 'scan.xml').lines
    g_word = PT.compile_pattern(PT.escape(asked), net.codec, True)
    g_word.text = asked
    want = S.search_pages(net, [(page, file_lines)], patterns=[g_word, alt, folded[1]], ignore_case=True, hits=2, batch_size=4, **FIXTURE_FORM)
    back = json.loads(out.read_text(encoding='utf-8'))
    assert len(back) == len(want) > 0
    for b, w in zip(back, want):
        assert b['page'] == xml and {k: b[k] for k in b if k not in ('page', 'quad')} == {k: w[k] for k in w if k not in ('page', 'quad')}
        assert b['quad'] == [list(p) for p in w['quad']]
    assert any(b['match'] == word for b in back if b['pattern'] == asked)
    assert S.main(['-m', str(tmp_path / 'model.tar'), '-e', 'a*', '-i', xml, str(out)]) == 1               # nothing left to search
    capsys.readouterr()
    assert I.main(['search', '--index', str(path), '-e', alt, '--ignore-case', '--hits', '2', str(out)]) == 0
    back = json.loads(out.read_text(encoding='utf-8'))
    want = I.search_index(path, patterns=[alt], ignore_case=True, hits=2)
    assert len(back) == len(want) > 0 and [(b['line'], b['match'], b['start'], b['end'], b['score']) for b in back] == \
        [(w['line'], w['match'], w['start'], w['end'], w['score']) for w in want]


# ---- 6. edges ----------------------------------------------------------------------------------------------------------------------------
def test_edges_prefix_threshold_and_reproducibility():
    rng = np.random.default_rng(9)
    codec = _letters(11)
    logits = (rng.integers(-64, 65, (3, 90, 11)) / 8.0).astype(np.float32)
    plants = ['cd', 'eee', 'abcdefg']
    for n in range(3):
        for pos in (4, 30, 61):
            _plant(logits[n], codec.encode(plants[n]), pos, 2)
    graphs = [PT.compile_pattern(t, codec) for t in ('c[de]', 'e+', 'abc(de|ed)fg')]
    out_lens = [90, 6, 80]                                                 # line 1: 6 frames, fewer than the 7 labels of pattern 2's shortest match
    eight = _check_exact(logits, out_lens, graphs, 8)
    assert eight[1][2] == [] and eight[1][1] != []
    assert _run(logits, out_lens, graphs, 1) == [[spots[:1] for spots in line] for line in eight]
    assert max(len(spots) for line in eight for spots in line) > 3
    cut = _check_exact(logits, out_lens, graphs, 8, -2.0)
    assert cut == [[[h for h in spots if h[2] >= -2.0] for spots in line] for line in eight]
    assert 0 < sum(len(s) for line in cut for s in line) < sum(len(s) for line in eight for s in line)
    assert _run(logits, out_lens, graphs, 8, min_score=np.inf) == [[[], [], []]] * 3
    assert _run(logits, out_lens, graphs, 8) == eight
    real = rng.standard_normal((3, 90, 11)).astype(np.float32)
    a, b = _raw(real, out_lens, graphs, 8), _raw(real, out_lens, graphs, 8)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _graph(cls, first, last, preds):
    return PT.PatternGraph('', cls, first, last, preds)


def test_argument_errors():
    eng = _engine()
    p = torch.zeros((1, 4, 3), device='cuda')
    ok = _graph([1, 2], [True, False], [False, True], [[], [0]])
    full = [list(range(70)) for _ in range(70)]
    bad = [
        _graph([3, 1], [True, False], [False, True], [[], [0]]),                    # class outside [1, ncls)
        _graph([0, 1], [True, False], [False, True], [[], [0]]),                    # the blank as a class
        _graph([], [], [], []),                                                    # P = 0
        _graph([1] * 257, [True] + [False] * 256, [False] * 256 + [True], [[]] + [[q - 1] for q in range(1, 257)]),
        _graph([1] * 70, [True] * 70, [True] * 70, full),                           # 4900 edges
        _graph([1, 2], [True, False], [False, True], [[], [2]]),                    # a predecessor outside [0, P)
        _graph([1, 2], [True, False], [False, True], [[], [-1]]),
        _graph([1, 2, 1], [True, False, False], [False, False, True], [[], [0], [1, 0]]),      # not ascending
        _graph([1, 2, 1], [True, False, False], [False, False, True], [[], [0], [1, 1]]),      # not strictly
        _graph([1, 2], [False, False], [False, True], [[], [0]]),                   # no first state
        _graph([1, 2], [True, False], [False, False], [[], [0]]),                   # no last state
    ]
    for g in bad:
        with pytest.raises(ValueError):
            eng.ctc_spot_pattern(p, [4], [ok, g])
    with pytest.raises(ValueError):
        eng.ctc_spot_pattern(p, [4], [ok], hits=0)
    with pytest.raises(ValueError):
        eng.ctc_spot_pattern(p, [4], [ok], hits=9)
    with pytest.raises(ValueError):
        eng.ctc_spot_pattern(p, [4], [])                                            # Q < 1
    with pytest.raises(ValueError):
        eng.ctc_spot_pattern(p, [5], [ok])                                          # more valid frames than frames
    with pytest.raises(ValueError):
        eng.ctc_spot_pattern(p, [-1], [ok])
    with pytest.raises(ValueError):
        eng.ctc_spot_pattern(p, [4], [ok], min_score=float('nan'))
    with pytest.raises(NotImplementedError):
        eng.ctc_spot_pattern(torch.zeros((1, 8001, 3), device='cuda'), [8001], [ok])
    with pytest.raises(NotImplementedError):
        eng.ctc_spot_pattern(torch.zeros((65536, 1, 3), device='cuda'), [1] * 65536, [ok])
    # the engine is still usable: all classes tie at the maximum, so 'ab' costs nothing anywhere; the latest end wins the tie
    assert eng.ctc_spot_pattern(p, [4], [ok]) == [[[(0, 3, 0.0, 1)]]]
    assert eng.ctc_spot(p, [4], [[1, 2]]) == [[[(0, 3, 0.0)]]]
    # the limits themselves are served
    wide = _graph([1] * 64, [True] * 64, [True] * 64, [list(range(64)) for _ in range(64)])           # 4096 edges
    assert eng.ctc_spot_pattern(p, [4], [wide]) == [[[(0, 3, 0.0, 0)]]]
    long_chain = PT.chain_graph([1, 2] * 128)                                                          # 256 label states
    assert eng.ctc_spot_pattern(p, [4], [long_chain]) == [[[]]]


def test_greedy_shortcut_is_not_disturbed(text_case):
    """`ctc_spot_pattern` between a forward and its `ctc_greedy`: the decoder epilogue's per-frame argmax still belongs to the logits."""
    tc = text_case('cfg2_text')
    net = _cased_net(tc, 'bf16')
    image, lens, idx = tc.batch(0)
    line = torch.from_numpy(image[:8]).cuda().squeeze(1)
    eng = net.engine(torch.device('cuda', 0))
    logits, out_lens = eng.forward(line, lens[:8])
    assert eng._argmax_is_fresh(logits)
    graphs = [PT.compile_pattern(PT.labels_text(net.codec, tc.ref_strings[i][:5]), net.codec, ignore_case=True) for i in idx[:8]]
    assert not any(g.is_chain for g in graphs)
    found = eng.ctc_spot_pattern(logits, out_lens, graphs, hits=2)
    assert all(found[n][n] for n in range(8))
    assert eng._argmax_is_fresh(logits)
    after = eng.ctc_greedy(logits, out_lens)
    logits2, out_lens2 = eng.forward(line, lens[:8])
    assert eng.ctc_greedy(logits2, out_lens2) == after
    assert eng.ctc_greedy(logits.clone(), out_lens) == after              # from the values, without the shortcut
