"""GPU: keyword spotting (cocr_ctc_spot) against the definition `search.spot_host`.

Exact where the arithmetic is exact: on logits that are multiples of 1/8 in [-8, 8] (planted spots 9.0) every r_t(c) and every partial
sum of the recursion is a multiple of 1/8 of magnitude <= 17 T, exactly representable in float32 while 17 * 8 * T < 2^24, so the device
must give the float64 definition's counts, starts, ends and scores bit for bit, ties included.  On real-valued logits the spans are
compared where the planted text decides them, and the score is held to the bound of section 7d,
    tol = 8 T 2^-23 max(1, |s*|)
(each of the at most T steps adds one rounding of the running sum and the rounding of one difference of two logits)."""
import json
import os

import numpy as np
import pytest
import torch

from conformer_ocr_amd import search as S
from conformer_ocr_amd.codec import ascii_codec
from conformer_ocr_amd.page import Line, recognize_pages
from conformer_ocr_amd.pred import PytorchRecognitionModel, save_safetensors
from tests import page_synth
from tests.test_hip_parity import _log          # appends a record to the parity log, as the parity tests do

pytestmark = pytest.mark.gpu
DROPS = dict(input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1)
NEG = -np.inf


def _engine():
    from conformer_ocr_amd.ctc_decoder import _scratch_engine
    return _scratch_engine(torch.device('cuda', 0))


def _run(logits, out_lens, queries, hits=1, min_score=NEG):
    return _engine().ctc_spot(torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).cuda(), out_lens, queries, hits, min_score)


def _want(logits, out_lens, queries, hits=1, min_score=NEG):
    return [[S.spot_host(logits[n, :int(out_lens[n])].T, q, hits, min_score) for q in queries] for n in range(logits.shape[0])]


# ---- 1. grid logits: everything, exactly ----------------------------------------------------------------------------------------------
def _plant(x, lab, pos, width):
    """`lab` from frame `pos` of the (T, C) line x: `width` frames of each label, then one blank frame."""
    for k, l in enumerate(lab):
        at = pos + (width + 1) * k
        x[at:at + width + 1] = np.minimum(x[at:at + width + 1], 8.0)
        x[at:at + width, l] = 9.0
        x[at + width, 0] = 9.0


def _grid_case(N, T, C, lens_q, seed, out_lens, width=2):
    """Q queries of the given lengths: query 1 repeats a label, query 2 is the tail of query 0 followed by one more label (their
    occurrences overlap), the last query is planted nowhere; the others are planted in some lines, query 0 twice back to back."""
    rng = np.random.default_rng(seed)
    logits = (rng.integers(-64, 65, (N, T, C)) / 8.0).astype(np.float32)
    queries = [[int(v) for v in rng.integers(1, C, L)] for L in lens_q]
    if len(queries) > 1 and len(queries[1]) > 1:
        queries[1][1] = queries[1][0]
    if len(queries) > 2 and len(queries[0]) > 1:
        queries[2] = (queries[0][1:] + queries[2])[:max(len(queries[2]), 2)]
    for n in range(N):
        at = int(rng.integers(0, 3))
        for qi, lab in enumerate(queries[:-1]):
            for _ in range(2 if qi == 0 else 1):
                span = (width + 1) * len(lab)
                if at + span <= out_lens[n] and (qi + n) % 3 != 2:
                    _plant(logits[n], lab, at, width)
                    at += span + (0 if qi == 0 else int(rng.integers(0, 4)))
    return logits, queries


@pytest.mark.parametrize('N,T,C,lens_q,K,out_lens,width', [
    (3, 37, 5, [2, 3, 2, 1, 4], 3, [37, 0, 30], 2),                               # SJ 1; Q = 5 is no multiple of 4; a line without frames
    (4, 300, 64, [7, 12, 8, 40, 1, 3, 25, 5, 9], 4, [300, 0, 251, 64], 2),        # SJ 2 (79 states)
    (2, 600, 40, [3, 6, 255, 2, 4, 1], 8, [600, 555], 1),                        # SJ 8 (509 states): the 255-label query is planted in line 1
    (1, 5150, 40, [30, 4], 8, [5150], 2),                                        # the workspace form of the candidate tables
    (5, 64, 9, [1, 2, 2, 5], 2, [64, 1, 63, 5, 0], 2),                            # Q = 4, lines of 0, 1 and 5 frames
])
def test_grid_logits_give_the_definition_exactly(N, T, C, lens_q, K, out_lens, width):
    assert 17 * 8 * T < 2 ** 24
    logits, queries = _grid_case(N, T, C, lens_q, 100 + T, out_lens, width)
    assert (logits * 8 == np.rint(logits * 8)).all() and np.abs(logits).max() <= 9.0
    got = _run(logits, out_lens, queries, K)
    want = _want(logits, out_lens, queries, K)
    exact_hits = sum(1 for line in want for spots in line for h in spots if h[2] == 0.0)
    total = sum(len(spots) for line in want for spots in line)
    print(f'T {T}: {total} hits, {exact_hits} at score 0')
    assert exact_hits >= 2 and total > exact_hits
    for n in range(N):
        for qi in range(len(queries)):
            assert got[n][qi] == want[n][qi], (n, qi)
    # the raw outputs: entries past the count are -1 / -1 / -inf
    eng = _engine()
    h = eng.ctc_spot_async(torch.from_numpy(logits).cuda(), out_lens, queries, K)
    eng.collect_spot(h)
    Q = len(queries)
    st, en = h[1][0].numpy()[:, :N * Q * K].reshape(2, N, Q, K)
    sc = h[1][1].numpy()[:N * Q * K].reshape(N, Q, K)
    cnt = h[1][2].numpy()[:N * Q].reshape(N, Q)
    for n in range(N):
        for qi in range(Q):
            c = len(want[n][qi])
            assert cnt[n, qi] == c
            assert (st[n, qi, c:] == -1).all() and (en[n, qi, c:] == -1).all() and (sc[n, qi, c:] == NEG).all()


# ---- 2. real-valued logits: planted spans, the score within the bound -----------------------------------------------------------------
def _tol(T, score):
    return 8 * T * 2.0 ** -23 * max(1.0, abs(score))


def _planted_lines(N, T, C, l_lo, l_hi, seed, gain):
    """tests/test_hip_align.py's recipe: a label sequence laid over the whole line with random run lengths, `gain` added to its classes."""
    rng = np.random.default_rng(seed)
    logits = np.empty((N, T, C), dtype=np.float32)
    labels, firsts = [], []
    for n in range(N):
        L = int(rng.integers(l_lo, l_hi + 1))
        lab = rng.integers(1, C, L)
        n_states = 2 * L + 1
        runs = np.zeros(n_states, dtype=np.int64)
        runs[1::2] = 1
        runs[2:-1:2] = lab[1:] == lab[:-1]
        runs += rng.multinomial(T - int(runs.sum()), [1.0 / n_states] * n_states)
        ext = np.zeros(n_states, dtype=np.int64)
        ext[1::2] = lab
        x = rng.standard_normal((T, C)).astype(np.float32)
        x[np.arange(T), np.repeat(ext, runs)] += np.float32(gain)
        logits[n] = x
        labels.append(lab)
        firsts.append(np.concatenate([[0], np.cumsum(runs)]))
    return logits, labels, firsts


@pytest.mark.parametrize('N,T,C,l_lo,l_hi,m,seed,gain', [(8, 300, 128, 25, 60, 6, 21, 8), (3, 600, 128, 100, 200, 90, 22, 8)])
def test_planted_queries_in_real_valued_logits(N, T, C, l_lo, l_hi, m, seed, gain):
    """Query n is labels k..k+m-1 of line n's planted sequence; the first hit of (line n, query n) is the planted span."""
    logits, labels, firsts = _planted_lines(N, T, C, l_lo, l_hi, seed, gain)
    queries, spans = [], []
    for n in range(N):
        k = (7 * n + 3) % (len(labels[n]) - m + 1)
        queries.append([int(l) for l in labels[n][k:k + m]])
        spans.append((int(firsts[n][2 * k + 1]), int(firsts[n][2 * (k + m - 1) + 2]) - 1))
    # query N + n: query n with its middle label replaced -- found at a score well below 0, where the float32 sums do round
    for n in range(N):
        wrong = list(queries[n])
        wrong[m // 2] = wrong[m // 2] % (C - 1) + 1
        queries.append(wrong)
    got = _run(logits, [T] * N, queries, 2)
    worst = 0.0
    for n in range(N):
        want = S.spot_host(logits[n].T, queries[N + n], 2)
        s_star, tol = want[0][2], _tol(T, want[0][2])
        assert s_star < -1.0 and got[n][N + n]
        gap = abs(got[n][N + n][0][2] - s_star)
        print(f'seed {seed} line {n}, misspelt: s* {s_star:.6g} device {got[n][N + n][0][2]:.6g} tol {tol:.3g}')
        assert gap <= tol, (n, gap, tol)
        worst = max(worst, gap / tol)
    for n in range(N):
        want = S.spot_host(logits[n].T, queries[n], 2)
        assert want and want[0][:2] == spans[n], (n, want, spans[n])
        assert got[n][n] and got[n][n][0][:2] == spans[n], (n, got[n][n], spans[n])
        s_star, tol = want[0][2], _tol(T, want[0][2])
        gap = abs(got[n][n][0][2] - s_star)
        print(f'seed {seed} line {n}: span {spans[n]} s* {s_star:.6g} device {got[n][n][0][2]:.6g} tol {tol:.3g}')
        assert gap <= tol, (n, gap, tol)
        worst = max(worst, gap / tol)
    _log('search_planted', {'seed': seed, 'T': T, 'lines': N, 'worst_gap_over_tol': worst})


# ---- 3. the model: a piece of the greedy string is found where the greedy decoder read it -------------------------------------------
def _net(tc, dtype):
    net = PytorchRecognitionModel(**tc.hp.as_dict(), **DROPS, codec=ascii_codec(tc.hp.num_classes), compute_dtype=dtype)
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    return net.to('cuda:0').eval()


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_own_greedy_substring_is_found_at_the_greedy_records(text_case, dtype):
    tc = text_case('cfg2_text')
    net = _net(tc, dtype)
    image, lens, idx = tc.batch(0)
    line, lens = torch.from_numpy(image).cuda(), torch.from_numpy(lens)
    greedy = net.predict_labels(line, lens)
    queries, where = [], []
    for n, recs in enumerate(greedy):
        assert len(recs) >= 6
        k = (5 * n + 1) % (len(recs) - 5)
        queries.append([r[0] for r in recs[k:k + 6]])
        where.append((recs[k][1], recs[k + 5][2]))
    found = net.spot_labels(line, lens, queries, hits=8)
    assert len(found) == len(greedy) and all(len(per_query) == len(queries) for per_query in found)
    for n in range(len(greedy)):
        zero = [h for h in found[n][n] if h[2] == 0.0]
        assert zero, (n, found[n][n])
        assert where[n] in [h[:2] for h in zero], (n, where[n], zero)
        for per_query in found[n]:
            assert all(h[2] <= 0.0 for h in per_query)
    # strings: the same through the codec; a query the codec cannot encode is reported, not searched
    codec = net.codec
    texts = [''.join(codec.l2c[(l,)] for l in q) for q in queries[:3]] + ['☃']
    by_text = net.spot(line, lens, texts, hits=8)
    assert by_text['skipped'][:3] == ['', '', ''] and by_text['skipped'][3] == '☃'
    logits, out_lens = net.forward(line, lens)
    assert by_text['frames'] == [int(l) for l in out_lens]
    for n in range(len(greedy)):
        assert by_text['hits'][n][:3] == found[n][:3] and by_text['hits'][n][3] == []


# ---- 4. pages -----------------------------------------------------------------------------------------------------------------------
KINDS = [('line', 0.0), ('line', 7.0), ('arc', 2600.0, 1), ('line', -7.0), ('line', 15.0), ('line', 0.0), ('line', -15.0),
         ('arc', 2500.0, -1), ('line', 0.0), ('line', 3.0)]
PICK = [3, 4, 14, 7, 11, 12, 16, 22, 23, 6]          # tests/test_hip_page.py PICK
FIXTURE_FORM = dict(pad=0, edge=1200)
M = 4                                                # a query is characters k .. k + M of the line's reading


def test_pages_are_searched_for_pieces_of_their_reading(text_case, tmp_path, capsys):
    from PIL import Image
    tc = text_case('cfg2_text')
    lines = [np.rint(tc.lines[i] * 255.0).astype(np.uint8) for i in PICK]
    page, placed = page_synth.text_page(lines, KINDS)
    page_lines = [Line(f'line{k}', P, B) for k, (_, P, B) in enumerate(placed)]
    net = _net(tc, 'bf16')
    read, = recognize_pages(net, [(page, page_lines)], batch_size=4, **FIXTURE_FORM)
    queries, ks = [], []
    for j, r in enumerate(read):
        assert len(r['cuts']) > M
        k = (3 * j + 1) % (len(r['cuts']) - M)
        q = r['text'][k:k + M + 1]
        if q in queries:                                 # (search_pages takes each string once)
            k = 0
            q = r['text'][:M + 1]
        assert q not in queries
        queries.append(q)
        ks.append(k)
    hits = S.search_pages(net, [(page, page_lines)], queries, hits=8, batch_size=4, **FIXTURE_FORM)
    assert all(set(h) == {'page', 'line', 'query', 'start', 'end', 'score', 'conf', 'quad'} for h in hits)
    order = [(int(h['line'][4:]), queries.index(h['query'])) for h in hits]
    assert order == sorted(order) and all(h['page'] == 0 for h in hits)
    for j, (r, q, k) in enumerate(zip(read, queries, ks)):
        mine = [h for h in hits if h['line'] == f'line{j}' and h['query'] == q]
        assert all(a['score'] >= b['score'] for a, b in zip(mine, mine[1:]))
        zero = [h for h in mine if h['score'] == 0.0]
        assert zero, (j, q, mine)
        first, last = r['cuts'][k][1], r['cuts'][k + M][1]
        want = [first[0], last[1], last[2], first[3]]
        assert any(np.allclose(np.asarray(h['quad']), np.asarray(want), rtol=0, atol=1e-6) for h in zero), (j, q, zero, want)
        assert all(h['conf'] == 1.0 for h in zero)
    for h in hits:
        assert 0 <= h['start'] <= h['end'] and 0.0 < h['conf'] <= 1.0 and h['conf'] == pytest.approx(np.exp(h['score'] / (M + 1)))
    # a threshold keeps, per line and query, the hits at or above it
    kept = S.search_pages(net, [(page, page_lines)], queries, hits=8, min_conf=0.5, batch_size=4, **FIXTURE_FORM)
    assert kept == [h for h in hits if h['conf'] >= 0.5] and 0 < len(kept) < len(hits)
    with pytest.raises(ValueError):
        S.search_pages(net, [(page, page_lines)], ['☃'], **FIXTURE_FORM)

    # the command on the same page
    Image.fromarray(page).save(tmp_path / 'scan.png')
    pts = lambda a: ' '.join(f'{x:.3f},{y:.3f}' for x, y in a)
    body = ''.join(f'<TextLine id="{l.id}"><Coords points="{pts(l.boundary)}"/><Baseline points="{pts(l.baseline)}"/></TextLine>\n' for l in page_lines)
    (tmp_path / 'scan.xml').write_text('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2019-07-15">'
                                       f'<Page imageFilename="scan.png"><TextRegion id="r">{body}</TextRegion></Page></PcGts>\n', encoding='utf-8')
    src = PytorchRecognitionModel(**tc.hp.as_dict(), **DROPS, codec=ascii_codec(tc.hp.num_classes))
    src.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    save_safetensors(src, tmp_path / 'model.tar')
    (tmp_path / 'queries.txt').write_text(queries[1] + '\n☃\n', encoding='utf-8')
    capsys.readouterr()
    out = tmp_path / 'out.json'
    xml = str(tmp_path / 'scan.xml')
    assert S.main(['-m', str(tmp_path / 'model.tar'), '-f', 'page', '-q', queries[0], '-Q', str(tmp_path / 'queries.txt'), '--hits', '2', '--pad', '0',
                   '--edge', '1200', '--batch-size', '4', '-i', xml, str(out)]) == 0
    err = capsys.readouterr().err
    assert 'skipped' in err and f'{xml}: ' in err and 'of 2 queries' in err
    with open(out, encoding='utf-8') as fp:
        back = json.load(fp)
    # the file's coordinates are rounded to 3 decimals: the command is held to `search_pages` on the lines as the file gives them
    from conformer_ocr_amd.page import read_page_xml
    from conformer_ocr_amd.dataset import normalize_text
    asked = [normalize_text(q, None, True) for q in queries[:2]]                 # the command strips the queries' outer whitespace
    assert len(set(asked)) == 2 and all(asked)
    want = S.search_pages(net, [(page, read_page_xml(tmp_path / 'scan.xml').lines)], asked, hits=2, batch_size=4, **FIXTURE_FORM)
    assert len(back) == len(want) > 0
    for b, w in zip(back, want):
        assert b['page'] == xml and (b['line'], b['query'], b['start'], b['end']) == (w['line'], w['query'], w['start'], w['end'])
        assert b['score'] == w['score'] and b['quad'] == [list(p) for p in w['quad']]
    assert S.main(['-m', str(tmp_path / 'model.tar'), '-q', '☃', '-i', xml, str(out)]) == 1           # no searchable query
    assert 'no query the model can encode' in capsys.readouterr().err


# ---- 5. edges -------------------------------------------------------------------------------------------------------------------------
def test_edges_prefix_threshold_and_reproducibility():
    rng = np.random.default_rng(9)
    logits = (rng.integers(-64, 65, (3, 90, 11)) / 8.0).astype(np.float32)
    queries = [[3, 4], [5], [1, 2, 3, 4, 5, 6, 7]]
    for n in range(3):
        for pos in (4, 30, 61):
            _plant(logits[n], queries[n], pos, 2)
    out_lens = [90, 6, 80]                                                 # line 1: 6 frames, fewer than query 2's 7 labels
    eight = _run(logits, out_lens, queries, 8)
    assert eight == _want(logits, out_lens, queries, 8)
    assert eight[1][2] == [] and eight[1][1] != []
    one = _run(logits, out_lens, queries, 1)
    assert one == [[spots[:1] for spots in line] for line in eight]
    assert max(len(spots) for line in eight for spots in line) > 3
    cut = _run(logits, out_lens, queries, 8, min_score=-2.0)
    assert cut == [[[h for h in spots if h[2] >= -2.0] for spots in line] for line in eight] == _want(logits, out_lens, queries, 8, -2.0)
    assert 0 < sum(len(s) for line in cut for s in line) < sum(len(s) for line in eight for s in line)
    assert _run(logits, out_lens, queries, 8, min_score=np.inf) == [[[], [], []]] * 3
    assert _run(logits, out_lens, queries, 8) == eight                     # bitwise: the scores are compared as floats
    real = rng.standard_normal((3, 90, 11)).astype(np.float32)
    assert _run(real, out_lens, queries, 8) == _run(real, out_lens, queries, 8)


def test_argument_errors(text_case):
    eng = _engine()
    p = torch.zeros((1, 4, 3), device='cuda')
    with pytest.raises(ValueError):
        eng.ctc_spot(p, [4], [[3]])                   # label outside [1, ncls)
    with pytest.raises(ValueError):
        eng.ctc_spot(p, [4], [[1], [0]])              # blank as a label
    with pytest.raises(ValueError):
        eng.ctc_spot(p, [4], [[1], []])               # an empty query
    with pytest.raises(ValueError):
        eng.ctc_spot(p, [4], [[1, 2] * 128])          # 256 labels
    with pytest.raises(ValueError):
        eng.ctc_spot(p, [5], [[1]])                   # more valid frames than frames
    with pytest.raises(ValueError):
        eng.ctc_spot(p, [-1], [[1]])
    with pytest.raises(ValueError):
        eng.ctc_spot(p, [4], [[1]], hits=0)
    with pytest.raises(ValueError):
        eng.ctc_spot(p, [4], [[1]], hits=9)
    with pytest.raises(ValueError):
        eng.ctc_spot(p, [4], [])                      # Q < 1
    with pytest.raises(ValueError):
        eng.ctc_spot(p, [4], [[1]], min_score=float('nan'))
    with pytest.raises(NotImplementedError):
        eng.ctc_spot(torch.zeros((1, 8001, 3), device='cuda'), [8001], [[1]])
    assert eng.ctc_spot(p, [4], [[1]]) == [[[(0, 3, 0.0)]]]                 # the engine is still usable: all classes tie at the maximum
    # the model-level call takes a query of more than 255 labels through the definition
    tc = text_case('cfg2_text')
    net = _net(tc, 'fp32')
    image, lens, idx = tc.batch(0)
    line, lens = torch.from_numpy(image[:2]).cuda(), torch.from_numpy(lens[:2])
    short = tc.ref_strings[idx[1]][:4]
    long_query = [1, 2] * 128
    got = net.spot_labels(line, lens, [long_query, short], hits=2)
    logits, out_lens = net.forward(line, lens)
    for n in range(2):
        assert got[n][0] == S.spot_host(logits[n, :int(out_lens[n])].T.cpu().numpy(), long_query, 2)
    assert got[1][1] and got[1][1][0][2] == 0.0


def test_greedy_shortcut_is_not_disturbed(text_case):
    """`ctc_spot` between a forward and its `ctc_greedy`: the decoder epilogue's per-frame argmax still belongs to the logits."""
    tc = text_case('cfg2_text')
    net = _net(tc, 'bf16')
    image, lens, idx = tc.batch(0)
    line = torch.from_numpy(image[:8]).cuda().squeeze(1)
    eng = net.engine(torch.device('cuda', 0))
    logits, out_lens = eng.forward(line, lens[:8])
    assert eng._argmax_is_fresh(logits)
    queries = [tc.ref_strings[i][:5] for i in idx[:8]]
    found = eng.ctc_spot(logits, out_lens, queries, hits=2)
    assert all(found[n][n] for n in range(8))
    assert eng._argmax_is_fresh(logits)
    after = eng.ctc_greedy(logits, out_lens)
    logits2, out_lens2 = eng.forward(line, lens[:8])
    assert eng.ctc_greedy(logits2, out_lens2) == after
    assert eng.ctc_greedy(logits.clone(), out_lens) == after              # from the values, without the shortcut
