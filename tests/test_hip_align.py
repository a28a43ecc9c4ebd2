"""GPU: forced alignment (cocr_ctc_align) against the definition `align.viterbi_align`.

Paths are compared where the inputs decide them: planted alignments whose runner-up lies far below the float32 error bound, a line's own
greedy string on the metric's model, pages aligned to the strings they were read as.  On random logits (runner-up gaps down to 1e-4 at
scores of -1500) the device's path may legitimately differ, so there the SCORE of the device's path is held to the bound
    tol = 8 T 2^-23 max(1, |s*|)
(each of the T steps adds one rounding of the running sum and the error of one log-probability, both a few ulp at magnitude <= |score|;
a wrong turn can only be taken between candidates closer than that accumulated error and then costs at most twice it), and the path
itself on every line whose runner-up gap exceeds the bound."""
import json
import os
from xml.sax.saxutils import escape

import numpy as np
import pytest
import torch

from conformer_ocr_amd import align as A
from conformer_ocr_amd.codec import ascii_codec
from conformer_ocr_amd.page import Line, recognize_pages
from conformer_ocr_amd.pred import PytorchRecognitionModel, save_safetensors
from tests import page_synth
from tests.test_hip_parity import _log          # appends a record to the parity log, as the parity tests do

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'ctc_loss.npz')
DROPS = dict(input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1)


def _engine():
    from conformer_ocr_amd.ctc_decoder import _scratch_engine
    return _scratch_engine(torch.device('cuda', 0))


def _run(logits, out_lens, targets, label_lens):
    return _engine().ctc_align(torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).cuda(), out_lens, targets, label_lens)


def _tol(T, score):
    return 8 * T * 2.0 ** -23 * max(1.0, abs(score))


def _ext(labels):
    ext = np.zeros(2 * len(labels) + 1, dtype=np.int64)
    ext[1::2] = labels
    return ext


def _runner_up_gap(lp, labels, states):
    """Best score minus the best score of any path that leaves the best path somewhere: max-plus forward table f and backward table g over
    the lattice (float64); f + g at a cell is the best score of any path through it.  lp (C, T)."""
    T = lp.shape[1]
    ext = _ext(labels)
    S = ext.shape[0]
    skip = np.zeros(S, dtype=bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    e = lp[ext]                                                     # (S, T)
    NEG = -np.inf
    f = np.full((T, S), NEG)
    f[0, :2] = e[:2, 0]
    for t in range(1, T):
        p = np.concatenate([[NEG, NEG], f[t - 1]])
        f[t] = np.maximum(np.maximum(p[2:], p[1:S + 1]), np.where(skip, p[:S], NEG)) + e[:, t]
    g = np.full((T, S), NEG)
    g[T - 1, max(S - 2, 0):] = 0.0
    skip_up = np.concatenate([skip, [False, False]])[2:]         # s -> s + 2 allowed
    for t in range(T - 2, -1, -1):
        n = np.concatenate([g[t + 1] + e[:, t + 1], [NEG, NEG]])
        g[t] = np.maximum(np.maximum(n[:S], n[1:S + 1]), np.where(skip_up, n[2:], NEG))
    through = f + g
    best = through[np.arange(T), states].max()
    through[np.arange(T), states] = NEG
    return float(best - through.max())


def _frame_classes(records, T):
    cls = np.zeros(T, dtype=np.int64)
    for l, st, en, _ in records:
        cls[st:en + 1] = l
    return cls


def _check_valid(records, labels, T):
    assert [r[0] for r in records] == [int(l) for l in labels]
    prev_end, prev_lab = -1, None
    for l, st, en, cf in records:
        assert 0 <= st <= en < T
        assert st > prev_end + (1 if l == prev_lab else 0)          # strictly increasing; equal neighbours at least one frame apart
        assert 0.0 < cf <= 1.0 + 1e-6
        prev_end, prev_lab = en, l


# ---- 1. planted alignments: the path itself -----------------------------------------------------------------------------------------
def _planted(N, T, C, l_lo, l_hi, seed, gain):
    rng = np.random.default_rng(seed)
    logits = np.empty((N, T, C), dtype=np.float32)
    labels, runs_all = [], []
    for n in range(N):
        L = int(rng.integers(l_lo, l_hi + 1))
        lab = rng.integers(1, C, L)
        S = 2 * L + 1
        runs = np.zeros(S, dtype=np.int64)
        runs[1::2] = 1
        runs[2:-1:2] = lab[1:] == lab[:-1]                          # a blank between equal neighbours
        runs += rng.multinomial(T - int(runs.sum()), [1.0 / S] * S)
        cls = np.repeat(_ext(lab), runs)
        x = rng.standard_normal((T, C)).astype(np.float32)
        x[np.arange(T), cls] += np.float32(gain)
        logits[n] = x
        labels.append(lab)
        runs_all.append(runs)
    return logits, labels, runs_all


@pytest.mark.parametrize('N,T,C,l_lo,l_hi,seed,gain', [(32, 300, 128, 25, 60, 11, 6), (8, 600, 128, 100, 255, 12, 6),
                                                       (2, 5150, 40, 255, 255, 13, 12), (2, 5150, 40, 3, 3, 14, 12)])
def test_planted_alignments(N, T, C, l_lo, l_hi, seed, gain):
    """The two batches of 5150 frames take the workspace form of the back-pointer table, the others the LDS form."""
    logits, labels, runs_all = _planted(N, T, C, l_lo, l_hi, seed, gain)
    got = _run(logits, [T] * N, np.concatenate(labels), [len(l) for l in labels])
    min_gap = np.inf
    for n in range(N):
        lab, runs = labels[n], runs_all[n]
        first = np.concatenate([[0], np.cumsum(runs)])
        planted = [(int(lab[k]), int(first[2 * k + 1]), int(first[2 * k + 2]) - 1) for k in range(len(lab))]
        want, s_star = A.viterbi_align(logits[n].T, lab)
        lp = A.log_softmax64(logits[n].T)
        states, _ = A.viterbi_path(lp, lab)
        tol = _tol(T, s_star)
        gap = _runner_up_gap(lp, lab, states)
        min_gap = min(min_gap, gap)
        print(f'planted seed {seed} line {n}: L {len(lab)} score {s_star:.4f} tol {tol:.3g} runner-up gap {gap:.4g}')
        assert gap > 2 * tol
        assert [r[:3] for r in want] == planted
        records, score = got[n]
        assert records is not None
        assert [r[:3] for r in records] == planted, n
        assert abs(score - s_star) <= tol, (n, score, s_star)
        np.testing.assert_allclose([r[3] for r in records], [r[3] for r in want], atol=1e-5, rtol=0)
    _log('align_planted', {'seed': seed, 'T': T, 'lines': N, 'min_runner_up_gap': min_gap})


def _check_seam_lines(Ls):
    from tests.test_hip_ctc_loss import seam_batch
    logits, lines = seam_batch(Ls)
    got = _run(logits, Ls, np.concatenate([lab for _, lab, _ in lines]), Ls)
    for n, (L, (_, lab, lp)) in enumerate(zip(Ls, lines)):
        own = lp[np.arange(L), lab]
        records, score = got[n]
        assert records is not None
        assert [r[:3] for r in records] == [(int(lab[k]), k, k) for k in range(L)], L
        assert abs(score - own.sum()) <= _tol(L, own.sum()), (L, score, own.sum())          # the bars of test_planted_alignments
        np.testing.assert_allclose([r[3] for r in records], np.exp(own), atol=1e-5, rtol=0)


@pytest.mark.parametrize('L', [32, 33, 64, 128, 255])
def test_register_seams_on_the_single_path(L):
    """tests/test_hip_ctc_loss.py `seam_line`: T = L frames for L labels, one path, label k on frame k -- every step crosses each
    register seam through the skip edge.  Each L in a call of its own (the kernel form follows the longest line of a call)."""
    _check_seam_lines([L])


def test_register_seams_on_the_single_path_in_one_batch():
    """All five lines at eight registers per lane."""
    _check_seam_lines([32, 33, 64, 128, 255])


# ---- 2. random logits: the score ----------------------------------------------------------------------------------------------------
def _random_batches():
    d = np.load(GOLD)
    for name in ('mixed', 'wide', 'long'):
        yield name, d[name + '.probits'], d[name + '.targets'], d[name + '.out_lens'], d[name + '.label_lens']
    for N, T, C, max_l in [(1, 1, 2, 1), (5, 33, 7, 16), (3, 130, 65, 64), (2, 260, 257, 127), (2, 520, 40, 255), (33, 300, 100, 120)]:
        g = np.random.default_rng(N * 1000 + T)
        probits = (g.standard_normal((N, T, C)) * 2.0).astype(np.float32)
        out_lens = g.integers(max(1, T // 2), T + 1, size=N)
        out_lens[0] = T
        label_lens = np.array([int(g.integers(0, min(max_l, l // 2) + 1)) for l in out_lens])
        label_lens[0] = min(max_l, T // 2)                              # the longest line carries the most labels (states per lane = template)
        targets = np.concatenate([g.integers(1, C, size=l) for l in label_lens] + [np.zeros(0, np.int64)])
        yield f'random{(N, T, C, max_l)}', probits, targets, out_lens, label_lens


def test_scores_on_random_logits():
    """Hard per line: feasibility, a valid alignment, the float64 score of the device's path and the device's own score within `tol` of
    the definition's.  The path itself on every line whose runner-up gap exceeds `tol`: 15 lines of these inputs (mixed 5 of 5, wide 3
    of 4, long 0 of 3, the random batches 1, 5, 0, 0, 1, 0)."""
    compared = same_anyway = others = infeasible = 0
    for name, probits, targets, out_lens, label_lens in _random_batches():
        got = _run(probits, out_lens, targets, label_lens)
        off = np.concatenate([[0], np.cumsum(label_lens)])
        worst_path = worst_score = worst_rel = 0.0
        n_cmp = 0
        for n in range(len(out_lens)):
            T, lab = int(out_lens[n]), np.asarray(targets[off[n]:off[n + 1]], dtype=np.int64)
            x = probits[n, :T].T
            want, s_star = A.viterbi_align(x, lab)
            records, score = got[n]
            if want is None:
                assert records is None and score == -np.inf, (name, n)
                infeasible += 1
                continue
            assert records is not None, (name, n)
            _check_valid(records, lab, T)
            lp = A.log_softmax64(x)
            tol = _tol(T, s_star)
            rescored = float(lp[_frame_classes(records, T), np.arange(T)].sum())
            gap_path, gap_score = s_star - rescored, abs(score - s_star)
            print(f'{name} line {n}: T {T} L {len(lab)} s* {s_star:.4f} tol {tol:.3g} path gap {gap_path:.3g} score gap {gap_score:.3g}')
            assert -1e-9 * max(1.0, abs(s_star)) <= gap_path <= tol, (name, n, gap_path, tol)
            assert gap_score <= tol, (name, n, gap_score, tol)
            worst_path, worst_score = max(worst_path, gap_path), max(worst_score, gap_score)
            worst_rel = max(worst_rel, gap_path / tol, gap_score / tol)
            same = [r[:3] for r in records] == [r[:3] for r in want]
            states, _ = A.viterbi_path(lp, lab)
            if T > 0 and _runner_up_gap(lp, lab, states) > tol:
                assert same, (name, n)
                n_cmp += 1
            else:
                same_anyway += int(same)
                others += 1
        compared += n_cmp
        _log('align_random_logits', {'case': name, 'path_gap': worst_path, 'score_gap': worst_score, 'worst_gap_over_tol': worst_rel,
                                     'paths_compared': n_cmp})
    print(f'paths compared {compared}; of the {others} other lines {same_anyway} have the same path; {infeasible} lines do not fit')
    assert infeasible == 1                                               # `mixed`: 6 labels in 4 frames
    assert compared >= 15


# ---- 3. greedy identity on the model ------------------------------------------------------------------------------------------------
def _net(tc, dtype):
    net = PytorchRecognitionModel(**tc.hp.as_dict(), **DROPS, codec=ascii_codec(tc.hp.num_classes), compute_dtype=dtype)
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    return net.to('cuda:0').eval()


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_own_greedy_string_aligns_to_the_greedy_records(text_case, dtype):
    """cfg2_text: `predict_labels` (greedy), then `align_labels` of those labels: the same (label, start, end).  fp32: on EVERY line --
    the premise (each line's smallest top-1 / top-2 margin, from the device's own logits, exceeds 2 tol) is asserted.  bf16: on every
    line whose smallest margin exceeds 2 tol; their number goes to parity.jsonl."""
    tc = text_case('cfg2_text')
    net = _net(tc, dtype)
    image, lens, idx = tc.batch(0)
    line, lens = torch.from_numpy(image).cuda(), torch.from_numpy(lens)
    greedy = net.predict_labels(line, lens)
    labels = [[r[0] for r in recs] for recs in greedy]
    aligned = net.align_labels(line, lens, [l for lab in labels for l in lab], [len(lab) for lab in labels])
    logits, out_lens = net.forward(line, lens)
    lg = logits.cpu().numpy()
    held = 0
    for n in range(len(idx)):
        T = int(out_lens[n])
        records, score = aligned[n]
        assert records is not None
        top2 = np.sort(lg[n, :T], axis=1)[:, -2:]
        margin = float((top2[:, 1] - top2[:, 0]).min())
        tol = _tol(T, score)
        print(f'{dtype} line {idx[n]}: score {score:.4f} tol {tol:.3g} smallest margin {margin:.4g}')
        if dtype == 'fp32':
            assert margin > 2 * tol, (n, margin, tol)
        if margin > 2 * tol:
            held += 1
            assert [r[:3] for r in records] == [r[:3] for r in greedy[n]], n
            s_def = A.viterbi_align(lg[n, :T].T, labels[n])[1]
            assert abs(score - s_def) <= tol
    _log('align_greedy_identity', {'dtype': dtype, 'lines': len(idx), 'lines_with_margin_over_2tol': held})
    if dtype == 'fp32':
        assert held == len(idx) == 32
        assert labels == [tc.ref_strings[i] for i in idx]
    # the ground truth of this fixture is what the reference reads: `align` on the strings gives the same records
    codec = net.codec
    strings = [''.join(codec.l2c[(l,)] for l in tc.texts[i]) for i in idx]
    by_text = net.align(line, lens, strings)
    for n, res in enumerate(by_text):
        assert res['frames'] == int(out_lens[n]) and res['skipped'] == ''
        if labels[n] == tc.texts[idx[n]]:
            assert [c[:3] for c in res['chars']] == [c[:3] for c in codec.decode(aligned[n][0])]
            assert abs(res['score'] - aligned[n][1]) <= _tol(res['frames'], res['score'])


# ---- 4. pages -----------------------------------------------------------------------------------------------------------------------
KINDS = [('line', 0.0), ('line', 7.0), ('arc', 2600.0, 1), ('line', -7.0), ('line', 15.0), ('line', 0.0), ('line', -15.0),
         ('arc', 2500.0, -1), ('line', 0.0), ('line', 3.0)]
# fixture lines the CPU oracle reads with a top-1 / top-2 margin >= 1 on every frame at those placements (tests/test_hip_page.py PICK)
PICK = [3, 4, 14, 7, 11, 12, 16, 22, 23, 6]
FIXTURE_FORM = dict(pad=0, edge=1200)


def test_pages_aligned_to_the_strings_they_were_read_as(text_case, tmp_path, capsys):
    from PIL import Image
    tc = text_case('cfg2_text')
    lines = [np.rint(tc.lines[i] * 255.0).astype(np.uint8) for i in PICK]
    page, placed = page_synth.text_page(lines, KINDS)
    page_lines = [Line(f'line{k}', P, B) for k, (_, P, B) in enumerate(placed)]
    net = _net(tc, 'bf16')
    read, = recognize_pages(net, [(page, page_lines)], batch_size=4, **FIXTURE_FORM)
    with_text = [Line(l.id, l.baseline, l.boundary, r['text']) for l, r in zip(page_lines, read)]
    with_text.append(Line('untranscribed', page_lines[0].baseline, page_lines[0].boundary, None))
    got, = A.align_pages(net, [(page, with_text)], batch_size=4, **FIXTURE_FORM)
    assert [g['id'] for g in got] == [l.id for l in with_text]
    for g, r in zip(got, read):
        assert g['text'] == r['text'] and g['skipped'] == '' and g['frames'] > 0 and np.isfinite(g['score']) and g['score'] < 0
        assert [(c, q) for c, q, _ in g['cuts']] == [(c, q) for c, q, _ in r['cuts']]
        # words: the runs between spaces, from the first character's left edge to the last one's right edge
        runs, run = [], []
        for cut in g['cuts'] + [(' ', None, None)]:
            if cut[0] == ' ':
                if run:
                    runs.append(run)
                run = []
            else:
                run.append(cut)
        assert [w[0] for w in g['words']] == [''.join(c[0] for c in run) for run in runs] and runs
        for w, run in zip(g['words'], runs):
            assert w[1] == [run[0][1][0], run[-1][1][1], run[-1][1][2], run[0][1][3]]
            assert w[2] == min(c[2] for c in run)
    last = got[-1]
    assert last['cuts'] is None and last['score'] is None and last['words'] == [] and last['text'] is None

    # the command on the same page
    Image.fromarray(page).save(tmp_path / 'scan.png')
    pts = lambda a: ' '.join(f'{x:.3f},{y:.3f}' for x, y in a)
    body = ''.join(f'<TextLine id="{l.id}"><Coords points="{pts(l.boundary)}"/><Baseline points="{pts(l.baseline)}"/>'
                   + (f'<TextEquiv><Unicode>{escape(l.text)}</Unicode></TextEquiv>' if l.text is not None else '') + '</TextLine>\n'
                   for l in with_text)
    (tmp_path / 'scan.xml').write_text('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2019-07-15">'
                                       f'<Page imageFilename="scan.png"><TextRegion id="r">{body}</TextRegion></Page></PcGts>\n', encoding='utf-8')
    src = PytorchRecognitionModel(**tc.hp.as_dict(), **DROPS, codec=ascii_codec(tc.hp.num_classes))
    src.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    save_safetensors(src, tmp_path / 'model.tar')
    capsys.readouterr()
    out = tmp_path / 'out.json'
    assert A.main(['-m', str(tmp_path / 'model.tar'), '-f', 'page', '-i', str(tmp_path / 'scan.xml'), str(out), '--pad', '0', '--edge', '1200',
                   '--batch-size', '4', '--worst', '3']) == 0
    err = capsys.readouterr().err
    assert f'{len(read)} lines aligned, 0 do not fit, 0 with skipped characters' in err
    assert len([l for l in err.splitlines() if 'scan.xml' in l and 'line' in l]) == 3          # --worst 3
    with open(out, encoding='utf-8') as fp:
        back = json.load(fp)
    # the file's coordinates are rounded to 3 decimals: the command is held to `align_pages` on the lines as the file gives them
    from conformer_ocr_amd.page import read_page_xml
    want, = A.align_pages(net, [(page, read_page_xml(tmp_path / 'scan.xml').lines)], batch_size=4, **FIXTURE_FORM)
    assert [b['id'] for b in back] == [l.id for l in with_text] == [w['id'] for w in want]
    for b, w, g in zip(back, want, got):
        assert b['text'] == w['text'] == g['text'] and b['frames'] == w['frames'] and b['skipped'] == w['skipped']
        if w['cuts'] is None:
            assert b['cuts'] is None and b['score'] is None and b['words'] == []
        else:
            assert abs(b['score'] - w['score']) <= _tol(w['frames'], w['score'])
            assert [(c, [list(p) for p in q]) for c, q, _ in w['cuts']] == [(c, q) for c, q, _ in b['cuts']]
            assert [(t, [list(p) for p in q]) for t, q, _ in w['words']] == [(t, q) for t, q, _ in b['words']]
            assert [c for c, _, _ in b['cuts']] == [c for c, _, _ in g['cuts']]


# ---- 5 - 8 --------------------------------------------------------------------------------------------------------------------------
def test_edge_lines():
    C = 5
    logits = np.random.default_rng(1).standard_normal((5, 6, C)).astype(np.float32)
    #            empty target   no frames+labels  no frames, no labels   'aa' in 2 frames (infeasible)   'aa' in 3 frames (one path)
    out_lens = [6, 0, 0, 2, 3]
    label_lens = [0, 2, 0, 2, 2]
    targets = [3, 4, 1, 1, 2, 2]
    eng = _engine()
    d_logits = torch.from_numpy(logits).cuda()
    h = eng.ctc_align_async(d_logits, out_lens, targets, label_lens)
    got = eng.collect_align(h)
    assert h[1][3].numpy().tolist() == [0, -1, 0, -1, 2]                 # counts
    lp0 = A.log_softmax64(logits[0].T)
    assert got[0][0] == [] and abs(got[0][1] - lp0[0].sum()) < 1e-4
    assert got[1] == (None, -np.inf) and got[3] == (None, -np.inf)
    assert got[2] == ([], 0.0)
    want, s = A.viterbi_align(logits[4, :3].T, [2, 2])
    assert [r[:3] for r in got[4][0]] == [(2, 0, 0), (2, 2, 2)] == [r[:3] for r in want]
    assert abs(got[4][1] - s) < 1e-5
    np.testing.assert_allclose([r[3] for r in got[4][0]], [r[3] for r in want], atol=1e-5)


def test_runs_are_bitwise_reproducible():
    d = np.load(GOLD)
    args = (d['long.probits'], d['long.out_lens'], d['long.targets'], d['long.label_lens'])
    assert _run(*args) == _run(*args)


def test_argument_errors(text_case):
    eng = _engine()
    p = torch.zeros((1, 4, 3), device='cuda')
    with pytest.raises(ValueError):
        eng.ctc_align(p, [4], [3], [1])             # label outside [1, ncls)
    with pytest.raises(ValueError):
        eng.ctc_align(p, [4], [0], [1])             # blank as a label
    with pytest.raises(ValueError):
        eng.ctc_align(p, [5], [1], [1])             # more valid frames than frames
    with pytest.raises(ValueError):
        eng.ctc_align(p, [4], [1, 2], [1])          # targets / label_lens disagree
    long_line = [1, 2] * 128
    with pytest.raises(ValueError):
        eng.ctc_align(torch.zeros((1, 600, 3), device='cuda'), [600], long_line, [256])
    assert eng.ctc_align(p, [4], [1], [1])[0][0] is not None            # the engine is still usable
    # the model-level call takes such a line through the definition
    tc = text_case('cfg2_text')
    net = _net(tc, 'fp32')
    image, lens, idx = tc.batch(0)
    line, lens = torch.from_numpy(image[:2]).cuda(), torch.from_numpy(lens[:2])
    short = tc.ref_strings[idx[1]]
    got = net.align_labels(line, lens, long_line + short, [256, len(short)])
    logits, out_lens = net.forward(line, lens)
    want = A.viterbi_align(logits[0, :int(out_lens[0])].T.cpu().numpy(), long_line)
    assert want[0] is not None and len(got[0][0]) == 256
    assert [r[:3] for r in got[0][0]] == [r[:3] for r in want[0]] and abs(got[0][1] - want[1]) < 1e-6 * abs(want[1])
    assert [r[0] for r in got[1][0]] == short


def test_greedy_shortcut_is_not_disturbed(text_case):
    """`ctc_align` between a forward and its `ctc_greedy`: the decoder epilogue's per-frame argmax still belongs to the logits."""
    tc = text_case('cfg2_text')
    net = _net(tc, 'bf16')
    image, lens, idx = tc.batch(0)
    line = torch.from_numpy(image[:8]).cuda().squeeze(1)
    eng = net.engine(torch.device('cuda', 0))
    logits, out_lens = eng.forward(line, lens[:8])
    assert eng._argmax_is_fresh(logits)
    labels = [tc.ref_strings[i] for i in idx[:8]]
    aligned = eng.ctc_align(logits, out_lens, [l for lab in labels for l in lab], [len(lab) for lab in labels])
    assert all(r is not None for r, _ in aligned)
    assert eng._argmax_is_fresh(logits)
    after = eng.ctc_greedy(logits, out_lens)
    logits2, out_lens2 = eng.forward(line, lens[:8])
    assert eng.ctc_greedy(logits2, out_lens2) == after
    assert eng.ctc_greedy(logits.clone(), out_lens) == after              # from the values, without the shortcut
