"""CPU: the definition of forced alignment (conformer_ocr_amd/align.py `viterbi_align`) against an enumeration
of every lattice path, its tie rule on hand-made cases, the greedy identity (a line's own greedy string aligns to the frame-wise argmax
path) on random logits and on the metric's fixture through the CPU oracle, the text / word plumbing, and the command's argument errors."""
import numpy as np
import torch

from conformer_ocr_amd import align as A
from conformer_ocr_amd.codec import PytorchCodec
from oracle import ctc_ref
from oracle.conformer_ref import Oracle


def _all_paths(lp, labels):
    """Every path of the lattice: (score, states), best first.  lp (C, T)."""
    T = lp.shape[1]
    S = 2 * len(labels) + 1
    ext = [0] * S
    ext[1::2] = [int(l) for l in labels]
    found = []

    def walk(path, score):
        t = len(path)
        if t == T:
            if path[-1] >= S - 2:
                found.append((score, tuple(path)))
            return
        if t == 0:
            nxt = [0, 1]
        else:
            s = path[-1]
            nxt = [s, s + 1]
            if (s + 2) % 2 == 1 and s + 2 < S and ext[s + 2] != ext[s]:
                nxt.append(s + 2)
        for ns in nxt:
            if ns < S:
                walk(path + [ns], score + lp[ext[ns], t])
    walk([], 0.0)
    return sorted(found, key=lambda f: -f[0])


def test_against_every_path_of_the_lattice():
    g = np.random.default_rng(5)
    feasible = infeasible = 0
    closest = np.inf
    for _ in range(200):
        T, C = int(g.integers(1, 8)), 4
        L = int(g.integers(0, 4))
        lab = g.integers(1, C, size=L)
        x = g.standard_normal((T, C)) * 2
        lp = A.log_softmax64(x.T)
        paths = _all_paths(lp, lab)
        records, score = A.viterbi_align(x.T, lab)
        states, score_p = A.viterbi_path(lp, lab)
        if not paths:
            assert records is None and score == -np.inf and states is None
            assert T < L + int((lab[1:] == lab[:-1]).sum())
            infeasible += 1
            continue
        feasible += 1
        assert abs(score - paths[0][0]) <= 1e-12 and score == score_p
        assert tuple(states.tolist()) == paths[0][1]
        if len(paths) > 1:
            closest = min(closest, paths[0][0] - paths[1][0])
        assert [r[0] for r in records] == lab.tolist()
        for k, (l, st, en, cf) in enumerate(records):
            on = [t for t, s in enumerate(paths[0][1]) if s == 2 * k + 1]
            assert (st, en) == (on[0], on[-1])
            assert abs(cf - np.exp(lp[l, st:en + 1].max())) < 1e-15
    assert feasible > 100 and infeasible > 0
    assert closest > 1e-3                           # ties play no part in these draws


def test_tie_rule():
    """All logits equal: every path scores the same and the rule alone decides -- a candidate replaces the running best only if strictly
    greater, in the order stay, s-1, s-2; the path ends in the last blank unless the last label is strictly better.  Derived by hand:
    [1] in 3 frames: frame 1 reaches state 2 only from state 1, frame 2 stays there (tie), the end is state 2: states 1 2 2.
    [1, 1] in 3 frames: the one path 1 2 3.
    [1, 2] in 4 frames: state 3 is first reached at frame 1 by the skip from 1, state 4 at frame 2 from 3, then stays: 1 3 4 4."""
    for labels, T, want_states, want in [([1], 3, [1, 2, 2], [(1, 0, 0)]),
                                         ([1, 1], 3, [1, 2, 3], [(1, 0, 0), (1, 2, 2)]),
                                         ([1, 2], 4, [1, 3, 4, 4], [(1, 0, 0), (2, 1, 1)])]:
        x = np.zeros((3, T))
        states, _ = A.viterbi_path(A.log_softmax64(x), labels)
        assert states.tolist() == want_states
        records, score = A.viterbi_align(x, labels)
        assert [r[:3] for r in records] == want
        assert abs(score - T * np.log(1 / 3)) < 1e-12
        assert all(abs(r[3] - 1 / 3) < 1e-12 for r in records)


def test_degenerate_lines():
    x = np.random.default_rng(0).standard_normal((4, 5))
    lp = A.log_softmax64(x)
    records, score = A.viterbi_align(x, [])
    assert records == [] and abs(score - lp[0].sum()) < 1e-12
    assert A.viterbi_align(np.zeros((4, 0)), []) == ([], 0.0)
    assert A.viterbi_align(np.zeros((4, 0)), [2]) == (None, -np.inf)
    assert A.viterbi_align(x[:, :2], [1, 1]) == (None, -np.inf)           # a repeat needs a blank between: 3 frames
    assert A.viterbi_align(x[:, :3], [1, 1])[0] is not None
    for bad in ([0], [4], [-1]):
        try:
            A.viterbi_align(x, bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_own_greedy_string_aligns_to_the_argmax_path():
    """The frame-wise argmax path is the best path over all label sequences, hence the best among the alignments of its own string."""
    g = np.random.default_rng(21)
    for _ in range(40):
        C, T = int(g.integers(2, 12)), int(g.integers(1, 60))
        x = (g.standard_normal((C, T)) * 3).astype(np.float32)
        x[0] += float(g.integers(0, 3))                                    # some lines with long blank runs
        greedy = ctc_ref.greedy_decoder(x)
        records, score = A.viterbi_align(x, [r[0] for r in greedy])
        assert [r[:3] for r in records] == [tuple(int(v) for v in r[:3]) for r in greedy]
        assert abs(score - A.log_softmax64(x).max(axis=0).sum()) < 1e-9


def test_text_and_word_plumbing():
    codec = PytorchCodec({'a': [1], 'ß': [2, 3], ' ': [4]})
    text = 'a ßxa'
    labels, skipped = A.encode_text(codec, text)
    assert labels == [1, 4, 2, 3, 1] and skipped == 'x'
    frames = [1, 1, 0, 4, 2, 3, 3, 0, 1]                                   # a a _ ' ' ß ß ß _ a
    x = np.random.default_rng(2).standard_normal((5, len(frames)))
    x[frames, np.arange(len(frames))] += 8.0
    res = A.align_text(codec, x, text)
    assert res['frames'] == 9 and res['skipped'] == 'x' and res['score'] < 0
    assert [c[:3] for c in res['chars']] == [('a', 0, 1), (' ', 3, 3), ('ß', 4, 6), ('a', 8, 8)]      # the two labels of 'ß' merged by decode
    lp = A.log_softmax64(x)
    assert abs(res['chars'][2][3] - np.exp(max(lp[2, 4], lp[3, 5:7].max()))) < 1e-12
    assert A.align_text(codec, x[:, :4], text)['chars'] is None            # 5 labels in 4 frames
    assert A.align_text(codec, x[:, :4], text)['score'] == -np.inf

    def quad(x0, x1):
        return [(x0, 0.0), (x1, 0.0), (x1, 10.0), (x0, 10.0)]
    cuts = [(c, quad(10.0 * st, 10.0 * (en + 1)), cf) for c, st, en, cf in res['chars']]
    words = A.word_records(cuts)
    assert [w[0] for w in words] == ['a', 'ßa']
    assert words[0][1] == quad(0.0, 20.0) and words[1][1] == quad(40.0, 90.0)
    assert words[1][2] == min(cuts[2][2], cuts[3][2])
    assert A.word_records(None) == [] and A.word_records([]) == []
    assert [w[0] for w in A.word_records([(' ', quad(0, 1), 1.0), ('a', quad(1, 2), 0.5), (' ', quad(2, 3), 1.0)])] == ['a']


def test_command_argument_errors(tmp_path, capsys):
    xml = tmp_path / 'page.xml'
    xml.write_text('<?xml version="1.0"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2019-07-15">'
                   '<Page imageFilename="scan.png"><TextRegion id="r"><TextLine id="l0"><Coords points="0,0 100,0 100,50 0,50"/>'
                   '<Baseline points="0,40 100,40"/></TextLine></TextRegion></Page></PcGts>\n')
    model = tmp_path / 'model.tar'
    model.write_bytes(b'')
    assert A.main(['-i', str(xml), str(tmp_path / 'out.json')]) == 1
    assert 'usage' in capsys.readouterr().err and not (tmp_path / 'out.json').exists()
    assert A.main(['-m', str(model)]) == 1
    assert 'usage' in capsys.readouterr().err
    assert A.main(['-m', str(model), '-i', str(xml), str(tmp_path / 'out.json')]) == 1                # no line with text
    err = capsys.readouterr().err
    assert 'usage' in err and 'no line with text' in err and not (tmp_path / 'out.json').exists()
    assert A.main(['-m', str(tmp_path / 'absent.tar'), '-i', str(xml), str(tmp_path / 'out.json')]) == 1
    assert 'no such file' in capsys.readouterr().err


def test_greedy_identity_on_the_metric_fixture(text_case):
    """cfg2_text, all 32 lines, through the CPU oracle (float32): each line's frame-wise argmax string, aligned, gives the argmax path.
    The premise is asserted: the smallest top-1 / top-2 margin of every line exceeds twice the float32 bound on the score."""
    tc = text_case('cfg2_text')
    image, lens, idx = tc.batch(0)
    assert len(idx) == 32
    with torch.no_grad():
        logits, ol = Oracle(tc.hp, tc.state).forward(torch.from_numpy(image), torch.from_numpy(lens))
    for k, i in enumerate(idx):
        T = int(ol[k])
        x = logits[k, :T].numpy().T                                        # (C, T)
        greedy = ctc_ref.greedy_decoder(x)
        labels = [int(r[0]) for r in greedy]
        assert labels == tc.ref_strings[i]
        lp = A.log_softmax64(x)
        states, score = A.viterbi_path(lp, labels)
        ext = np.zeros(2 * len(labels) + 1, dtype=np.int64)
        ext[1::2] = labels
        np.testing.assert_array_equal(ext[states], x.argmax(axis=0))
        records, score2 = A.viterbi_align(x, labels)
        assert score2 == score
        assert [r[:3] for r in records] == [tuple(int(v) for v in r[:3]) for r in greedy]
        top2 = np.sort(x, axis=0)[-2:]
        tol = 8 * T * 2.0 ** -23 * max(1.0, abs(score))
        assert float((top2[1] - top2[0]).min()) > 2 * tol
