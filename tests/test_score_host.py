"""Host side of the GPU scorer (conformer_ocr_amd/score.py) and of the `test` command, no device needed: packing, the numpy tallies against
evaluate.compute_confusions / render_report, argument handling."""
import numpy as np
import pytest

from conformer_ocr_amd import score
from conformer_ocr_amd.evaluate import ErrorRate, compute_confusions, global_align, render_report

MIXED = 'abcdeé ABC' + 'αβγδ' + 'אבגד' + 'é' + '\U0001d538\U0001f600'


def _ops(truths, preds):
    """Ops derived from evaluate.global_align's own output, and the aligned symbol lists compute_confusions takes."""
    ops, algn_gt, algn_pred = [], [], []
    for t, p in zip(truths, preds):
        _, a1, a2 = global_align(t, p)
        ops.append(score.ops_from_alignment(a1, a2))
        algn_gt.extend(a1)
        algn_pred.extend(a2)
    return (np.concatenate(ops) if ops else np.zeros(0, dtype=np.uint8)), algn_gt, algn_pred


def _perturb(g, text, alphabet, rate):
    out = []
    for c in text:
        r = g.random()
        if r < rate:
            continue
        out.append(alphabet[int(g.integers(len(alphabet)))] if r < 2 * rate else c)
        if r > 1 - rate:
            out.append(alphabet[int(g.integers(len(alphabet)))])
    return ''.join(out)


def _lines(g, n, alphabet, rate, lo=0, hi=40):
    truths = [''.join(alphabet[int(k)] for k in g.integers(0, len(alphabet), int(g.integers(lo, hi)))) for _ in range(n)]
    return truths, [_perturb(g, t, alphabet, rate) for t in truths]


def _check_tally(truths, preds):
    ops, algn_gt, algn_pred = _ops(truths, preds)
    a, _ = score.pack(truths)
    b, _ = score.pack(preds)
    got = score.tally(a, b, ops)
    want = compute_confusions(algn_gt, algn_pred)
    for g, w, name in zip(got, want, ('confusions', 'scripts', 'ins', 'dels', 'subs')):
        assert g == w, name
        if isinstance(w, dict):
            assert list(g.items()) == list(w.items()), name + ' (order)'
    assert render_report('m', 10, 3, 0.7, 0.5, *got) == render_report('m', 10, 3, 0.7, 0.5, *want)
    return got


def test_pack_round_trip():
    strings = ['', 'abc', '\U0001d538x\U0001f600', 'éé', '  a \t b  c  ', '', 'אב αβ']
    cps, offs = score.pack(strings)
    assert cps.dtype == np.int32 and offs.dtype == np.int64
    assert offs.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in strings])]).tolist()
    assert cps.tolist() == [ord(c) for s in strings for c in s]
    assert score.unpack(cps, offs) == strings
    cps, offs = score.pack([])
    assert cps.shape == (0,) and offs.tolist() == [0]
    assert score.pack(['', ''])[1].tolist() == [0, 0, 0]


def test_pack_words_splits_like_error_rate():
    truths = ['the  quick\tbrown fox', '', '   ', 'a b a', 'x y z']
    preds = ['the quick brown  fax ', 'extra', '', 'a a b', 'x y']
    a, a_offs, b, b_offs, table = score.pack_words(preds, truths)
    assert [[table[i] for i in a[a_offs[k]:a_offs[k + 1]]] for k in range(len(truths))] == [t.split() for t in truths]
    assert [[table[i] for i in b[b_offs[k]:b_offs[k + 1]]] for k in range(len(preds))] == [p.split() for p in preds]
    assert len(set(table)) == len(table)
    counts, _, _ = score.align_pairs(None, a, a_offs, b, b_offs)
    wer = ErrorRate(True)
    wer.update(preds, truths)
    assert int(counts[:, 0].sum()) == wer.errors and int(a_offs[-1]) == wer.total


def test_align_pairs_on_the_host_equals_global_align():
    g = np.random.default_rng(1)
    truths, preds = _lines(g, 60, 'ab', 0.1)
    a, a_offs = score.pack(truths)
    b, b_offs = score.pack(preds)
    counts, ops, offs = score.align_pairs(None, a, a_offs, b, b_offs, want_ops=True)
    want, _, _ = _ops(truths, preds)
    assert np.array_equal(ops, want)
    for k, (t, p) in enumerate(zip(truths, preds)):
        o = ops[offs[k]:offs[k + 1]]
        assert counts[k].tolist() == [global_align(t, p)[0], int((o == 3).sum()), int((o == 2).sum()), int((o == 1).sum())]


@pytest.mark.parametrize('seed', [0, 1])
def test_tallies_equal_compute_confusions_on_three_letters(seed):
    g = np.random.default_rng(seed)
    truths, preds = _lines(g, 300, 'abc', 0.08)
    got = _check_tally(truths, preds)
    assert len(got[0]) >= 10 and got[3] > 0


def test_tallies_equal_compute_confusions_on_mixed_scripts():
    g = np.random.default_rng(7)
    truths, preds = _lines(g, 300, MIXED, 0.06, lo=5, hi=60)
    got = _check_tally(truths, preds)
    assert len(got[0]) > 100 and len(got[1]) >= 4          # many distinct confusions, Latin / Greek / Hebrew / Combining / ...


def test_tallies_order_more_than_thirty_confusions_of_equal_count():
    """Forty distinct substitutions, each once (then two of them twice): the report shows the first thirty, so the order of first
    occurrence among equal counts decides its text."""
    gt = [chr(0x100 + (k * 7) % 40) + chr(0x3b1 + k % 20) for k in range(40)]          # Latin Extended-A against Cyrillic, a Greek letter kept
    pr = [chr(0x410 + (k * 7) % 40) + chr(0x3b1 + k % 20) for k in range(40)]
    got = _check_tally(gt, pr)
    assert len(got[0]) > 30 and set(got[0].values()) == {1}
    got = _check_tally(gt + gt[35:37], pr + pr[35:37])
    assert list(got[0].values())[:3] == [2, 2, 1]


def test_tallies_of_nothing_and_of_gaps_only():
    _check_tally([], [])
    _check_tally(['', 'abc', ''], ['xy', '', ''])


def test_score_on_the_host_equals_the_error_rates():
    g = np.random.default_rng(3)
    truths, preds = _lines(g, 50, 'ab cd', 0.1, lo=0, hi=50)
    s = score.score(None, preds, truths, report=True)
    cer, wer = ErrorRate(False), ErrorRate(True)
    cer.update(preds, truths)
    wer.update(preds, truths)
    assert (s['char_errors'], s['chars'], s['word_errors'], s['words']) == (cer.errors, cer.total, wer.errors, wer.total)
    _, algn_gt, algn_pred = _ops(truths, preds)
    assert s['tallies'] == compute_confusions(algn_gt, algn_pred)


def test_use_device(monkeypatch):
    monkeypatch.delenv('COCR_HOST_SCORE', raising=False)
    eng = object()
    assert score.use_device(None, eng) and score.use_device('device', eng)
    assert not score.use_device('host', eng) and not score.use_device(None, None)
    with pytest.raises(RuntimeError):
        score.use_device('device', None)
    with pytest.raises(ValueError):
        score.use_device('gpu', eng)
    monkeypatch.setenv('COCR_HOST_SCORE', '1')
    assert not score.use_device(None, eng) and score.use_device('device', eng)


# ---- the command's argument handling ------------------------------------------------------------------------------------------
def test_command_defaults():
    from conformer_ocr_amd import test as cmd
    args = cmd.parser().parse_args(['-m', 'a.safetensors', 'x.xml'])
    assert args.model == ['a.safetensors'] and args.test_set == ['x.xml'] and args.evaluation_files == []
    assert (args.batch_size, args.pad, args.normalization, args.normalize_whitespace, args.format_type) == (32, 16, None, True, 'path')
    assert (args.device, args.edge, args.scorer) == ('cuda:0', 200, 'device')
    args = cmd.parser().parse_args(['-m', 'a', '-m', 'b', '-f', 'alto', '-u', 'NFC', '--no-normalize-whitespace', '-B', '8', '--scorer', 'host'])
    assert args.model == ['a', 'b'] and args.format_type == 'alto' and args.normalization == 'NFC' and not args.normalize_whitespace
    assert args.batch_size == 8 and args.scorer == 'host'
    with pytest.raises(SystemExit):
        cmd.parser().parse_args(['-m', 'a', '-f', 'binary', 'x'])
    assert 'python-bidi' in cmd.parser().format_help()


def test_command_expands_manifests_and_globs(tmp_path):
    from conformer_ocr_amd import test as cmd
    for name in ('p2.xml', 'p1.xml', 'q.xml'):
        (tmp_path / name).write_text('<x/>')
    (tmp_path / 'list.txt').write_text(f'{tmp_path}/q.xml\n\n  {tmp_path}/p1.xml  \n')
    args = cmd.parser().parse_args(['-m', 'a', '-e', str(tmp_path / 'list.txt'), str(tmp_path / 'p*.xml'), str(tmp_path / 'none*.xml')])
    assert cmd.gather_files(args) == [f'{tmp_path}/p1.xml', f'{tmp_path}/p2.xml', f'{tmp_path}/none*.xml', f'{tmp_path}/q.xml', f'{tmp_path}/p1.xml']


def test_command_error_exits(tmp_path, capsys):
    from conformer_ocr_amd import test as cmd
    assert cmd.main(['x.xml']) == 1
    assert 'No model to evaluate given.' in capsys.readouterr().err
    model = tmp_path / 'm.safetensors'
    model.write_bytes(b'')
    assert cmd.main(['-m', str(model)]) == 1
    assert 'No evaluation data' in capsys.readouterr().err
    assert cmd.main(['-m', str(model), str(tmp_path / 'missing.png')]) == 1
    assert 'no such file' in capsys.readouterr().err
    (tmp_path / 'line.png').write_bytes(b'')
    (tmp_path / 'line.gt.txt').write_text(' \n')
    with pytest.warns(UserWarning, match='empty ground truth'):
        assert cmd.main(['-m', str(model), str(tmp_path / 'line.png')]) == 1
    err = capsys.readouterr().err
    assert 'usage:' in err and 'no usable line' in err
