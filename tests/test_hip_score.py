"""Scoring on the GPU: cocr_edit_align (csrc/score.hip.h) against evaluate.global_align / edit_distance -- counts and
alignment ops exactly equal --, evaluate / validate / GroundTruthDataset.validate with the device scorer against the host scorer, and the
command `python -m conformer_ocr_amd.test`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conformer_ocr_amd import score, synth
from conformer_ocr_amd.evaluate import edit_distance, global_align

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def eng():
    from conformer_ocr_amd.engine import HipRecognizer
    return HipRecognizer(synth.hparams('tiny'), torch.device('cuda:0'), 'fp32')


def _pack(seqs):
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    flat = np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs]) if offs[-1] else np.zeros(0, dtype=np.int32)
    return flat.astype(np.int32), offs


def _host(sa, sb):
    cost, al1, al2 = global_align(list(sa), list(sb))
    ops = score.ops_from_alignment(al1, al2)
    assert cost == edit_distance(list(sa), list(sb))
    return [cost, int((ops == 3).sum()), int((ops == 2).sum()), int((ops == 1).sum())], ops


def _check(eng, pairs):
    """Raw entry point on `pairs` of (a, b) symbol lists: counts and ops equal the host definition's; returns the raw outputs."""
    a, a_offs = _pack([p[0] for p in pairs])
    b, b_offs = _pack([p[1] for p in pairs])
    counts, raw, used = eng.edit_align(a, a_offs, b, b_offs, want_ops=True)
    only, _, _ = eng.edit_align(a, a_offs, b, b_offs, want_ops=False)
    assert np.array_equal(only, counts)
    for k, (sa, sb) in enumerate(pairs):
        want_counts, want_ops = _host(sa, sb)
        end = int(a_offs[k + 1] + b_offs[k + 1])
        got = raw[end - int(used[k]):end]
        assert counts[k].tolist() == want_counts, (k, len(sa), len(sb), counts[k].tolist(), want_counts)
        assert used[k] == want_ops.shape[0] and np.array_equal(got, want_ops), \
            (k, len(sa), len(sb), int(np.argmax(got != want_ops)) if used[k] == want_ops.shape[0] else (int(used[k]), want_ops.shape[0]))
    return counts, raw, used


def _edited(g, n, m, alphabet):
    """A sequence of n symbols and a copy with a few per cent of edits, cut or filled to m symbols."""
    a = g.integers(0, alphabet, n).tolist()
    b = []
    for x in a:
        r = g.random()
        if r < 0.03:
            continue
        b.append(int(g.integers(0, alphabet)) if r < 0.06 else x)
        if r > 0.97:
            b.append(int(g.integers(0, alphabet)))
    b = b[:m] + g.integers(0, alphabet, max(0, m - len(b))).tolist()
    return a, b


@pytest.mark.timeout(600)
def test_kernel_equals_global_align_on_the_length_cases(eng):
    g = np.random.default_rng(5)
    shapes = [(0, 0), (0, 5), (5, 0), (1, 1), (63, 64), (64, 64), (65, 63), (300, 310), (1000, 900), (4096, 1)]
    pairs = [_edited(g, n, m, 30) for n, m in shapes]
    _check(eng, pairs)
    # both placements of the op-code table were used
    place = [eng.edit_align_lds(n, m) for n, m in shapes]
    assert place[shapes.index((300, 310))] > 0 and place[shapes.index((64, 64))] > 0
    assert place[shapes.index((1000, 900))] == 0


@pytest.mark.timeout(900)
def test_kernel_equals_global_align_on_4096_by_4096(eng):
    g = np.random.default_rng(6)
    assert eng.edit_align_lds(4096, 4096) == 0
    _check(eng, [_edited(g, 4096, 4096, 50), ([1, 2, 3], [1, 3])])


@pytest.mark.timeout(600)
@pytest.mark.parametrize('alphabet', [2, 1000])
def test_kernel_equals_global_align_on_random_pairs(eng, alphabet):
    """Two letters: many paths of equal cost, so this is the tie-breaking test."""
    g = np.random.default_rng(alphabet)
    pairs = []
    for k in range(300):
        n, m = int(g.integers(0, 201)), int(g.integers(0, 201))
        pairs.append(_edited(g, n, m, alphabet) if k % 2 else (g.integers(0, alphabet, n).tolist(), g.integers(0, alphabet, m).tolist()))
    r1 = _check(eng, pairs)
    a, a_offs = _pack([p[0] for p in pairs])
    b, b_offs = _pack([p[1] for p in pairs])
    r2 = eng.edit_align(a, a_offs, b, b_offs, want_ops=True)
    c1, ops1, _ = score.align_pairs(eng, a, a_offs, b, b_offs, want_ops=True)
    c2, ops2, _ = score.align_pairs(eng, a, a_offs, b, b_offs, want_ops=True)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[2], r2[2])
    assert np.array_equal(c1, c2) and ops1.tobytes() == ops2.tobytes()           # the same call twice: identical bytes
    lds = [eng.edit_align_lds(len(x), len(y)) for x, y in pairs]
    assert min(lds) > 0 and max(lds) > 8 * 1024 and min(lds) <= 2 * 1024       # three LDS classes in one call


@pytest.mark.timeout(600)
def test_the_workspace_placement_runs_the_same_code_on_short_pairs(monkeypatch):
    """COCR_SCORE_LDS_MAX=0: every pair's op-code table in the global workspace, several pairs per workgroup."""
    from conformer_ocr_amd.engine import HipRecognizer
    monkeypatch.setenv('COCR_SCORE_LDS_MAX', '0')
    e2 = HipRecognizer(synth.hparams('tiny'), torch.device('cuda:0'), 'fp32')
    g = np.random.default_rng(9)
    pairs = [_edited(g, int(g.integers(0, 150)), int(g.integers(0, 150)), 2) for _ in range(100)]
    assert all(e2.edit_align_lds(len(x), len(y)) == 0 for x, y in pairs)
    _check(e2, pairs)


@pytest.mark.timeout(600)
def test_limits(eng):
    a, a_offs = _pack([[1] * 4097, [1, 2]])
    b, b_offs = _pack([[1, 2, 1], [2]])
    with pytest.raises(ValueError):
        eng.edit_align(a, a_offs, b, b_offs)
    with pytest.raises(ValueError):
        eng.edit_align(b, b_offs, a, a_offs, want_ops=True)
    with pytest.raises(ValueError):
        eng.edit_align(a[:10], np.array([0, 7, 5, 10]), a[:10], np.array([0, 3, 6, 10]))
    counts, raw, used = eng.edit_align(a[:0], np.zeros(1, dtype=np.int64), a[:0], np.zeros(1, dtype=np.int64), want_ops=True)
    assert counts.shape == (0, 4) and raw.shape == (0,) and used.shape == (0,)
    # the same pairs through score.align_pairs: the long one is scored by the host functions and merged in
    counts, ops, offs = score.align_pairs(eng, a, a_offs, b, b_offs, want_ops=True)
    for k, (sa, sb) in enumerate([([1] * 4097, [1, 2, 1]), ([1, 2], [2])]):
        want_counts, want_ops = _host(sa, sb)
        assert counts[k].tolist() == want_counts
        assert np.array_equal(ops[offs[k]:offs[k + 1]], want_ops)


# ---- the callers: evaluate / validate / GroundTruthDataset.validate ----------------------------------------------------------------
DROPS = dict(input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1)


def _model(hp, state, codec, dtype='bf16'):
    from conformer_ocr_amd.pred import PytorchRecognitionModel
    net = PytorchRecognitionModel(**hp.as_dict(), **DROPS, codec=codec, compute_dtype=dtype)
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return net.to('cuda:0').eval()


def _same(dev, host):
    assert list(dev) == list(host)
    for k in host:
        assert dev[k] == host[k], k
        if isinstance(host[k], dict):
            assert list(dev[k].items()) == list(host[k].items()), k


@pytest.mark.timeout(600)
def test_evaluate_with_the_device_scorer_equals_the_host_scorer(text_case, monkeypatch):
    from conformer_ocr_amd.codec import ascii_codec
    from conformer_ocr_amd.evaluate import evaluate
    monkeypatch.delenv('COCR_HOST_SCORE', raising=False)
    tc = text_case('cfg2_text')
    codec = ascii_codec(tc.hp.num_classes)
    net = _model(tc.hp, tc.state, codec)
    g = np.random.default_rng(2)
    truths = []
    for i, labels in enumerate(tc.texts):
        t = [codec.l2c[(l,)] for l in labels]
        for _ in range(i % 4):                                 # every fourth line stays as it is
            k = int(g.integers(0, len(t)))
            r = g.random()
            if r < 0.4:
                t[k] = ' '
            elif r < 0.7:
                del t[k]
            else:
                t.insert(k, 'é')
        truths.append(''.join(t))
    host = evaluate(net, tc.lines, truths, report=True, model_name='m', scorer='host', batch_size=32)
    dev = evaluate(net, tc.lines, truths, report=True, model_name='m', batch_size=32)
    assert host['errors'] > 20 and len(host['confusions']) > 5 and host['wer'] > 0
    _same(dev, host)
    _same(evaluate(net, tc.lines, truths, scorer='device', batch_size=32), evaluate(net, tc.lines, truths, scorer='host', batch_size=32))
    monkeypatch.setenv('COCR_HOST_SCORE', '1')
    _same(evaluate(net, tc.lines, truths, report=True, model_name='m', batch_size=32), host)


@pytest.mark.timeout(600)
def test_validation_with_the_device_scorer_equals_the_host_scorer(tmp_path, monkeypatch):
    from conformer_ocr_amd.dataset import GroundTruthDataset
    from conformer_ocr_amd.evaluate import validate
    from tests import gt_synth
    monkeypatch.delenv('COCR_HOST_SCORE', raising=False)
    pages = gt_synth.make_pages(str(tmp_path))
    files = [x for x, _, _ in pages]
    data = GroundTruthDataset(files, evaluation_files=files, format_type='xml', batch_size=8, seed=1)
    hp = synth.hparams('cfg2', num_encoder_layers=2, num_classes=data.codec.max_label + 1)
    net = _model(hp, synth.make_state_dict(hp, seed=1, decoder_gain=8.0), data.codec)
    dev, host = data.validate(net), data.validate(net, scorer='host')
    assert dev == host and host > 0.0
    vi = np.arange(data.n_train, len(data.lines))
    im, lens = data._images(vi, int(data.widths[vi].max()))
    lines = [im[k, :, :int(lens[k])].cpu().numpy().astype(np.float32) / 255.0 for k in range(len(vi))]
    truths = [data.lines[i].text for i in vi]
    _same(validate(net, lines, truths, batch_size=8), validate(net, lines, truths, batch_size=8, scorer='host'))


# ---- the command --------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_test_command_prints_the_report(tmp_path):
    from conformer_ocr_amd.codec import ascii_codec
    from conformer_ocr_amd.evaluate import ErrorRate, compute_confusions, render_report
    from conformer_ocr_amd.ocr import load_image, load_model
    from conformer_ocr_amd.page import read_xml, recognize_pages
    from conformer_ocr_amd.pred import PytorchRecognitionModel, save_safetensors
    from tests import gt_synth
    pages = gt_synth.make_pages(str(tmp_path))
    files = [x for x, _, _ in pages]
    hp = synth.hparams('cfg2', num_encoder_layers=2)
    models = []
    for k in range(2):
        src = PytorchRecognitionModel(**hp.as_dict(), **DROPS, codec=ascii_codec(hp.num_classes))
        state = synth.make_state_dict(hp, seed=40 + k, decoder_gain=8.0)
        src.nn.load_state_dict({n: torch.from_numpy(np.asarray(v)) for n, v in state.items()})
        models.append(str(tmp_path / f'model{k}.tar'))
        save_safetensors(src, models[-1])
    (tmp_path / 'list.txt').write_text(files[1] + '\n')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('COCR_HOST_SCORE', None)

    def run(*extra):
        cmd = [sys.executable, '-m', 'conformer_ocr_amd.test', '-f', 'xml', '-e', str(tmp_path / 'list.txt'), files[0], *extra]
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
        assert r.returncode == 0, r.stdout + r.stderr[-3000:]
        return r.stdout
    out = run('-m', models[0])
    # the same files, read the same way, recognized here and scored by the host functions
    docs = [read_xml(f) for f in files]
    truths = [ln.text for d in docs for ln in d.lines]
    assert truths == [ln.text for _, _, lines in pages for ln in lines]
    net = load_model(models[0])
    res = recognize_pages(net, [(load_image(os.path.join(str(tmp_path), d.image)), d.lines) for d in docs])
    preds = [r['text'] for recs in res for r in recs]
    cer, wer = ErrorRate(False), ErrorRate(True)
    cer.update(preds, truths)
    wer.update(preds, truths)
    algn_gt, algn_pred = [], []
    for t, p in zip(truths, preds):
        _, a1, a2 = global_align(t, p)
        algn_gt.extend(a1)
        algn_pred.extend(a2)
    want = render_report(models[0], cer.total, cer.errors, 1.0 - cer.compute(), 1.0 - wer.compute(), *compute_confusions(algn_gt, algn_pred))
    assert cer.errors > 0
    assert want in out, out
    assert f'{sum(len(t) for t in truths)}\tCharacters' in out
    assert run('-m', models[0], '--scorer', 'host') == out
    both = run('-m', models[0], '-m', models[1])
    assert both.count('=== report ') == 2 and want in both
    tail = both.strip().split('\n')[-2:]
    assert tail[0].startswith('Average character accuracy: ') and '(stddev: ' in tail[0]
    assert tail[1].startswith('Average word accuracy: ') and '(stddev: ' in tail[1]
    # no usable line: exit 1 with a usage message
    (tmp_path / 'empty.xml').write_text('<?xml version="1.0"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2019-07-15">'
                                        '<Page imageFilename="page_0.png"><TextRegion id="r"></TextRegion></Page></PcGts>\n')
    r = subprocess.run([sys.executable, '-m', 'conformer_ocr_amd.test', '-f', 'xml', '-m', models[0], str(tmp_path / 'empty.xml')], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=100)
    assert r.returncode == 1 and 'usage:' in r.stderr and 'no usable line' in r.stderr
