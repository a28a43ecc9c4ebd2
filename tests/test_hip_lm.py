"""GPU: the beam search with a character n-gram model (cocr_ctc_beam_lm, csrc/ctc_lm.hip.h) against its host definition
(conformer_ocr_amd/lm.py beam_decode_host) and, with the model switched off, against cocr_ctc_beam on the same logits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conformer_ocr_amd.codec import ascii_codec
from conformer_ocr_amd.ctc_decoder import LMDecoder
from conformer_ocr_amd.lm import NGramLM, beam_decode_host, build_lm
from conformer_ocr_amd.pred import PytorchRecognitionModel
from tests import beam_cases as bc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPS = dict(input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1)
GAP = 2e-5          # the device logaddexp differs from numpy's in the last ulps: a decision this close in the definition itself may flip


def _engine():
    from conformer_ocr_amd.ctc_decoder import _scratch_engine
    return _scratch_engine(torch.device('cuda', 0))


def _chain_lm(C, order, seed, n=200):
    """A model of `n` label sequences drawn from a random first-order chain."""
    g = np.random.default_rng(seed)
    P = g.dirichlet(np.full(C - 1, 0.3), size=C - 1)
    seqs = []
    for _ in range(n):
        s = [int(g.integers(1, C))]
        for _ in range(int(g.integers(4, 30))):
            s.append(1 + int(g.choice(C - 1, p=P[s[-1] - 1])))
        seqs.append(s)
    return build_lm(seqs, order, C)


def _logits(C, T, N):
    g = np.random.default_rng(C * 1000 + T)
    x = (g.normal(size=(N, T, C)) * 2.5).astype(np.float32)
    x[:, :, 0] += 1.5
    return x


@pytest.mark.parametrize('C,T,beam', [(5, 12, 4), (11, 40, 16), (128, 48, 16), (93, 33, 8), (300, 20, 8), (7, 500, 32), (40, 1500, 16)])
def test_without_the_model_every_field_equals_the_plain_beam(C, T, beam):
    """alpha = beta = 0 and every class a candidate: cocr_ctc_beam's output, field for field.  The entry point takes at most 64
    candidate classes; for more than 65 classes the 64 best are passed, which decides nothing: without the model an extension by a
    class of rank > beam never survives (the pruning argument of ctc_beam_walk_kernel), and beam <= 32.  (300, 20, 8): more than
    256 classes; (7, 500, 32): back-pointers in more than 64 KB of LDS; (40, 1500, 16): in global memory."""
    x = torch.from_numpy(_logits(C, T, 5)).cuda()
    lens = [T, T - 3, T // 2, 1, 0]
    eng = _engine()
    lm = _chain_lm(C, 3, seed=C, n=20)
    want = eng.ctc_beam(x, lens, beam)
    got, score = eng.ctc_beam_lm(x, lens, lm, beam, min(C - 1, 64), 0.0, 0.0, return_scores=True)
    assert got == want
    assert got[4] == [] and score[4].tolist() == [0.0, 0.0]
    assert (score[:, 1] == 0.0).all() and (score[:4, 0] < 0.0).all() and np.isfinite(score).all()


def _against_host(eng, x, lens, lm, beam, classes, alpha, beta):
    """Device against definition, line by line: labels, starts, ends exact, conf and both scores to 1e-4; returns how many lines were
    left out because the definition's own smallest decision gap is below GAP."""
    got, score = eng.ctc_beam_lm(torch.from_numpy(x).cuda(), lens, lm, beam, classes, alpha, beta, return_scores=True)
    left_out = 0
    for n, L in enumerate(lens):
        want, (ctc, lmv), gap = beam_decode_host(x[n, :L].T, lm, beam, classes, alpha, beta, return_scores=True, return_gap=True)
        if gap < GAP:
            left_out += 1
            continue
        assert [r[:3] for r in got[n]] == [r[:3] for r in want], (n, gap, got[n], want)
        np.testing.assert_allclose([r[3] for r in got[n]], [r[3] for r in want], rtol=1e-4)
        np.testing.assert_allclose(score[n], [ctc, lmv], rtol=1e-4, atol=1e-6)
    return left_out


def test_equals_the_definition_with_a_real_model():
    """24 lines; the prototype's smallest decision gap over them was 9.9e-5, so none should be left out; at most one may be."""
    left_out = 0
    for C, T, beam, classes, order in [(5, 12, 4, 4, 2), (11, 40, 16, 8, 3), (32, 60, 16, 8, 5), (128, 48, 16, 8, 4), (93, 33, 8, 5, 8),
                                       (300, 20, 8, 8, 3)]:
        lm = _chain_lm(C, order, seed=C * 31 + order)
        left_out += _against_host(_engine(), _logits(C, T, 4), [T, T - 3, max(1, T // 2), 1], lm, beam, classes, 0.7, 0.5)
    print(f'lines left out for a decision gap below {GAP}: {left_out} of 24')
    assert left_out <= 1


@pytest.mark.parametrize('name,C,order,beam,classes,empty', [('order 1', 12, 1, 8, 6, False), ('order 8', 9, 8, 8, 5, False),
                                                            ('one class', 12, 3, 8, 1, False), ('64 classes of 39', 40, 3, 8, 64, False),
                                                            ('empty model', 9, 3, 8, 4, True), ('beam 1', 12, 4, 1, 6, False)])
def test_edges(name, C, order, beam, classes, empty):
    lm = build_lm([], order, C) if empty else _chain_lm(C, order, seed=C + order)
    T = 24
    assert _against_host(_engine(), _logits(C, T, 2), [T, T - 5], lm, beam, classes, 0.7, 0.5) == 0, name


@pytest.mark.parametrize('name', list(bc.LM))
def test_every_form_with_the_model_on(name):
    """tests/beam_cases.py LM: beam 32 x 64 classes (all 2048 candidates of the key array), beams 17 and 31, the planted long lines
    (back-pointers in 68 KB of LDS at T = 500, in global memory for beam 32 at T = 730 and for beam 16 at T = 1386), masked classes.  Every line: integer fields
    exact, conf and both scores to 1e-4 (tests/test_beam_cases_host.py asserts the definition's gap of every line: none is left out)."""
    spec, beam, classes, _, _ = bc.LM[name]
    lm, rows = bc.lm_host(name)
    x, lens = bc.inputs(spec)
    got, score = _engine().ctc_beam_lm(torch.from_numpy(x).cuda(), lens, lm, beam, classes, bc.LM_ALPHA, bc.LM_BETA, return_scores=True)
    for n, (want, (ctc, lmv), gap) in enumerate(rows):
        assert gap >= GAP
        assert [r[:3] for r in got[n]] == [r[:3] for r in want], (name, n, gap)
        np.testing.assert_allclose([r[3] for r in got[n]], [r[3] for r in want], rtol=1e-4)
        print(f'{name} line {n}: scores {score[n].tolist()} definition {[ctc, lmv]}')
        np.testing.assert_allclose(score[n], [ctc, lmv], rtol=1e-4, atol=1e-6)


def test_arguments_are_checked():
    import ctypes as C
    from conformer_ocr_amd import _lib
    eng = _engine()
    lm = _chain_lm(6, 3, seed=1, n=20)
    x = torch.zeros((1, 4, 6)).cuda()
    with pytest.raises(ValueError, match='classes must be in 1..64'):
        eng.ctc_beam_lm(x, [4], lm, 8, 65)
    with pytest.raises(ValueError, match='classes must be in 1..64'):
        eng.ctc_beam_lm(x, [4], lm, 8, 0)
    with pytest.raises(ValueError, match='beam must be in 1..32'):
        eng.ctc_beam_lm(x, [4], lm, 33, 4)
    with pytest.raises(ValueError, match='the logits have 7 classes, the language model 6'):
        eng.ctc_beam_lm(torch.zeros((1, 4, 7)).cuda(), [4], lm, 8, 4)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def create(order=3, ncls=6, nkeys=lm.ngram_keys, cslots=None):
        h = C.c_void_p()
        nlogp = np.zeros(nkeys.shape[0], dtype=np.float32)
        rc = eng.lib.cocr_lm_create(eng._h, order, ncls, vp(lm.unigram), vp(nkeys), vp(nlogp), nkeys.shape[0], vp(lm.ctx_keys), vp(lm.ctx_bow),
                                    lm.ctx_keys.shape[0] if cslots is None else cslots, C.byref(h))
        if rc == 0:
            eng.lib.cocr_lm_destroy(h)
        return _lib.check(rc)
    assert create() == 0
    with pytest.raises(ValueError, match='order must be in 1..8'):
        create(order=9)
    with pytest.raises(ValueError, match='ncls must be in 2..65535'):
        create(ncls=65536)
    with pytest.raises(ValueError, match='not a power of two'):
        create(cslots=lm.ctx_keys.shape[0] - 1)
    with pytest.raises(ValueError, match='no empty slot'):
        create(nkeys=np.arange(1, 9, dtype=np.int64))


def test_a_damaged_table_ends(tmp_path):
    """Every slot but one holds a foreign key: lookups walk the whole table and end; the text may be wrong, the call returns."""
    lm = _chain_lm(6, 3, seed=2, n=20)
    bad = NGramLM(3, 6, lm.unigram, np.where(lm.ngram_keys == 0, 12345, lm.ngram_keys), lm.ngram_logp,
                  np.where(lm.ctx_keys == 0, 54321, lm.ctx_keys), lm.ctx_bow)
    bad.ngram_keys[3] = 0
    bad.ctx_keys[5] = 0
    got = _engine().ctc_beam_lm(torch.from_numpy(_logits(6, 12, 1)).cuda(), [12], bad, 4, 4, 0.7, 0.5)
    assert len(got) == 1


def _tiny_net(case, decoder):
    hp, state, image, lens, g = case('tiny')
    net = PytorchRecognitionModel(**hp.as_dict(), **DROPS, codec=ascii_codec(hp.num_classes), ctc_decoder=decoder, compute_dtype='fp32')
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return net.to('cuda:0'), image, lens, g


def test_public_surface_routes_the_decoder_to_the_batch_kernel(case):
    from conformer_ocr_amd.evaluate import recognize
    lm = _chain_lm(11, 3, seed=5)
    dec = LMDecoder(lm, beam_size=8, alpha=0.7, beta=0.5, classes=6)
    net, image, lens, g = _tiny_net(case, dec)
    x, xl = torch.from_numpy(image).cuda(), torch.from_numpy(lens)
    recs = net.predict_labels(x, xl)
    for n in range(image.shape[0]):
        want = beam_decode_host(g['logits'][n, :int(g['out_lens'][n])].T, lm, 8, 6, 0.7, 0.5)
        assert [r[0] for r in recs[n]] == [r[0] for r in want]
    strings = net.predict_string(x, xl)
    codec = net.codec
    assert strings == [''.join(c[0] for c in codec.decode(r)) for r in recs]
    assert [''.join(c[0] for c in p) for p in net.predict(x, xl)] == strings
    lines = [image[n, 0, :, :int(lens[n])] for n in range(image.shape[0])]
    for streams in (1, 2):
        out = recognize(net, lines, batch_size=image.shape[0], edge=image.shape[3], streams=streams)
        assert [out[n] for n in range(len(lines))] == strings, streams
    # the decoder object on one line's (C, T) matrix, like the other decoders
    one = g['logits'][0, :int(g['out_lens'][0])].T
    assert [r[0] for r in dec(one)] == [r[0] for r in beam_decode_host(one, lm, 8, 6, 0.7, 0.5)]


# ---- the point of it: noisy logits of the metric's model, read with and without the fixture's own language ------------------------
NOISE_SIGMA, NOISE_SEED, PLAIN_ERRORS = 2.0, 2026, 230


def _errors(records, truths):
    from conformer_ocr_amd.evaluate import edit_distance
    return sum(edit_distance([r[0] for r in rec], list(t)) for rec, t in zip(records, truths))


def test_noisy_lines_are_read_with_the_model(text_case):
    """cfg2_text, its first 8 lines (189 characters), fp32 logits + seeded Gaussian noise added on the host, an order-5 model of the
    fixture's 32 reference strings, beam 16, 8 classes, alpha 1, beta 0.  The noise level was chosen on the CPU with the definitions:
    at sigma = 2.0 (seed 2026) the plain beam (oracle/ctc_ref.py::beam_decoder) commits 230 character errors on these lines
    and the LM beam (lm.beam_decode_host) 0; at sigma = 3.0 they commit 602 and 11.  The definition's smallest decision gap on the 8
    lines is 4.6e-5.  Here: the device output equals the definition on the same logits, hence the same counts."""
    from tests.hip_util import make_engine
    tc = text_case('cfg2_text')
    image, lens, idx = tc.batch(0)
    n = 8
    eng = make_engine(tc.hp, tc.state, 'fp32')
    logits, out_lens = eng.forward(torch.from_numpy(image[:n, 0]).cuda(), lens[:n])
    noise = np.random.default_rng(NOISE_SEED).normal(size=tuple(logits.shape)).astype(np.float32) * np.float32(NOISE_SIGMA)
    x = logits.cpu().numpy() + noise
    truths = [tc.texts[i] for i in idx[:n]]
    lm = build_lm(tc.texts, 5, tc.hp.num_classes)
    xd = torch.from_numpy(x).cuda()
    plain = _errors(eng.ctc_beam(xd, out_lens, 16), truths)
    got = eng.ctc_beam_lm(xd, out_lens, lm, 16, 8, 1.0, 0.0)
    with_lm = _errors(got, truths)
    print(f'character errors on {sum(len(t) for t in truths)} characters: plain beam {plain}, LM beam {with_lm}')
    assert _against_host(eng, x, [int(v) for v in out_lens], lm, 16, 8, 1.0, 0.0) == 0
    assert plain >= 20 and 2 * with_lm <= plain
    assert (plain, with_lm) == (PLAIN_ERRORS, 0)


def test_ocr_command_with_a_language_model(text_case, tmp_path):
    """`ocr --beam 16 --lm FILE` writes the text `recognize_pages` gives with the decoder set by hand."""
    from PIL import Image
    from conformer_ocr_amd.page import Line, recognize_pages
    from conformer_ocr_amd.pred import save_safetensors
    from tests import page_synth
    from tests.test_hip_page import FIXTURE_FORM, KINDS, PICK
    tc = text_case('cfg2_text')
    lines = [np.rint(tc.lines[i] * 255.0).astype(np.uint8) for i in PICK[:4]]
    page, placed = page_synth.text_page(lines, KINDS[:4])
    page_lines = [Line(f'line{k}', P, B) for k, (_, P, B) in enumerate(placed)]
    Image.fromarray(page).save(tmp_path / 'scan.png')
    pts = lambda a: ' '.join(f'{x:.3f},{y:.3f}' for x, y in a)
    body = ''.join(f'<TextLine id="{l.id}"><Coords points="{pts(l.boundary)}"/><Baseline points="{pts(l.baseline)}"/></TextLine>\n'
                   for l in page_lines)
    (tmp_path / 'scan.xml').write_text('<?xml version="1.0"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2019-07-15">'
                                       f'<Page imageFilename="scan.png"><TextRegion id="r">{body}</TextRegion></Page></PcGts>\n')
    codec = ascii_codec(tc.hp.num_classes)
    src = PytorchRecognitionModel(**tc.hp.as_dict(), **DROPS, codec=codec)
    src.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    save_safetensors(src, tmp_path / 'model.tar')
    lm = build_lm(tc.texts, 5, tc.hp.num_classes, {'codec': {k: list(v) for k, v in codec.c2l.items()}})
    lm.save(str(tmp_path / 'lm.safetensors'))
    src.ctc_decoder = LMDecoder(lm, beam_size=16, alpha=0.8, beta=0.25, classes=6)
    want, = recognize_pages(src.to('cuda:0').eval(), [(page, page_lines)], **FIXTURE_FORM)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = tmp_path / 'out.txt'
    p = subprocess.run([sys.executable, '-m', 'conformer_ocr_amd.ocr', '-m', str(tmp_path / 'model.tar'), '-f', 'page', '-i', str(tmp_path / 'scan.xml'),
                        str(out), '--pad', '0', '--edge', '1200', '--beam', '16', '--lm', str(tmp_path / 'lm.safetensors'), '--lm-weight', '0.8',
                        '--lm-bonus', '0.25', '--lm-classes', '6'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert out.read_text(encoding='utf-8').split('\n')[:-1] == [r['text'] for r in want]
    assert [r['text'] for r in want] == [''.join(codec.l2c[(l,)] for l in tc.texts[i]) for i in PICK[:4]]


def test_tune_command_prints_the_grid(text_case, tmp_path, capsys):
    """`lm tune` on four fixture lines as line images: one forward, then a decode per cell; every cell reads them right."""
    from PIL import Image
    from conformer_ocr_amd import lm as lmmod
    from conformer_ocr_amd.pred import save_safetensors
    tc = text_case('cfg2_text')
    codec = ascii_codec(tc.hp.num_classes)
    files = []
    for i in range(4):
        Image.fromarray(np.rint(tc.lines[i] * 255.0).astype(np.uint8)).save(tmp_path / f'l{i}.png')
        (tmp_path / f'l{i}.gt.txt').write_text(''.join(codec.l2c[(l,)] for l in tc.texts[i]), encoding='utf-8')
        files.append(str(tmp_path / f'l{i}.png'))
    src = PytorchRecognitionModel(**tc.hp.as_dict(), **DROPS, codec=codec)
    src.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    save_safetensors(src, tmp_path / 'model.tar')
    build_lm(tc.texts, 5, tc.hp.num_classes, {'codec': {k: list(v) for k, v in codec.c2l.items()}}).save(str(tmp_path / 'lm.safetensors'))
    assert lmmod.main(['tune', '-m', str(tmp_path / 'model.tar'), '--lm', str(tmp_path / 'lm.safetensors'), '-f', 'path', '--pad', '0', '--edge', '1200',
                       '--alphas', '0,1', '--betas', '0,0.5,1', '-u', 'NFC'] + files) == 0
    out = capsys.readouterr().out.splitlines()
    rows = [l.split() for l in out if l.strip() and l.split()[0] in ('0.00', '1.00')]
    assert [len(r) for r in rows] == [4, 4] and all(float(v) == 0.0 for r in rows for v in r[1:]), out
    assert any(l.startswith('best: alpha 0, beta 0, CER 0.00% (4 lines, 6 cells') for l in out), out
