"""Host: the character n-gram model (conformer_ocr_amd/lm.py): Witten-Bell tables against a direct dictionary
computation, the file round trip, the collision refusal, the LM beam search's definition against oracle/ctc_ref.py::beam_decoder
(alpha = beta = 0) and a hand-made case that pins its effect, and the commands' argument checks.  No GPU."""
import io
import json
import math
import os
import tarfile

import numpy as np
import pytest

from conformer_ocr_amd import lm as lmmod
from conformer_ocr_amd.lm import NGramLM, beam_decode_host, build_lm
from oracle.ctc_ref import beam_decoder as ref_beam


def _sequences(C, n, seed, lo=3, hi=15):
    g = np.random.default_rng(seed)
    return [g.integers(1, C, size=int(g.integers(lo, hi))).tolist() for _ in range(n)]


def _direct(seqs, order, C):
    """Interpolated Witten-Bell straight from the formula, float64, on dictionaries."""
    count = {}
    for s in seqs:
        for k in range(order):
            for i in range(len(s) - k):
                g = tuple(s[i:i + k + 1])
                count[g] = count.get(g, 0) + 1
    succ = {}
    for g, n in count.items():
        succ.setdefault(g[:-1], {})[g[-1]] = n

    def p(ctx, c):
        ctx = tuple(ctx)
        lower = p(ctx[1:], c) if ctx else 1.0 / (C - 1)
        s = succ.get(ctx)
        if not s:
            return lower
        N, D = sum(s.values()), len(s)
        return (s.get(c, 0) + D * lower) / (N + D)
    return count, p


@pytest.fixture(scope='module')
def small():
    seqs = _sequences(7, 40, seed=7)
    return seqs, build_lm(seqs, 4, 7)


def test_probabilities_sum_to_one(small):
    seqs, lm = small
    for ctx in [(), (1,), (1, 2), (3, 3, 3), (6, 5, 4, 3, 2)]:
        total = sum(math.exp(float(lm.logp(ctx, c))) for c in range(1, 7))
        assert abs(total - 1.0) < 1e-6, (ctx, total)


def test_lookup_equals_the_formula(small):
    """Seen n-grams: one stored float32 log (+ nothing), so the float32 rounding of log P: 1e-6 relative is 8 ulps.  Unseen ones sum
    at most order float32 terms of magnitude < 20: 4 roundings of 1.2e-6 each, 1e-5 absolute."""
    seqs, lm = small
    count, p = _direct(seqs, 4, 7)
    seen = [g for g in count if len(g) >= 2]
    assert len(seen) > 100
    for g in seen:
        assert float(lm.logp(g[:-1], g[-1])) == pytest.approx(math.log(p(g[:-1], g[-1])), rel=1e-6, abs=1e-7), g
    rng = np.random.default_rng(11)
    unseen = 0
    while unseen < 200:
        g = tuple(rng.integers(1, 7, size=int(rng.integers(2, 5))).tolist())
        if g in count:
            continue
        unseen += 1
        assert float(lm.logp(g[:-1], g[-1])) == pytest.approx(math.log(p(g[:-1], g[-1])), abs=1e-5), g
    for c in range(1, 7):
        assert float(lm.logp((), c)) == pytest.approx(math.log(p((), c)), rel=1e-6)


def test_context_longer_than_the_order_uses_its_tail(small):
    _, lm = small
    assert lm.logp((6, 5, 4, 3, 2), 1) == lm.logp((4, 3, 2), 1)


def test_empty_model_is_uniform():
    lm = build_lm([], 3, 5)
    for ctx in [(), (1, 2)]:
        for c in range(1, 5):
            assert float(lm.logp(ctx, c)) == pytest.approx(math.log(0.25), rel=1e-6)


def test_save_load_round_trip_is_bit_exact(small, tmp_path):
    seqs, lm = small
    lm.meta['codec'] = {'a': [1], 'b': [2]}
    path = str(tmp_path / 'lm.safetensors')
    lm.save(path)
    back = NGramLM.load(path)
    assert back.order == lm.order and back.num_classes == lm.num_classes
    for name in ('unigram', 'ngram_keys', 'ngram_logp', 'ctx_keys', 'ctx_bow'):
        a, b = getattr(lm, name), getattr(back, name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    assert back.meta['codec'] == {'a': [1], 'b': [2]} and back.meta['tokens'] == sum(len(s) for s in seqs) and back.meta['lines'] == 40
    rng = np.random.default_rng(3)
    for _ in range(200):
        ctx = tuple(rng.integers(1, 7, size=int(rng.integers(0, 5))).tolist())
        c = int(rng.integers(1, 7))
        assert np.float32(lm.logp(ctx, c)).tobytes() == np.float32(back.logp(ctx, c)).tobytes()
    # slot counts: powers of two, at least twice the entries
    for keys in (lm.ngram_keys, lm.ctx_keys):
        n = keys.shape[0]
        assert n & (n - 1) == 0 and n >= 2 * int((keys != 0).sum())


def test_forged_key_collision_is_refused(monkeypatch):
    seqs = _sequences(7, 10, seed=1)
    real = lmmod._mix_np

    def forged(h, c, k):
        out = real(h, c, k).copy()
        if k == 2 and out.shape[0] > 1 and np.ndim(c):          # two different trigrams, one key
            out[1] = out[0]
        return out
    monkeypatch.setattr(lmmod, '_mix_np', forged)
    with pytest.raises(ValueError, match='share a 64-bit key'):
        build_lm(seqs, 3, 7)


def _logits(C, T, N=1):
    g = np.random.default_rng(C * 1000 + T)
    x = (g.normal(size=(N, T, C)) * 2.5).astype(np.float32)
    x[:, :, 0] += 1.5
    return x


@pytest.mark.parametrize('C,T,beam', [(5, 12, 4), (11, 40, 16), (93, 33, 8)])
def test_definition_without_the_model_is_the_plain_beam(C, T, beam):
    x = _logits(C, T)[0]
    lm = build_lm(_sequences(C, 20, seed=C), 3, C)
    got = beam_decode_host(x.T, lm, beam, C - 1, 0.0, 0.0)
    want = ref_beam(x.T, beam)
    assert [r[:3] for r in got] == [r[:3] for r in want]
    assert [r[3] for r in got] == [r[3] for r in want]


def test_known_answer_the_model_changes_the_reading():
    """a = 1, b = 2.  The frames say a, blank, then a (0.5) over b (0.4): the plain beam reads 'aa'.  In the corpus b always follows
    a (P(b|a) = 0.9706, P(a|a) = 0.0147), so with alpha = 1 the reading becomes 'ab'."""
    lm = build_lm([[1, 2]] * 8 + [[1, 2, 1, 2]] * 4, 3, 3)
    assert math.exp(float(lm.logp((1,), 2))) == pytest.approx(0.9706, abs=5e-5)
    probs = np.array([[.05, .9, .05], [.9, .05, .05], [.1, .5, .4]], dtype=np.float32)
    x = np.log(probs).T                                   # (C, T)
    assert [r[0] for r in ref_beam(x, 16)] == [1, 1]
    assert [r[0] for r in beam_decode_host(x, lm, 16, 2, 0.0, 0.0)] == [1, 1]
    recs, (ctc, lmv) = beam_decode_host(x, lm, 16, 2, 1.0, 0.0, return_scores=True)
    assert [r[0] for r in recs] == [1, 2]
    assert lmv == pytest.approx(float(lm.logp((), 1)) + float(lm.logp((1,), 2)), rel=1e-6)
    assert ctc < 0.0


def test_bonus_lengthens_and_scores_are_reported():
    x = _logits(11, 40)[0]
    lm = build_lm(_sequences(11, 50, seed=2), 3, 11)
    short = beam_decode_host(x.T, lm, 8, 4, 0.5, 0.0)
    recs, (ctc, lmv), gap = beam_decode_host(x.T, lm, 8, 4, 0.5, 3.0, return_scores=True, return_gap=True)
    assert len(recs) >= len(short) and gap >= 0.0
    want = np.float32(0.0)
    for i, r in enumerate(recs):                          # lmv is the float32 chain over the labels
        want = np.float32(want + np.float32(np.float32(np.float32(0.5) * lm.logp([q[0] for q in recs[:i]], r[0])) + np.float32(3.0)))
    assert lmv == float(want)


# ---------------------------------------------------------------------------------------------- commands
def _model_archive(path, c2l, num_classes):
    """A model archive as `save_safetensors` writes it, with a one-block network."""
    import safetensors.torch
    import torch
    from conformer_ocr_amd.codec import PytorchCodec
    from conformer_ocr_amd.pred import PytorchRecognitionModel, save_safetensors
    net = PytorchRecognitionModel(num_classes=num_classes, height=16, encoder_dim=16, num_encoder_layers=1, num_attention_heads=1,
                                  feed_forward_expansion_factor=2, conv_expansion_factor=2, input_dropout_p=0.1, feed_forward_dropout_p=0.1,
                                  attention_dropout_p=0.1, conv_dropout_p=0.1, conv_kernel_size=3, half_step_residual=True,
                                  subsampling_conv_channels=8, subsampling_factor=4, codec=PytorchCodec(c2l))
    save_safetensors(net, path)
    return net


def test_build_command_from_plain_text(tmp_path, capsys):
    model = str(tmp_path / 'model.tar')
    _model_archive(model, {'a': [1], 'b': [2], ' ': [3]}, 4)
    text = tmp_path / 'corpus.txt'
    text.write_text('ab ab\nabba\n\nab c ab\n  a   b \n', encoding='utf-8')
    out = str(tmp_path / 'lm.safetensors')
    assert lmmod.main(['build', '-m', model, '-o', out, '--order', '3', '-f', 'text', str(text)]) == 0
    err = capsys.readouterr().err
    assert 'corpus.txt' in err and '1 line(s) skipped' in err            # 'ab c ab': the codec has no c
    lm = NGramLM.load(out)
    assert (lm.order, lm.num_classes, lm.meta['lines'], lm.meta['skipped_lines']) == (3, 4, 3, 1)
    assert lm.meta['tokens'] == len('ab ab') + len('abba') + len('a b')   # whitespace runs collapse like ground truth's
    assert lm.meta['codec'] == {'a': [1], 'b': [2], ' ': [3]}
    want = build_lm([[1, 2, 3, 1, 2], [1, 2, 2, 1], [1, 3, 2]], 3, 4)
    assert want.ngram_keys.tobytes() == lm.ngram_keys.tobytes() and want.ngram_logp.tobytes() == lm.ngram_logp.tobytes()


def test_command_argument_checks(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        lmmod.main(['tune', '--help'])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for word in ('--alphas', '--betas', '--classes', '--lm', 'placeholders'):
        assert word in out
    with pytest.raises(SystemExit) as e:                   # build needs a model and an output
        lmmod.main(['build', 'x.txt'])
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        lmmod.main(['build', '-m', 'm', '-o', 'o', '-f', 'binary', 'x.txt'])
    args = lmmod.parser().parse_args(['tune', '-m', 'm', '--lm', 'l', '--alphas', '0,0.5,1', '--betas', '0,1', 'e.xml'])
    assert args.alphas == [0.0, 0.5, 1.0] and args.betas == [0.0, 1.0] and args.classes == 8 and args.beam == 16
    model = str(tmp_path / 'model.tar')
    _model_archive(model, {'a': [1]}, 2)
    assert lmmod.main(['build', '-m', model, '-o', str(tmp_path / 'o'), '--order', '9', '-f', 'text', model]) == 1


def test_codec_mismatch_is_refused_naming_the_first_difference(tmp_path):
    import argparse
    from conformer_ocr_amd.ocr import add_decoder_arguments, set_decoder
    net = _model_archive(str(tmp_path / 'model.tar'), {'a': [1], 'b': [2], 'c': [3]}, 4)
    ap = argparse.ArgumentParser()
    add_decoder_arguments(ap)
    assert vars(ap.parse_args([])) == {'beam': 0, 'lm': None, 'lm_weight': 0.5, 'lm_bonus': 0.0, 'lm_classes': 8}
    greedy = net.ctc_decoder
    set_decoder(net, ap.parse_args([]))
    assert net.ctc_decoder is greedy                       # the default: today's behaviour

    def lm_file(name, codec, C):
        p = str(tmp_path / name)
        build_lm([[1, 2, 1]], 2, C, {'codec': codec}).save(p)
        return p
    with pytest.raises(ValueError, match='built for 5 classes, the model has 4'):
        set_decoder(net, ap.parse_args(['--lm', lm_file('c5', {'a': [1], 'b': [2], 'c': [3]}, 5)]))
    with pytest.raises(ValueError, match=r"grapheme 'b' has labels \[3\] in the language model and \[2\] in the model"):
        set_decoder(net, ap.parse_args(['--lm', lm_file('swap', {'a': [1], 'b': [3], 'c': [2]}, 4)]))
    with pytest.raises(ValueError, match='--beam must be in 0..32'):
        set_decoder(net, ap.parse_args(['--beam', '33']))
    from conformer_ocr_amd.ctc_decoder import BeamDecoder, LMDecoder
    set_decoder(net, ap.parse_args(['--lm', lm_file('ok', {'a': [1], 'b': [2], 'c': [3]}, 4), '--lm-weight', '0.7']))
    d = net.ctc_decoder
    assert isinstance(d, LMDecoder) and (d.beam_size, d.alpha, d.beta, d.classes) == (16, 0.7, 0.0, 8)      # --lm alone: beam 16
    set_decoder(net, ap.parse_args(['--beam', '4']))
    assert isinstance(net.ctc_decoder, BeamDecoder) and net.ctc_decoder.beam_size == 4
