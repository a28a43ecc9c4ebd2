"""CPU: the host side of knowledge distillation -- the definition `distill.kd_loss_host` against torch's own
`kl_div` and autograd, its exact zeros and its behaviour under underflow, `check_teacher`, the command's flags, the state record, and
the two new names in the header and the binding."""
import os
import re

import pytest
import torch

from conformer_ocr_amd import _lib, synth, train
from conformer_ocr_amd.codec import ascii_codec
from conformer_ocr_amd.distill import check_teacher, kd_loss_host
from conformer_ocr_amd.pred import PytorchRecognitionModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, LENS = 3, 19, [19, 0, 7]


def _draw(ncls, scale=3.0, seed=0):
    g = torch.Generator().manual_seed(seed + ncls)
    return (torch.randn((N, T, ncls), generator=g, dtype=torch.float64) * scale, torch.randn((N, T, ncls), generator=g, dtype=torch.float64) * scale)


@pytest.mark.parametrize('ncls', [2, 97, 300])
@pytest.mark.parametrize('tau', [0.5, 1.0, 4.0])
def test_definition_equals_torch_kl_div_and_its_autograd(ncls, tau):
    F = torch.nn.functional
    zs, zt = _draw(ncls)
    kd, grad = kd_loss_host(zs, zt, LENS, tau, torch.float64)
    x = zs.clone().requires_grad_(True)
    want = [tau * tau * F.kl_div(F.log_softmax(x[n, :L] / tau, -1), F.log_softmax(zt[n, :L] / tau, -1), reduction='sum', log_target=True)
            for n, L in enumerate(LENS)]
    torch.stack(want).sum().backward()
    want = [w.detach() for w in want]
    assert kd.dtype == torch.float64 and grad.shape == zs.shape
    for n in range(N):
        assert abs(float(kd[n]) - float(want[n])) <= 1e-12 * max(1.0, abs(float(want[n])))
    assert float(kd[1]) == 0.0
    assert float((grad - x.grad).abs().max()) <= 1e-12
    for n, L in enumerate(LENS):
        assert not bool(grad[n, L:].any())                                              # exact zeros behind the line


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_equal_rows_give_exact_zeros(dtype):
    zs, _ = _draw(97, scale=8.0)
    zs = zs.to(dtype)
    kd, grad = kd_loss_host(zs, zs, LENS, 2.0, dtype)
    assert kd.dtype == dtype and not bool(kd.any()) and not bool(grad.any())


def test_underflowing_teacher_probabilities_stay_finite():
    """Logits of magnitude about 60 at tau = 0.5: a - max reaches -240, exp of it is 0 in float32; 0 x (finite) is 0, not NaN."""
    zs, zt = _draw(97, scale=20.0, seed=3)
    for dtype in (torch.float32, torch.float64):
        kd, grad = kd_loss_host(zs.to(dtype), zt.to(dtype), LENS, 0.5, dtype)
        assert bool(torch.isfinite(kd).all()) and bool(torch.isfinite(grad).all())
    assert float(torch.softmax(zt.float() / 0.5, -1).min()) == 0.0                     # (the case does underflow)
    assert float(kd[0]) > 0.0


def test_definition_refuses_malformed_input():
    zs, zt = _draw(5)
    with pytest.raises(ValueError, match='temperature'):
        kd_loss_host(zs, zt, LENS, 0.0)
    with pytest.raises(ValueError, match='one shape'):
        kd_loss_host(zs, zt[:, :, :4], LENS, 1.0)
    with pytest.raises(ValueError, match='out_lens'):
        kd_loss_host(zs, zt, [19, 0, 20], 1.0)


def _model(name='tiny', codec=None, **over):
    hp = synth.hparams(name, **over)
    return PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.0, feed_forward_dropout_p=0.0, attention_dropout_p=0.0, conv_dropout_p=0.0,
                                   codec=codec or ascii_codec(hp.num_classes))


def test_check_teacher_names_the_first_difference():
    net = _model()
    check_teacher(net, _model(encoder_dim=2 * net.hparams_record.encoder_dim))         # another width, same alphabet: fits
    ncls = net.hparams_record.num_classes
    with pytest.raises(ValueError, match='num_classes'):
        check_teacher(net, _model(num_classes=ncls + 1))
    with pytest.raises(ValueError, match='height'):
        check_teacher(net, _model(height=2 * net.hparams_record.height))
    with pytest.raises(ValueError, match='subsampling_factor'):
        check_teacher(net, _model(subsampling_factor=2))
    c2l = dict(net.codec.c2l)
    a, b = sorted(c2l)[:2]
    c2l[a], c2l[b] = c2l[b], c2l[a]
    from conformer_ocr_amd.codec import PytorchCodec
    with pytest.raises(ValueError, match='codecs differ'):
        check_teacher(net, _model(codec=PytorchCodec(c2l)))


def test_train_command_parses_and_checks_the_distillation_flags(capsys):
    ap = train.build_parser()
    a = ap.parse_args(['gt.xml'])
    train.check_args(ap, a)
    assert (a.teacher, a.distill_weight, a.distill_temperature) == (None, None, None)
    a = ap.parse_args(['gt.xml', '--teacher', 'big.safetensors'])
    train.check_args(ap, a)
    assert a.teacher == 'big.safetensors'
    a = ap.parse_args(['gt.xml', '--teacher', 'big.safetensors', '--distill-weight', '1', '--distill-temperature', '4'])
    train.check_args(ap, a)
    assert (a.distill_weight, a.distill_temperature) == (1.0, 4.0)
    a = ap.parse_args(['gt.xml', '--resume', 'm_state.safetensors', '--teacher', 'big.safetensors'])
    train.check_args(ap, a)
    for bad in (['--distill-weight', '0.3'], ['--distill-temperature', '2'], ['--teacher', 't', '--distill-weight', '1.5'],
                ['--teacher', 't', '--distill-weight', '-0.1'], ['--teacher', 't', '--distill-temperature', '0'],
                ['--teacher', 't', '--distill-temperature', '-1']):
        a = ap.parse_args(['gt.xml'] + bad)
        with pytest.raises(SystemExit) as e:
            train.check_args(ap, a)
        assert e.value.code == 2 and '--distill' in capsys.readouterr().err, bad
    text = ap.format_help()
    assert text.count('not tuned on real material') == 2


def test_state_record_round_trips_with_and_without_a_teacher():
    sd = {'hyper': {'base_lr': 1e-3}, 'counters': {'global_step': 4, 'frozen_steps': 1}}
    up = train.upgrade_state(sd)
    assert up['distill'] is None and 'distill' not in sd                               # no key: no teacher
    rec = {'weight': 0.5, 'temperature': 2.0, 'teacher': {'hyper_params': {'num_classes': 12}, 'codec': {'a': [1]}, 'compute_dtype': 'bf16'}}
    up = train.upgrade_state(dict(sd, distill=rec))
    assert up['distill'] == rec
    assert train.upgrade_state(up) == up                                                # idempotent


def test_state_file_keeps_the_distill_record(tmp_path):
    rec = {'weight': 0.25, 'temperature': 4.0, 'teacher': {'hyper_params': {'num_classes': 12}, 'codec': {'a': [1]}, 'compute_dtype': 'bf16'}}
    path = str(tmp_path / 's.safetensors')
    train.write_state_file(path, {'values': torch.zeros(3)}, {'format': 1, 'distill': rec, 'trainer': {}})
    _, meta = train.read_state_file(path, tensors=False)
    assert meta['distill'] == rec


def test_header_and_binding_hold_both_new_names():
    with open(os.path.join(ROOT, 'include', 'cocr.h'), encoding='utf-8') as fp:
        declared = set(re.findall(r'\b(cocr_[a-z_0-9]+)\s*\(', fp.read()))
    for name in ('cocr_distill_loss', 'cocr_train_step_distill'):
        assert name in declared and name in _lib.SYMBOLS
    assert len(_lib.SYMBOLS['cocr_distill_loss'][1]) == 14 and len(_lib.SYMBOLS['cocr_train_step_distill'][1]) == 16
