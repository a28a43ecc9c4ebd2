"""Host side of the gradient window (no GPU): the clip coefficient against torch's own clipping, the command's three
options, and a state written before the window existed."""
import numpy as np
import pytest
import torch

from conformer_ocr_amd.train import WINDOW_HYPER, Trainer, build_parser, check_args, clip_coef, upgrade_state


@pytest.mark.parametrize('n', [3, 257, 120001])
@pytest.mark.parametrize('scale', [1e-3, 1.0, 10.0])
def test_clip_coef_is_the_factor_torch_applies(n, scale):
    """`clip_grad_norm_(max_norm)` on a CPU tensor against `clip_coef` of the float64 norm: the factor torch applied (largest element
    after / before) within 1e-5 relative, for a max_norm below the norm; a max_norm above the norm gives exactly 1.0."""
    g = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * scale).float()
    norm = float(np.sqrt(np.sum(g.numpy().astype(np.float64) ** 2)))
    for max_norm in (0.5 * norm, 0.01 * norm):
        p = torch.nn.Parameter(torch.zeros(n))
        p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([p], max_norm)
        i = int(g.abs().argmax())
        applied = float(p.grad[i].double() / g[i].double())
        c = clip_coef(norm, max_norm)
        assert c < 1.0 and abs(c - applied) <= 1e-5 * applied, (n, scale, max_norm, c, applied)
    for max_norm in (1.01 * norm, 2.0 * norm, 1e30):
        assert clip_coef(norm, max_norm) == 1.0
    p = torch.nn.Parameter(torch.zeros(n))
    p.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([p], 2.0 * norm)
    assert torch.equal(p.grad, g)


def test_clip_coef_is_a_float32_quotient():
    assert clip_coef(2.0, 1.0) == float(np.float32(1.0) / (np.float32(2.0) + np.float32(1e-6)))
    assert clip_coef(0.0, 1.0) == 1.0
    assert clip_coef(float('inf'), 1.0) == 0.0 and np.isnan(clip_coef(float('nan'), 1.0))


def test_the_command_takes_the_three_options_and_checks_them(capsys):
    ap = build_parser()
    args = ap.parse_args(['lines.txt'])
    check_args(ap, args)
    assert (args.accumulate, args.clip_norm, args.skip_nonfinite) == (1, None, False)
    args = ap.parse_args(['lines.txt', '--accumulate', '4', '--clip-norm', '0.5', '--skip-nonfinite'])
    check_args(ap, args)
    assert (args.accumulate, args.clip_norm, args.skip_nonfinite) == (4, 0.5, True)
    for bad in (['--accumulate', '0'], ['--accumulate', '-2'], ['--clip-norm', '0'], ['--clip-norm', '-1']):
        args = ap.parse_args(['lines.txt'] + bad)
        with pytest.raises(SystemExit) as e:
            check_args(ap, args)
        assert e.value.code == 2
    capsys.readouterr()


def _old_state():
    """The records of a `Trainer.state_dict()` as the code before the gradient window wrote them."""
    hyper = {'base_lr': 1e-3, 'weight_decay': 1e-2, 'optimizer': 'SGD', 'momentum': 0.9, 'warmup': 3, 'schedule': 'constant', 'gamma': 0.1,
             'cos_t_max': 50, 'cos_min_lr': 1e-4, 'step_size': 10, 'rop_factor': 0.1, 'rop_patience': 5, 'seed': 5, 'matmul_precision': 'highest',
             'freeze_backbone': 12}
    counters = {'epoch': 1, 'global_step': 7, 'samples_seen': 28, 'frozen_steps': 3, '_adopted': True, 'lr': 1e-3, '_sched_lr': 1e-3, '_best': 0.5,
                '_bad': 0}
    return {'hyper': hyper, 'counters': counters, 'optim': {'kind': 'SGD', 'step': 4, 'dec_steps': 3}}


def test_a_state_without_the_new_keys_loads_into_the_defaults():
    old = _old_state()
    sd = upgrade_state(old)
    assert set(sd['hyper']) == set(Trainer.HYPER) and set(sd['counters']) == set(Trainer.COUNTERS)
    assert {k: sd['hyper'][k] for k in WINDOW_HYPER} == {'accumulate_grad_batches': 1, 'gradient_clip_val': None, 'skip_nonfinite': False}
    c = sd['counters']
    assert c['batches_seen'] == c['global_step'] == 7 and c['frozen_batches'] == c['frozen_steps'] == 3
    assert c['skipped_steps'] == 0 and c['_window'] == 0 and c['_window_frozen'] is False
    for k, v in old['hyper'].items():
        assert sd['hyper'][k] == v
    for k, v in old['counters'].items():
        assert sd['counters'][k] == v
    assert sd['optim'] == old['optim'] and 'accum' not in sd
    assert old == _old_state()                                                  # (the input is left as it was)


def test_a_state_with_the_new_keys_keeps_them():
    new = _old_state()
    new['hyper'].update(accumulate_grad_batches=3, gradient_clip_val=0.25, skip_nonfinite=True)
    new['counters'].update(batches_seen=20, frozen_batches=6, skipped_steps=2, _window=2, _window_frozen=False)
    sd = upgrade_state(new)
    assert sd['hyper'] == new['hyper'] and sd['counters'] == new['counters']


def test_the_constructor_refuses_an_empty_window_and_a_clip_of_nothing():
    for kw in (dict(accumulate_grad_batches=0), dict(gradient_clip_val=0.0), dict(gradient_clip_val=-1.0)):
        with pytest.raises(ValueError, match='accumulate_grad_batches|gradient_clip_val'):
            Trainer(None, **kw)
