"""No GPU: the numpy statement of the four optimizer steps (tests/optim_ref.py) against torch.optim in float64, the `train` command's
optimizer / schedule / resume flags, and the state file of `fit(save_state=True)` on hand-made tensors."""
import numpy as np
import pytest
import torch

from conformer_ocr_amd import train
from tests import optim_ref

CASES = [('AdamW', 0.0), ('Adam', 0.0), ('SGD', 0.9), ('SGD', 0.0), ('RMSprop', 0.9), ('RMSprop', 0.0)]


@pytest.mark.parametrize('kind,momentum', CASES)
@pytest.mark.parametrize('weight_decay', [0.1, 0.0])
def test_numpy_statement_equals_torch_optim_in_float64(kind, momentum, weight_decay):
    """Five steps of random gradients on three tensors, one of which has an exactly zero gradient throughout (the key projection's
    bias of the network is such a parameter): every parameter within 1e-12 absolute of torch.optim.<kind> after every step."""
    g = torch.Generator().manual_seed(7)
    shapes = [(5, 3), (7,), (4,)]
    tparams = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64)) for s in shapes]
    kw = dict(lr=1e-3, weight_decay=weight_decay)
    if kind in ('SGD', 'RMSprop'):
        kw['momentum'] = momentum
    opt = getattr(torch.optim, kind)(tparams, **kw)
    params = [p.detach().numpy().copy() for p in tparams]
    states = [optim_ref.new_state(p) for p in params]
    for step in range(5):
        grads = [torch.randn(s, generator=g, dtype=torch.float64) * 10.0 ** (step - 2) for s in shapes]
        grads[2] = torch.zeros(shapes[2], dtype=torch.float64)
        for p, gr in zip(tparams, grads):
            p.grad = gr.clone()
        opt.step()
        for i, gr in enumerate(grads):
            params[i] = optim_ref.step(kind, params[i], gr.numpy(), states[i], lr=1e-3, weight_decay=weight_decay, momentum=momentum)
            err = float(np.abs(params[i] - tparams[i].detach().numpy()).max())
            assert err <= 1e-12, (step, i, err)
    if kind == 'SGD' and momentum == 0:
        assert all(not s['slot0'].any() and not s['slot1'].any() for s in states)          # the slots are not touched


def test_adam_is_not_adamw():
    """Coupled and decoupled decay give different parameters: a test that cannot tell them apart would pass either kernel."""
    p0 = np.linspace(-1, 1, 12)
    g = np.cos(np.arange(12.0))
    out = {}
    for kind in ('Adam', 'AdamW'):
        p, st = p0.copy(), optim_ref.new_state(p0)
        for _ in range(3):
            p = optim_ref.step(kind, p, g, st, lr=1e-3, weight_decay=0.1)
        out[kind] = p
    assert np.abs(out['Adam'] - out['AdamW']).max() > 1e-5


def test_train_command_parses_the_optimizer_schedule_and_resume_flags():
    ap = train.build_parser()
    a = ap.parse_args(['gt.xml'])
    train.check_args(ap, a)
    # the reference's defaults (default_specs.py)
    assert (a.optimizer, a.momentum, a.gamma, a.step_size, a.sched_patience, a.save_state, a.resume) == ('AdamW', 0.9, 0.1, 10, 5, False, None)
    a = ap.parse_args(['gt.xml', '--optimizer', 'RMSprop', '-m', '0.5', '-g', '0.3', '-ss', '4', '--sched-patience', '2', '--save-state'])
    train.check_args(ap, a)
    assert (a.optimizer, a.momentum, a.gamma, a.step_size, a.sched_patience, a.save_state) == ('RMSprop', 0.5, 0.3, 4, 2, True)
    a = ap.parse_args(['gt.xml', '--momentum', '0', '--gamma', '0.5', '--step-size', '2', '--resume', 'm_state.safetensors', '-N', '7'])
    train.check_args(ap, a)
    assert a.resume == 'm_state.safetensors' and a.save_state is True and a.epochs == 7          # --resume implies --save-state
    with pytest.raises(SystemExit):
        ap.parse_args(['gt.xml', '--optimizer', 'Adagrad'])


@pytest.mark.parametrize('extra', [['-i', 'model.safetensors'], ['-c', 'codec.json'], ['-i', 'model.safetensors', '--resize', 'union']])
def test_resume_excludes_what_describes_another_model(extra, capsys):
    ap = train.build_parser()
    a = ap.parse_args(['gt.xml', '--resume', 'm_state.safetensors'] + extra)
    with pytest.raises(SystemExit) as e:
        train.check_args(ap, a)
    assert e.value.code == 2 and '--resume' in capsys.readouterr().err
    a = ap.parse_args(['gt.xml', '-m', '-0.1'])
    with pytest.raises(SystemExit):
        train.check_args(ap, a)


def test_state_file_round_trip_and_fingerprint(tmp_path):
    g = torch.Generator().manual_seed(1)
    tensors = {'values': torch.randn(37, generator=g), 'slot0': torch.randn(33, generator=g), 'slot1': torch.zeros(33),
               'decoder_state': torch.randn(3 * 11, generator=g)}
    fp = {'n_train': 16, 'n_val': 4, 'seed': 1, 'batch_size': 4, 'edge': 200, 'augment': True, 'height': 96, 'pad': 16}
    meta = {'format': 1, 'data': fp, 'codec': {'a': [1], 'ch': [2, 3]}, 'hyper_params': {'num_classes': 4, 'input_dropout_p': 0.1},
            'compute_dtype': 'bf16',
            'fit': {'best_epoch': 1, 'best_cer': 0.1 + 0.2, 'bad': 0, 'history': [[12.5, 100.0, 1.0], [1e-3 / 3, 99.0, 0.30000000000000004]]},
            'trainer': {'optim': {'kind': 'SGD', 'step': 9, 'dec_steps': 2},
                        'counters': {'epoch': 2, 'global_step': 9, 'lr': 1e-3 * (2 / 3), '_best': None, '_bad': 0, '_adopted': False},
                        'hyper': {'base_lr': 1e-3, 'optimizer': 'SGD', 'momentum': 0.9}}}
    path = str(tmp_path / 'm_state.safetensors')
    train.write_state_file(path, tensors, meta)
    assert not (tmp_path / 'm_state.safetensors.tmp').exists()
    got, meta2 = train.read_state_file(path)
    assert meta2 == meta                                              # floats round-trip exactly through JSON (repr)
    assert set(got) == set(tensors) and all(torch.equal(got[k], tensors[k]) for k in tensors)
    none, meta3 = train.read_state_file(path, tensors=False)          # the header alone
    assert none is None and meta3 == meta
    train.write_state_file(path, {'values': torch.ones(2)}, dict(meta, format=2))      # replaces the file in one move
    assert train.read_state_file(path)[1]['format'] == 2

    class Data:
        n_train, lines, seed, batch_size, edge, augment, height, pad = 16, [None] * 20, 1, 4, 200, True, 96, 16
    assert train.data_fingerprint(Data()) == fp
    train.check_fingerprint(fp, train.data_fingerprint(Data()))
    for field, value in [('batch_size', 8), ('augment', False), ('n_val', 5), ('seed', 2)]:
        with pytest.raises(ValueError, match=field):
            train.check_fingerprint(fp, dict(fp, **{field: value}))
    bad = str(tmp_path / 'plain.safetensors')
    import safetensors.torch
    safetensors.torch.save_file({'x': torch.ones(1)}, bad)
    with pytest.raises(ValueError, match='not a training state file'):
        train.read_state_file(bad)


def test_trainer_arguments_are_checked_before_any_device_work():
    with pytest.raises(ValueError, match='optimizer'):
        train.Trainer(None, optimizer='Adagrad')
    with pytest.raises(ValueError, match='momentum'):
        train.Trainer(None, optimizer='SGD', momentum=-0.5)
    with pytest.raises(ValueError, match='optimizer'):
        train.DecoderTrainer(None, optimizer='Adagrad')
    with pytest.raises(ValueError):
        train.Trainer(None, schedule='1cycle')
