"""GPU: the optimizer step of every kind (cocr_train_optim_step / cocr_decoder_optim_step: Adam, SGD, RMSprop, and AdamW through the
same kernel) against torch.optim fed the device's own gradients, the hand-over of a frozen phase per kind, and resuming an interrupted
`fit` from its state file, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conformer_ocr_amd import synth
from conformer_ocr_amd.engine import HipRecognizer
from conformer_ocr_amd.pred import PytorchRecognitionModel
from conformer_ocr_amd.spec import model_state_spec
from conformer_ocr_amd.train import Trainer, fit, read_state_file
from tests import gt_synth
from tests.test_hip_finetune import _decoder_grads, _tiny_net
from tests.test_hip_train_full import CASES, _engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [('Adam', 0.0), ('SGD', 0.9), ('SGD', 0.0), ('RMSprop', 0.9), ('RMSprop', 0.0)]
LR, WD = 1e-3, 0.1


def _tiny_case():
    c = CASES['tiny']
    hp = c['hp']()
    names = [k for k, (_, kind) in model_state_spec(hp).items() if kind == 'param']
    if sum(int(np.prod(model_state_spec(hp)[k][0])) for k in names) % 4 == 0:
        hp = synth.hparams('tiny', num_classes=hp.num_classes + 1)
    state = synth.make_state_dict(hp, seed=c['seed'], decoder_gain=1.0)
    image, lens = synth.make_lines(c['n'], hp.height, c['W'], seed=c['seed'], widths=c['widths'])
    tg, tl = [x for s in c['targets'] for x in s], [len(s) for s in c['targets']]
    return hp, state, names, torch.from_numpy(image[:, 0]).cuda(), lens, tg, tl


def _torch_optimizer(kind, params, momentum, lr=LR, weight_decay=WD):
    kw = dict(lr=lr, weight_decay=weight_decay)
    if kind in ('SGD', 'RMSprop'):
        kw['momentum'] = momentum
    return getattr(torch.optim, kind)(params, **kw)


def _three_steps(kind, momentum, check=True):
    """Three steps on a fixed batch; with `check`, torch.optim.<kind> (fp32) fed the gradients read back from the device follows along
    and every parameter is compared after every step.  Returns the final values."""
    hp, state, names, x, lens, tg, tl = _tiny_case()
    eng = _engine(hp, state)
    tparams = {k: torch.tensor(np.asarray(state[k], dtype=np.float32), requires_grad=True) for k in names}
    opt = _torch_optimizer(kind, list(tparams.values()), momentum)
    worst = 0.0
    for step in range(3):
        eng.train_step(x, lens, tg, tl)
        for k in names:
            tparams[k].grad = torch.from_numpy(eng.train_grad(k).reshape(tparams[k].shape).copy())
        opt.step()
        eng.train_optim_step(kind, LR, weight_decay=WD, momentum=momentum)
        if check:
            for k in names:
                err = float(np.abs(eng.train_value(k) - tparams[k].detach().numpy()).max())
                worst = max(worst, err)
                assert err <= 2e-6, (kind, momentum, step, k, err)
    print(f'{kind} momentum {momentum}: largest parameter error over three steps {worst:.3e}')
    st = eng.train_optim_state()
    assert st['kind'] == kind and st['step'] == 3 and st['dec_steps'] == 0
    if kind == 'SGD' and momentum == 0:
        assert not bool(st['slot0'].any()) and not bool(st['slot1'].any())          # the slots are not touched
    return {k: eng.train_value(k) for k in names}


@pytest.mark.parametrize('kind,momentum', KINDS)
def test_each_kind_follows_torch(kind, momentum):
    """Three optimizer steps on a fixed batch, lr 1e-3, weight_decay 0.1: after every step every parameter is within 2e-6 absolute of
    torch.optim.<kind> in fp32 fed the SAME gradients (read back from the device, for the reason
    test_adamw_steps_follow_torch_and_lower_the_loss gives).  The bound is that test's: the largest single update is RMSprop's first,
    lr g / sqrt(0.01 g^2) = 10 lr = 1e-2, a few fp32 roundings of which stay below 1e-8, and the parameters are O(1) with an ulp of
    1.2e-7.  The model's parameter count is no multiple of 4.  (The library pads every tensor of its flat vector to 16 bytes, so the whole
    vector goes 16 bytes per lane; the one-by-one path runs where the vectors' alignments differ: the output layer's state in
    test_frozen_phase_and_hand_over_follow_torch.)"""
    hp, _, names, *_ = _tiny_case()
    assert sum(int(np.prod(model_state_spec(hp)[k][0])) for k in names) % 4 != 0
    got = _three_steps(kind, momentum)
    if kind == 'Adam':
        # coupled decay must not pass for decoupled decay: an AdamW run from the same start ends elsewhere
        other = _three_steps('AdamW', 0.0, check=False)
        assert max(float(np.abs(got[k] - other[k]).max()) for k in names) > 1e-5


def test_adamw_through_the_general_step_equals_train_adamw_bit_for_bit():
    hp, state, names, x, lens, tg, tl = _tiny_case()
    old, new = _engine(hp, state), _engine(hp, state)
    for step in range(3):
        assert old.train_step(x, lens, tg, tl) == new.train_step(x, lens, tg, tl)
        old.train_adamw(LR, weight_decay=WD)
        new.train_optim_step('AdamW', LR, weight_decay=WD)
        for k in names:
            assert np.array_equal(old.train_value(k), new.train_value(k)), (step, k)
    a, b = old.train_optim_state(), new.train_optim_state()
    assert a['kind'] == b['kind'] == 'AdamW' and a['step'] == b['step'] == 3
    assert torch.equal(a['slot0'], b['slot0']) and torch.equal(a['slot1'], b['slot1'])
    old.train_optim_step('AdamW', LR, weight_decay=WD)          # the two entry points share one state
    new.train_adamw(LR, weight_decay=WD)
    for k in names:
        assert np.array_equal(old.train_value(k), new.train_value(k)), k


def test_kind_is_sticky_and_hyper_parameters_are_checked():
    hp, state, names, x, lens, tg, tl = _tiny_case()
    eng = _engine(hp, state)
    eng.train_step(x, lens, tg, tl)
    before = eng.train_value('decoder.bias').copy()
    with pytest.raises(ValueError, match='invalid learning rate'):                       # COCR_EINVAL, nothing stepped
        eng.train_optim_step('SGD', -1e-3, momentum=0.9)
    with pytest.raises(ValueError, match='invalid momentum'):
        eng.train_optim_step('SGD', 1e-3, momentum=-0.1)
    with pytest.raises(ValueError, match='invalid momentum'):
        eng.train_optim_step('RMSprop', 1e-3, momentum=-0.1)
    with pytest.raises(ValueError, match='invalid beta'):
        eng.train_optim_step('Adam', 1e-3, betas=(1.0, 0.999))
    with pytest.raises(ValueError, match='unknown optimizer'):
        eng.train_optim_step('Adagrad', 1e-3)
    assert eng.train_optim_state()['kind'] is None and np.array_equal(eng.train_value('decoder.bias'), before)
    eng.train_optim_step('SGD', 1e-3, momentum=0.9)
    with pytest.raises(RuntimeError, match="the optimizer state is SGD's: a RMSprop step cannot follow"):      # COCR_ESTATE
        eng.train_optim_step('RMSprop', 1e-3)
    with pytest.raises(RuntimeError, match='not AdamW'):
        eng.train_adamw(1e-3)
    eng.train_optim_step('SGD', 1e-3, momentum=0.0)                                      # the same kind goes on
    assert eng.train_optim_state()['step'] == 2


@pytest.mark.parametrize('kind,momentum', KINDS)
def test_frozen_phase_and_hand_over_follow_torch(kind, momentum):
    """Two frozen steps, then two whole-network steps (dropout 0, fp32 serving engine), against ONE torch optimizer over all parameters
    that receives gradients for the output layer only during the frozen steps -- torch then creates no state for the other tensors:
    their momentum buffers start at their first whole-network step, Adam's bias corrections count per tensor.  Fed the device's
    gradients; every parameter within 2e-6 absolute (the bound of test_each_kind_follows_torch)."""
    net, hp, batch = _tiny_net('fp32', dropout=0.0)
    n = int(batch['image'].shape[0])
    tr = Trainer(net, lr=LR, weight_decay=WD, optimizer=kind, momentum=momentum, freeze_backbone=2 * n)
    names = [k for k, (_, kd) in model_state_spec(hp).items() if kd == 'param']
    sd = net.nn.state_dict()
    tparams = {k: torch.nn.Parameter(sd[k].detach().cpu().clone()) for k in names}
    opt = _torch_optimizer(kind, list(tparams.values()), momentum)
    for step in range(2):
        tparams['decoder.weight'].grad, tparams['decoder.bias'].grad = _decoder_grads(net, batch)
        opt.step()
        assert tr.frozen
        tr.training_step(batch)
        st = net._engine.decoder_state()
        for k in ('decoder.weight', 'decoder.bias'):
            assert np.abs(st[k] - tparams[k].detach().numpy()).max() <= 2e-6, (step, k)
    d = net._engine.decoder_optim_state()
    assert d['kind'] == kind and d['step'] == 2 and d['state'].numel() % 3 == 0
    assert not tr.frozen
    worst = {}
    for step in range(2):
        tr.training_step(batch)
        for k in names:
            tparams[k].grad = torch.from_numpy(tr.engine.train_grad(k).reshape(tparams[k].shape).copy())
        opt.step()
        for k in names:
            err = float(np.abs(tr.engine.train_value(k).reshape(tparams[k].shape) - tparams[k].detach().numpy()).max())
            worst[k] = max(worst.get(k, 0.0), err)
    print(f'{kind} momentum {momentum}: hand-over, largest parameter error', max(worst.values()), 'decoder.weight', worst['decoder.weight'])
    bad = {k: e for k, e in worst.items() if not e <= 2e-6}
    assert not bad, dict(sorted(bad.items(), key=lambda kv: -kv[1])[:8])
    st = tr.engine.train_optim_state()
    assert (st['kind'], st['step'], st['dec_steps']) == (kind, 2, 2) and tr.global_step == 4 and tr.frozen_steps == 2


def test_adoption_refuses_states_of_different_kinds():
    from tests.hip_util import make_engine
    hp, state, names, x, lens, tg, tl = _tiny_case()
    dst = _engine(hp, state)
    dst.train_step(x, lens, tg, tl)
    dst.train_optim_step('SGD', LR, momentum=0.9)
    src = make_engine(hp, state, 'fp32')
    gw = torch.zeros((hp.num_classes, hp.encoder_dim), device='cuda')
    gb = torch.ones((hp.num_classes,), device='cuda')
    src.decoder_optim_step('RMSprop', gw, gb, LR)
    with pytest.raises(ValueError, match='different optimizer kinds'):                    # COCR_EINVAL
        dst.train_adopt_decoder(src)
    with pytest.raises(RuntimeError, match='cannot follow'):
        src.decoder_optim_step('SGD', gw, gb, LR)
    with pytest.raises(RuntimeError, match="the output layer's optimizer state is RMSprop's: a AdamW step cannot follow"):
        src.decoder_adamw(gw, gb, LR)


# ---- resuming a fit ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gt(tmp_path_factory):
    """Eight lines on one page, batches of four (two steps per epoch), augmentation on, lines scaled to the tiny model's 16 rows."""
    from conformer_ocr_amd.dataset import GroundTruthDataset
    d = tmp_path_factory.mktemp('gt')
    pages = gt_synth.make_pages(str(d), formats=('page',), lines_per_page=8)
    files = [x for x, _, _ in pages]
    data = GroundTruthDataset(files, evaluation_files=files, format_type='xml', batch_size=4, augment=True, seed=1, height=16)
    assert data.n_train == 8 and len(data.plan(0)) == 2
    return files, data


def _fresh_net(data):
    hp = synth.hparams('tiny', num_classes=data.codec.max_label + 1)
    net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1,
                                  codec=data.codec, compute_dtype='bf16')
    state = synth.make_state_dict(hp, seed=1, decoder_gain=1.0)
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return net.to('cuda:0').eval()


@pytest.mark.parametrize('optimizer,freeze', [('AdamW', 0), ('SGD', 0), ('AdamW', 12), ('RMSprop', 12)])
def test_resume_is_exact(gt, tmp_path, optimizer, freeze):
    """fit(epochs=3) against fit(epochs=1) + a fresh model and trainer from the state file run to epoch 3: the same weights, BatchNorm
    statistics, optimizer state, losses, CERs and trainer counters, bit for bit -- the step is deterministic given (seed, global_step)
    (test_dropout_is_reproducible_and_changes_the_step), the batch plan and the augmentation keys depend on (seed, epoch) only.  The
    warm-up (3 steps) crosses the epoch boundary; with freeze_backbone = 12 samples the interruption falls inside the frozen phase
    (two of its three steps done) and the hand-over happens after the resume.  Of a history entry (loss, lines/s, CER) the rate is a
    wall-clock reading and is left out."""
    _, data = gt
    kw = dict(lr=1e-3, weight_decay=1e-2, warmup=3, schedule='reduceonplateau', rop_patience=0, optimizer=optimizer, seed=5, freeze_backbone=freeze)
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    whole = fit(_fresh_net(data), data, epochs=3, output=a, log=None, save_state=True, **kw)
    part = fit(_fresh_net(data), data, epochs=1, output=b, log=None, save_state=True, **kw)
    assert len(part['history']) == 1 and bool(part['trainer'].frozen_steps and not part['trainer']._adopted) == bool(freeze)
    del part
    rest = fit(None, data, epochs=3, output=b, log=None, save_state=True, resume=b + '_state.safetensors')
    assert rest['net'] is not whole['net'] and rest['trainer'].optimizer == optimizer
    assert [(h[0], h[2]) for h in rest['history']] == [(h[0], h[2]) for h in whole['history']] and len(rest['history']) == 3
    assert (rest['best_epoch'], rest['best_cer']) == (whole['best_epoch'], whole['best_cer'])
    for k in Trainer.COUNTERS + Trainer.HYPER:
        assert getattr(rest['trainer'], k) == getattr(whole['trainer'], k), k
    assert whole['trainer'].global_step == 6 and whole['trainer'].frozen_steps == (3 if freeze else 0)
    sa, sb = whole['net'].nn.state_dict(), rest['net'].nn.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    (ta, ma), (tb, mb) = read_state_file(a + '_state.safetensors'), read_state_file(b + '_state.safetensors')
    assert set(ta) == set(tb) and all(torch.equal(ta[k], tb[k]) for k in ta), [k for k in ta if not torch.equal(ta[k], tb[k])]
    assert ma['trainer'] == mb['trainer'] and ma['trainer']['optim']['kind'] == optimizer
    assert bool(ta['slot0'].any())                                                      # (a state worth restoring)
    for e in range(3):
        assert os.path.exists(f'{b}_{e}.safetensors')


def test_resume_refuses_another_data_set_or_model(gt, tmp_path):
    from conformer_ocr_amd.dataset import GroundTruthDataset
    files, data = gt
    out = str(tmp_path / 'm')
    fit(_fresh_net(data), data, epochs=1, output=out, log=None, save_state=True, lr=1e-3, optimizer='SGD')
    other = GroundTruthDataset(files, evaluation_files=files, format_type='xml', batch_size=8, augment=True, seed=1, height=16)
    with pytest.raises(ValueError, match='batch_size is 8, was 4'):
        fit(None, other, epochs=2, output=out, log=None, resume=out + '_state.safetensors')
    hp = synth.hparams('tiny', num_classes=data.codec.max_label + 1, num_encoder_layers=1)
    net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1,
                                  codec=data.codec).to('cuda:0').eval()
    with pytest.raises(ValueError, match='num_encoder_layers'):
        fit(net, data, epochs=2, output=out, log=None, resume=out + '_state.safetensors')
    with pytest.raises(ValueError, match='save_state needs an output'):
        fit(_fresh_net(data), data, epochs=1, output=None, log=None, save_state=True)


@pytest.mark.timeout(600)
def test_train_command_saves_its_state_and_resumes(gt, tmp_path):
    files, _ = gt
    hp = synth.hparams('tiny').as_dict()
    for k in ('num_classes', 'height'):
        hp.pop(k)
    out = str(tmp_path / 'm')
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = [sys.executable, '-m', 'conformer_ocr_amd.train', '-f', 'xml', '-B', '4', '--line-height', '16', '-o', out, '-e', files[0], files[0]]
    r = subprocess.run(common + ['-N', '1', '--warmup', '3', '-r', '1e-3', '--optimizer', 'RMSprop', '--save-state', '--hyper-params', json.dumps(hp)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 1) and 'epoch 0:' in r.stdout, r.stdout + r.stderr[-3000:]          # (1: "did not improve", still a run)
    assert os.path.exists(out + '_state.safetensors') and os.path.exists(out + '_0.safetensors')
    meta = read_state_file(out + '_state.safetensors', tensors=False)[1]
    assert meta['trainer']['optim'] == {'kind': 'RMSprop', 'step': 2, 'dec_steps': 0} and meta['trainer']['hyper']['momentum'] == 0.9
    r = subprocess.run(common + ['-N', '2', '--resume', out + '_state.safetensors'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 1), r.stdout + r.stderr[-3000:]
    assert 'epoch 1:' in r.stdout and 'epoch 0:' not in r.stdout, r.stdout
    assert os.path.exists(out + '_1.safetensors')
    assert read_state_file(out + '_state.safetensors', tensors=False)[1]['trainer']['optim']['step'] == 4
