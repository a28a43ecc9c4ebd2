"""GPU: knowledge distillation.

* the kernel alone: `cocr_distill_loss` against the float64 definition `distill.kd_loss_host`, within max(8 e32, floor) where e32 is the
  error of the definition's own float32 evaluation on the CPU (tests/distill_ref.py); its exact conditions; its argument checks;
* through the step: `cocr_train_step_distill` against float64 autograd through the oracle's train mode + criterion + KD term; the bits
  of `cocr_train_step` at weight 0;
* `train.Trainer` with a real teacher, the frozen window, save and resume, and the step behind torch autograd."""
import os

import numpy as np
import pytest
import torch

from conformer_ocr_amd import _lib, synth
from conformer_ocr_amd.codec import ascii_codec
from conformer_ocr_amd.distill import kd_loss_host
from conformer_ocr_amd.engine import HipRecognizer
from conformer_ocr_amd.pred import PytorchRecognitionModel
from conformer_ocr_amd.spec import model_state_spec
from conformer_ocr_amd.train import Trainer, fit
from tests import distill_ref as R
from tests import gt_synth
from tests.test_hip_train_full import CASES

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def eng():
    """Any finalized model: the kernel belongs to its handle, not to its weights."""
    from tests.hip_util import make_engine
    hp = synth.hparams('tiny')
    return make_engine(hp, synth.make_state_dict(hp, seed=1), 'fp32')


def _misaligned(t):
    """A device copy of `t` whose data pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---- the kernel alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ncls', R.NCLS)
def test_kernel_against_the_float64_definition(eng, ncls):
    for scale in R.SCALES:
        zs, zt = R.logits(ncls, scale)
        ds, dt = zs.to(DEV), zt.to(DEV)
        forms = [('aligned', ds)] + ([('student + 4 bytes', _misaligned(zs))] if scale == 8.0 else [])
        for tau in R.TAUS:
            kd64, g64, kd_tol, g_tol = R.case_reference(ncls, scale, tau)
            for form, s in forms:
                kd, g = eng.distill_loss(s, dt, R.LENS, tau)
                e_kd, e_g = (kd.cpu().double() - kd64).abs(), float((g.cpu().double() - g64).abs().max())
                print(f'ncls {ncls} scale {scale} tau {tau} {form}: |dKD| {e_kd.tolist()} (bound {kd_tol.tolist()}), |dgrad| {e_g:.3e} (bound {g_tol:.3e})')
                assert bool((e_kd <= kd_tol).all()), (scale, tau, form, e_kd.tolist(), kd_tol.tolist())
                assert e_g <= g_tol, (scale, tau, form, e_g, g_tol)
                assert float(kd[1]) == 0.0                                             # the line of length 0
                for n, L in enumerate(R.LENS):
                    assert not bool(g[n, L:].any())                                    # exact zeros behind the line
                kd_only, none = eng.distill_loss(s, dt, R.LENS, tau, with_grad=False)
                assert none is None and torch.equal(kd_only, kd)


@pytest.mark.parametrize('ncls', R.NCLS)
def test_kernel_exact_conditions(eng, ncls):
    zs, zt = R.logits(ncls, 8.0)
    ds, dt = zs.to(DEV), zt.to(DEV)
    for s in (ds, _misaligned(zs)):
        kd, g = eng.distill_loss(s, s.clone() if s is ds else ds, R.LENS, 2.0)          # teacher == student (values)
        assert not bool(kd.any()) and not bool(g.any())
        old = torch.randn(zs.shape, generator=torch.Generator().manual_seed(7), dtype=torch.float32).to(DEV)
        acc = old.clone()
        kd, g = eng.distill_loss(s, s.clone() if s is ds else ds, R.LENS, 2.0, grad=acc, ctc_weight=0.25, kd_weight=0.75)
        assert g is acc and torch.equal(acc, 0.25 * old)                                # q - p is exactly 0 everywhere
    a = eng.distill_loss(ds, dt, R.LENS, 0.5)
    b = eng.distill_loss(ds, dt, R.LENS, 0.5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                          # the same bytes on every call
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()


@pytest.mark.parametrize('ncls', R.NCLS)
def test_kernel_accumulates_the_two_term_gradient(eng, ncls):
    zs, zt = R.logits(ncls, 8.0)
    old = torch.randn(zs.shape, generator=torch.Generator().manual_seed(ncls), dtype=torch.float32)
    for tau in (1.0, 2.0):
        kd64, g64, kd_tol, g_tol = R.case_reference(ncls, 8.0, tau)
        for s in (zs.to(DEV), _misaligned(zs)):
            acc = old.to(DEV)
            kd, g = eng.distill_loss(s, zt.to(DEV), R.LENS, tau, grad=acc, ctc_weight=0.25, kd_weight=0.75)
            want = 0.25 * old.double() + 0.75 * g64
            bound = g_tol                                                              # the bound of the gradient alone
            err = float((acc.cpu().double() - want).abs().max())
            print(f'ncls {ncls} tau {tau}: accumulate |d| {err:.3e} (bound {bound:.3e})')
            assert err <= bound
            assert bool(((kd.cpu().double() - kd64).abs() <= kd_tol).all())
            for n, L in enumerate(R.LENS):
                assert torch.equal(acc[n, L:].cpu(), 0.25 * old[n, L:])                 # exactly ctc_weight x the old value


def test_kernel_refuses_bad_arguments_before_any_launch(eng):
    zs, zt = R.logits(11, 1.0)
    ds, dt = zs.to(DEV), zt.to(DEV)
    lib, h, i32 = eng.lib, eng._h, _lib.C.POINTER(_lib.C.c_int32)
    kd = torch.full((R.N,), 7.0, device=DEV)
    g = torch.full(zs.shape, 7.0, device=DEV)
    lens = np.asarray(R.LENS, dtype=np.int32)

    def call(N=R.N, T=R.T, ncls=11, lens=lens, tau=1.0, cw=1.0, kw=1.0, acc=0, s=ds, t=dt, out=kd):
        return lib.cocr_distill_loss(h, s.data_ptr() if s is not None else None, t.data_ptr() if t is not None else None, N, T, ncls,
                                     lens.ctypes.data_as(i32), tau, out.data_ptr() if out is not None else None, g.data_ptr(), cw, kw, acc, None)
    inf, nan = float('inf'), float('nan')
    bad = [dict(N=0), dict(T=0), dict(ncls=1), dict(lens=np.asarray([19, 0, 20], dtype=np.int32)), dict(lens=np.asarray([19, -1, 7], dtype=np.int32)),
           dict(tau=0.0), dict(tau=-1.0), dict(tau=inf), dict(tau=nan), dict(cw=-0.5), dict(cw=nan), dict(kw=inf), dict(kw=-1.0), dict(acc=2),
           dict(s=None), dict(t=None), dict(out=None)]
    for kw in bad:
        assert call(**kw) == _lib.EINVAL, kw
        assert eng.lib.cocr_last_error()
    assert call(ncls=16385) == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((kd == 7.0).all()) and bool((g == 7.0).all())                           # nothing was launched
    with pytest.raises(ValueError, match='temperature'):
        eng.distill_loss(ds, dt, R.LENS, 0.0)
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert float(kd[1]) == 0.0 and not bool((g == 7.0).any())


# ---- through the step -------------------------------------------------------------------------------------------------------------------
def _case(name):
    c = CASES[name]
    hp = c['hp']()
    state = synth.make_state_dict(hp, seed=c['seed'], decoder_gain=c['gain'])
    image, lens = synth.make_lines(c['n'], hp.height, c['W'], seed=c['seed'], widths=c['widths'])
    tg, tl = [x for s in c['targets'] for x in s], [len(s) for s in c['targets']]
    return c, hp, state, image, lens, tg, tl


def _train_engine(hp, state):
    e = HipRecognizer(hp, torch.device('cuda', 0), 'fp32')
    e.load_state(state)
    e.train_begin()
    return e


def _teacher_logits(e, hp, n, W, seed=99):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, e.out_len(W), hp.num_classes), generator=g, dtype=torch.float32) * 4.0


@pytest.mark.parametrize('name', ['tiny', 'cfg2x2'])
def test_weight_zero_keeps_the_bits_of_the_plain_step(name):
    c, hp, state, image, lens, tg, tl = _case(name)
    x = torch.from_numpy(image[:, 0]).cuda()
    a, b = _train_engine(hp, state), _train_engine(hp, state)
    tz = _teacher_logits(a, hp, c['n'], c['W'])
    loss = a.train_step(x, lens, tg, tl)
    ctc, kd = b.train_step(x, lens, tg, tl, teacher_logits=tz.cuda(), tau=2.0, distill_weight=0.0)
    assert np.float32(ctc).tobytes() == np.float32(loss).tobytes()
    assert torch.equal(a.train_grad_buffer(), b.train_grad_buffer())
    # the reported KD: the kernel's sum on the float64 oracle's train-mode logits (the step's own differ from them by fp32 rounding)
    _, kd64, probits64, _, _ = R.distill_train_grads(hp, state, image, lens, c['targets'], tz, 2.0, 0.0)
    out_lens = [a.out_len(int(w)) for w in lens]
    kdv, _ = b.distill_loss(torch.from_numpy(probits64).float().cuda(), tz.cuda(), out_lens, 2.0, with_grad=False)
    assert abs(kd - float(kdv.sum())) <= 2e-4 * abs(kd), (kd, float(kdv.sum()))
    assert abs(kd - kd64) <= 2e-4 * abs(kd64)
    with pytest.raises(ValueError, match=r'outside \[0, 1\]'):
        b.train_step(x, lens, tg, tl, teacher_logits=tz.cuda(), tau=2.0, distill_weight=1.5)
    with pytest.raises(ValueError, match='temperature'):
        b.train_step(x, lens, tg, tl, teacher_logits=tz.cuda(), tau=0.0, distill_weight=0.5)
    with pytest.raises(ValueError, match='teacher_logits'):
        b.train_step(x, lens, tg, tl, teacher_logits=tz[:, :-1].cuda(), tau=1.0, distill_weight=0.5)


@pytest.mark.parametrize('lam,tau', [(0.5, 1.0), (0.5, 2.0), (1.0, 1.0), (1.0, 2.0)])
@pytest.mark.parametrize('name', ['tiny', 'cfg2x2'])
def test_every_gradient_against_autograd_of_the_oracle_with_a_teacher(name, lam, tau):
    c, hp, state, image, lens, tg, tl = _case(name)
    e = _train_engine(hp, state)
    tz = _teacher_logits(e, hp, c['n'], c['W'])
    ctc64, kd64, probits64, grads64, bn = R.distill_train_grads(hp, state, image, lens, c['targets'], tz, tau, lam)
    ctc, kd = e.train_step(torch.from_numpy(image[:, 0]).cuda(), lens, tg, tl, teacher_logits=tz.cuda(), tau=tau, distill_weight=lam)
    print(f'{name} lambda {lam} tau {tau}: CTC {ctc} ({ctc64}), KD {kd} ({kd64})')
    assert abs(ctc - ctc64) <= 2e-4 * abs(ctc64), (ctc, ctc64)
    assert abs(kd - kd64) <= 2e-4 * abs(kd64), (kd, kd64)
    bad, nparams = {}, 0
    for k, (shape, kind) in model_state_spec(hp).items():
        if kind != 'param':
            continue
        nparams += 1
        got, ref = e.train_grad(k), grads64[k].reshape(shape)
        err = float(np.abs(got - ref).max())
        if not err <= 2e-3 * float(np.abs(ref).max()) + 1e-5:
            bad[k] = (err, float(np.abs(ref).max()))
    assert nparams == len(grads64) and not bad, dict(sorted(bad.items(), key=lambda kv: -kv[1][0])[:12])
    M = probits64.shape[0] * probits64.shape[1]
    for l, (mu, var) in bn.items():
        p = f'encoder.layers.{l}.sequential.2.module.sequential.5.'
        rm = 0.9 * state[p + 'running_mean'].astype(np.float64) + 0.1 * mu.numpy()
        rv = 0.9 * state[p + 'running_var'].astype(np.float64) + 0.1 * var.numpy() * M / (M - 1)
        assert np.abs(e.train_value(p + 'running_mean') - rm).max() <= 1e-5
        assert np.abs(e.train_value(p + 'running_var') - rv).max() <= 1e-5


# ---- the Trainer --------------------------------------------------------------------------------------------------------------------------
def _net(hp, seed, codec=None, dtype='fp32', dropout=0.0, train=False):
    net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=dropout, feed_forward_dropout_p=dropout, attention_dropout_p=dropout,
                                  conv_dropout_p=dropout, codec=codec or ascii_codec(hp.num_classes), compute_dtype=dtype)
    state = synth.make_state_dict(hp, seed=seed, decoder_gain=1.0)
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net = net.to(DEV)
    return net.train() if train else net.eval()


def _tiny_pair(dtype='fp32', **over):
    """(student, teacher of twice the width and one block more with the same classes, batch)."""
    c = CASES['tiny']
    hp = synth.hparams('tiny', **over)
    image, lens = synth.make_lines(c['n'], hp.height, c['W'], seed=c['seed'], widths=c['widths'])
    batch = {'image': torch.from_numpy(image).cuda(), 'seq_lens': torch.from_numpy(lens), 'target': torch.tensor([x for s in c['targets'] for x in s]),
             'target_lens': torch.tensor([len(s) for s in c['targets']])}
    big = synth.hparams('tiny', encoder_dim=64, num_encoder_layers=3, **over)
    return _net(hp, c['seed'], dtype=dtype), _net(big, 17, dtype='fp32'), batch


def test_trainer_learns_from_a_real_teacher():
    net, teacher, batch = _tiny_pair()
    tr = Trainer(net, lr=1e-3, weight_decay=0.0, teacher=teacher, distill_weight=1.0, distill_temperature=2.0)
    kds = []
    for _ in range(12):
        total = tr.training_step(batch)
        assert total == tr.last_kd_loss                                                 # (1 - 1) CTC + 1 KD
        kds.append(tr.last_kd_loss)
    assert np.isfinite(kds).all() and np.isfinite(tr.last_ctc_loss)
    assert kds[-1] < kds[0], kds
    # the gradient window on top: nothing about it changes
    tr2 = Trainer(net, lr=1e-3, teacher=teacher, distill_weight=0.5, distill_temperature=2.0, accumulate_grad_batches=2, gradient_clip_val=1.0)
    for _ in range(4):
        total = tr2.training_step(batch)
        assert abs(total - (0.5 * tr2.last_ctc_loss + 0.5 * tr2.last_kd_loss)) <= 1e-6 * abs(total)
    assert tr2.global_step == 2 and np.isfinite(tr2.last_grad_norm)
    # without a teacher nothing is reported
    tr3 = Trainer(net, lr=1e-3)
    loss = tr3.training_step(batch)
    assert tr3.last_kd_loss is None and tr3.last_ctc_loss == loss
    with pytest.raises(ValueError, match='num_classes'):
        Trainer(net, teacher=_net(synth.hparams('tiny', num_classes=12), 3))
    with pytest.raises(ValueError, match='distill_weight'):
        Trainer(net, teacher=teacher, distill_weight=1.5)


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_frozen_window_combines_the_two_gradients_ahead_of_the_decoder_backward(dtype):
    lam, tau = 0.5, 2.0
    net, teacher, batch = _tiny_pair(dtype)
    before = {k: v.detach().clone() for k, v in net.nn.state_dict().items()}
    tr = Trainer(net, lr=2e-3, weight_decay=1e-2, freeze_backbone=10 ** 9, teacher=teacher, distill_weight=lam, distill_temperature=tau,
                 accumulate_grad_batches=2)
    # the host-combined gradient at the current weights, through the same decoder backward
    o = net.step(batch, with_grad=True)
    tz, _ = teacher.forward(batch['image'], batch['seq_lens'])
    kd_host, g_kd = kd_loss_host(o['probits'], tz, o['output_lens'], tau, torch.float64)
    comb = ((1.0 - lam) * o['grad_probits'].cpu().double() + lam * g_kd).float().cuda()
    gw, gb, _ = net._engine.decoder_backward(comb)
    want = torch.cat([gw.reshape(-1), gb]).cpu().numpy()
    ctc = float(o['loss'])
    total = tr.training_step(batch)
    assert tr.frozen and tr._window == 1
    got = 2.0 * tr._accum.cpu().numpy()                                                 # (the window holds fl(1/2) g)
    np.testing.assert_allclose(got, want, rtol=2e-3, atol=2e-3)
    assert abs(tr.last_ctc_loss - ctc) <= 1e-6 * abs(ctc) and abs(tr.last_kd_loss - float(kd_host.sum())) <= 2e-4 * float(kd_host.sum())
    assert abs(total - ((1 - lam) * tr.last_ctc_loss + lam * tr.last_kd_loss)) <= 1e-6 * abs(total)
    tr.training_step(batch)
    assert tr.global_step == 1 and tr.frozen_steps == 1
    tr.sync_module()
    after = net.nn.state_dict()
    for k, v in after.items():
        if not k.startswith('decoder.'):
            assert torch.equal(v, before[k]), k
    assert not torch.equal(after['decoder.weight'], before['decoder.weight'])


# ---- save and resume ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gt(tmp_path_factory):
    from conformer_ocr_amd.dataset import GroundTruthDataset
    d = tmp_path_factory.mktemp('gt')
    files = [x for x, _, _ in gt_synth.make_pages(str(d), formats=('page',), lines_per_page=8)]
    return files, GroundTruthDataset(files, evaluation_files=files, format_type='xml', batch_size=4, augment=True, seed=1, height=16)


def test_resume_with_a_teacher_is_exact(gt, tmp_path):
    _, data = gt
    hp = synth.hparams('tiny', num_classes=data.codec.max_label + 1)
    big = synth.hparams('tiny', num_classes=data.codec.max_label + 1, encoder_dim=64, num_encoder_layers=3)
    teacher = _net(big, 17, codec=data.codec)
    kw = dict(lr=1e-3, weight_decay=1e-2, warmup=3, seed=5, teacher=teacher, distill_weight=0.5, distill_temperature=2.0)
    a, b = str(tmp_path / 'a'), str(tmp_path / 'b')
    lines = []
    whole = fit(_net(hp, 1, data.codec, 'bf16', 0.1), data, epochs=3, output=a, log=lines.append, save_state=True, **kw)
    assert all('CTC' in l and 'KD' in l for l in lines) and len(lines) == 3
    fit(_net(hp, 1, data.codec, 'bf16', 0.1), data, epochs=2, output=b, log=None, save_state=True, **kw)
    from conformer_ocr_amd.train import read_state_file
    _, meta = read_state_file(b + '_state.safetensors', tensors=False)
    assert meta['distill']['weight'] == 0.5 and meta['distill']['temperature'] == 2.0
    assert meta['distill']['teacher']['hyper_params']['encoder_dim'] == 64
    with pytest.raises(ValueError, match='give the teacher again'):
        fit(None, data, epochs=3, output=b, log=None, resume=b + '_state.safetensors')
    with pytest.raises(ValueError, match='temperature is 4.0, was 2.0'):
        fit(None, data, epochs=3, output=b, log=None, resume=b + '_state.safetensors', teacher=teacher, distill_temperature=4.0)
    with pytest.raises(ValueError, match='teacher differs'):
        fit(None, data, epochs=3, output=b, log=None, resume=b + '_state.safetensors', teacher=_net(hp, 3, data.codec))
    rest = fit(None, data, epochs=3, output=b, log=None, save_state=True, resume=b + '_state.safetensors', teacher=teacher)
    assert len(rest['history']) == 3 and [(h[0], h[2]) for h in rest['history']] == [(h[0], h[2]) for h in whole['history']]
    assert rest['trainer'].distill_weight == 0.5 and rest['trainer'].distill_temperature == 2.0
    with open(a + '_2.safetensors', 'rb') as fa, open(b + '_2.safetensors', 'rb') as fb:
        assert fa.read() == fb.read()
    assert os.path.getsize(a + '_2.safetensors') > 0


def test_train_command_distills_and_resumes(gt, tmp_path):
    """`--teacher` through the command: the log line carries both loss parts, the state file the distill record; `--resume` continues
    with the teacher given again (its refusal without one: test_resume_with_a_teacher_is_exact)."""
    import json
    import subprocess
    import sys
    from conformer_ocr_amd.pred import save_safetensors
    from conformer_ocr_amd.train import read_state_file
    files, data = gt
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    big = synth.hparams('tiny', num_classes=data.codec.max_label + 1, encoder_dim=64, num_encoder_layers=3)
    tpath = str(tmp_path / 'big.safetensors')
    save_safetensors(_net(big, 17, codec=data.codec), tpath)
    hp = synth.hparams('tiny').as_dict()
    for k in ('num_classes', 'height'):
        hp.pop(k)
    out = str(tmp_path / 'm')
    env = dict(os.environ, PYTHONPATH=root)
    common = [sys.executable, '-m', 'conformer_ocr_amd.train', '-f', 'xml', '-B', '4', '--line-height', '16', '-o', out, '-e', files[0], files[0]]
    r = subprocess.run(common + ['-N', '1', '-r', '1e-3', '--warmup', '0', '--save-state', '--hyper-params', json.dumps(hp), '--teacher', tpath,
                                 '--distill-weight', '0.25', '--distill-temperature', '4'], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 1) and 'epoch 0:' in r.stdout and '(CTC ' in r.stdout and 'KD ' in r.stdout, r.stdout + r.stderr[-3000:]
    meta = read_state_file(out + '_state.safetensors', tensors=False)[1]
    assert (meta['distill']['weight'], meta['distill']['temperature']) == (0.25, 4.0)
    r = subprocess.run(common + ['-N', '2', '--resume', out + '_state.safetensors', '--teacher', tpath], cwd=root, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode in (0, 1) and 'epoch 1:' in r.stdout and '(CTC ' in r.stdout, r.stdout + r.stderr[-3000:]
    assert os.path.exists(out + '_1.safetensors')


# ---- behind torch autograd ----------------------------------------------------------------------------------------------------------------
def test_autograd_step_with_a_teacher_leaves_the_engines_gradient():
    from conformer_ocr_amd.autograd import training_step
    c, hp, state, image, lens, tg, tl = _case('tiny')
    net = _net(hp, c['seed'], train=True)
    net.nn.requires_grad_(True)
    batch = {'image': torch.from_numpy(image).cuda(), 'seq_lens': torch.from_numpy(lens), 'target': torch.tensor(tg), 'target_lens': torch.tensor(tl)}
    e = _train_engine(hp, state)
    tz = _teacher_logits(e, hp, c['n'], c['W']).cuda()
    ctc, kd = e.train_step(batch['image'][:, 0], lens, tg, tl, teacher_logits=tz, tau=2.0, distill_weight=0.5)
    loss = training_step(net, batch, teacher_logits=tz, tau=2.0, distill_weight=0.5)
    assert loss.requires_grad and loss.dim() == 0
    assert abs(float(loss.detach()) - (0.5 * ctc + 0.5 * kd)) <= 1e-6 * abs(float(loss.detach()))
    loss.backward()
    for k, p in net.nn.named_parameters():
        assert np.array_equal(p.grad.cpu().numpy(), e.train_grad(k).reshape(tuple(p.shape))), k
    # without the new arguments: the plain step's scalar
    net.nn.zero_grad()
    plain = training_step(net, batch)
    assert abs(float(plain.detach()) - ctc) <= 1e-5 * abs(ctc)
