"""GPU: the gradient window -- cocr_grad_accumulate and cocr_grad_norm on raw vectors, the optimizer step with
the scale fused in, and the Trainer's accumulation, clipping, skipping, resuming, frozen phase and data-parallel ordering.

Model: the `tiny` case widened as tests/test_hip_optim._tiny_case does (a parameter count that is no multiple of 4), dropout 0, three
different batches (synth.make_lines with seeds s, s + 1, s + 2 on the case's widths and targets)."""
import math

import numpy as np
import pytest
import torch

from conformer_ocr_amd import synth
from conformer_ocr_amd.codec import ascii_codec
from conformer_ocr_amd.spec import model_state_spec
from conformer_ocr_amd.train import Trainer, clip_coef
from tests.test_hip_finetune import _assert_decoder, _decoder_grads, _net
from tests.test_hip_optim import LR, WD, _tiny_case, _torch_optimizer
from tests.test_hip_train_full import CASES, _engine

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 3, 4, 255, 256, 257, 4099, 2 ** 20 + 5]
F32 = np.float32


# ---- shared, read-only material -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def model():
    hp, state, names, _, lens, tg, tl = _tiny_case()
    c = CASES['tiny']
    batches = []
    for i in range(3):
        image, l = synth.make_lines(c['n'], hp.height, c['W'], seed=c['seed'] + i, widths=c['widths'])
        batches.append({'image': torch.from_numpy(image).cuda(), 'seq_lens': torch.from_numpy(l), 'target': torch.tensor(tg),
                        'target_lens': torch.tensor(tl)})
    assert not torch.equal(batches[0]['image'], batches[1]['image'])
    return {'hp': hp, 'state': state, 'names': names, 'batches': batches, 'n': c['n']}


@pytest.fixture(scope='module')
def eng(model):
    """An engine for the raw-vector calls (they belong to no model; the methods live on the engine)."""
    return _engine(model['hp'], model['state'])


def _fresh_net(model):
    return _net(model['hp'], model['state'], ascii_codec(model['hp'].num_classes), 'fp32', dropout=0.0)


def _raw_step(e, b, seed=0):
    return e.train_step(b['image'][:, 0], b['seq_lens'].numpy(), b['target'].numpy(), b['target_lens'].numpy(), seed=seed)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _state_of(tr):
    """(values incl. BatchNorm statistics, slot 0, slot 1, the library's step count) as host copies."""
    st = tr.engine.train_optim_state()
    return tr.engine.train_value_buffer().cpu().numpy().copy(), st['slot0'].cpu().numpy().copy(), st['slot1'].cpu().numpy().copy(), st['step']


def _nparam(tr):
    return tr.engine.train_grad_buffer().numel()


def _norm64(arrays):
    return math.sqrt(sum(float(np.sum(np.asarray(a, dtype=np.float64) ** 2)) for a in arrays))


def _accumulate_ref(acc, g, k):
    """The numpy rule of test_grad_accumulate_equals_numpy_float32: A = fl(A + fl(fl(1/k) g))."""
    s = F32(1.0) / F32(k)
    return (acc + (s * g).astype(F32)).astype(F32)


# ---- 1. cocr_grad_accumulate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_grad_accumulate_equals_numpy_float32(eng, n):
    """dst = fl(dst + fl(f32(scale) src)) (or fl(f32(scale) src) with overwrite) against numpy float32, bit for bit, at scale 1/3: views
    at float offsets 0 and 1 of larger allocations in all four combinations (aligned alike: 16 bytes per lane with a scalar head and tail;
    not alike: one by one), and the aliased in-place scale.  The floats around the view keep their values."""
    rng = np.random.default_rng(n)
    scale, pad = 1.0 / 3.0, 8
    for do, so in ((0, 0), (1, 1), (0, 1), (1, 0)):
        for overwrite in (False, True):
            d0, s0 = rng.standard_normal(n + pad).astype(F32), rng.standard_normal(n + pad).astype(F32)
            d, s = torch.from_numpy(d0).cuda(), torch.from_numpy(s0).cuda()
            eng.grad_accumulate(d[do:do + n], s[so:so + n], scale, overwrite=overwrite)
            t = (F32(scale) * s0[so:so + n]).astype(F32)
            want = d0.copy()
            want[do:do + n] = t if overwrite else (d0[do:do + n] + t).astype(F32)
            assert np.array_equal(_bits(d.cpu().numpy()), _bits(want)), (n, do, so, overwrite)
            assert np.array_equal(_bits(s.cpu().numpy()), _bits(s0))
    for off in (0, 1):
        a0 = rng.standard_normal(n + pad).astype(F32)
        a = torch.from_numpy(a0).cuda()
        v = a[off:off + n]
        eng.grad_accumulate(v, v, scale, overwrite=True)
        want = a0.copy()
        want[off:off + n] = (F32(scale) * a0[off:off + n]).astype(F32)
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(want)), (n, off)


# ---- 2. cocr_grad_norm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_grad_norm_is_the_float64_norm_and_repeats(eng, n):
    """Within 1e-9 relative of sqrt(sum(float64(g)^2)): the terms are non-negative and summed in double, so each sum is off by at most
    (n - 1) 2^-53 relative, 1.2e-10 at 2^20, and numpy's own error has that order.  Two calls give the same bits, and so does the same
    data at another alignment (the result is a function of the values and n alone).  Zeros give 0."""
    rng = np.random.default_rng(100 + n)
    g0 = (rng.standard_normal(n) * 3.0).astype(F32)
    want = math.sqrt(float(np.sum(g0.astype(np.float64) ** 2)))
    got = []
    for off in (0, 1):
        base = torch.zeros(n + 8, dtype=torch.float32, device='cuda')
        base[off:off + n] = torch.from_numpy(g0).cuda()
        v = base[off:off + n]
        a, b = eng.grad_norm(v), eng.grad_norm(v)
        assert a == b and math.copysign(1.0, a) == 1.0
        assert abs(a - want) <= 1e-9 * want, (n, off, a, want)
        got.append(a)
    assert got[0] == got[1]
    assert eng.grad_norm(torch.zeros(n + 1, dtype=torch.float32, device='cuda')[1:]) == 0.0


def test_grad_norm_edge_values(eng):
    """Buffers of 1e30 / 1e-30 (their squares overflow / vanish in float32) give sqrt(n) |v| -- exactly where that is a double (n = 1, 4:
    v^2 and 4 v^2 are exact in double and sqrt is correctly rounded), within 1e-9 elsewhere; one +Inf gives inf, one NaN gives NaN, Inf
    and NaN give NaN, wherever in the buffer they sit."""
    for v in (1e30, 1e-30, -1e30):
        fv = abs(float(F32(v)))
        for n in (1, 4):
            assert eng.grad_norm(torch.full((n,), v, dtype=torch.float32, device='cuda')) == math.sqrt(n) * fv
        for n in (257, 4099, 70001):
            got = eng.grad_norm(torch.full((n,), v, dtype=torch.float32, device='cuda'))
            assert abs(got - math.sqrt(n) * fv) <= 1e-9 * math.sqrt(n) * fv, (v, n, got)
    for n in (5, 4099, 2 ** 20 + 5):
        for at in sorted({0, n // 2, n - 1}):
            g = torch.ones(n, dtype=torch.float32, device='cuda')
            g[at] = float('inf')
            assert eng.grad_norm(g) == float('inf')
            g[at] = float('-inf')
            assert eng.grad_norm(g) == float('inf')
            g[(at + 1) % n] = float('nan')
            assert math.isnan(eng.grad_norm(g))
            g[at] = 1.0
            assert math.isnan(eng.grad_norm(g))


def test_grad_norm_of_the_gradient_vector_sees_zero_padding(model):
    """The norm of the flat gradient vector (every tensor padded to 16 bytes) equals the norm of the per-name gradients within the 1e-9
    of test_grad_norm_is_the_float64_norm_and_repeats: a padding float that is not zero would show."""
    e = _engine(model['hp'], model['state'])
    for b in model['batches'][:2]:                       # (the second step writes over what the first left in the vector)
        _raw_step(e, b)
        want = _norm64([e.train_grad(k) for k in model['names']])
        got = e.grad_norm(e.train_grad_buffer())
        assert want > 0 and abs(got - want) <= 1e-9 * want, (got, want)
    assert e.train_grad_buffer().numel() > sum(int(np.prod(model_state_spec(model['hp'])[k][0])) for k in model['names'])      # (there IS padding)


# ---- 3. the fused scale ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,momentum', [('AdamW', 0.0), ('Adam', 0.0), ('SGD', 0.9), ('SGD', 0.0), ('RMSprop', 0.9), ('RMSprop', 0.0)])
def test_fused_scale_equals_scaling_in_place_first(model, kind, momentum):
    """train_optim_step(grad_scale=c) against grad_accumulate(G, G, c, overwrite) + the plain step: values and both slots bit for bit,
    over two steps (the second on slots that are no longer zero); c = 1.0 and grad = a clone of the own vector equal the plain entry."""
    c = 0.37
    fused, plain, own, unit = (_engine(model['hp'], model['state']) for _ in range(4))
    for step in range(2):
        b = model['batches'][step]
        assert _raw_step(fused, b) == _raw_step(plain, b) and _raw_step(own, b) == _raw_step(unit, b)
        fused.train_optim_step(kind, LR, weight_decay=WD, momentum=momentum, grad_scale=c)
        g = plain.train_grad_buffer()
        plain.grad_accumulate(g, g, c, overwrite=True)
        plain.train_optim_step(kind, LR, weight_decay=WD, momentum=momentum)
        own.train_optim_step(kind, LR, weight_decay=WD, momentum=momentum)
        unit.train_optim_step(kind, LR, weight_decay=WD, momentum=momentum, grad=unit.train_grad_buffer().clone(), grad_scale=1.0)
        for a, bb in ((fused, plain), (unit, own)):
            sa, sb = a.train_optim_state(), bb.train_optim_state()
            assert torch.equal(a.train_value_buffer(), bb.train_value_buffer()), (kind, step)
            assert torch.equal(sa['slot0'], sb['slot0']) and torch.equal(sa['slot1'], sb['slot1']), (kind, step)
            assert sa['step'] == sb['step'] == step + 1
    assert not torch.equal(fused.train_value_buffer(), own.train_value_buffer())        # (the scale did something)
    before = fused.train_value_buffer().clone()
    for bad in (-1.0, float('inf')):
        with pytest.raises(ValueError, match='invalid grad_scale'):                      # COCR_EINVAL, nothing stepped
            fused.train_optim_step(kind, LR, momentum=momentum, grad_scale=bad)
    assert torch.equal(fused.train_value_buffer(), before) and fused.train_optim_state()['step'] == 2


# ---- 4. a window against torch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,momentum', [('AdamW', 0.0), ('SGD', 0.9)])
def test_a_clipped_window_follows_torch(model, kind, momentum):
    """k = 3, four calls: one full window and one flushed window of a single batch, gradient_clip_val = half the first window's norm.
    Reference: torch.optim on the CPU fed the device's own per-call gradients (for the reason
    test_adamw_steps_follow_torch_and_lower_the_loss gives), accumulated by the numpy rule of
    test_grad_accumulate_equals_numpy_float32, scaled by clip_coef of their float64 norm, then opt.step().  Every parameter within 2e-6
    absolute after each optimizer step (test_each_kind_follows_torch's bound, for its reason: the coefficient enters only through
    updates <= 1e-2).  global_step and the rate under a 3-step warm-up advance per optimizer step; last_grad_norm is the reference
    norm within 1e-9."""
    names, batches = model['names'], model['batches']
    calls = [batches[0], batches[1], batches[2], batches[1]]
    pre = _engine(model['hp'], model['state'])                 # the first window's gradients do not depend on anything a step changes
    acc = {k: np.zeros(model_state_spec(model['hp'])[k][0], F32) for k in names}
    for b in calls[:3]:
        _raw_step(pre, b)
        acc = {k: _accumulate_ref(acc[k], pre.train_grad(k), 3) for k in names}
    clip = 0.5 * _norm64(acc.values())
    tr = Trainer(_fresh_net(model), lr=LR, weight_decay=WD, optimizer=kind, momentum=momentum, warmup=3, accumulate_grad_batches=3,
                 gradient_clip_val=clip)
    tparams = {k: torch.tensor(np.asarray(model['state'][k], dtype=F32), requires_grad=True) for k in names}
    opt = _torch_optimizer(kind, list(tparams.values()), momentum)

    def reference_step(acc, lr):
        norm = _norm64(acc.values())
        coef = F32(clip_coef(norm, clip))
        for k in names:
            tparams[k].grad = torch.from_numpy((coef * acc[k]).astype(F32).reshape(tparams[k].shape))
        for group in opt.param_groups:
            group['lr'] = lr
        opt.step()
        assert abs(tr.last_grad_norm - norm) <= 1e-9 * norm, (tr.last_grad_norm, norm)
        worst = max(float(np.abs(tr.engine.train_value(k) - tparams[k].detach().numpy()).max()) for k in names)
        bad = {k: e for k in names if not (e := float(np.abs(tr.engine.train_value(k) - tparams[k].detach().numpy()).max())) <= 2e-6}
        assert not bad, dict(sorted(bad.items(), key=lambda kv: -kv[1])[:8])
        return norm, float(coef), worst

    acc = {k: np.zeros_like(v) for k, v in acc.items()}
    assert tr.lr == LR and tr.last_grad_norm is None
    for i, b in enumerate(calls[:3]):
        lr = tr.lr
        tr.training_step(b)
        acc = {k: _accumulate_ref(acc[k], tr.engine.train_grad(k), 3) for k in names}
        assert tr.global_step == (1 if i == 2 else 0) and tr.batches_seen == i + 1
        assert tr.lr == (LR if i < 2 else min(1.0, 1 / 3) * LR)
    norm, coef, worst = reference_step(acc, lr)
    assert coef < 0.51 and tr.engine.train_optim_state()['step'] == 1
    print(f'{kind}: window 1 norm {norm:.6e} coefficient {coef:.6f}, largest parameter error {worst:.3e}')
    acc = {k: np.zeros_like(v) for k, v in acc.items()}
    lr = tr.lr
    tr.training_step(calls[3])
    acc = {k: _accumulate_ref(acc[k], tr.engine.train_grad(k), 3) for k in names}
    assert tr.global_step == 1 and tr.lr == lr and tr.engine.train_optim_state()['step'] == 1      # (an open window moves nothing)
    tr.flush()
    norm, coef, worst = reference_step(acc, lr)
    print(f'{kind}: flushed window norm {norm:.6e} coefficient {coef:.6f}, largest parameter error {worst:.3e}')
    assert tr.global_step == 2 and tr.lr == min(1.0, 2 / 3) * LR and tr.batches_seen == 4 and tr.samples_seen == 4 * model['n']
    tr.flush()                                                 # (nothing open: nothing happens)
    assert tr.global_step == 2 and tr.engine.train_optim_state()['step'] == 2


# ---- 5. an inactive clip is free ---------------------------------------------------------------------------------------------------------
def test_an_inactive_clip_changes_no_bit(model):
    """gradient_clip_val = 1e30 (coefficient exactly 1.0), a Trainer with accumulate_grad_batches = 1 and nothing else, and a manual
    train_step + train_optim_step sequence end bit-identical after three steps; the first reports a finite norm."""
    clipped = Trainer(_fresh_net(model), lr=LR, weight_decay=WD, gradient_clip_val=1e30, seed=3)
    plain = Trainer(_fresh_net(model), lr=LR, weight_decay=WD, accumulate_grad_batches=1, seed=3)
    manual = _engine(model['hp'], model['state'])
    for i, b in enumerate(model['batches']):
        la, lb = clipped.training_step(b), plain.training_step(b)
        lc = _raw_step(manual, b, seed=3 * 1000003 + i)
        manual.train_optim_step('AdamW', LR, weight_decay=WD)
        assert la == lb == lc
        assert math.isfinite(clipped.last_grad_norm) and clipped.last_grad_norm > 0 and plain.last_grad_norm is None
    a, b = _state_of(clipped), _state_of(plain)
    st = manual.train_optim_state()
    c = (manual.train_value_buffer().cpu().numpy(), st['slot0'].cpu().numpy(), st['slot1'].cpu().numpy(), st['step'])
    for x, y, z in zip(a[:3], b[:3], c[:3]):
        assert np.array_equal(_bits(x), _bits(y)) and np.array_equal(_bits(x), _bits(z))
    assert a[3] == b[3] == c[3] == 3 and clipped.global_step == plain.global_step == 3


# ---- 6. skipping a window whose norm is not finite ------------------------------------------------------------------------------------------
def _poison_second_call(tr):
    """After the second real `train_step` of `tr`'s engine, element 5 of the gradient vector becomes +Inf (a float value)."""
    real, calls = tr.engine.train_step, []

    def train_step(*a, **kw):
        loss = real(*a, **kw)
        calls.append(loss)
        if len(calls) == 2:
            tr.engine.train_grad_buffer()[5] = float('inf')
        return loss
    tr.engine.train_step = train_step


def test_a_window_with_an_infinite_gradient_is_skipped(model):
    """skip_nonfinite: the poisoned second call moves no parameter, no slot, neither step count; skipped_steps counts it and the log gets
    a line; the third, clean call steps, and the final parameters and slots equal a run that was never given the second batch, bit for
    bit.  (The BatchNorm running statistics behind the parameters in the value vector did see the skipped batch's forward, as under
    torch; they are left out of both comparisons.)"""
    b = model['batches']
    log = []
    tr = Trainer(_fresh_net(model), lr=LR, weight_decay=WD, optimizer='SGD', momentum=0.9, skip_nonfinite=True, log=log.append)
    _poison_second_call(tr)
    n = _nparam(tr)
    tr.training_step(b[0])
    before = _state_of(tr)
    assert tr.global_step == 1 and math.isfinite(tr.last_grad_norm)
    tr.training_step(b[1])
    after = _state_of(tr)
    assert tr.last_grad_norm == float('inf') and tr.skipped_steps == 1 and tr.global_step == 1 and tr.batches_seen == 2
    assert np.array_equal(_bits(before[0][:n]), _bits(after[0][:n]))
    assert np.array_equal(_bits(before[1]), _bits(after[1])) and np.array_equal(_bits(before[2]), _bits(after[2])) and before[3] == after[3] == 1
    assert len(log) == 1 and 'skipped' in log[0]
    tr.training_step(b[2])
    assert tr.global_step == 2 and tr.skipped_steps == 1 and math.isfinite(tr.last_grad_norm)
    other = Trainer(_fresh_net(model), lr=LR, weight_decay=WD, optimizer='SGD', momentum=0.9, skip_nonfinite=True)
    other.training_step(b[0])
    other.training_step(b[2])
    x, y = _state_of(tr), _state_of(other)
    assert np.array_equal(_bits(x[0][:n]), _bits(y[0][:n])) and np.array_equal(_bits(x[1]), _bits(y[1])) and np.array_equal(_bits(x[2]), _bits(y[2]))
    assert x[3] == y[3] == 2 and not np.array_equal(_bits(x[0][:n]), _bits(before[0][:n]))


def test_clipping_refuses_an_infinite_gradient(model):
    """Clipping on, skip_nonfinite off: the poisoned call raises FloatingPointError naming the step and leaves parameters, slots and
    both step counts as they were; the next call trains on."""
    b = model['batches']
    tr = Trainer(_fresh_net(model), lr=LR, weight_decay=WD, gradient_clip_val=1.0)
    _poison_second_call(tr)
    n = _nparam(tr)
    tr.training_step(b[0])
    before = _state_of(tr)
    with pytest.raises(FloatingPointError, match='optimizer step 1 is inf'):
        tr.training_step(b[1])
    after = _state_of(tr)
    assert np.array_equal(_bits(before[0][:n]), _bits(after[0][:n]))
    assert np.array_equal(_bits(before[1]), _bits(after[1])) and np.array_equal(_bits(before[2]), _bits(after[2])) and before[3] == after[3] == 1
    assert tr.global_step == 1 and tr.skipped_steps == 0
    tr.training_step(b[2])
    assert tr.global_step == 2 and math.isfinite(tr.last_grad_norm)


# ---- 7. resuming inside a window --------------------------------------------------------------------------------------------------------
def test_a_state_taken_inside_a_window_resumes_exactly(model):
    """state_dict() after the second call of a k = 3 window into a fresh Trainer on a fresh net; the window is finished and one more run
    on both: values (BatchNorm statistics included), slots and counters bit-identical to the uninterrupted run."""
    b = model['batches']
    kw = dict(lr=LR, weight_decay=WD, optimizer='SGD', momentum=0.9, warmup=3, accumulate_grad_batches=3, seed=2)
    whole = Trainer(_fresh_net(model), gradient_clip_val=0.5, **kw)
    whole.training_step(b[0])
    whole.training_step(b[1])
    sd = whole.state_dict()
    assert sd['counters']['_window'] == 2 and sd['accum'].numel() == _nparam(whole) and bool(sd['accum'].any())
    rest = Trainer(_fresh_net(model), **kw)                    # (the clip value comes with the state)
    rest.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in sd.items()})
    assert rest.gradient_clip_val == 0.5 and rest.batches_seen == 2 and rest.global_step == 0
    for tr in (whole, rest):
        for x in (b[2], b[1], b[0], b[2]):
            tr.training_step(x)
    assert whole.global_step == rest.global_step == 2 and whole.last_grad_norm == rest.last_grad_norm
    x, y = _state_of(whole), _state_of(rest)
    for p, q in zip(x[:3], y[:3]):
        assert np.array_equal(_bits(p), _bits(q))
    assert x[3] == y[3] == 2
    for k in Trainer.COUNTERS + Trainer.HYPER:
        assert getattr(whole, k) == getattr(rest, k), k
    assert 'accum' not in whole.state_dict()


# ---- 8. the frozen phase ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('clipped', [False, True])
def test_frozen_windows_accumulate_and_hand_over_between_windows(model, clipped):
    """freeze_backbone = the lines of 3 batches, k = 2: the threshold falls inside the second window, so both windows run frozen -- no
    encoder parameter or BatchNorm statistic moves -- and the hand-over happens at the fifth call.  The output layer follows
    torch.optim.AdamW fed the device's own (gw, gb), accumulated by the numpy rule and (clipped) scaled by clip_coef of their float64
    norm at half the first window's norm, within tests/test_hip_finetune._assert_decoder's bound."""
    b, n = model['batches'], model['n']
    calls = [b[0], b[1], b[2], b[0]]
    net = _fresh_net(model)
    clip = None
    if clipped:
        acc = [0, 0]
        for x in calls[:2]:
            acc = [_accumulate_ref(a, g.numpy(), 2) for a, g in zip(acc, _decoder_grads(net, x))]
        clip = 0.5 * _norm64(acc)
    before = {k: v.detach().clone() for k, v in net.nn.state_dict().items()}
    tr = Trainer(net, lr=2e-3, weight_decay=1e-2, freeze_backbone=3 * n, accumulate_grad_batches=2, gradient_clip_val=clip)
    W = torch.nn.Parameter(net.nn['decoder'].weight.detach().cpu().clone())
    bias = torch.nn.Parameter(net.nn['decoder'].bias.detach().cpu().clone())
    opt = torch.optim.AdamW([W, bias], lr=2e-3, weight_decay=1e-2)
    for w in range(2):
        acc = [0, 0]
        for x in calls[2 * w:2 * w + 2]:
            acc = [_accumulate_ref(a, g.numpy(), 2) for a, g in zip(acc, _decoder_grads(net, x))]
            tr.training_step(x)
        norm = _norm64(acc)
        coef = F32(clip_coef(norm, clip)) if clipped else F32(1.0)
        W.grad, bias.grad = (torch.from_numpy((coef * a).astype(F32)) for a in acc)
        opt.step()
        if clipped:
            assert abs(tr.last_grad_norm - norm) <= 1e-9 * norm and (coef < 0.51 if w == 0 else True)
        else:
            assert tr.last_grad_norm is None
        assert tr.frozen_steps == tr.global_step == w + 1 and tr.frozen_batches == 2 * w + 2 and not tr._adopted
        tr.sync_module()
        _assert_decoder(net, W, bias)
    assert tr.samples_seen == 4 * n and not tr.frozen
    after = net.nn.state_dict()
    for k, v in after.items():
        if not k.startswith('decoder.'):
            assert torch.equal(v, before[k]), k
    assert not torch.equal(after['decoder.weight'], before['decoder.weight'])
    assert net._engine.decoder_optim_state()['step'] == 2
    tr.training_step(b[1])                                     # the fifth call opens a whole-network window
    assert tr._adopted and tr.global_step == 2 and tr.frozen_batches == 4
    tr.flush()
    st = tr.engine.train_optim_state()
    assert tr.global_step == 3 and (st['step'], st['dec_steps']) == (1, 2)
    tr.sync_module()
    moved = [k for k, v in net.nn.state_dict().items() if not k.startswith('decoder.') and not torch.equal(v, before[k])]
    assert moved
    assert int(net.nn.state_dict()[[k for k in before if k.endswith('num_batches_tracked')][0]]) == 1      # (one train-mode forward)


# ---- 9. one collective per optimizer step ---------------------------------------------------------------------------------------------------
def test_data_parallel_reduces_once_per_optimizer_step(model, monkeypatch):
    """torch.distributed.all_reduce replaced by a counting no-op, a world of one: six calls at k = 3 reduce twice, each time the whole
    accumulation vector."""
    seen = []
    monkeypatch.setattr(torch.distributed, 'all_reduce', lambda t, op=None, group=None: seen.append(t.numel()))
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda group=None: 1)
    tr = Trainer(_fresh_net(model), lr=LR, weight_decay=WD, accumulate_grad_batches=3, distributed=True)
    for i in range(6):
        tr.training_step(model['batches'][i % 3])
        assert len(seen) == (i + 1) // 3
    assert seen == [_nparam(tr)] * 2 and tr.global_step == 2
