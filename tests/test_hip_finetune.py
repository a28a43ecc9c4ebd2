"""GPU: fine-tuning a loaded model -- the resized output layer on the device, the frozen-backbone phase of
`train.Trainer` against torch.optim.AdamW, its hand-over into the whole-network step (per-tensor AdamW step counts), and the whole
route end to end: a recognizer trained on 24 glyphs learns 8 more."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conformer_ocr_amd import synth
from conformer_ocr_amd.codec import PytorchCodec, ascii_codec, resize_codec
from conformer_ocr_amd.pred import PytorchRecognitionModel, resize_output, save_safetensors
from conformer_ocr_amd.spec import model_state_spec
from conformer_ocr_amd.train import Trainer
from tests import gt_synth, page_synth
from tests.test_hip_parity import FP32_TOL, _log
from tests.test_hip_train_full import CASES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(hp, state, codec, dtype='bf16', dropout=0.1):
    net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=dropout, feed_forward_dropout_p=dropout, attention_dropout_p=dropout,
                                  conv_dropout_p=dropout, codec=codec, compute_dtype=dtype)
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return net.to('cuda:0').eval()


def _tiny_net(dtype, dropout=0.1):
    c = CASES['tiny']
    hp = c['hp']()
    state = synth.make_state_dict(hp, seed=c['seed'], decoder_gain=1.0)
    image, lens = synth.make_lines(c['n'], hp.height, c['W'], seed=c['seed'], widths=c['widths'])
    batch = {'image': torch.from_numpy(image).cuda(), 'seq_lens': torch.from_numpy(lens), 'target': torch.tensor([x for s in c['targets'] for x in s]),
             'target_lens': torch.tensor([len(s) for s in c['targets']])}
    return _net(hp, state, ascii_codec(hp.num_classes), dtype, dropout), hp, batch


# ---- the resized output layer on the device ---------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize('name', ['tiny', 'cfg1'])
def test_logits_after_surgery_match_the_oracle_on_the_resized_state(case, name):
    """fp32 logits of the resized model against the CPU oracle run on the RESIZED state dict, within the project's fp32 bound; the
    largest difference between the kept columns and the base model's own columns goes to the parity log (expected 0; recorded)."""
    from oracle.conformer_ref import Oracle
    hp, state, image, lens, _ = case(name)
    net = _net(hp, state, ascii_codec(hp.num_classes), 'fp32')
    x, l = torch.from_numpy(image).cuda(), torch.from_numpy(lens)
    base, _ = net.forward(x, l)
    base = base.cpu().numpy()
    new, row_map = resize_codec(net.codec, ['一丁!', '丂'], 'union', hp.num_classes)
    assert len(row_map) == hp.num_classes + 3
    resize_output(net, new, row_map, seed=3)
    got, got_lens = net.forward(x, l)                       # (the device model re-packs by itself)
    got = got.cpu().numpy()
    assert got.shape[-1] == hp.num_classes + 3
    hp2 = net.hparams_record
    state2 = {k: v.detach().cpu().numpy() for k, v in net.nn.state_dict().items()}
    want, want_lens = Oracle(hp2, state2).forward(torch.from_numpy(image), torch.from_numpy(lens))
    assert got_lens.tolist() == want_lens.tolist()
    dev = float(np.abs(got - want.numpy()).max())
    kept = float(np.abs(got[..., :hp.num_classes] - base).max())
    _log('finetune_logits_after_surgery', {'case': name, 'classes': int(hp2.num_classes), 'dev_vs_oracle': dev, 'kept_columns_vs_base': kept})
    print(f'{name}: max |dlogit| vs oracle {dev:.3e}; kept columns vs base {kept:.3e}')
    assert dev <= FP32_TOL


# ---- the frozen phase ---------------------------------------------------------------------------------------------------------------
def _decoder_grads(net, batch):
    """The device's own gradients of the output layer at the current weights (what the frozen step is about to apply)."""
    o = net.step(batch, with_grad=True)
    gw, gb, _ = net._engine.decoder_backward(o['grad_probits'])
    return gw.cpu().clone(), gb.cpu().clone()


def _torch_decoder(net, **kw):
    W = torch.nn.Parameter(net.nn['decoder'].weight.detach().cpu().clone())
    b = torch.nn.Parameter(net.nn['decoder'].bias.detach().cpu().clone())
    return W, b, torch.optim.AdamW([W, b], **kw)


def _emulated_frozen_step(tr, net, batch, W, b, opt):
    W.grad, b.grad = _decoder_grads(net, batch)
    for g in opt.param_groups:
        g['lr'] = tr.lr
    opt.step()
    assert tr.frozen
    return tr.training_step(batch)


def _assert_decoder(net, W, b):
    sd = net.nn.state_dict()
    np.testing.assert_allclose(sd['decoder.weight'].cpu().numpy(), W.detach().numpy(), rtol=2e-6, atol=2e-7)
    np.testing.assert_allclose(sd['decoder.bias'].cpu().numpy(), b.detach().numpy(), rtol=2e-6, atol=2e-7)


@pytest.mark.timeout(300)
@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_frozen_phase_moves_the_output_layer_only_and_follows_torch_adamw(dtype):
    """Three frozen steps (warm-up running): every state-dict entry but decoder.* is bit-identical afterwards, `num_batches_tracked`
    included; decoder.* equals torch.optim.AdamW fed the device's own gradients within the bounds of `test_adamw_matches_torch`."""
    net, hp, batch = _tiny_net(dtype)
    before = {k: v.detach().clone() for k, v in net.nn.state_dict().items()}
    tr = Trainer(net, lr=2e-3, weight_decay=1e-2, warmup=2, freeze_backbone=10 ** 9)
    W, b, opt = _torch_decoder(net, lr=2e-3, weight_decay=1e-2)
    lrs, losses = [], []
    for _ in range(3):
        lrs.append(tr.lr)
        losses.append(_emulated_frozen_step(tr, net, batch, W, b, opt))
    np.testing.assert_allclose(lrs, [2e-3, 1e-3, 2e-3], rtol=1e-12)              # the whole-network step's warm-up arithmetic
    assert tr.global_step == 3 and tr.frozen_steps == 3 and tr.samples_seen == 3 * batch['image'].shape[0]
    assert all(np.isfinite(losses))
    eng = net._engine
    tr.sync_module()
    after = net.nn.state_dict()
    assert list(after) == list(before)
    for k, v in after.items():
        if not k.startswith('decoder.'):
            assert torch.equal(v, before[k]), k
    assert not torch.equal(after['decoder.weight'], before['decoder.weight'])
    _assert_decoder(net, W, b)
    assert net.engine() is eng                                                   # kept, with its AdamW state


@pytest.mark.timeout(300)
def test_frozen_phase_keeps_its_moments_across_a_validation_pass():
    """frozen step, sync_module, a prediction through the serving path, frozen step: still the torch emulation's two-step result (a
    re-pack between the steps would have zeroed the moments and restarted the bias corrections)."""
    net, hp, batch = _tiny_net('bf16')
    tr = Trainer(net, lr=2e-3, weight_decay=1e-2, freeze_backbone=10 ** 9)
    W, b, opt = _torch_decoder(net, lr=2e-3, weight_decay=1e-2)
    _emulated_frozen_step(tr, net, batch, W, b, opt)
    eng = net._engine
    tr.sync_module()
    recs = net.predict_labels(batch['image'], batch['seq_lens'])
    assert len(recs) == batch['image'].shape[0] and net._engine is eng
    other = dict(batch, target=batch['target'].flip(0), target_lens=batch['target_lens'].flip(0))      # (a gradient unlike the first step's)
    _emulated_frozen_step(tr, net, other, W, b, opt)
    tr.sync_module()
    _assert_decoder(net, W, b)


# ---- the hand-over ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_hand_over_keeps_per_tensor_adamw_state():
    """Two frozen batches, then two whole-network steps (dropout 0), against ONE torch.optim.AdamW over all parameters in which only
    decoder.* carry gradients during the frozen steps -- so torch's per-parameter `state['step']` is 3 for the output layer and 1 for
    everything else at the first whole-network step.  Fed the device's gradients; every parameter within 2e-6 absolute."""
    net, hp, batch = _tiny_net('fp32', dropout=0.0)
    n = int(batch['image'].shape[0])
    lr = 1e-3
    tr = Trainer(net, lr=lr, weight_decay=1e-2, freeze_backbone=2 * n)
    names = [k for k, (_, kind) in model_state_spec(hp).items() if kind == 'param']
    sd = net.nn.state_dict()
    tparams = {k: torch.nn.Parameter(sd[k].detach().cpu().clone()) for k in names}
    opt = torch.optim.AdamW(list(tparams.values()), lr=lr, weight_decay=1e-2)
    for step in range(2):
        tparams['decoder.weight'].grad, tparams['decoder.bias'].grad = _decoder_grads(net, batch)
        opt.step()
        assert tr.frozen
        tr.training_step(batch)
        st = net._engine.decoder_state()
        for k in ('decoder.weight', 'decoder.bias'):
            assert np.abs(st[k] - tparams[k].detach().numpy()).max() <= 2e-6, (step, k)
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
    print('hand-over: largest parameter error', max(worst.values()), 'decoder.weight', worst['decoder.weight'])
    bad = {k: e for k, e in worst.items() if not e <= 2e-6}
    assert not bad, dict(sorted(bad.items(), key=lambda kv: -kv[1])[:8])
    assert {opt.state[tparams['decoder.weight']]['step'].item(), opt.state[tparams[names[0]]]['step'].item()} == {4.0, 2.0}
    assert tr.global_step == 4 and tr.frozen_steps == 2
    tr.sync_module()
    sd = net.nn.state_dict()
    np.testing.assert_allclose(sd['decoder.weight'].cpu().numpy(), tparams['decoder.weight'].detach().numpy(), rtol=0, atol=2e-6)
    tracked = [int(v) for k, v in sd.items() if k.endswith('num_batches_tracked')]
    assert tracked and all(t == 2 for t in tracked)                                # train-mode forwards only


@pytest.mark.timeout(300)
def test_adopt_decoder_refuses_what_it_cannot_do_and_takes_a_source_that_never_stepped():
    from tests.hip_util import make_engine
    from conformer_ocr_amd.engine import HipRecognizer
    c = CASES['tiny']
    hp = c['hp']()
    state = synth.make_state_dict(hp, seed=c['seed'], decoder_gain=1.0)
    src = make_engine(hp, state, 'bf16')
    dst = HipRecognizer(hp, torch.device('cuda', 0), 'fp32')
    dst.load_state(state)
    with pytest.raises(RuntimeError):
        dst.train_adopt_decoder(src)                                               # COCR_ESTATE: no training state
    dst.train_begin()
    hp2 = synth.hparams('tiny', num_classes=hp.num_classes + 2)
    other = make_engine(hp2, synth.make_state_dict(hp2, seed=1), 'bf16')
    with pytest.raises(ValueError):
        dst.train_adopt_decoder(other)                                             # COCR_EINVAL: shapes differ
    state2 = dict(state)
    state2['decoder.weight'] = np.asarray(state['decoder.weight']) * np.float32(0.5)
    fresh = make_engine(hp, state2, 'bf16')
    dst.train_adopt_decoder(fresh)                                                 # never stepped: values, zero moments, k = 0
    assert np.array_equal(dst.train_value('decoder.weight'), state2['decoder.weight'])
    assert np.array_equal(dst.train_value('decoder.bias'), np.asarray(state['decoder.bias'], np.float32))
    name = 'encoder.layers.0.sequential.0.module.sequential.1.linear.weight'
    assert np.array_equal(dst.train_value(name), np.asarray(state[name], np.float32))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
ALPHABET = [chr(ord('a') + i) for i in range(26)] + list('ABCDEF')                # glyph g (label g + 1) is written ALPHABET[g]


def render_lines(n, height, width, seed, allowed, first=None):
    """`synth.make_text_lines` over ONE 32-glyph alphabet (`synth.text_alphabet(3, 32)`) with the glyphs of a line drawn from `allowed`
    (glyph indices); `first`: the glyphs the first character of every line is drawn from.  Returns (image (N,1,H,W) float32,
    seq_lens, texts: one string over ALPHABET per line)."""
    pats = synth.text_alphabet(3, 32)
    g = np.random.default_rng([seed, 0xF17E])
    img = np.zeros((n, height, width), dtype=np.float32)
    cell_h = -(-height // 6)
    texts = []
    for i in range(n):
        x, txt = int(g.integers(8, 20)), []
        while True:
            pool = first if (first is not None and not txt) else allowed
            a = int(pool[int(g.integers(0, len(pool)))])
            p, w = pats[a]
            if x + w + 8 > width:
                break
            img[i, :, x:x + w] = np.kron(p, np.ones((cell_h, -(-w // 4)), dtype=np.float32))[:height, :w] * np.float32(g.uniform(0.75, 1.0))
            txt.append(ALPHABET[a])
            x += w + int(g.integers(12, 21))
        texts.append(''.join(txt))
    img = np.clip(img + g.normal(0.0, 0.03, img.shape).astype(np.float32), 0.0, 1.0)
    u8 = np.rint(img * 255.0).astype(np.uint8)[:, None, :, :]
    return u8.astype(np.float32) / np.float32(255.0), np.full((n,), width, dtype=np.int64), texts


def make_batch(image, lens, texts, codec):
    labels = [codec.encode(t) for t in texts]
    return {'image': torch.from_numpy(image).cuda(), 'seq_lens': torch.from_numpy(lens), 'target': torch.tensor([c for t in labels for c in t]),
            'target_lens': torch.tensor([len(t) for t in labels])}


def cer_of(net, batch, texts):
    from conformer_ocr_amd.evaluate import ErrorRate
    e = ErrorRate()
    e.update(net.predict_string(batch['image'], batch['seq_lens']), texts)
    return e.compute()


def base_model(glyphs=24, steps=300):
    """The existing from-scratch recipe (tests/test_hip_train_full.py: 2-block model of the metric's shapes, random weights, 300 AdamW
    steps at 1e-3, warm-up 10, dropout 0.1) on 16 lines over the first `glyphs` glyphs."""
    codec = PytorchCodec({ALPHABET[i]: [i + 1] for i in range(glyphs)})
    hp = synth.hparams('cfg2', num_encoder_layers=2, num_classes=glyphs + 1)
    net = _net(hp, synth.make_state_dict(hp, seed=1, decoder_gain=1.0), codec, 'bf16')
    image, lens, texts = render_lines(16, hp.height, 600, 11, list(range(glyphs)))
    batch = make_batch(image, lens, texts, codec)
    tr = Trainer(net, lr=1e-3, weight_decay=1e-2, warmup=10)
    for _ in range(steps):
        tr.training_step(batch)
    tr.sync_module()
    return net, hp, batch, texts


FROZEN_STEPS, FULL_STEPS = 40, 260        # calibrated once on an MI355X (see the docstring below); 300 optimizer steps in total


@pytest.mark.timeout(600)
def test_a_model_of_24_glyphs_learns_8_more_within_the_from_scratch_budget():
    """Base: 16 lines over glyphs 1..24, the from-scratch recipe.  Fine-tune set: 16 lines over all 32 glyphs, each starting with one
    of glyphs 25..32.  `resize='fail'` raises; before tuning the CER is at least the share of new-glyph characters (each is at least
    one error); after 'union' + FROZEN_STEPS frozen steps + FULL_STEPS whole-network steps (300 in total, the from-scratch budget;
    lr 1e-3, warm-up 10, dropout 0.1) the bf16 serving path reads the fine-tune lines with CER <= 0.05.
    Calibration (one MI355X, once; CER after frozen + whole-network steps): 0 + 300 -> 0.0, 20 + 280 -> 0.0, 40 + 260 -> 0.0 (chosen:
    the frozen phase takes the loss from 681 to 84, the whole run ends at 0.41), 100 + 200 -> 0.0; shorter runs 40 + 160, 0 + 200,
    40 + 110 and 0 + 150 also reached 0.0.  CER before tuning 0.4032 at a new-glyph share of 0.3602."""
    net, hp, base_batch, base_texts = base_model()
    assert cer_of(net, base_batch, base_texts) <= 0.05                            # the base reads its own material
    image, lens, texts = render_lines(16, hp.height, 600, 12, list(range(32)), first=list(range(24, 32)))
    assert all(t[0] in ALPHABET[24:] for t in texts)
    with pytest.raises(ValueError, match='does not cover the training alphabet'):
        resize_codec(net.codec, texts, 'fail', hp.num_classes)
    share = sum(c in ALPHABET[24:] for t in texts for c in t) / sum(len(t) for t in texts)
    before = cer_of(net, make_batch(image, lens, texts, net.codec), texts)
    print(f'new-glyph share {share:.4f}; CER before tuning {before:.4f}')
    assert before >= share
    old_w = net.nn['decoder'].weight.detach().clone()
    new, row_map = resize_codec(net.codec, texts, 'union', hp.num_classes)
    resize_output(net, new, row_map, seed=0)
    assert net.hparams_record.num_classes == 33 and torch.equal(net.nn['decoder'].weight[:25], old_w)
    batch = make_batch(image, lens, texts, new)
    assert int(batch['target'].max()) == 32
    tr = Trainer(net, lr=1e-3, weight_decay=1e-2, warmup=10, freeze_backbone=FROZEN_STEPS * 16)
    losses = [tr.training_step(batch) for _ in range(FROZEN_STEPS + FULL_STEPS)]
    assert tr.frozen_steps == FROZEN_STEPS and tr.global_step == FROZEN_STEPS + FULL_STEPS <= 300
    tr.sync_module()
    after = cer_of(net, batch, texts)
    print(f'CER after {FROZEN_STEPS} frozen + {FULL_STEPS} whole-network steps: {after:.4f}; loss {losses[0]:.2f} -> {losses[FROZEN_STEPS - 1]:.2f} '
          f'(frozen) -> {losses[-1]:.4f}')
    assert after <= 0.05


@pytest.mark.timeout(600)
def test_a_decoder_only_run_leaves_the_encoder_alone_and_lowers_the_loss():
    """Freeze longer than the run: 100 frozen steps at lr 1e-3 on the fine-tune set.  The encoder stays bit-identical and the loss
    falls, each value <= 1.05 x the previous (the criterion of tests/test_hip_train.py).  The CER reached is recorded, not bounded:
    how linearly separable eight new glyphs are in an encoder trained on 24 is a measurement.  Measured once on
    an MI355X: loss 680.8 -> 21.3, largest step ratio 0.985, CER 0.4032 -> 0.0108 (300 such steps: 0.0)."""
    net, hp, _, _ = base_model()
    image, lens, texts = render_lines(16, hp.height, 600, 12, list(range(32)), first=list(range(24, 32)))
    new, row_map = resize_codec(net.codec, texts, 'union', hp.num_classes)
    resize_output(net, new, row_map, seed=0)
    batch = make_batch(image, lens, texts, new)
    enc = {k: v.detach().clone() for k, v in net.nn['encoder'].state_dict().items()}
    start = cer_of(net, batch, texts)
    tr = Trainer(net, lr=1e-3, weight_decay=1e-2, freeze_backbone=10 ** 9)
    losses = [tr.training_step(batch) for _ in range(100)]
    tr.sync_module()
    end = cer_of(net, batch, texts)
    print(f'decoder-only: loss {losses[0]:.2f} -> {losses[-1]:.2f}, largest step ratio {max(b / a for a, b in zip(losses, losses[1:])):.4f}; '
          f'CER {start:.4f} -> {end:.4f}')
    _log('finetune_decoder_only', {'loss_first': losses[0], 'loss_last': losses[-1], 'cer_before': start, 'cer_after': end})
    assert all(torch.equal(v, enc[k]) for k, v in net.nn['encoder'].state_dict().items())
    assert losses[-1] < losses[0]
    assert all(b <= a * 1.05 for a, b in zip(losses, losses[1:])), losses


@pytest.mark.timeout(600)
def test_new_mode_makes_the_codec_the_training_alphabet(tmp_path):
    """Fine-tune data over 8 old + 8 new glyphs: 17 classes, the kept characters carry their rows, both phases train the smaller
    layer, and the saved archive loads with the 16-grapheme codec and reads like the model that wrote it."""
    net, hp, _, _ = base_model(steps=60)
    glyphs = list(range(4, 12)) + list(range(24, 32))
    image, lens, texts = render_lines(8, hp.height, 600, 13, glyphs)
    assert {c for t in texts for c in t} == {ALPHABET[g] for g in glyphs}
    old_w, old_b = net.nn['decoder'].weight.detach().clone(), net.nn['decoder'].bias.detach().clone()
    new, row_map = resize_codec(net.codec, texts, 'new', hp.num_classes)
    assert len(new) == 16 and row_map.tolist() == [0] + list(range(5, 13)) + [-1] * 8
    resize_output(net, new, row_map, seed=0)
    assert net.hparams_record.num_classes == 17
    assert torch.equal(net.nn['decoder'].weight[:9], old_w[[0] + list(range(5, 13))]) and torch.equal(net.nn['decoder'].bias[1:9], old_b[5:13])
    batch = make_batch(image, lens, texts, new)
    tr = Trainer(net, lr=1e-3, weight_decay=1e-2, freeze_backbone=5 * 8)
    losses = [tr.training_step(batch) for _ in range(15)]
    assert tr.frozen_steps == 5 and all(np.isfinite(losses)) and losses[-1] < losses[0]
    tr.sync_module()
    path = str(tmp_path / 'new.safetensors')
    save_safetensors(net, path)
    back = PytorchRecognitionModel.load_safetensors(path).to('cuda:0')
    assert len(back.codec) == 16 and back.codec.c2l == new.c2l and back.hparams_record.num_classes == 17
    assert back.predict_string(batch['image'], batch['seq_lens']) == net.predict_string(batch['image'], batch['seq_lens'])


# ---- the command ------------------------------------------------------------------------------------------------------------------------
def _page_set(directory, name, seed, glyphs, first=None, n=6):
    from PIL import Image
    image, _, texts = render_lines(n, 96, 600, seed, glyphs, first)
    u8 = np.rint(image * 255.0).astype(np.uint8)[:, 0]
    kinds = [('line', 0.0), ('line', 2.0), ('line', -2.0), ('line', 1.0)]
    page, placed = page_synth.text_page(list(u8), [kinds[i % 4] for i in range(n)])
    Image.fromarray(page).save(os.path.join(directory, name + '.png'))
    xml = os.path.join(directory, name + '.xml')
    gt_synth.write_page_xml(xml, name + '.png', page.shape, [(f'{name}_l{i}', P, bd, t) for i, ((_, P, bd), t) in enumerate(zip(placed, texts))])
    return xml, texts


@pytest.mark.timeout(600)
def test_train_command_resizes_and_unfreezes(tmp_path):
    xml_a, _ = _page_set(str(tmp_path), 'set_a', 21, list(range(24)))
    xml_b, texts_b = _page_set(str(tmp_path), 'set_b', 22, list(range(32)), first=list(range(24, 32)))
    hp = synth.hparams('cfg2', num_encoder_layers=2).as_dict()
    for k in ('num_classes', 'height'):
        hp.pop(k)
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = [sys.executable, '-m', 'conformer_ocr_amd.train', '-f', 'xml', '-B', '3', '--warmup', '5', '-r', '1e-3', '--no-augment']
    out_a, out_b = str(tmp_path / 'm'), str(tmp_path / 'ft')
    r = subprocess.run(common + ['-N', '2', '-o', out_a, '--hyper-params', json.dumps(hp), '-e', xml_a, xml_a], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=400)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    tune = common + ['-N', '3', '-o', out_b, '-i', out_a + '_best.safetensors', '-e', xml_b, xml_b]
    r = subprocess.run(tune, cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode != 0 and 'does not cover the training alphabet' in r.stderr, r.stdout + r.stderr[-3000:]
    r = subprocess.run(tune + ['--resize', 'union', '--freeze-backbone', '9'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    n_new = len({c for t in texts_b for c in t} - set(ALPHABET[:24]))
    assert f'resize union: 25 -> {25 + n_new} classes; kept 24, added {n_new}' in r.stdout, r.stdout
    m = re.search(r'backbone unfrozen after (\d+) samples \((\d+) steps\)', r.stdout)
    assert m and 9 <= int(m.group(1)) < 12 and int(m.group(2)) >= 3, r.stdout         # batches of at most 3 lines, none split
    assert 'epoch 2:' in r.stdout
    net = PytorchRecognitionModel.load_safetensors(out_b + '_best.safetensors')
    assert net.hparams_record.num_classes == 25 + n_new and len(net.codec) == 24 + n_new
    txt = str(tmp_path / 'set_b.txt')
    r = subprocess.run([sys.executable, '-m', 'conformer_ocr_amd.ocr', '-m', out_b + '_best.safetensors', '-i', xml_b, txt], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(txt, encoding='utf-8') as fp:
        assert len(fp.read().split('\n')) - 1 == len(texts_b)
