"""GPU: the training step (cocr_train_step) at every kernel form that the model's dimensions select, each against the float64 oracle on the
CPU.  tests/test_hip_train_full.py and tests/test_hip_train_pin.py hold the step at two model shapes (D = 32 with 4 heads of 8, D = 256 with 4
heads of 64 and kernel 31), which take most of the step's branches one way only; the cases of tests/train_ref.py SHAPE_CASES take them the
other way -- one encoder block, at most 75 output frames:

  cfg1_1        the reference's default model: row attention at dh = 36 with T = 75 > 64, D = 144 / 288 / 576 (partial 128-wide tiles in every
                weight gradient), 32 conv channels, the <31> depthwise kernels with 144 of 256 lanes
  cfg1_h2       dh = 72: the second pass of every `d += 64` loop of the row kernels
  cfg1_h8       dh = 18: their scalar path
  h8 / h2       batched attention at dh = 32 (one k-chunk; T = 70, Tk = 96, Rk = 160) and dh = 128; h8 also through the row kernels
  k15 / k33     k_dw1d_rows<., 0> / k_dw1d_bwd_w<0> at D = 256 with a partial last frame chunk; the flat depthwise kernels (K > 32)
  d512k7        D = 512: two column blocks, 8 splits in the feed-forward weight gradients
  nohalf97ff2   ffr = 1, ff = 2 D, 97 classes (nclp = 100)
  widest        D = 1024: four column blocks, dh = 128, splits == 1 for the (1024, 16384) frontend linear, 2 for the feed-forward, the flat tfc

Every test first asserts that its case still selects what it exists for (train_ref.SHAPE_PRE, also checked without a GPU in
tests/test_train_ref_host.py).  Tolerances: the suite's own -- gradients |got - ref| <= 2e-3 max|ref| + 1e-5 per tensor, loss 2e-4 relative,
running statistics 1e-5; the oracle in float32 against itself in float64 stays within 1.8e-4 of a tensor's largest entry on these inputs (loss
1.7e-7), with dropout off and on.  'medium': 4 e_ref and 1e-5 + 4 e_bn from train_ref.E_REF / E_BN.  Measurements: DESIGN.md section 6."""
import os

import numpy as np
import pytest
import torch

from conformer_ocr_amd import synth
from tests.test_hip_train_pin import check, reference, step
from tests.train_ref import DROP_SEED, E_BN, E_REF, MEDIUM_SHAPE_CASES, NO_DROP, P4, SHAPE_CASES, assert_shape_selects

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', list(SHAPE_CASES))
def test_shape_against_the_oracle(name):
    assert_shape_selects(name)
    eng, loss = step(name)
    check(name, eng, loss, reference(name))


@pytest.mark.parametrize('name', list(SHAPE_CASES))
def test_shape_with_dropout_at_every_site_against_the_masked_oracle(name):
    """All six sites on.  The attention-weight mask is indexed `row * T + key` in both attention forms although the batched form's buffers have
    rows of Tk floats: here at head sizes 18, 36, 72 (rows) and 32, 64, 128 (batched) with T = 70 / 75 < Tk = 96 and T = 35 < Tk = 64."""
    assert_shape_selects(name)
    eng, loss = step(name, P4, DROP_SEED)
    check(name, eng, loss, reference(name, P4, DROP_SEED))


def test_row_attention_at_one_k_chunk_with_dropout(monkeypatch):
    """COCR_TRAIN_ATTN_NAIVE=1 on 'h8': k_attn_fwd / k_attn_bwd_rows / k_attn_bwd_cols / k_attn_bwd_pos at 8 heads of 32 and T = 70 (half a
    wave of head dimensions; a lane walks two keys)."""
    f = assert_shape_selects('h8')
    assert f['dh'] < 64 < f['T']
    monkeypatch.setenv('COCR_TRAIN_ATTN_NAIVE', '1')
    eng, loss = step('h8', P4, DROP_SEED)
    check('h8', eng, loss, reference('h8', P4, DROP_SEED))


@pytest.mark.parametrize('name', MEDIUM_SHAPE_CASES)
def test_shape_under_medium_against_the_rounded_oracle(name):
    """'medium' without dropout against MediumOracle, as test_hip_train_pin.test_medium_against_the_rounded_oracle: every gradient within
    4 e_ref of its tensor's largest entry (+ 1e-5), the loss within 2e-4, the running statistics within 1e-5 + 4 e_bn.  cfg1_1: partial tiles
    through gemm_tn; d512k7: 8 splits; nohalf97ff2: a 97-class decoder under `gemm`'s own rounding rule (train_ref.medium_rules: bf16 forward
    and weight gradient, fp32 input gradient); widest: lin_bwd_bf16 with splits == 1."""
    f = assert_shape_selects(name)
    hp = SHAPE_CASES[name]['hp']()
    # (which Linears take lin_fwd's bf16 branch: both dimensions multiples of 8 -- every one but a 97-class decoder)
    assert all(x % 8 == 0 for x in (f['D'], f['ff'], f['C'], f['C'] * f['F'])) and (hp.num_classes % 8 == 0) == (name != 'nohalf97ff2')
    eng, loss = step(name, NO_DROP, 0, 'medium')
    check(name, eng, loss, reference(name, NO_DROP, 0, True), rel=4 * E_REF[(name, False)], running_tol=1e-5 + 4 * E_BN[(name, False)])


def test_cfg1_trained_in_its_own_layout_is_served_as_the_padded_bf16_model():
    """The reference's default model (D = 144, 4 heads of 36) is served in bf16 as a zero-padded 256-wide model, while the step trains the
    model's own 144-wide layout: three Trainer steps, sync_module, then net.forward equals -- bit for bit -- the forward of a fresh bf16 model
    loaded from the synced state dict, and differs from the logits before training."""
    from conformer_ocr_amd.codec import ascii_codec
    from conformer_ocr_amd.pred import PytorchRecognitionModel
    from conformer_ocr_amd.train import Trainer
    hp = synth.hparams('cfg1', num_encoder_layers=1)
    assert 128 <= hp.encoder_dim < 256 and not os.environ.get('COCR_NO_PAD')          # (cocr_api.hip set_engine_dims: the zero-padded layout)
    state = synth.make_state_dict(hp, seed=41, decoder_gain=1.0)
    image, lens = synth.make_lines(3, hp.height, 300, seed=41, widths=[300, 137, 222])
    targets = [[5, 9, 9, 3], [17], [2, 2, 40]]

    def model():
        return PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1,
                                       codec=ascii_codec(hp.num_classes), compute_dtype='bf16')
    net = model()
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net = net.to('cuda:0').eval()
    x, sl = torch.from_numpy(image).cuda(), torch.from_numpy(lens)
    before = net.forward(x, sl)[0].float().cpu().clone()
    batch = {'image': torch.from_numpy(image), 'seq_lens': sl, 'target': torch.tensor([c for s in targets for c in s]),
             'target_lens': torch.tensor([len(s) for s in targets])}
    tr = Trainer(net, lr=1e-3, weight_decay=1e-2, seed=5)
    losses = [tr.training_step(batch) for _ in range(3)]
    tr.sync_module()
    after, after_len = net.forward(x, sl)
    fresh = model()
    fresh.nn.load_state_dict({k: v.detach().cpu().clone() for k, v in net.nn.state_dict().items()})
    fresh = fresh.to('cuda:0').eval()
    want, want_len = fresh.forward(x, sl)
    moved = float((after.float().cpu() - before).abs().max())
    print(f'cfg1 hand-over: losses {losses}; logits moved by {moved:.3e}; served vs fresh {float((after.float() - want.float()).abs().max()):.3e}')
    assert after.dtype == want.dtype and after.shape == want.shape == (3, 75, hp.num_classes)
    assert torch.equal(after, want) and torch.equal(after_len.cpu(), want_len.cpu())
    assert np.isfinite(moved) and moved > 0.0
