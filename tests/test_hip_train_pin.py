"""GPU: the training step (cocr_train_step) pinned where tests/test_hip_train_full.py leaves it free -- under dropout, under 'medium' matmul
precision and at row counts that fill more than one split / chunk -- each against a float64 restatement on the CPU:

  dropout   the oracle with the device's masks at the reference's six sites (tests/train_ref.py: DroppedOracle; the restated generator is
            checked in tests/test_train_ref_host.py, the placement against the reference's own nn.Dropout modules by
            tests/golden/tiny_train_drop.npz)
  rows      M = N T of 750, 2000 and 2096: split-K weight gradients of which several (750, 2096) or all (2000) partial sums hold rows, the last
            of those partly padding; Mp = 4096, more than 32 column-sum chunks in the encoder, the 64- and 256-row chunk forms in the frontend
  medium    the oracle with every Linear / pointwise-conv product on bf16-rounded operands as lin_fwd / lin_bwd_bf16 / lin_bwd round them
            (MediumOracle), at a bound measured from that restatement's own float32-versus-float64 difference

Every reference is computed once per session and shared.  Tolerances: gradients |got - ref| <= 2e-3 max|ref| + 1e-5 per tensor and loss 2e-4
relative (the suite's own, tests/test_hip_train_full.py) unless a test says otherwise."""
import functools
import os

import numpy as np
import pytest
import torch

from conformer_ocr_amd.engine import HipRecognizer
from conformer_ocr_amd.spec import model_state_spec
from oracle.conformer_ref import out_len
from tests.test_hip_train_full import CASES as FULL
from tests.train_ref import (CASES, DROP_SEED, E_BN, E_REF, NO_DROP, P4, bn_running, inputs, oracle_train_grads_dropped, oracle_train_grads_medium,
                             tiny_sampled_e_ref)

pytestmark = pytest.mark.gpu

CASES.update({k: FULL[k] for k in ('tiny2', 'tiny8', 'cfg2x2')})          # (train_ref.inputs reads this table)
assert all(FULL['tiny'][k] == CASES['tiny'][k] for k in ('seed', 'n', 'W', 'widths', 'targets')) and FULL['tiny']['hp']() == CASES['tiny']['hp']()


@functools.lru_cache(maxsize=None)
def reference(name, p4=NO_DROP, seed=0, medium=False):
    """(loss, probits, gradients, running statistics after the step) in float64; computed once, never modified."""
    hp, state, image, lens, targets = inputs(name)
    fn = oracle_train_grads_medium if medium else oracle_train_grads_dropped
    loss, probits, grads, bn = fn(hp, state, image, lens, targets, p4, seed)
    for g in grads.values():
        g.setflags(write=False)
    return loss, probits, grads, bn_running(state, bn, probits.shape[0] * probits.shape[1])


def step(name, p4=NO_DROP, seed=0, precision='highest'):
    hp, state, image, lens, targets = inputs(name)
    eng = HipRecognizer(hp, torch.device('cuda', 0), 'fp32')
    eng.load_state(state)
    eng.train_begin(precision)
    loss = eng.train_step(torch.from_numpy(image[:, 0]).cuda(), lens, [x for s in targets for x in s], [len(s) for s in targets], dropout=p4, seed=seed)
    return eng, loss


def check(name, eng, loss, ref, rel=2e-3, floor=1e-5, loss_rel=2e-4, running_tol=1e-5, rel_per_tensor=None):
    """Loss, every parameter's gradient (|got - ref| <= rel max|ref| + floor per tensor; rel_per_tensor: a tensor named there also within its own
    figure) and the BatchNorm running statistics (within running_tol).  Prints the worst figures before asserting."""
    hp = inputs(name)[0]
    loss64, _, grads64, running = ref
    errs, nparams = {}, 0
    for k, (shape, kind) in model_state_spec(hp).items():
        if kind != 'param':
            continue
        nparams += 1
        r = grads64[k].reshape(shape)
        errs[k] = (float(np.abs(eng.train_grad(k) - r).max()), float(np.abs(r).max()))
    worst = max(errs.items(), key=lambda kv: kv[1][0] / (kv[1][1] + floor / rel))
    print(f'{name}: loss {loss!r} vs {loss64!r} (rel {abs(loss - loss64) / abs(loss64):.2e}); worst gradient {worst[0]}: '
          f'err {worst[1][0]:.3e} of max {worst[1][1]:.3e} (ratio {worst[1][0] / max(worst[1][1], 1e-300):.2e}, {worst[1][0] / (rel * worst[1][1] + floor):.3f} '
          f'of its bound); largest err / max|ref| over the tensors with max|ref| > 1e-9: {max(e[0] / e[1] for e in errs.values() if e[1] > 1e-9):.2e}')
    assert abs(loss - loss64) <= loss_rel * abs(loss64), (loss, loss64)
    bad = {k: e for k, e in errs.items() if not e[0] <= rel * e[1] + floor}
    if rel_per_tensor:
        own = max(errs, key=lambda k: errs[k][0] / (rel_per_tensor.get(k, rel) * errs[k][1] + floor))
        print(f'{name}: against its own bound, worst {own}: err {errs[own][0]:.3e}, bound {rel_per_tensor.get(own, rel) * errs[own][1] + floor:.3e}')
        bad.update({k: e + (rel_per_tensor[k],) for k, e in errs.items() if k in rel_per_tensor and not e[0] <= rel_per_tensor[k] * e[1] + floor})
    assert nparams == len(grads64) and not bad, dict(sorted(bad.items(), key=lambda kv: -kv[1][0])[:12])
    rerr = {k: float(np.abs(eng.train_value(k) - v).max()) for k, v in running.items()}
    print(f'{name}: running statistics: worst {max(rerr.values()):.3e} (bound {running_tol:.3e})')
    assert all(e <= running_tol for e in rerr.values()), rerr


# ---- dropout against float64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['tiny', 'cfg2x2'])
def test_dropout_at_every_site_against_the_masked_oracle(name):
    """All six sites on, four distinct probabilities: 'tiny' (3 ragged lines, one wave per attention row) and 'cfg2x2' at (2, 120) (attention as
    batched products: the mask applied in k_attn_softmax, k_attn_softmax_bwd and k_btranspose)."""
    eng, loss = step(name, P4, DROP_SEED)
    check(name, eng, loss, reference(name, P4, DROP_SEED))


def test_dropout_at_every_site_with_row_attention_at_the_metric_models_shapes(monkeypatch):
    """COCR_TRAIN_ATTN_NAIVE=1 on 'cfg2x2': k_attn_fwd / k_attn_bwd_rows / k_attn_bwd_cols at 4 heads of 64 and T = 30."""
    monkeypatch.setenv('COCR_TRAIN_ATTN_NAIVE', '1')
    eng, loss = step('cfg2x2', P4, DROP_SEED)
    check('cfg2x2', eng, loss, reference('cfg2x2', P4, DROP_SEED))


def test_dropout_step_equals_the_reference_fixture():
    """tests/golden/tiny_train_drop.npz directly (the reference's own modules with the restated masks), without the oracle in between."""
    from tests.conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, 'tiny_train_drop.npz'))
    hp, state = inputs('tiny')[:2]
    assert tuple(g['dropout'].tolist()) == P4 and int(g['drop_seed']) == DROP_SEED
    eng, loss = step('tiny', P4, DROP_SEED)
    grads = {k[5:]: g[k] for k in g.files if k.startswith('grad:')}
    running = {k[4:]: g[k] for k in g.files if k.startswith('buf:') and 'running_' in k}
    assert len(running) == 2 * hp.num_encoder_layers
    check('tiny', eng, loss, (float(g['loss']), None, grads, running))


@pytest.mark.parametrize('which', range(4))
def test_dropout_at_one_site_group_at_a_time(which):
    """Exactly one of the four probabilities non-zero (0.5), so that a failure names its site: input / feed-forward (hidden and out, both
    modules) / attention (weights and out) / conv."""
    p4 = tuple(0.5 if i == which else 0.0 for i in range(4))
    eng, loss = step('tiny', p4, DROP_SEED + 1 + which)
    check('tiny', eng, loss, reference('tiny', p4, DROP_SEED + 1 + which))


@pytest.mark.parametrize('name', ['tiny8', 'tiny2'])
def test_dropout_behind_the_other_frontends(name):
    """Subsampling factors 8 and 2: the input-dropout site (forward and backward) behind the other frontend forms."""
    eng, loss = step(name, P4, DROP_SEED)
    check(name, eng, loss, reference(name, P4, DROP_SEED))


# ---- many rows against float64 -------------------------------------------------------------------------------------------------------------------
def _row_counts(name):
    hp, _, image, lens, _ = inputs(name)
    c = CASES[name]
    T1, T2 = int(out_len(c['W'], 1)), int(out_len(c['W'], 2))
    F1, F2 = int(out_len(hp.height, 1)), int(out_len(hp.height, 2))
    return c['n'] * T2, c['n'] * T1 * F1, c['n'] * T2 * F2


def _assert_many_rows():
    M, front1, front2 = _row_counts('rows')
    # (a later change of shapes must not silently lose the coverage: Mp = round_up(M, 2048) above 2048, colsum_chunk_rows leaving its 32-row
    # form for the 64-row one (> 16384) and the 256-row one (> 65536), more than 32 chunks of 32 rows in the encoder)
    assert M > 2048 and front2 > 16384 and front1 > 65536 and (M + 31) // 32 > 32, (M, front1, front2)


def test_many_rows_against_the_oracle():
    _assert_many_rows()
    eng, loss = step('rows')
    check('rows', eng, loss, reference('rows'))


def test_many_rows_with_dropout_against_the_masked_oracle():
    _assert_many_rows()
    eng, loss = step('rows', P4, DROP_SEED)
    check('rows', eng, loss, reference('rows', P4, DROP_SEED))


def test_a_partly_filled_last_split_against_the_oracle():
    """3 lines of width 1000 on 'cfg2x2': M = 750 rows over 32 splits of 64 -- several splits hold rows, the last of them partly padding, the
    rest only zeros."""
    M = _row_counts('cfg2x2_1000')[0]
    assert 64 < M < 2048 and M % 64 != 0, M
    eng, loss = step('cfg2x2_1000')
    check('cfg2x2_1000', eng, loss, reference('cfg2x2_1000'))


def test_every_split_holding_rows_against_the_oracle():
    """M = 2000 <= 2048 = 32 splits x 64 rows: no split of any weight gradient is empty, in the encoder (ceil(M / 64) = 32) and in the frontend
    (16000 rows over 32 splits of 512), and each one's last split is partly padding."""
    M, _, front2 = _row_counts('rows_full')
    assert (M + 63) // 64 == 32 and M % 64 != 0 and (front2 + 511) // 512 == 32 and front2 % 512 != 0, (M, front2)
    eng, loss = step('rows_full')
    check('rows_full', eng, loss, reference('rows_full'))


# ---- 'medium' against the rounded float64 restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('drop', [False, True], ids=['nodrop', 'drop'])
@pytest.mark.parametrize('name', ['tiny', 'cfg2x2_232', 'rows'])
def test_medium_against_the_rounded_oracle(name, drop):
    """Every gradient within 4 e_ref of its tensor's largest entry (+ 1e-5), the loss within 2e-4, the running statistics within 1e-5 + 4 E_BN
    (train_ref.E_REF / E_BN: MediumOracle in float32 against itself in float64, the largest figure over the tensors).  4 e_ref is 1.2e-2 .. 4.2e-2.
    On 'tiny' without dropout every tensor is ALSO held within 4 x its own figure, sampled over 16 float32 runs (tests/golden/
    tiny_medium_e_ref.json, train_ref.medium_e_ref_sampled): late-block weight gradients have figures of 1e-4, where the worst tensor's bound
    hides one product operand left unrounded.  Measurements: DESIGN.md section 6."""
    p4, seed = (P4, DROP_SEED) if drop else (NO_DROP, 0)
    eng, loss = step(name, p4, seed, 'medium')
    own = {k: 4 * e for k, e in tiny_sampled_e_ref().items()} if (name, drop) == ('tiny', False) else None
    check(name, eng, loss, reference(name, p4, seed, True), rel=4 * E_REF[(name, drop)], running_tol=1e-5 + 4 * E_BN[(name, drop)], rel_per_tensor=own)
