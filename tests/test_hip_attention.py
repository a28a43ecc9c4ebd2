"""GPU: the attention core alone (cocr_debug_attention) in every kernel form against the float64 softmax of tests/attention_cases.py, on
inputs that take the online softmax's rescale branch -- and leave it alone, and take it for one query of a walk only, and in the second
and third key pass of the LDS-resident kernel.  tests/test_attention_cases_host.py holds the patterns' conditions.

Bounds come from the case's float64 data, never from kernel output (attention_cases.bound_bf16 / bound_fp32 state the derivations):
    bf16   |ctx - ref| <= 2^-7 (|ref| + Vmax)
    fp32   |ctx - ref| <= Vmax (2 (ln 2 e_score + 2^-22) + (2 T + 16) 2^-24),   e_score = 134 x 2^-24 max_j (sum_d |products| + 2 max |score|)
The exact expectations (one dominating key: that key's v row; equal scores: the mean of the T valid rows) are the reference's values to
1e-12 (host test) and are held to the same bounds.  max(dev / bound) per form and pattern goes to the parity log of the other
parity tests (test_hip_bf16_path._log)."""
import numpy as np
import pytest
import torch

from tests import attention_cases as ac
from tests.hip_util import make_engine
from tests.test_hip_bf16_path import _log

pytestmark = pytest.mark.gpu

RESIDENT = {'COCR_ATT_RESIDENT_MIN': '1', 'COCR_ATT_RESIDENT_LONG': '1'}
# form -> (geometry, compute dtype, switches, (heads, dh, dhp) of the library's layout)
FORMS = {
    'bf16_dh64_tiled': ('dh64', 'bf16', {'COCR_ATT_TILED': '1'}, (4, 64, 64)),      # merged 64-key form
    'bf16_dh64_resident': ('dh64', 'bf16', RESIDENT, (4, 64, 64)),                   # LDS-resident: one pass up to 320 frames, key passes beyond (321, 600, 705)
    'bf16_dh32': ('dh32', 'bf16', {}, (8, 32, 32)),                                   # merged form, one k-chunk
    'bf16_dh128': ('dh128', 'bf16', {}, (4, 128, 128)),                               # 32-key form
    'bf16_dh36': ('dh36', 'bf16', {'COCR_NO_PAD': '1'}, (4, 36, 64)),                 # the model's own layout: dh != dhp, masked operands, partial store
    'fp32_dh64': ('dh64', 'fp32', {}, (4, 64, 64)),                                   # 32-key form, float32 products
    'fp32_dh36': ('dh36', 'fp32', {}, (4, 36, 64)),
}
_ENGINES = {}


def _engine(form, monkeypatch):
    """One engine per form for the whole session (the switches are read when an engine is made)."""
    if form not in _ENGINES:
        geometry, dtype, env, layout = FORMS[form]
        for k in ('COCR_ATT_TILED', 'COCR_ATT_RESIDENT_MIN', 'COCR_ATT_RESIDENT_LONG', 'COCR_NO_PAD'):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = make_engine(ac.hparams(geometry), ac.weights(geometry), dtype)
        assert eng.attention_layout(1, 65)[:3] == layout and eng.attention_layout(2, 65)[3] == 128
        _ENGINES[form] = eng
    return _ENGINES[form]


def _run(eng, case, dtype):
    _, _, dhp, Tp = eng.attention_layout(case.N, case.T)
    td = torch.bfloat16 if dtype == 'bf16' else torch.float32
    q, k, v = (torch.from_numpy(ac.device_layout(a, dhp, Tp)).cuda().to(td) for a in (case.q, case.k, case.v))
    return eng.attention_core(q, k, v, case.layer, case.T)


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('pattern', ac.PATTERNS)
def test_attention_core_against_the_float64_softmax(pattern, form, monkeypatch):
    geometry, dtype, _, _ = FORMS[form]
    eng = _engine(form, monkeypatch)
    worst, bad = {}, {}
    for T in ac.LENGTHS:
        case = ac.make(pattern, geometry, T)
        got = _run(eng, case, dtype).float().cpu().numpy().astype(np.float64).reshape(case.N, T, case.heads, case.dh)
        ref = ac.reference(case, dtype)
        bound = ac.bound_bf16(case, ref) if dtype == 'bf16' else ac.bound_fp32(case)
        assert np.isfinite(got).all(), T
        ratio = float((np.abs(got - ref) / bound).max())
        print(f'{form} {pattern} T={T} N={case.N}: max dev {np.abs(got - ref).max():.3g}, max dev / bound {ratio:.3g}')
        worst[T] = ratio
        if not ratio <= 1.0:
            bad[T] = ratio
    _log(f'attention_core_{form}_{pattern}', {'max_dev_over_bound': max(worst.values()), 'by_length': worst})
    assert not bad, bad


@pytest.mark.parametrize('pattern', ac.PATTERNS)
def test_resident_and_tiled_kernels_give_the_same_bits_on_inputs_that_rescale(pattern, monkeypatch):
    """The LDS-resident kernel (one pass up to 320 frames, key passes beyond) against the tiled merged kernel: same products, same shift,
    the same rescale decisions per 16-query walk -- identical bits on every case, and from run to run."""
    res, tiled = _engine('bf16_dh64_resident', monkeypatch), _engine('bf16_dh64_tiled', monkeypatch)
    for T in ac.LENGTHS:
        case = ac.make(pattern, 'dh64', T)
        runs = [_run(res, case, 'bf16').view(torch.int16).cpu() for _ in range(3)]
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]), T
        t = _run(tiled, case, 'bf16').view(torch.int16).cpu()
        assert torch.equal(runs[0], t), (T, int((runs[0] != t).sum()))


def test_attention_core_checks_its_arguments(monkeypatch):
    eng = _engine('bf16_dh64_tiled', monkeypatch)
    case = ac.make('equal', 'dh64', 65)
    q = torch.zeros((case.N, 4, 128, 64), dtype=torch.bfloat16, device='cuda')
    assert eng.attention_core(q, q, q, 1, 65).shape == (case.N, 65, 256)
    for args in ((q, q, q, 2, 65), (q, q, q, -1, 65), (q, q, q, 0, 64), (q, q, q, 0, 129), (q, q, q, 0, 0), (q[:, :, :, :32].contiguous(),) * 3 + (0, 65)):
        with pytest.raises(ValueError):
            eng.attention_core(*args)
    with pytest.raises(ValueError):
        eng.attention_core(q.float(), q.float(), q.float(), 0, 65)
    with pytest.raises(ValueError):
        eng.attention_core(q, q[:1], q, 0, 65)
