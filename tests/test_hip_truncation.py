"""GPU: rows truncated at max_per_line (include/cocr.h) through the C ABI of every decoder.  A call with max_per_line = 3 must write
the full call's counts and, in every field, the full call's first three records -- conf bit for bit -- and nothing beyond them.  The
last kept record is the one at stake: its end and conf are bounded by the start of the next label, which the truncated row does not
hold."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import beam_cases as bc
from tests.hip_util import fresh_decoder_engine
from tests.test_nbest_host import chain_lm

pytestmark = pytest.mark.gpu
CUT = 3
SHORT = ('random', 11, 40, 5, 2.0)
LONG = 'long'                                # 730 frames: beam 32 keeps its back-pointers in global memory


def _inputs(spec):
    """SHORT, or the planted 730-frame line of tests/beam_cases.py with label 2 held for a second frame (8) and still above the blank on
    frame 9, where label 3 starts: record 2 ends at 8 only because record 3 starts at 9."""
    if spec != LONG:
        return bc.inputs(spec)
    x, labels = bc.planted_line(362, 6, 6.0, 5)
    assert labels[2] != labels[3]
    x = x.copy()
    x[8] = x[7]
    x[9, labels[2]] = x[9, 0] + np.float32(1.0)
    return x[None], [x.shape[0]]


def _call(eng, fn, x, lens, mpl, extra=()):
    """A 1-best entry point with device outputs prefilled with a pattern: dict of numpy arrays."""
    N, T, ncls = x.shape
    out = {k: torch.full((N, mpl), -7, dtype=torch.int32, device=x.device) for k in ('labels', 'starts', 'ends')}
    out['conf'] = torch.full((N, mpl), -7.0, device=x.device)
    out['counts'] = torch.full((N,), -7, dtype=torch.int32, device=x.device)
    ln = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    p = {k: C.c_void_p(v.data_ptr()) for k, v in out.items()}
    assert fn(eng._h, C.c_void_p(x.data_ptr()), N, T, ncls, ln.ctypes.data_as(C.POINTER(C.c_int32)), p['labels'], p['starts'], p['ends'], p['conf'],
              p['counts'], mpl, *extra, None) == 0
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _cut_equals_full(eng, fn, spec, extra=(), bites=True):
    x, lens = _inputs(spec)
    xd = torch.from_numpy(x).cuda()
    full, cut = _call(eng, fn, xd, lens, x.shape[1], extra), _call(eng, fn, xd, lens, CUT, extra)
    assert (cut['counts'] == full['counts']).all() and full['counts'].max() > CUT
    for n, cnt in enumerate(full['counts'].tolist()):
        keep = min(cnt, CUT)
        for k in ('labels', 'starts', 'ends'):
            assert (cut[k][n, :keep] == full[k][n, :keep]).all(), (k, n, cut[k][n], full[k][n, :CUT])
            assert (cut[k][n, keep:] == -7).all(), (k, n)
        assert cut['conf'][n, :keep].tobytes() == full['conf'][n, :keep].tobytes(), (n, cut['conf'][n], full['conf'][n, :CUT])
        assert (cut['conf'][n, keep:] == -7.0).all(), n
    # the cut falls where it matters: on some line record 2 ends where record 3 starts, and would run on without that bound
    assert not bites or any(cnt > CUT and full['ends'][n, CUT - 1] + 1 == full['starts'][n, CUT] and
                            x[n, full['starts'][n, CUT], full['labels'][n, CUT - 1]] > x[n, full['starts'][n, CUT], 0] for n, cnt in enumerate(full['counts'].tolist()))


def test_greedy():
    eng = fresh_decoder_engine()
    _cut_equals_full(eng, eng.lib.cocr_ctc_greedy, SHORT, bites=False)       # (a greedy record ends with its run: nothing to bound)


@pytest.mark.parametrize('form', ['fast, back-pointers in LDS', 'fast, back-pointers in global memory', 'exhaustive'])
def test_beam(form, monkeypatch):
    if form == 'exhaustive':
        monkeypatch.setenv('COCR_BEAM_REF', '1')
    eng = fresh_decoder_engine()
    if 'global' in form:
        _cut_equals_full(eng, eng.lib.cocr_ctc_beam, LONG, (32,))
    else:
        _cut_equals_full(eng, eng.lib.cocr_ctc_beam, SHORT, (16,))


@pytest.mark.parametrize('spec,beam', [(SHORT, 16), (LONG, 32)], ids=['back-pointers in LDS', 'back-pointers in global memory'])
def test_beam_lm(spec, beam):
    eng = fresh_decoder_engine()
    lm = chain_lm(_inputs(spec)[0].shape[2], 3, seed=5)
    dlm = lm.to_device(eng)

    def fn(h, *args):
        return eng.lib.cocr_ctc_beam_lm(h, dlm.handle, *args)
    _cut_equals_full(eng, fn, spec, (beam, 5, C.c_float(bc.LM_ALPHA), C.c_float(bc.LM_BETA), None))


@pytest.mark.parametrize('with_lm', [False, True], ids=['plain', 'lm'])
def test_beam_nbest(with_lm):
    from tests.test_hip_nbest import _raw
    eng = fresh_decoder_engine()
    x, lens = bc.inputs(SHORT)
    xd = torch.from_numpy(x).cuda()
    kw = dict(lm=chain_lm(11, 3, seed=5), classes=5, alpha=bc.LM_ALPHA, beta=bc.LM_BETA) if with_lm else {}
    (rc, full), (rc2, cut) = _raw(eng, xd, lens, 16, 8, **kw), _raw(eng, xd, lens, 16, 8, mpl=CUT, **kw)
    assert rc == rc2 == 0 and full['counts'].max() > CUT
    for k in ('counts', 'nhyp'):
        assert (cut[k] == full[k]).all(), k
    assert np.array_equal(cut['scores'], full['scores'], equal_nan=True)
    for n in range(len(lens)):
        for j in range(8):
            keep = min(CUT, int(full['counts'][n, j])) if j < full['nhyp'][n] else 0
            for k in ('labels', 'starts', 'ends'):
                assert (cut[k][n, j, :keep] == full[k][n, j, :keep]).all(), (k, n, j)
                assert (cut[k][n, j, keep:] == -7).all(), (k, n, j)
            assert cut['conf'][n, j, :keep].tobytes() == full['conf'][n, j, :keep].tobytes(), (n, j)
            assert (cut['conf'][n, j, keep:] == -7.0).all(), (n, j)
    # the cut falls where it matters, as in _cut_equals_full: in some hypothesis record 2 ends where record 3 starts
    assert any(full['counts'][n, j] > CUT and full['ends'][n, j, CUT - 1] + 1 == full['starts'][n, j, CUT] and
               x[n, full['starts'][n, j, CUT], full['labels'][n, j, CUT - 1]] > x[n, full['starts'][n, j, CUT], 0]
               for n in range(len(lens)) for j in range(int(full['nhyp'][n])))
