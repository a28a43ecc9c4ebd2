"""GPU: n-best decoding (cocr_ctc_beam_nbest, csrc/ctc_nbest.hip.h) against the 1-best decoders (hypothesis 0, bit for bit), its
exhaustive path, the definition (conformer_ocr_amd/nbest.py nbest_host, on the cases whose decision gaps tests/test_nbest_host.py
asserts), the criterion (cocr_ctc_loss), and through the public surface."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

from conformer_ocr_amd import _lib
from conformer_ocr_amd.lm import _log_softmax, records_host
from conformer_ocr_amd.nbest import ctc_logp, lm_sum, nbest_host
from tests import beam_cases as bc
from tests.hip_util import fresh_decoder_engine
from tests.test_nbest_host import CASES, FEWER, case_inputs, chain_lm, host_case

pytestmark = pytest.mark.gpu


def _engine():
    from conformer_ocr_amd.ctc_decoder import _scratch_engine
    return _scratch_engine(torch.device('cuda', 0))


def _raw(eng, x, lens, beam, nbest, lm=None, classes=8, alpha=0.5, beta=0.0, mpl=None, null=None):
    """The C call with device outputs prefilled with a pattern: (rc, dict of numpy arrays)."""
    N, T, ncls = x.shape
    mpl = T if mpl is None else mpl
    dev = x.device
    out = {k: torch.full((N, max(nbest, 1), mpl), -7, dtype=torch.int32, device=dev) for k in ('labels', 'starts', 'ends')}
    out['conf'] = torch.full((N, max(nbest, 1), mpl), -7.0, device=dev)
    out['counts'] = torch.full((N, max(nbest, 1)), -7, dtype=torch.int32, device=dev)
    out['nhyp'] = torch.full((N,), -7, dtype=torch.int32, device=dev)
    out['scores'] = torch.full((N, max(nbest, 1), 2), -7.0, device=dev)
    p = {k: (None if k == null else C.c_void_p(v.data_ptr())) for k, v in out.items()}
    ln = np.ascontiguousarray(np.asarray(lens, dtype=np.int32))
    dlm = lm.to_device(eng) if lm is not None else None
    rc = eng.lib.cocr_ctc_beam_nbest(eng._h, dlm.handle if dlm else None, None if null == 'logits' else C.c_void_p(x.data_ptr()), N, T, ncls,
                                     ln.ctypes.data_as(C.POINTER(C.c_int32)), beam, nbest, classes, C.c_float(alpha), C.c_float(beta), p['labels'], p['starts'],
                                     p['ends'], p['conf'], p['counts'], p['nhyp'], p['scores'], mpl, None)
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def _beam_shape(Cn, T, scale):
    g = np.random.default_rng(Cn * 7919 + T)
    logits = (g.normal(size=(7, T, Cn)) * scale).astype(np.float32)
    logits[:, :, 0] += 1.0
    logits[1, :, 1:] = np.round(logits[1, :, 1:] * 2) / 2          # exact ties between classes
    return logits, [T, T - 1, T // 2, 1, T, 7, 0]


# the shapes of test_beam_pruned_equals_exhaustive; (40, 1120, 16) in place of (40, 1500, 16): with nbest = beam = 16 a line takes
# 4 + 64 + 64 bytes of LDS per frame, so 1118 frames are the first that do not fit 144 KB (nbest = 1 still fits: both forms run)
SHAPES = [(128, 300, 16, 2.5), (128, 300, 16, 0.3), (200, 120, 32, 1.5), (17, 90, 16, 1.0), (3, 50, 8, 1.0), (7, 500, 32, 1.0), (40, 1120, 16, 2.0),
          (256, 40, 16, 2.0), (2, 30, 4, 1.0)]


def _same(a, b):
    """Hypothesis lists equal field for field, NaN scores matching NaN."""
    assert len(a) == len(b)
    for ha, hb in zip(a, b):
        assert len(ha) == len(hb)
        for (ra, pa, la), (rb, pb, lb) in zip(ha, hb):
            assert ra == rb and la == lb and (pa == pb or (math.isnan(pa) and math.isnan(pb)))


@pytest.mark.parametrize('Cn,T,beam,scale', SHAPES + [(300, 20, 8, 2.0)])
def test_first_hypothesis_is_the_beam_and_fast_equals_exhaustive(Cn, T, beam, scale, monkeypatch):
    """Hypothesis 0 = cocr_ctc_beam on every field for nbest 1 and beam; the whole n-best output of the fast path = that of the
    exhaustive path (COCR_BEAM_REF=1).  300 classes: the exhaustive path alone."""
    logits, lens = _beam_shape(Cn, T, scale)
    x = torch.from_numpy(logits).cuda()
    eng = fresh_decoder_engine()
    want = eng.ctc_beam(x, lens, beam)
    full = None
    for nbest in (1, beam):
        full = eng.ctc_beam_nbest(x, lens, beam, nbest)
        assert [h[0][0] for h in full] == want
        assert all(h[0][2] == 0.0 for h in full)
        assert all(1 <= len(h) <= nbest for h in full)
    assert full[6] == [([], 0.0, 0.0)]                               # the line of length 0
    monkeypatch.setenv('COCR_BEAM_REF', '1')
    _same(full, fresh_decoder_engine().ctc_beam_nbest(x, lens, beam, beam))


@pytest.mark.parametrize('Cn,T,beam', [(17, 90, 16), (128, 60, 16)])
def test_first_hypothesis_is_the_lm_beam(Cn, T, beam):
    logits, lens = _beam_shape(Cn, T, 1.5)
    x = torch.from_numpy(logits).cuda()
    lm = chain_lm(Cn, 3, seed=Cn)
    eng = _engine()
    want = eng.ctc_beam_lm(x, lens, lm, beam, 8, 0.7, 0.3)
    for nbest in (1, beam):
        got = eng.ctc_beam_nbest(x, lens, beam, nbest, lm, 8, 0.7, 0.3)
        assert [h[0][0] for h in got] == want
    for hyps in got:                                                 # the raw n-gram sum: the host's float32 sum, bit for bit
        for recs, _, lmv in hyps:
            labels, acc = [r[0] for r in recs], np.float32(0.0)
            for k, c in enumerate(labels):
                acc = np.float32(acc + lm.logp(labels[:k], c))
            assert lmv == float(acc)


def _loss_of(eng, x, lens, hyps):
    """-cocr_ctc_loss of every hypothesis of every line (one call per hypothesis rank); None for one the criterion does not take (more
    than 255 labels)."""
    out = [[None] * len(h) for h in hyps]
    for j in range(max(len(h) for h in hyps)):
        rows = [n for n, h in enumerate(hyps) if j < len(h) and len(h[j][0]) <= 255]
        if not rows:
            continue
        labs = [[r[0] for r in hyps[n][j][0]] for n in rows]
        nll, _ = eng.ctc_loss(x[rows].contiguous(), [lens[n] for n in rows], np.asarray([c for l in labs for c in l], dtype=np.int32),
                              [len(l) for l in labs], with_grad=False)
        for n, v in zip(rows, nll.cpu().numpy().tolist()):
            out[n][j] = -v
    return out


@pytest.mark.parametrize('Cn,T,beam,nbest', CASES)
def test_against_the_definition(Cn, T, beam, nbest):
    logits, lens = case_inputs(Cn, T)
    x = torch.from_numpy(logits).cuda()
    eng = _engine()
    got = eng.ctc_beam_nbest(x, lens, beam, nbest)
    want = [h for h, _ in host_case(Cn, T, beam, nbest)]
    assert [len(h) for h in got] == [len(h) for h in want] == FEWER.get((Cn, T, beam, nbest), [nbest] * 4)
    loss = _loss_of(eng, x, lens, got)
    for n in range(4):
        for j, ((recs, logp, lmv), (wrecs, wlogp, _)) in enumerate(zip(got[n], want[n])):
            assert [r[:3] for r in recs] == [r[:3] for r in wrecs], (n, j)
            np.testing.assert_allclose([r[3] for r in recs], [r[3] for r in wrecs], rtol=1e-4)
            print(f'({Cn},{T}) line {n} hyp {j}: logp {logp!r} definition {wlogp!r} -loss {loss[n][j]!r}')
            np.testing.assert_allclose(logp, wlogp, rtol=2e-6, atol=1e-3)
            np.testing.assert_allclose(logp, loss[n][j], rtol=2e-6, atol=1e-3)
            assert lmv == 0.0


@pytest.mark.parametrize('Cn,T,beam,nbest', [(11, 40, 16, 8), (5, 12, 4, 4)])
def test_against_the_definition_with_a_language_model(Cn, T, beam, nbest):
    logits, lens = case_inputs(Cn, T)
    lm = chain_lm(Cn, 3, seed=Cn)
    got = _engine().ctc_beam_nbest(torch.from_numpy(logits).cuda(), lens, beam, nbest, lm, 6, 0.7, 0.3)
    for n, L in enumerate(lens):
        want, gaps = nbest_host(logits[n, :L].T, beam, nbest, lm, 6, 0.7, 0.3, return_gap=True)
        if min(gaps) < 1e-4:                                         # (printed: the plain cases above are the asserted ones)
            print(f'({Cn},{T}) line {n}: gap {min(gaps):.3g}, not compared')
            continue
        assert len(got[n]) == len(want)
        for (recs, logp, lmv), (wrecs, wlogp, wlmv) in zip(got[n], want):
            assert [r[:3] for r in recs] == [r[:3] for r in wrecs]
            np.testing.assert_allclose(logp, wlogp, rtol=2e-6, atol=1e-3)
            assert lmv == wlmv


# ---- the scorer's widths, seams and stack placements: every hypothesis against independent references on ITS OWN labels and starts
# ---- (no decision of the search is involved: tests/beam_cases.py NBEST_L)
def _planted_batch(Ls, Cn=bc.NBEST_C, gain=bc.NBEST_GAIN, wide=0):
    """The planted lines of Ls in one zero-padded batch; `wide`: that many classes in all, the added ones noise two below the rest."""
    lines = [bc.planted_line(L, Cn, gain, 0)[0] for L in Ls]
    if wide:
        g = np.random.default_rng(wide)
        lines = [np.concatenate([l, g.standard_normal((l.shape[0], wide - Cn)).astype(np.float32) - np.float32(2.0)], axis=1) for l in lines]
    x = np.zeros((len(lines), max(l.shape[0] for l in lines), lines[0].shape[1]), dtype=np.float32)
    for n, l in enumerate(lines):
        x[n, :l.shape[0]] = l
    return x, [l.shape[0] for l in lines]


def _check_on_own_labels(eng, x, lens, got, lm=None):
    """logp against float64 `ctc_logp` and against -cocr_ctc_loss (rtol 2e-6, atol 1e-3), NaN exactly beyond 255 labels; ends exact and
    conf to 1e-4 against the post-pass restated on the host (lm.records_host) from the hypothesis's labels and starts; with `lm`,
    lmv = nbest.lm_sum bit for bit.  Returns the label counts seen."""
    loss = _loss_of(eng, torch.from_numpy(x).cuda(), lens, got)
    seen, worst = [], 0.0
    for n, L in enumerate(lens):
        line = x[n, :L].T
        lp = _log_softmax(line)
        for j, (recs, logp, lmv) in enumerate(got[n]):
            labels = [r[0] for r in recs]
            seen.append(len(labels))
            want = records_host(lp, labels, [r[1] for r in recs])
            assert [r[:3] for r in recs] == [r[:3] for r in want], (n, j)
            np.testing.assert_allclose([r[3] for r in recs], [r[3] for r in want], rtol=1e-4)
            assert math.isnan(logp) == (len(labels) > 255), (n, j, len(labels), logp)
            if len(labels) <= 255:
                ref = ctc_logp(line, labels)
                worst = max(worst, abs(logp - ref))
                np.testing.assert_allclose(logp, ref, rtol=2e-6, atol=1e-3, err_msg=f'line {n} hypothesis {j}: {len(labels)} labels')
                np.testing.assert_allclose(logp, loss[n][j], rtol=2e-6, atol=1e-3, err_msg=f'line {n} hypothesis {j}: {len(labels)} labels')
            assert lmv == (lm_sum(lm, labels) if lm is not None else 0.0), (n, j)
    print(f'{len(seen)} hypotheses of {sorted(set(seen))} labels: worst |logp - float64 definition| {worst:.3g}')
    return seen


_SEAM = {31: 31, 32: 31, 63: 63, 127: 127, 128: 127, 254: 255, 255: 255}      # labels: at most this many on one side, more on the other


@pytest.mark.parametrize('Ls', [(L,) for L in bc.NBEST_L] + [bc.NBEST_L], ids=lambda Ls: '-'.join(map(str, Ls)))
def test_scores_and_records_across_the_scorer_seams(Ls):
    """nbest_forward<1|2|4|8>: 2 labels + 1 states, 64 per register; the seams are at 31 | 32, 63 | 64 and 127 | 128 labels, the limit
    at 255 | 256.  Each planted line alone (the narrowest instantiation that holds its longest hypothesis) and all in one call (narrow
    hypotheses in the widest instantiation).  The order of the hypotheses is the definition's (its gaps on these lines:
    tests/test_beam_cases_host.py)."""
    x, lens = _planted_batch(Ls)
    eng = _engine()
    got = eng.ctc_beam_nbest(torch.from_numpy(x).cuda(), lens, bc.NBEST_BEAM, bc.NBEST_BEAM)
    seen = _check_on_own_labels(eng, x, lens, got)
    for n, L in enumerate(Ls):
        want = nbest_host(x[n, :lens[n]].T, bc.NBEST_BEAM, bc.NBEST_BEAM)
        assert [[r[:2] for r in h[0]] for h in got[n]] == [[r[:2] for r in h[0]] for h in want], L
        counts = [len(h[0]) for h in got[n]]
        assert min(counts) <= _SEAM[L] < max(counts), (L, counts)                    # both sides of the seam within one line
    if len(Ls) > 1:
        for lo, hi in ((0, 31), (32, 63), (64, 127), (128, 255), (256, 10 ** 6)):     # S <= 64, <= 128, <= 256, <= 511, and no score
            assert any(lo <= c <= hi for c in seen), (lo, hi)


def test_workspace_stacks_equal_lds_stacks():
    """beam = nbest = 32 on a line of 570 frames: 4 + (32 + 32) * 4 = 260 bytes of LDS per frame pass 144 KB from 568 frames on, so the
    chains' stacks (and the back-pointer rows) are read from the workspace (IN_LDS = false) in the width-8 instantiation; nbest = 4 on
    the same lines (148 bytes per frame, 84 KB) stays in LDS.
    Hypotheses 0..3 must be equal in every byte.  The 282 labels of the long line have no score; the second line (200 labels, 401
    states) is scored in that form, and checked against the references."""
    x, lens = _planted_batch((282, 200), gain=6.0)
    assert lens == [570, 406]
    eng = _engine()
    xd = torch.from_numpy(x).cuda()
    rc, big = _raw(eng, xd, lens, 32, 32)
    rc2, small = _raw(eng, xd, lens, 32, 4)
    assert rc == rc2 == 0 and (small['nhyp'] == 4).all() and (big['nhyp'] >= 4).all()
    for k in ('labels', 'starts', 'ends', 'conf', 'counts', 'scores'):
        assert big[k][:, :4].tobytes() == small[k].tobytes(), k
    assert (small['counts'][0] > 255).all() and np.isnan(small['scores'][0, :, 0]).all()
    assert (small['counts'][1] > 127).all() and (small['counts'][1] <= 255).all()
    seen = _check_on_own_labels(eng, x, lens, eng.ctc_beam_nbest(xd, lens, 32, 32))
    assert len(seen) == 64


def test_ngram_sum_across_the_chunk_border():
    """Hypotheses of 111..114 labels: the n-gram sum runs in two chunks of 64 lookups, the contexts of labels 64..66 reach back across
    the border.  lmv = the host's float32 sum bit for bit, for every hypothesis; logp and records as above."""
    x, lens = _planted_batch((127,))
    lm = chain_lm(bc.NBEST_C, 3, seed=5)
    eng = _engine()
    got = eng.ctc_beam_nbest(torch.from_numpy(x).cuda(), lens, bc.NBEST_BEAM, bc.NBEST_BEAM, lm, 5, 0.7, 0.5)
    seen = _check_on_own_labels(eng, x, lens, got, lm)
    assert len(seen) == bc.NBEST_BEAM and min(seen) > 64 + 8
    assert len({h[2] for h in got[0]}) > 1                                         # (not one sum for all)


def test_exhaustive_trail_on_long_hypotheses():
    """300 classes: ctc_beam_kernel leaves the trail (log Z at stride 1).  The L = 63 line with 294 noise classes added."""
    x, lens = _planted_batch((63,), wide=300)
    eng = _engine()
    got = eng.ctc_beam_nbest(torch.from_numpy(x).cuda(), lens, bc.NBEST_BEAM, bc.NBEST_BEAM)
    seen = _check_on_own_labels(eng, x, lens, got)
    assert len(seen) == bc.NBEST_BEAM and min(seen) > 31


def _peaked(path, Cn=4, hi=12.0, lo=-6.0):
    m = np.full((len(path), Cn), lo, dtype=np.float32)
    m[np.arange(len(path)), path] = hi
    return m


def test_edges():
    eng = _engine()
    # len 1: blank or one label
    x = torch.from_numpy(case_inputs(5, 12)[0][:1, :1]).cuda()
    (hyps,) = eng.ctc_beam_nbest(x, [1], 4, 4)
    want = nbest_host(x[0].cpu().numpy().T, 4, 4)
    assert [h[0] for h in hyps] == [[r[:3] + (pytest.approx(r[3], rel=1e-4),) for r in w[0]] for w in want]
    np.testing.assert_allclose([h[1] for h in hyps], [w[1] for w in want], rtol=2e-6, atol=1e-3)
    # 600 peaked frames alternating two labels with blanks between: 300 labels, no score; the other lines of the call are unaffected
    T = 600
    long_line = _peaked([0 if t % 2 else 1 + (t // 2) % 2 for t in range(T)])
    short = np.zeros((T, 4), dtype=np.float32)
    short[:9] = _peaked([0, 2, 2, 0, 2, 3, 3, 0, 1])                  # 2 2 3 1 with a repeated label: the lattice's skip rule
    x = torch.from_numpy(np.stack([long_line, short, long_line])).cuda()
    got = eng.ctc_beam_nbest(x, [T, 9, 9], 4, 2)
    recs, logp, _ = got[0][0]
    assert len(recs) == 300 and math.isnan(logp)
    assert [r[:3] for r in recs] == [(1 + k % 2, 2 * k, 2 * k) for k in range(300)]
    assert recs == eng.ctc_beam(x, [T, 9, 9], 4)[0]
    for n in (1, 2):                                                  # (the runners-up of a peaked line are near-ties: each against its own labels)
        line = x[n, :9].cpu().numpy().T
        assert [r[:3] for r in got[n][0][0]] == [r[:3] for r in nbest_host(line, 4, 1)[0][0]]
        for recs, logp, _ in got[n]:
            np.testing.assert_allclose(logp, ctc_logp(line, [r[0] for r in recs]), rtol=2e-6, atol=1e-3)
    assert [r[0] for r in got[1][0][0]] == [2, 2, 3, 1]
    # max_per_line smaller than a hypothesis: the full count and the head of the full rows, as the 1-best writes them
    logits, lens = case_inputs(11, 40)
    x = torch.from_numpy(logits).cuda()
    rc, full = _raw(eng, x, lens, 16, 8)
    rc2, cut = _raw(eng, x, lens, 16, 8, mpl=3)
    assert rc == rc2 == 0 and (full['counts'] == cut['counts']).all() and full['counts'][0].max() > 3
    one = {k: torch.full((4, 3), -7, dtype=torch.int32).cuda() for k in ('labels', 'starts', 'ends')}
    conf1, cnt1 = torch.full((4, 3), -7.0).cuda(), torch.zeros(4, dtype=torch.int32).cuda()
    ln = np.asarray(lens, dtype=np.int32)
    assert eng.lib.cocr_ctc_beam(eng._h, C.c_void_p(x.data_ptr()), 4, 40, 11, ln.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(one['labels'].data_ptr()),
                                 C.c_void_p(one['starts'].data_ptr()), C.c_void_p(one['ends'].data_ptr()), C.c_void_p(conf1.data_ptr()),
                                 C.c_void_p(cnt1.data_ptr()), 3, 16, None) == 0
    torch.cuda.synchronize()
    for k in one:
        assert (cut[k][:, 0] == one[k].cpu().numpy()).all(), k
    assert cut['conf'][:, 0].tobytes() == conf1.cpu().numpy().tobytes() and (cut['counts'][:, 0] == cnt1.cpu().numpy()).all()
    for n in range(4):
        for j in range(int(full['nhyp'][n])):
            keep = min(3, int(full['counts'][n, j]))
            for k in ('labels', 'starts', 'ends'):                    # every field of the full row: the last kept record is bounded by the next label's start
                assert (cut[k][n, j, :keep] == full[k][n, j, :keep]).all(), (k, n, j)
            assert cut['conf'][n, j, :keep].tobytes() == full['conf'][n, j, :keep].tobytes(), (n, j)
            assert (cut['labels'][n, j, keep:] == -7).all()
    assert np.array_equal(cut['scores'], full['scores'], equal_nan=True)
    # slots past nhyp: counts 0 and both scores -inf
    rc, few = _raw(eng, torch.from_numpy(case_inputs(3, 6)[0]).cuda(), [6, 3, 3, 1], 16, 16)
    assert rc == 0 and few['nhyp'].tolist() == [16, 9, 9, 3]
    for n, nh in enumerate(few['nhyp'].tolist()):
        assert (few['counts'][n, nh:] == 0).all() and np.isneginf(few['scores'][n, nh:]).all() and np.isfinite(few['scores'][n, :nh]).all()


def test_arguments_are_checked_without_a_launch():
    eng = _engine()
    x = torch.from_numpy(case_inputs(5, 12)[0]).cuda()
    lens = [12, 9, 6, 1]
    untouched = lambda out: all((v == -7).all() for v in out.values())
    for kw in (dict(nbest=0), dict(nbest=5), dict(null='scores'), dict(null='nhyp'), dict(null='labels'), dict(null='logits')):
        rc, out = _raw(eng, x, lens, 4, kw.get('nbest', 2), null=kw.get('null'))
        assert rc == _lib.EINVAL and untouched(out), kw
    rc, out = _raw(eng, x, lens, 4, 2, lm=chain_lm(7, 3, seed=1, n=10))                 # a model of another class count
    assert rc == _lib.EINVAL and untouched(out)
    rc, out = _raw(eng, x, [12, 13, 6, 1], 4, 2)
    assert rc == _lib.EINVAL and untouched(out)
    with pytest.raises(ValueError):
        eng.ctc_beam_nbest(x, lens, 4, 0)


def test_two_calls_give_equal_bytes():
    logits, lens = case_inputs(128, 48)
    x = torch.from_numpy(logits).cuda()
    lm = chain_lm(128, 3, seed=2, n=50)
    eng = _engine()
    for kw in (dict(), dict(lm=lm)):
        (rc, a), (rc2, b) = _raw(eng, x, lens, 16, 16, **kw), _raw(eng, x, lens, 16, 16, **kw)
        assert rc == rc2 == 0
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k


# ---- surface
def _tiny_net(case, decoder):
    from conformer_ocr_amd.codec import ascii_codec
    from conformer_ocr_amd.pred import PytorchRecognitionModel
    hp, state, image, lens, g = case('tiny')
    net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1,
                                  codec=ascii_codec(hp.num_classes), ctc_decoder=decoder, compute_dtype='fp32')
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return net.to('cuda:0'), image, lens, g


def test_predict_nbest(case):
    from conformer_ocr_amd.ctc_decoder import BeamDecoder, GreedyDecoder, LMDecoder
    from conformer_ocr_amd.nbest import oracle_errors, recognize_nbest, rescore
    net, image, lens, g = _tiny_net(case, BeamDecoder(16))
    x, xl = torch.from_numpy(image).cuda(), torch.from_numpy(lens)
    strings = net.predict_string(x, xl)
    hyps = net.predict_nbest(x, xl, 4)
    assert [h[0][0] for h in hyps] == strings
    labels = net.predict_labels(x, xl)
    assert [h[0][3] for h in hyps] == labels
    for n, hs in enumerate(hyps):
        want = nbest_host(g['logits'][n, :int(g['out_lens'][n])].T, 16, 4)
        assert len(hs) == len(want) and all(lmv == 0.0 for _, _, lmv, _ in hs)
        np.testing.assert_allclose(hs[0][1], want[0][1], rtol=2e-6, atol=1e-3)
        assert rescore(hs, 0.0, 0.0)[0][1] == max(h[1] for h in hs)
    # the oracle distance of the 4-best on the device = the host functions', and no worse than the 1-best's
    truths = [s[:-1] + 'x' for s in strings]
    texts = [[h[0] for h in hs] for hs in hyps]
    dev = oracle_errors(texts, truths, engine=net._engine)
    assert dev == oracle_errors(texts, truths, scorer='host')
    assert all(d <= e for d, e in zip(dev, oracle_errors([t[:1] for t in texts], truths, engine=net._engine)))
    lines = [image[n, 0, :, :int(lens[n])] for n in range(image.shape[0])]
    out = recognize_nbest(net, lines, 4, batch_size=image.shape[0], edge=image.shape[3])
    assert [out[n][0][0] for n in range(len(lines))] == strings
    lm = chain_lm(11, 3, seed=5)
    net.ctc_decoder = LMDecoder(lm, beam_size=8, alpha=0.7, beta=0.5, classes=6)
    hyps = net.predict_nbest(x, xl, 3)
    assert [h[0][0] for h in hyps] == net.predict_string(x, xl)
    net.ctc_decoder = GreedyDecoder()
    with pytest.raises(ValueError, match='beam'):
        net.predict_nbest(x, xl, 4)


def _saved_text_model(tc, tmp_path):
    from conformer_ocr_amd.codec import ascii_codec
    from conformer_ocr_amd.pred import PytorchRecognitionModel, save_safetensors
    codec = ascii_codec(tc.hp.num_classes)
    src = PytorchRecognitionModel(**tc.hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1,
                                  codec=codec)
    src.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    save_safetensors(src, tmp_path / 'model.tar')
    return src, codec


def test_ocr_command_writes_the_nbest_json(text_case, tmp_path):
    """`ocr --beam 16 --nbest 3` on a synthetic page: the JSON's first entries are the text file's lines; without --nbest the text file
    has the same bytes, which are `recognize_pages`' with the decoder set by hand, and no JSON is written."""
    from PIL import Image
    from conformer_ocr_amd import ocr
    from conformer_ocr_amd.ctc_decoder import BeamDecoder
    from conformer_ocr_amd.page import Line, recognize_pages
    from tests import page_synth
    from tests.test_hip_page import FIXTURE_FORM, KINDS, PICK
    tc = text_case('cfg2_text')
    lines = [np.rint(tc.lines[i] * 255.0).astype(np.uint8) for i in PICK[:4]]
    page, placed = page_synth.text_page(lines, KINDS[:4])
    page_lines = [Line(f'line{k}', P, B) for k, (_, P, B) in enumerate(placed)]
    Image.fromarray(page).save(tmp_path / 'scan.png')
    pts = lambda a: ' '.join(f'{x:.3f},{y:.3f}' for x, y in a)
    body = ''.join(f'<TextLine id="{l.id}"><Coords points="{pts(l.boundary)}"/><Baseline points="{pts(l.baseline)}"/></TextLine>\n'
                   for l in page_lines)
    (tmp_path / 'scan.xml').write_text('<?xml version="1.0"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2019-07-15">'
                                       f'<Page imageFilename="scan.png"><TextRegion id="r">{body}</TextRegion></Page></PcGts>\n')
    src, codec = _saved_text_model(tc, tmp_path)
    base = ['-m', str(tmp_path / 'model.tar'), '-f', 'page', '--pad', '0', '--edge', '1200', '--beam', '16']
    assert ocr.main(base + ['-i', str(tmp_path / 'scan.xml'), str(tmp_path / 'a.txt'), '--nbest', '3']) == 0
    assert ocr.main(base + ['-i', str(tmp_path / 'scan.xml'), str(tmp_path / 'b.txt')]) == 0
    text = (tmp_path / 'a.txt').read_bytes()
    assert text == (tmp_path / 'b.txt').read_bytes() and not (tmp_path / 'b.txt.nbest.json').exists()
    src.ctc_decoder = BeamDecoder(16)
    want, = recognize_pages(src.to('cuda:0').eval(), [(page, page_lines)], **FIXTURE_FORM)
    assert text.decode('utf-8').split('\n')[:-1] == [r['text'] for r in want]
    doc = json.loads((tmp_path / 'a.txt.nbest.json').read_text(encoding='utf-8'))
    assert list(doc) == [l.id for l in page_lines]
    assert [doc[l.id][0]['text'] for l in page_lines] == [r['text'] for r in want]
    for l in page_lines:
        assert 1 <= len(doc[l.id]) <= 3
        for h in doc[l.id]:
            assert set(h) == {'text', 'logp', 'lm_logp', 'conf'} and len(h['conf']) == len(h['text']) and h['logp'] <= 0.0 and h['lm_logp'] == 0.0
    with pytest.raises(SystemExit, match='--nbest needs a beam'):
        ocr.main(base[:-2] + ['-i', str(tmp_path / 'scan.xml'), str(tmp_path / 'c.txt'), '--nbest', '3'])


def test_test_command_prints_the_oracle_cer(text_case, tmp_path, capsys):
    """`test --beam 16 --nbest 4` on four fixture lines as line images, two of them with a wrong character in their ground truth: one
    more line, an oracle CER no larger than the 1-best CER; the rest of the output is that of the run without --nbest."""
    from PIL import Image
    from conformer_ocr_amd import test as testcmd
    tc = text_case('cfg2_text')
    src, codec = _saved_text_model(tc, tmp_path)
    files = []
    for i in range(4):
        Image.fromarray(np.rint(tc.lines[i] * 255.0).astype(np.uint8)).save(tmp_path / f'l{i}.png')
        truth = ''.join(codec.l2c[(l,)] for l in tc.texts[i])
        (tmp_path / f'l{i}.gt.txt').write_text(truth if i % 2 else truth[:-1] + ('a' if truth[-1] != 'a' else 'b'), encoding='utf-8')
        files.append(str(tmp_path / f'l{i}.png'))
    base = ['-m', str(tmp_path / 'model.tar'), '-f', 'path', '--pad', '0', '--edge', '1200', '--beam', '16'] + files
    assert testcmd.main(base) == 0
    plain = capsys.readouterr().out
    assert testcmd.main(base + ['--nbest', '4']) == 0
    out = capsys.readouterr().out
    extra = [l for l in out.splitlines() if l.startswith('oracle CER in the 4-best: ')]
    assert len(extra) == 1
    assert ''.join(l + '\n' for l in out.splitlines() if l not in extra) == plain
    best, first = float(extra[0].split()[5]), float(extra[0].split()[7].rstrip(')'))
    assert 0.0 <= best <= first and first > 0.0
