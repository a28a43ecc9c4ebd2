"""CPU: the definition of n-best decoding (conformer_ocr_amd/nbest.py nbest_host) against the definitions it extends, its exact CTC
score against the criterion's float64 restatement, `rescore`, and the gap condition of the cases the GPU test compares
(tests/test_hip_nbest.py imports CASES and `case_inputs` from here: a case added later that breaks the condition fails here)."""
import math

import numpy as np
import pytest

from conformer_ocr_amd.lm import beam_decode_host, build_lm
from conformer_ocr_amd.nbest import ctc_logp, lm_sum, nbest_host, oracle_errors, rescore
from oracle.ctc_loss_ref import ctc_line
from oracle.ctc_ref import beam_decoder as ref_beam

GAP = 1e-4          # a decision of the definition this close may flip on the device (its logaddexp differs from numpy's in the last ulps)
CASES = [(5, 12, 4, 4), (11, 40, 16, 8), (128, 48, 16, 5), (93, 33, 8, 8), (2, 30, 4, 4), (3, 6, 16, 16)]      # (C, T, beam, nbest)
FEWER = {(2, 30, 4, 4): [4, 4, 4, 2], (3, 6, 16, 16): [16, 9, 9, 3]}                                            # nhyp where lines run out of prefixes


def case_inputs(C, T):
    g = np.random.default_rng(C * 1000 + T)
    logits = (g.normal(size=(4, T, C)) * 2.5).astype(np.float32)
    logits[:, :, 0] += 1.5
    return logits, [T, T - 3, max(1, T // 2), 1]


def chain_lm(C, order, seed, n=200):
    """A model of `n` label sequences drawn from a random first-order chain."""
    g = np.random.default_rng(seed)
    P = g.dirichlet(np.full(C - 1, 0.3), size=C - 1)
    seqs = []
    for _ in range(n):
        s = [int(g.integers(1, C))]
        for _ in range(int(g.integers(4, 30))):
            s.append(1 + int(g.choice(C - 1, p=P[s[-1] - 1])))
        seqs.append(s)
    return build_lm(seqs, order, C)


_host = {}


def host_case(C, T, beam, nbest):
    """The definition on the four lines of a case, computed once: per line (hypotheses, (frame gap, final gap))."""
    key = (C, T, beam, nbest)
    if key not in _host:
        logits, lens = case_inputs(C, T)
        _host[key] = [nbest_host(logits[n, :L].T, beam, nbest, return_gap=True) for n, L in enumerate(lens)]
    return _host[key]


@pytest.mark.parametrize('C,T,beam,nbest', CASES)
def test_gap_condition_of_the_gpu_cases(C, T, beam, nbest):
    rows = host_case(C, T, beam, nbest)
    for n, (hyps, (frame_gap, final_gap)) in enumerate(rows):
        print(f'({C},{T},{beam},{nbest}) line {n}: {len(hyps)} hypotheses, frame gap {frame_gap:.3g}, final gap {final_gap:.3g}')
        assert frame_gap >= GAP and final_gap >= GAP, (n, frame_gap, final_gap)
    if (C, T, beam, nbest) in FEWER:
        assert [len(h) for h, _ in rows] == FEWER[(C, T, beam, nbest)]
    else:
        assert [len(h) for h, _ in rows] == [nbest] * 4


@pytest.mark.parametrize('C,T,beam', [(5, 12, 4), (11, 40, 16), (3, 6, 16)])
def test_first_hypothesis_is_the_plain_beam(C, T, beam):
    logits, lens = case_inputs(C, T)
    for n, L in enumerate(lens):
        x = logits[n, :L].T
        (recs, logp, lmv), = nbest_host(x, beam, 1)
        assert recs == ref_beam(x, beam)
        assert lmv == 0.0 and logp <= 0.0


@pytest.mark.parametrize('C,T,beam,classes', [(11, 40, 16, 6), (17, 30, 8, 8)])
def test_first_hypothesis_is_the_lm_beam(C, T, beam, classes):
    logits, lens = case_inputs(C, T)
    lm = chain_lm(C, 3, seed=C)
    for n, L in enumerate(lens):
        x = logits[n, :L].T
        want, gap = beam_decode_host(x, lm, beam, classes, 0.7, 0.3, return_gap=True)
        hyps, (frame_gap, final_gap) = nbest_host(x, beam, 3, lm, classes, 0.7, 0.3, return_gap=True)
        assert hyps[0][0] == want
        assert min(frame_gap, final_gap) <= gap or gap == math.inf           # the same frame gaps; one final pair more
        labels = [r[0] for r in want]
        acc = np.float32(0.0)
        for k, c in enumerate(labels):
            acc = np.float32(acc + lm.logp(labels[:k], c))
        assert hyps[0][2] == float(acc) == lm_sum(lm, labels)


@pytest.mark.parametrize('C,T,beam,nbest', CASES[:4])
def test_logp_is_the_criterion(C, T, beam, nbest):
    logits, lens = case_inputs(C, T)
    for n, (hyps, _) in enumerate(host_case(C, T, beam, nbest)):
        for recs, logp, _ in hyps:
            nll, _ = ctc_line(logits[n, :lens[n]].astype(np.float64), [r[0] for r in recs])
            assert abs(logp + nll) <= 1e-9, (n, logp, nll)


def test_logp_pinned_cases():
    g = np.random.default_rng(3)
    x = g.normal(size=(4, 9)).astype(np.float32)                   # (C, T)
    lp = x.astype(np.float64) - np.log(np.exp(x.astype(np.float64)).sum(axis=0, keepdims=True))
    assert abs(ctc_logp(x, []) - lp[0].sum()) <= 1e-12            # the empty hypothesis: every frame blank
    assert ctc_logp(x[:, :0], []) == 0.0
    assert nbest_host(x[:, :0], 4, 4) == [([], 0.0, 0.0)]          # a line of length 0: the empty hypothesis alone
    hyps, gaps = nbest_host(x[:, :0], 4, 4, return_gap=True)
    assert gaps == (math.inf, math.inf)
    # a repeated label needs the blank between: two frames cannot hold (1, 1)
    assert ctc_logp(x[:, :2], [1, 1]) == -math.inf
    assert abs(ctc_logp(x[:, :3], [1, 1]) - (lp[1, 0] + lp[0, 1] + lp[1, 2])) <= 1e-12


def test_more_than_255_labels_have_no_score():
    T = 520
    x = np.full((3, T), -8.0, dtype=np.float32)
    for t in range(T):
        x[0 if t % 2 else 1 + (t // 2) % 2, t] = 8.0               # 1 _ 2 _ 1 _ ...: 260 labels
    (recs, logp, lmv), = nbest_host(x, 2, 1)
    assert len(recs) == 260 and math.isnan(logp) and lmv == 0.0
    assert [r[0] for r in recs[:4]] == [1, 2, 1, 2] and [r[1] for r in recs[:3]] == [0, 2, 4]


def test_nbest_bounds():
    x = np.zeros((3, 4), dtype=np.float32)
    for bad in (0, 5):
        with pytest.raises(ValueError):
            nbest_host(x, 4, bad)


def test_rescore_order_ties_and_nan():
    r = lambda k: [(1, 0, 0, 1.0)] * k
    hyps = [(r(2), -3.0, -4.0), (r(3), -3.5, -1.0), (r(1), math.nan, 0.0), (r(2), -3.0, -4.0), (r(0), -9.0, 0.0)]
    assert rescore(hyps, 0.0, 0.0) == [hyps[0], hyps[3], hyps[1], hyps[4], hyps[2]]              # ties keep beam order, NaN last
    assert rescore(hyps, 1.0, 0.0) == [hyps[1], hyps[0], hyps[3], hyps[4], hyps[2]]              # -4.5 | -7, -7 | -9
    assert rescore(hyps, 0.0, 4.0)[0] is hyps[1]                                                  # the length bonus: 8.5 | 5, 5 | -9
    four = [('ab', -1.0, -2.0, r(2)), ('abc', -1.5, 0.0, r(3))]                                   # predict_nbest's form
    assert rescore(four, 1.0, 0.0) == [four[1], four[0]]
    assert rescore([], 1.0, 1.0) == []


def test_oracle_errors_on_the_host():
    hyps = [['kitten', 'sitten', 'sitting'], ['abc'], []]
    assert oracle_errors(hyps, ['sitting', 'abd', 'xyz'], scorer='host') == [0, 1, 3]
    with pytest.raises(ValueError):
        oracle_errors(hyps, ['a'])
