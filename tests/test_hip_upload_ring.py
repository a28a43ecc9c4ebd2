"""GPU: the pinned upload rings of the host layer (UploadRing in model.hip.h) -- per-line lengths of the decoders,
the targets of loss and forced alignment, the pair tables of the edit-distance alignment.  A ring has 16 slots; these tests keep more calls
than that in flight behind other device work, make a ring regrow while earlier calls are pending, and alternate loss and alignment on the
ring they share.  Every call has its own lengths / targets (all within the logits' shape: a stale slot can only give a wrong answer), and
every result is held to its reference with the comparison of the entry point's own test module."""
import numpy as np
import pytest
import torch

from conformer_ocr_amd import align as A
from oracle import ctc_loss_ref as R
from oracle.ctc_ref import greedy_decoder as ref_greedy
from tests.test_hip_align import _check_valid, _frame_classes, _runner_up_gap, _tol
from tests.test_hip_score import _check as _check_pairs

pytestmark = pytest.mark.gpu
N, T, C = 5, 40, 11


def _fresh_engine():
    """A scratch engine of its own: the rings of the shared one (ctc_decoder._scratch_engine) have grown in earlier tests."""
    from conformer_ocr_amd.engine import HipRecognizer
    from conformer_ocr_amd.spec import HParams
    hp = HParams(num_classes=2, height=16, encoder_dim=16, num_encoder_layers=1, num_attention_heads=1, conv_kernel_size=3,
                 subsampling_conv_channels=8)
    return HipRecognizer(hp, torch.device('cuda', 0), 'fp32')


@pytest.fixture(scope='module')
def eng():
    return _fresh_engine()


def _backlog(n=48):
    """About 50 ms of work on the current stream (an estimate: n chained 4096^2 fp32 products), so that what is enqueued next waits."""
    x = torch.full((4096, 4096), 1.0 / 4096, device='cuda')         # x @ x == x: the chain neither grows nor vanishes
    y = x
    for _ in range(n):
        y = torch.matmul(y, x)
    return y


def _logits(g, n):
    return (g.standard_normal((n, T, C)) * 2.0).astype(np.float32)


def _targets(g, n, hi=6):
    label_lens = g.integers(0, hi + 1, size=n)
    return np.concatenate([g.integers(1, C, size=l) for l in label_lens] + [np.zeros(0, np.int64)]), label_lens


def _check_greedy(got, logits, lens):
    for n in range(logits.shape[0]):
        want = ref_greedy(logits[n, :lens[n]].T)
        assert [x[:3] for x in got[n]] == [x[:3] for x in want], n
        np.testing.assert_array_equal(np.float32([x[3] for x in got[n]]), np.float32([x[3] for x in want]))


def _check_align(got, logits, lens, targets, label_lens):
    """test_hip_align.test_scores_on_random_logits, per line: feasibility, a valid alignment, the float64 score of the device's path and
    the device's own score within `_tol` of the definition's, and the path itself where the runner-up lies further off than that."""
    off = np.concatenate([[0], np.cumsum(label_lens)])
    for n in range(len(lens)):
        t, lab = int(lens[n]), np.asarray(targets[off[n]:off[n + 1]], dtype=np.int64)
        x = logits[n, :t].T
        want, s_star = A.viterbi_align(x, lab)
        records, score = got[n]
        if want is None:
            assert records is None and score == -np.inf, n
            continue
        assert records is not None, n
        _check_valid(records, lab, t)
        lp = A.log_softmax64(x)
        tol = _tol(t, s_star)
        gap_path = s_star - float(lp[_frame_classes(records, t), np.arange(t)].sum())
        assert -1e-9 * max(1.0, abs(s_star)) <= gap_path <= tol, (n, gap_path, tol)
        assert abs(score - s_star) <= tol, (n, score, s_star, tol)
        states, _ = A.viterbi_path(lp, lab)
        if t > 0 and _runner_up_gap(lp, lab, states) > tol:
            assert [r[:3] for r in records] == [r[:3] for r in want], n


def _check_loss(nll, probits, lens, targets, label_lens):
    want, _ = R.ctc_loss(probits, targets, lens, label_lens)
    np.testing.assert_allclose(nll.cpu().numpy(), want, rtol=2e-6, atol=1e-3)        # test_hip_ctc_loss's bar


def test_more_calls_in_flight_than_slots(eng):
    """40 decodes, then 40 alignments, enqueued behind a backlog and collected only at the end: each answers for its own lengths."""
    g = np.random.default_rng(40)
    calls = 40
    logits = [_logits(g, N) for _ in range(calls)]
    dev = [torch.from_numpy(x).cuda() for x in logits]
    lens = [g.integers(0, T + 1, size=N) for _ in range(calls)]
    lens[0][0], lens[1][1] = 0, T
    assert len({tuple(l) for l in lens}) == calls
    busy = _backlog()
    handles = [eng.ctc_greedy_async(dev[i], lens[i]) for i in range(calls)]
    got = [eng.collect(h) for h in handles]
    for i in range(calls):
        _check_greedy(got[i], logits[i], lens[i])

    tg = [_targets(g, N) for _ in range(calls)]
    assert len({(tuple(t), tuple(l)) for t, l in tg}) == calls
    busy = _backlog()
    handles = [eng.ctc_align_async(dev[i], lens[i], *tg[i]) for i in range(calls)]
    got = [eng.collect_align(h) for h in handles]
    for i in range(calls):
        _check_align(got[i], logits[i], lens[i], *tg[i])
    del busy


def test_regrowth_with_work_pending():
    """Each ring grows while earlier calls of a fresh engine are enqueued and not collected."""
    eng = _fresh_engine()
    g = np.random.default_rng(41)
    # lengths ring: three decodes of 2 lines, then three of 9
    batches = [(_logits(g, n), g.integers(0, T + 1, size=n)) for n in (2, 2, 2, 9, 9, 9)]
    dev = [torch.from_numpy(x).cuda() for x, _ in batches]          # (before the backlog: a copy from pageable memory waits for the stream)
    busy = _backlog(16)
    handles = [eng.ctc_greedy_async(d, l) for d, (_, l) in zip(dev, batches)]
    for h, (x, l) in zip(handles, batches):
        _check_greedy(eng.collect(h), x, l)
    # targets ring: 4 labels in all, then 60
    cases = []
    for label_lens in ([1, 3], [0, 4], [2, 2], [6] * 10, [12] * 5, [20, 10, 30]):
        n = len(label_lens)
        cases.append((_logits(g, n), g.integers(T // 2, T + 1, size=n), g.integers(1, C, size=sum(label_lens)), np.array(label_lens)))
    dev = [torch.from_numpy(c[0]).cuda() for c in cases]
    busy = _backlog(16)
    nll = [eng.ctc_loss(d, l, tg, tl, with_grad=False)[0] for d, (_, l, tg, tl) in zip(dev, cases)]
    for v, (x, l, tg, tl) in zip(nll, cases):
        _check_loss(v, x, l, tg, tl)
    # score ring: 3 pairs, then 300
    for pairs in (3, 300):
        _check_pairs(eng, [(g.integers(0, 5, int(g.integers(0, 13))).tolist(), g.integers(0, 5, int(g.integers(0, 13))).tolist())
                           for _ in range(pairs)])
    del busy


def test_loss_and_alignment_interleaved_on_the_shared_ring(eng):
    """One batch of logits, ten target sets for the loss and ten for the alignment, enqueued alternately and collected at the end."""
    g = np.random.default_rng(42)
    logits = _logits(g, N)
    dev = torch.from_numpy(logits).cuda()
    lens = g.integers(T // 2, T + 1, size=N)
    tg = [_targets(g, N) for _ in range(20)]
    busy = _backlog(16)
    nll, handles = [], []
    for i in range(10):
        nll.append(eng.ctc_loss(dev, lens, *tg[2 * i], with_grad=False)[0])
        handles.append(eng.ctc_align_async(dev, lens, *tg[2 * i + 1]))
    for i in range(10):
        _check_loss(nll[i], logits, lens, *tg[2 * i])
        _check_align(eng.collect_align(handles[i]), logits, lens, *tg[2 * i + 1])
    del busy
