"""The host plumbing every decode and search call of `HipRecognizer` shares -- the argument check, the pool of pinned output buffers,
the handle -- for each family of calls at one tiny shape.  What the kernels compute is the business of the families' own suites."""
import numpy as np
import pytest
import torch

from conformer_ocr_amd import pattern as PT
from tests.test_hip_lm import _chain_lm

pytestmark = pytest.mark.gpu
N, T, NCLS = 2, 12, 6
LENS = [12, 9]
QUERIES = [[1], [2, 3], [4, 5, 1]]
LABELS, LABEL_LENS = [1, 2, 3, 4, 5], [3, 2]
PAGES = [[0, 1]]
_LM = []


def _engine():
    from conformer_ocr_amd.ctc_decoder import _scratch_engine
    return _scratch_engine(torch.device('cuda', 0))


def _lm():
    if not _LM:
        _LM.append(_chain_lm(NCLS, 2, seed=NCLS, n=20))
    return _LM[0]


def _graph():
    return PT.PatternGraph('', [1, 2], [True, False], [False, True], [[], [0]])


# engine method (its `_async` form enqueues) -> (the arguments after (logits, out_lens), the `collect_*` of its handle, the keyword
# whose value the C prologue refuses: a beam or a hit count of 0, a label >= ncls)
FAMILIES = {
    'ctc_greedy': (lambda: (), 'collect', None),
    'ctc_beam': (lambda beam=4: (beam,), 'collect', dict(beam=0)),
    'ctc_beam_lm': (lambda beam=4: (_lm(), beam, 4, 0.7, 0.5), 'collect', dict(beam=0)),
    'ctc_beam_nbest': (lambda beam=4: (beam, 3), 'collect_nbest', dict(beam=0)),
    'ctc_align': (lambda label=3: ([1, 2, label, 4, 5], LABEL_LENS), 'collect_align', dict(label=NCLS)),
    'ctc_align_page': (lambda label=3: (PAGES, [[1, 2, label, 4]]), 'collect_align_page', dict(label=NCLS)),
    'ctc_spot': (lambda hits=2: (QUERIES, hits), 'collect_spot', dict(hits=0)),
    'ctc_spot_pattern': (lambda hits=2: ([_graph()], hits), 'collect_spot_pattern', dict(hits=0)),
}


def _plain(v):
    """Results as nested lists of numbers: `collect_align_page` returns arrays among its tuples."""
    if isinstance(v, np.ndarray):
        return v.tolist()
    return [_plain(e) for e in v] if isinstance(v, (list, tuple)) else v


@pytest.fixture(scope='module')
def logits():
    """Two seeded (N, T, ncls) batches on the host, and per family what its synchronous method returns for each of them alone."""
    x = (np.random.default_rng(2026).normal(size=(2, N, T, NCLS)) * 2).astype(np.float32)
    eng = _engine()
    want = {name: [_plain(getattr(eng, name)(torch.from_numpy(x[i]).cuda(), LENS, *args())) for i in range(2)] for name, (args, _, _) in FAMILIES.items()}
    return x, want


@pytest.mark.parametrize('name', FAMILIES)
def test_two_handles_in_flight(name, logits):
    """Two calls of one pool key enqueued, the second collected first: each returns what the synchronous call returns for its tensor --
    they do not share buffers, and each handle keeps the tensor it reads alive (the caller drops it at once here)."""
    x, want = logits
    args, collect, _ = FAMILIES[name]
    eng = _engine()
    h0 = getattr(eng, name + '_async')(torch.from_numpy(x[0]).cuda(), LENS, *args())
    h1 = getattr(eng, name + '_async')(torch.from_numpy(x[1]).cuda(), LENS, *args())
    assert h0.key == h1.key and not {b.data_ptr() for b in h0.host} & {b.data_ptr() for b in h1.host}
    got1 = _plain(getattr(eng, collect)(h1))
    got0 = _plain(getattr(eng, collect)(h0))
    assert got0 == want[name][0] and got1 == want[name][1]
    assert want[name][0] != want[name][1]                               # (the two tensors do tell the calls apart)


@pytest.mark.parametrize('name', [n for n, f in FAMILIES.items() if f[2] is not None])
def test_a_refused_call_gives_its_buffers_back(name, logits):
    """Good call, a call of the same shapes that the C prologue refuses, good call: the third runs on the first one's pinned buffers.
    (Greedy has no refusal that valid Python arguments reach.)"""
    x, want = logits
    args, collect, bad = FAMILIES[name]
    eng = _engine()
    d = torch.from_numpy(x[0]).cuda()
    first = getattr(eng, name + '_async')(d, LENS, *args())
    ptrs = [b.data_ptr() for b in first.host]
    assert _plain(getattr(eng, collect)(first)) == want[name][0]
    with pytest.raises(ValueError):
        getattr(eng, name + '_async')(d, LENS, *args(**bad))
    third = getattr(eng, name + '_async')(d, LENS, *args())
    assert third.key == first.key and [b.data_ptr() for b in third.host] == ptrs
    assert _plain(getattr(eng, collect)(third)) == want[name][0]


@pytest.mark.parametrize('name', FAMILIES)
def test_out_lens_of_the_wrong_length_is_refused_before_any_launch(name, logits):
    x, want = logits
    args, _, _ = FAMILIES[name]
    eng = _engine()
    d = torch.from_numpy(x[1]).cuda()
    for method in (name, name + '_async'):
        with pytest.raises(ValueError):
            getattr(eng, method)(d, LENS[:N - 1], *args())
    assert _plain(getattr(eng, name)(d, LENS, *args())) == want[name][1]
