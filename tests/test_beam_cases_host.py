"""CPU: the conditions under which the cases of tests/beam_cases.py may be compared with the device line by line, none left out.
For every line the definition's smallest decision gap (the beam-th against the (beam+1)-th candidate of any frame, and the final
top two) is at least the GAP of the comparing file -- the device's logaddexp differs from numpy's in the last ulps, and a decision
closer than that may fall the other way -- and, for the plain search, the definition evaluated in float64 returns the labels,
starts and ends of its float32 evaluation.  A case added later that breaks either fails here."""
import math

import numpy as np
import pytest

from conformer_ocr_amd.nbest import nbest_host
from tests import beam_cases as bc

PLAIN = [(name, beam) for table in (bc.PLAIN, bc.PLAIN_EXHAUSTIVE) for name, (_, beams) in table.items() for beam in beams]


@pytest.mark.parametrize('name,beam', PLAIN)
def test_plain_cases_are_decided_and_float32_equals_float64(name, beam):
    spec = (bc.PLAIN.get(name) or bc.PLAIN_EXHAUSTIVE[name])[0]
    rows32, rows64 = bc.plain_host(spec, beam), bc.plain_host(spec, beam, np.float64)
    for n, ((r32, (frame_gap, final_gap)), (r64, _)) in enumerate(zip(rows32, rows64)):
        print(f'{name}, beam {beam}, line {n}: {len(r32)} labels, frame gap {frame_gap:.3g}, final gap {final_gap:.3g}')
        assert frame_gap >= bc.GAP_PLAIN and final_gap >= bc.GAP_PLAIN, (n, frame_gap, final_gap)
        assert [r[:3] for r in r32] == [r[:3] for r in r64], n
        np.testing.assert_allclose([r[3] for r in r32], [r[3] for r in r64], rtol=1e-5)


@pytest.mark.parametrize('name', list(bc.LM))
def test_lm_cases_are_decided(name):
    _, rows = bc.lm_host(name)
    for n, (recs, _, gap) in enumerate(rows):
        print(f'{name}, line {n}: {len(recs)} labels, gap {gap:.3g}')
        assert gap >= bc.GAP_LM, (n, gap)


def test_generators_are_pinned():
    """The recipes, so that a change of them shows here and not as a changed case: the planted path and the gain on it, the ragged
    lengths, the masks."""
    x, labels = bc.planted_line(31, 6, 4.0, 0)
    noise = np.random.default_rng(9031).standard_normal((68, 6)).astype(np.float32)
    assert x.shape == (68, 6) and x.dtype == np.float32 and len(labels) == 31 and all(1 <= c <= 5 for c in labels)
    path = np.zeros(68, dtype=np.int64)
    path[3:3 + 62:2] = labels
    d = x - noise
    assert (d[np.arange(68), path] == (noise[np.arange(68), path] + np.float32(4.0)) - noise[np.arange(68), path]).all()
    d[np.arange(68), path] = 0
    assert (d == 0).all()
    x, lens = bc.random_case(11, 24, 5, 2.0)
    assert x.shape == (5, 24, 11) and lens == [24, 21, 12, 1, 0]
    x, lens = bc.masked_case()
    assert np.isneginf(x[:, :, [1, 4, 7, 10]]).all() and np.isfinite(x[0][:, [0, 2, 3, 5, 6, 8, 9, 11]]).all()
    assert np.isneginf(x[1, ::5, 0]).all() and np.isfinite(x[2, 7]).sum() == 2


def test_nbest_lines_lie_on_both_sides_of_every_seam():
    """The definition's 8-best of the planted n-best lines: hypotheses of 2 L + 1 states in each of the scorer's four widths, on both
    sides of each seam within single lines, and beyond the 255-label limit; and the definition's gaps on them (every frame's cut and every
    adjacent pair of the 8 + 1 final scores), since tests/test_hip_nbest.py compares the order of the hypotheses with the definition's."""
    lens = {}
    for L in bc.NBEST_L:
        x, _ = bc.planted_line(L, bc.NBEST_C, bc.NBEST_GAIN, 0)
        hyps, (frame_gap, final_gap) = nbest_host(x.T, bc.NBEST_BEAM, bc.NBEST_BEAM, return_gap=True)
        lens[L] = sorted({len(h[0]) for h in hyps})
        assert all(math.isnan(h[1]) == (len(h[0]) > 255) for h in hyps)
        print(f'L = {L}: hypotheses of {lens[L]} labels, frame gap {frame_gap:.3g}, smallest adjacent final gap {final_gap:.3g}')
        assert frame_gap >= bc.GAP_PLAIN and final_gap >= bc.GAP_PLAIN, (L, frame_gap, final_gap)      # the GPU test compares the order of all 8
    every = {c for v in lens.values() for c in v}
    for lo, hi in ((31, 32), (63, 64), (127, 128), (255, 256)):           # S = 2 labels + 1: 63 | 65, 127 | 129, 255 | 257, 511 | no score
        assert lo in every and hi in every, (lo, hi, lens)
    assert min(lens[32]) <= 31 and max(lens[32]) >= 32 or min(lens[31]) <= 31 and max(lens[31]) >= 32
