"""The rows per workgroup of the row-chain kernels: the 64-row form of the 256-wide engine, and the choice of the form from the number of
batches the process can really overlap (include/cocr.h: cocr_get_chain_rows).  Every form computes a row with the same arithmetic in the
same order, so all comparisons are bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conformer_ocr_amd import synth
from tests.hip_util import make_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_64_row_form_is_bit_identical_also_on_its_first_launch():
    """5 lines of 96 x 1200, ragged: M = 1500 = 23 x 64 + 28 rows -- blocks straddle line ends (300 frames per line), the last one is partial;
    two encoder blocks run every chain shape of a forward.  The FIRST forward of a fresh engine is compared too, behind a forward of other
    data: a wait that lets an operand tile or the depthwise window arrive late shows on LDS that still holds another launch's bytes
    (DESIGN section 4a), not on a repeated forward of the same batch."""
    hp = synth.hparams('cfg2', num_encoder_layers=2)
    state = synth.make_state_dict(hp, seed=3, decoder_gain=1.0, style='text')
    img, lens = synth.make_lines(5, hp.height, 1200, seed=11, widths=[1200, 1111, 800, 37, 1023])
    other, other_lens = synth.make_lines(5, hp.height, 1200, seed=12)
    x, xo = torch.from_numpy(img[:, 0]).cuda(), torch.from_numpy(other[:, 0]).cuda()
    ref = make_engine(hp, state, 'bf16')
    ref.set_chain_rows(32)
    assert ref.chain_rows(5, 1200) == 32
    want = ref.forward(x, lens)[0].cpu().numpy()
    ref.forward(xo, other_lens)                       # other data through the chip last
    torch.cuda.synchronize()
    eng = make_engine(hp, state, 'bf16')
    eng.set_chain_rows(64)
    assert eng.chain_rows(5, 1200) == 64              # the form exists: not mapped to a neighbour
    first = eng.forward(x, lens)[0].cpu().numpy()
    again = eng.forward(x, lens)[0].cpu().numpy()
    assert np.isfinite(want).all() and want.max() - want.min() > 1.0
    np.testing.assert_array_equal(first, want)
    np.testing.assert_array_equal(again, want)
    eng.set_chain_rows(80)                            # no 80-row form: the 64-row one
    assert eng.chain_rows(5, 1200) == 64


_CHILD = {}


def _child(queues, group_run=False):
    """One fresh process per value of GPU_MAX_HW_QUEUES (the library reads it once); the 4-queue one also runs the group comparison."""
    key = (queues, group_run)
    if key not in _CHILD:
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        for k in ('GPU_MAX_HW_QUEUES', 'COCR_TEST_QUEUES_UNSET', 'COCR_TEST_GROUP_RUN', 'COCR_CHAIN_ROWS'):
            env.pop(k, None)
        if queues is None:
            env['COCR_TEST_QUEUES_UNSET'] = '1'
        else:
            env['GPU_MAX_HW_QUEUES'] = str(queues)
        if group_run:
            env['COCR_TEST_GROUP_RUN'] = '1'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'chain_forms_child.py')], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _CHILD[key] = json.loads(r.stdout.strip().splitlines()[-1])
    return _CHILD[key]


@pytest.mark.parametrize('queues, four', [(4, 64), (8, 96), (None, 64)])
def test_form_follows_the_batches_that_can_overlap(queues, four):
    """32 x 1200 (M = 9600 rows) on one-block cfg2 models.  Four models on one set of weights: on 4 queues (3 for their streams) two
    forwards overlap, and 2 x 100 workgroups of 96 rows leave 56 CUs idle -> 64 rows (2 x 150); on 8 queues four overlap -> 96 rows.
    Three models on 4 queues overlap threefold -> 96.  The variable unset: the runtime's default of 4 queues."""
    got = _child(queues, group_run=queues == 4)
    assert got['queues_env'] == (None if queues is None else str(queues))
    assert got['four'] == [four] * 4                          # the owner and the three models that read its weights agree
    assert got['three'] == [96] * 3
    assert got['lone'] == 96
    assert got['four_one_line'] == [32] * 4 and got['lone_one_line'] == 32
    assert got['explicit48'] == [48, 48, 48, four]            # cocr_set_chain_rows wins, for that model only
    assert got['four_minus_destroyed'] == [96] * 3            # a destroyed model left the owner's count ...
    assert got['four_minus_two'] == [64, 64]                  # ... and so did one finalized on weights of its own: two overlap on any queue count
    assert got['leaver'] == 96


def test_group_computes_what_a_lone_model_computes_in_another_form():
    """11 lines x 1200 on a one-block cfg2 model under 4 queues: M = 3300 rows.  A model alone runs 32-row blocks; as one of four on one
    set of weights the same model runs a taller form (69 blocks of 48 rows: no form covers the chip twofold, the shortest with 50 or more
    blocks is taken).  Its launch sequences were captured with the old grid before the other three joined: they must be dropped, and every
    forward of the group -- plain, captured, replayed -- must equal the lone model's bit for bit."""
    g = _child(4, group_run=True)['group_run']
    assert g['finite'] and g['spread'] > 1.0
    assert g['rows_alone'] == 32 and g['rows_before'] == 32
    assert g['rows_after'] == 48 and g['rows_siblings'] == [48] * 3
    assert g['rows_after'] != g['rows_alone']
    assert g['before_equal'] and g['after_equal'] and g['siblings_equal']
