"""Child process of tests/test_hip_chain_forms.py: the library reads GPU_MAX_HW_QUEUES once, so every value gets a fresh process.

    python tests/chain_forms_child.py            (GPU_MAX_HW_QUEUES as the parent set it; COCR_TEST_QUEUES_UNSET=1: not set at all)

Prints one JSON line: the rows per workgroup `cocr_get_chain_rows` reports for each model group, and -- with COCR_TEST_GROUP_RUN=1 -- the
comparison of a group's forwards against a lone model's."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import conformer_ocr_amd  # noqa: E402  (sets GPU_MAX_HW_QUEUES=8 when the caller left it unset)

if os.environ.get('COCR_TEST_QUEUES_UNSET'):
    # the library's own default (a caller of the C ABI that never set the variable): taken away again before the library or HIP read it
    os.environ.pop('GPU_MAX_HW_QUEUES', None)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from conformer_ocr_amd import synth  # noqa: E402
from conformer_ocr_amd.engine import HipRecognizer  # noqa: E402

DEV = torch.device('cuda', 0)
HP = synth.hparams('cfg2', num_encoder_layers=1)
STATE = synth.make_state_dict(HP, seed=77, decoder_gain=4.0)


def owner_engine():
    eng = HipRecognizer(HP, DEV, 'bf16')
    eng.load_state(STATE)
    eng.finalize()
    return eng


def group(n):
    """n models on one set of weights: the owner first."""
    engines = [owner_engine()]
    for _ in range(n - 1):
        e = HipRecognizer(HP, DEV, 'bf16')
        e.share_weights(engines[0])
        engines.append(e)
    return engines


def main():
    out = {'queues_env': os.environ.get('GPU_MAX_HW_QUEUES')}
    four, three, lone = group(4), group(3), group(1)
    out['four'] = [e.chain_rows(32, 1200) for e in four]
    out['three'] = [e.chain_rows(32, 1200) for e in three]
    out['lone'] = lone[0].chain_rows(32, 1200)
    out['four_one_line'] = [e.chain_rows(1, 1200) for e in four]
    out['lone_one_line'] = lone[0].chain_rows(1, 1200)
    for e in (four[0], four[2], lone[0]):
        e.set_chain_rows(48)
    out['explicit48'] = [four[0].chain_rows(32, 1200), four[2].chain_rows(32, 1200), lone[0].chain_rows(32, 1200), four[1].chain_rows(32, 1200)]
    for e in (four[0], four[2], lone[0]):
        e.set_chain_rows(0)
    # a model leaves the group: destroyed, or finalized on weights of its own again
    gone = four.pop()
    del gone
    out['four_minus_destroyed'] = [e.chain_rows(32, 1200) for e in four]
    leaver = four.pop()
    leaver.load_state(STATE)
    leaver.finalize()
    out['four_minus_two'] = [e.chain_rows(32, 1200) for e in four]
    out['leaver'] = leaver.chain_rows(32, 1200)

    if os.environ.get('COCR_TEST_GROUP_RUN'):
        # 11 lines x 1200: M = 3300 rows.  A model alone runs them in 32-row blocks (fewer than 50 blocks of 96); a group picks a taller form
        img, lens = synth.make_lines(11, HP.height, 1200, seed=21, widths=[1200, 1170, 64, 900, 1200, 333, 1024, 777, 1199, 500, 1200])
        x = torch.from_numpy(img[:, 0]).to(DEV)
        alone = owner_engine()
        want = alone.forward(x, lens)[0].cpu().numpy()
        first = owner_engine()
        first.set_graph(True)
        rows_before = first.chain_rows(11, 1200)
        before = [first.forward(x, lens)[0].cpu().numpy() for _ in range(3)]           # plain, captured, replayed
        siblings = []
        for _ in range(3):
            e = HipRecognizer(HP, DEV, 'bf16')
            e.share_weights(first)
            e.set_graph(True)
            siblings.append(e)
        rows_after = first.chain_rows(11, 1200)
        after = [first.forward(x, lens)[0].cpu().numpy() for _ in range(3)]            # the captured grid is stale: dropped, captured again
        sib = [[e.forward(x, lens)[0].cpu().numpy() for _ in range(3)][-1] for e in siblings]
        torch.cuda.synchronize()
        out['group_run'] = {
            'rows_alone': alone.chain_rows(11, 1200), 'rows_before': rows_before, 'rows_after': rows_after,
            'rows_siblings': [e.chain_rows(11, 1200) for e in siblings],
            'before_equal': all(np.array_equal(a, want) for a in before),
            'after_equal': all(np.array_equal(a, want) for a in after),
            'siblings_equal': all(np.array_equal(a, want) for a in sib),
            'finite': bool(np.isfinite(want).all()), 'spread': float(want.max() - want.min()),
        }
    print(json.dumps(out))


if __name__ == '__main__':
    main()
