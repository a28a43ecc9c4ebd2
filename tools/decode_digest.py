#!/usr/bin/env python3
"""Digests of everything behind the forward -- the CTC criterion, forced alignment, keyword and pattern spotting, the beam searches, the
greedy decoder -- for comparing two builds of the library bit for bit:   python tools/decode_digest.py [--out FILE]
(the library is the tree's, or the one COCR_LIB_PATH names).  None of these kernels has floating-point atomics, so two builds that do
the same arithmetic in the same order print the same JSON.  The sibling of tools/train_digest.py.

The inputs are the seeded ones of the GPU tests, taken from the test modules themselves, and between them they reach every
instantiation of the kernels:
  loss, align   the batches of tests/test_hip_align.py `_random_batches()` (SJ 1, 2, 4, 8) and its two planted 5150-frame batches (the
                workspace form of the back-pointer table at SJ 8 and SJ 1): nll and gradient; records and scores
  spot          the five grid cases of tests/test_hip_search.py (SJ 1, 2, 8, the workspace form, lines without frames)
  spot_pattern  the chain cases (SJ 1, 2, 4) and the grid cases of tests/test_hip_pattern.py (in-degree 10 across a register seam, K 1
                and 3): cocr_ctc_spot_pattern's raw outputs
  beam          the nine shapes of tests/test_hip_beam.py `test_beam_pruned_equals_exhaustive`, and again with COCR_BEAM_REF=1
  beam_lm       the seven shapes of tests/test_hip_lm.py `test_without_the_model_every_field_equals_the_plain_beam` with alpha = beta
                = 0, and the six of `test_equals_the_definition_with_a_real_model` with their models
  greedy        the logits of the beam shapes
  post/         the beam searches' post-passes: plain and LM beam on the planted 500-, 730- and 1386-frame lines of tests/beam_cases.py
                (back-pointers in the raised LDS limit and in global memory); the raw buffers of the truncated calls of
                tests/test_hip_truncation.py (every decoder, every back-pointer placement); n-best on the definition cases of
                tests/test_hip_nbest.py with and without a model, its workspace-stack case, a planted line on each side of a scorer seam,
                and the exhaustive kernel's trail
A value is the sha256 of the outputs' bit patterns.  Each environment leg runs in a process of its own (the switch is read when the
engine is made); this process only starts them and does not open the GPU."""
import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {'default': {}, 'beam_ref': {'COCR_BEAM_REF': '1'}}


def _feed(h, v):
    """Nested lists / tuples of ints, floats, None, arrays and tensors, bit for bit."""
    import numpy as np
    import torch
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    if isinstance(v, np.ndarray):
        h.update(str((v.dtype.str, v.shape)).encode() + np.ascontiguousarray(v).tobytes())
    elif isinstance(v, (list, tuple)):
        h.update(b'[%d' % len(v))
        for e in v:
            _feed(h, e)
    elif isinstance(v, (float, np.floating)):
        h.update(b'f' + struct.pack('<d', float(v)))
    elif v is None:
        h.update(b'n')
    else:
        h.update(b'i' + struct.pack('<q', int(v)))


def sha(*values):
    h = hashlib.sha256()
    _feed(h, values)
    return h.hexdigest()


def _params(test):
    """The argument tuples of a parametrised test."""
    return [tuple(p) for m in test.pytestmark if m.name == 'parametrize' for p in m.args[1]]


def post_pass_legs(leg, eng, dev):
    """The `post/` keys: what the beam searches' post-passes write (the back-pointer walks, the ends / confidences pass, n-best's
    records), on the inputs of tests/beam_cases.py, tests/test_hip_truncation.py and tests/test_hip_nbest.py."""
    import ctypes as C
    from tests import beam_cases as bc, test_hip_nbest as TN, test_hip_truncation as TT
    from tests.test_nbest_host import CASES, case_inputs, chain_lm
    assert leg in ('default', 'beam_ref')                             # (the keys below carry no leg name: a further leg needs one)
    out = {}
    raw = lambda d: sha([d[k] for k in sorted(d)])

    def cut(fn, spec, extra=()):                                       # a 1-best call truncated at max_per_line 3: the raw output buffers
        x, lens = TT._inputs(spec)
        return raw(TT._call(eng, fn, dev(x), lens, TT.CUT, extra))

    def nbest(x, lens, beam, n, **kw):
        rc, got = TN._raw(eng, dev(x), lens, beam, n, **kw)
        assert rc == 0
        return raw(got)
    nbest_lm = dict(lm=chain_lm(11, 3, seed=5), classes=5, alpha=bc.LM_ALPHA, beta=bc.LM_BETA)
    if leg == 'beam_ref':                                              # ctc_beam_kernel where production runs the fast path
        out['post/beam_ref/cut/beam'] = cut(eng.lib.cocr_ctc_beam, TT.SHORT, (16,))
        out['post/beam_ref/nbest/trail'] = nbest(*bc.inputs(TT.SHORT), 16, 8)
        out['post/beam_ref/nbest/cut'] = nbest(*bc.inputs(TT.SHORT), 16, 8, mpl=TT.CUT)
        return out
    # back-pointers in 68 KB of LDS (the raised limit), and in global memory for beam 32 and for beam 16
    for name in ('planted 500', 'planted 730', 'planted 1386'):
        spec, beams = bc.PLAIN[name]
        x, lens = bc.inputs(spec)
        out[f'post/beam/{name}'] = sha(eng.ctc_beam(dev(x), lens, beams[0]))
        spec, beam, classes, order, seed = bc.LM[name]
        x, lens = bc.inputs(spec)
        got, score = eng.ctc_beam_lm(dev(x), lens, chain_lm(x.shape[2], order, seed), beam, classes, bc.LM_ALPHA, bc.LM_BETA, return_scores=True)
        out[f'post/beam_lm/{name}'] = {'records': sha(got), 'score': sha(score)}
    out['post/cut/greedy'] = cut(eng.lib.cocr_ctc_greedy, TT.SHORT)
    out['post/cut/beam/lds'] = cut(eng.lib.cocr_ctc_beam, TT.SHORT, (16,))
    out['post/cut/beam/global'] = cut(eng.lib.cocr_ctc_beam, TT.LONG, (32,))
    for form, spec, beam in (('lds', TT.SHORT, 16), ('global', TT.LONG, 32)):
        dlm = chain_lm(TT._inputs(spec)[0].shape[2], 3, seed=5).to_device(eng)
        out[f'post/cut/beam_lm/{form}'] = cut(lambda h, *a: eng.lib.cocr_ctc_beam_lm(h, dlm.handle, *a), spec,
                                              (beam, 5, C.c_float(bc.LM_ALPHA), C.c_float(bc.LM_BETA), None))
    out['post/cut/nbest/plain'] = nbest(*bc.inputs(TT.SHORT), 16, 8, mpl=TT.CUT)
    out['post/cut/nbest/lm'] = nbest(*bc.inputs(TT.SHORT), 16, 8, mpl=TT.CUT, **nbest_lm)
    for Cn, T, beam, n in CASES:                                       # the definition cases
        out[f'post/nbest/plain/{(Cn, T, beam, n)}'] = nbest(*case_inputs(Cn, T), beam, n)
    for Cn, T, beam, n in _params(TN.test_against_the_definition_with_a_language_model):
        out[f'post/nbest/lm/{(Cn, T, beam, n)}'] = nbest(*case_inputs(Cn, T), beam, n, lm=chain_lm(Cn, 3, seed=Cn), classes=6, alpha=0.7, beta=0.3)
    x, lens = TN._planted_batch((282, 200), gain=6.0)                  # the chains' stacks in the workspace, and in LDS
    out['post/nbest/workspace stacks'] = {'nbest 32': nbest(x, lens, 32, 32), 'nbest 4': nbest(x, lens, 32, 4)}
    for L in (31, 32, 127, 128):                                       # one planted line on each side of a scorer seam
        out[f'post/nbest/seam/{L}'] = nbest(*TN._planted_batch((L,)), bc.NBEST_BEAM, bc.NBEST_BEAM)
    out['post/nbest/exhaustive trail, 300 classes'] = nbest(*TN._planted_batch((63,), wide=300), bc.NBEST_BEAM, bc.NBEST_BEAM)
    return out


def run_leg(leg):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from conformer_ocr_amd.ctc_decoder import _scratch_engine
    from tests import test_hip_align as TA, test_hip_beam as TB, test_hip_lm as TL, test_hip_pattern as TP, test_hip_search as TS
    from conformer_ocr_amd import pattern as PT
    eng = _scratch_engine(torch.device('cuda', 0))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    out = {}
    beam_cases = []
    for C, T, beam, scale in _params(TB.test_beam_pruned_equals_exhaustive):      # the test's own recipe
        g = np.random.default_rng(C * 7919 + T)
        logits = (g.normal(size=(6, T, C)) * scale).astype(np.float32)
        logits[:, :, 0] += 1.0
        logits[1, :, 1:] = np.round(logits[1, :, 1:] * 2) / 2
        beam_cases.append(((C, T, beam, scale), dev(logits), [T, T - 1, T // 2, 1, T, 7], beam))
    for key, x, lens, beam in beam_cases:
        out[f'{leg}/beam/{key}'] = sha(eng.ctc_beam(x, lens, beam))
    out.update(post_pass_legs(leg, eng, dev))
    if leg != 'default':
        return out
    for key, x, lens, beam in beam_cases:
        out[f'greedy/{key}'] = sha(eng.ctc_greedy(x, lens))
    batches = list(TA._random_batches())
    for N, T, C, l_lo, l_hi, seed, gain in _params(TA.test_planted_alignments):
        if T > 5000:
            logits, labels, _ = TA._planted(N, T, C, l_lo, l_hi, seed, gain)
            batches.append((f'planted{(N, T, C, l_lo, l_hi)}', logits, np.concatenate(labels), [T] * N, [len(l) for l in labels]))
    for name, probits, targets, out_lens, label_lens in batches:
        x = dev(probits)
        nll, grad = eng.ctc_loss(x, out_lens, targets, label_lens)
        out[f'loss/{name}'] = {'nll': sha(nll), 'grad': sha(grad), 'nll_only': sha(eng.ctc_loss(x, out_lens, targets, label_lens, with_grad=False)[0])}
        out[f'align/{name}'] = sha(eng.ctc_align(x, out_lens, targets, label_lens))
    for N, T, C, lens_q, K, out_lens, width in _params(TS.test_grid_logits_give_the_definition_exactly):
        logits, queries = TS._grid_case(N, T, C, lens_q, 100 + T, out_lens, width)
        h = eng.ctc_spot_async(dev(logits), out_lens, queries, K)
        records = eng.collect_spot(h)
        Q = len(queries)
        raw = [h[1][0].numpy()[:, :N * Q * K], h[1][1].numpy()[:N * Q * K], h[1][2].numpy()[:N * Q]]      # entries past the count too
        out[f'spot/{(N, T, C, K)}'] = {'records': sha(records), 'raw': sha(raw)}
    raw_pattern = lambda x, lens, graphs, K: sha(list(eng.collect_spot_pattern(eng.ctc_spot_pattern_async(dev(x), lens, graphs, K), raw=True)))
    for N, T, C, lens_q, K, out_lens, width in _params(TP.test_literal_chains_equal_the_string_kernel):
        logits, queries = TS._grid_case(N, T, C, lens_q, 100 + T, out_lens, width)
        out[f'spot_pattern/chains/{(N, T, C, K)}'] = raw_pattern(logits, out_lens, [PT.chain_graph(q) for q in queries], K)
    for N, T, C, out_lens, width in TP.GRID_SHAPES:
        logits, graphs = TP._pattern_case(N, T, C, out_lens, 300 + T, width)
        for K in (1, 3):
            out[f'spot_pattern/grid/{(N, T, C, K)}'] = raw_pattern(logits, out_lens, graphs, K)
    for C, T, beam in _params(TL.test_without_the_model_every_field_equals_the_plain_beam):
        lm = TL._chain_lm(C, 3, seed=C, n=20)
        got, score = eng.ctc_beam_lm(dev(TL._logits(C, T, 5)), [T, T - 3, T // 2, 1, 0], lm, beam, min(C - 1, 64), 0.0, 0.0, return_scores=True)
        out[f'beam_lm/off/{(C, T, beam)}'] = {'records': sha(got), 'score': sha(score)}
    for C, T, beam, classes, order in [(5, 12, 4, 4, 2), (11, 40, 16, 8, 3), (32, 60, 16, 8, 5), (128, 48, 16, 8, 4), (93, 33, 8, 5, 8), (300, 20, 8, 8, 3)]:
        lm = TL._chain_lm(C, order, seed=C * 31 + order)
        got, score = eng.ctc_beam_lm(dev(TL._logits(C, T, 4)), [T, T - 3, max(1, T // 2), 1], lm, beam, classes, 0.7, 0.5, return_scores=True)
        out[f'beam_lm/model/{(C, T, beam, classes, order)}'] = {'records': sha(got), 'score': sha(score)}
    # text-to-page alignment: the planted pages of its test (one, two and eight registers per lane), every output of the call
    from tests import test_hip_align_page as TG
    for P, K, T, C, L, seed in _params(TG.test_planted_pages):
        rng = np.random.default_rng(seed)
        pages = [TG._planted_page(K, T, C, L + p, rng) for p in range(P)]
        h = eng.ctc_align_page_async(dev(np.concatenate([pg[0] for pg in pages])), [T] * (P * K), [list(range(p * K, (p + 1) * K)) for p in range(P)],
                                     [pg[2] for pg in pages], [pg[3] for pg in pages])
        records = eng.collect_align_page(h)
        total = sum(len(pg[2]) for pg in pages)
        ints, conf, score, counts, line_score = h[1]
        raw = [ints.numpy()[:, :total], conf.numpy()[:total], score.numpy()[:P], counts.numpy()[:P], line_score.numpy()[:P * K]]
        out[f'align_page/{(P, K, T, C, L)}'] = {'records': sha([(r, s, None if l is None else l.tolist()) for r, s, l in records]), 'raw': sha(raw)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=sorted(LEGS))
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(run_leg(args.leg)))
        return 0
    out = {}
    for leg, env in LEGS.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', leg], env={**os.environ, **env}, stdout=subprocess.PIPE, text=True, timeout=300)
        if r.returncode != 0:
            print(f'leg {leg} ended with status {r.returncode}', file=sys.stderr)
            return r.returncode or 1
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    # the digests older runs have, sorted as they always were, then those of text-to-page alignment, then those of the beam searches'
    # post-passes: the head of the output compares
    text = ''
    for prefix in ('post/', 'align_page/'):
        new = {k: out.pop(k) for k in sorted(out) if k.startswith(prefix)}
        if new:
            text = ',\n' + json.dumps(new, indent=1, sort_keys=True)[2:-2] + text
    text = json.dumps(out, indent=1, sort_keys=True)[:-2] + text + '\n}'
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text + '\n')
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
