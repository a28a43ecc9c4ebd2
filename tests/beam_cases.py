"""The inputs on which the beam decoders are compared with their host definitions (tests/test_hip_beam.py, test_hip_lm.py,
test_hip_nbest.py), and the definitions' answers on them, computed once per process.  tests/test_beam_cases_host.py asserts, without
a GPU, that every line here is decided by a margin the device's arithmetic cannot close (the gap condition) and, for the plain
search, that float32 and float64 evaluation of the definition agree; the GPU tests then compare every line and leave none out.

Two generators.  `random_case`: the recipe of the older beam tests.  `planted_line`: a known label string on a noisy background --
long random lines do not meet the gap condition (scores of -300 .. -2000, where one float32 step is 3e-5 .. 1.2e-4, and frame gaps
of 0 .. 9e-5), planted lines keep the scores small at any length."""
import numpy as np

from conformer_ocr_amd.lm import beam_decode_host
from oracle.ctc_ref import beam_decoder as ref_beam
from tests.test_nbest_host import chain_lm

GAP_PLAIN = 1e-4        # tests/test_nbest_host.py GAP
GAP_LM = 2e-5           # tests/test_hip_lm.py GAP
LM_ALPHA, LM_BETA = 0.7, 0.5


def random_case(C, T, N, scale):
    """N lines of T frames and C classes: normal * scale, blank + 1.0; ragged lengths T, T - 3, T // 2, 1, 0 (the first N)."""
    g = np.random.default_rng(C * 7919 + T)
    x = (g.normal(size=(N, T, C)) * scale).astype(np.float32)
    x[:, :, 0] += 1.0
    return x, [T, max(T - 3, 1), max(T // 2, 1), 1, 0][:N]


def planted_line(L, C, gain, seed):
    """(T, C) float32 logits, T = 2 L + 6: standard normal noise with `gain` added along one path -- L random labels, label k on
    frame 3 + 2 k, blank on every other frame.  Returns (logits, labels)."""
    rng = np.random.default_rng(9000 + L + seed)
    T = 2 * L + 6
    x = rng.standard_normal((T, C)).astype(np.float32)
    labels = [1 + int(rng.integers(0, C - 1)) for _ in range(L)]
    path = np.zeros(T, dtype=np.int64)
    path[3 + 2 * np.arange(L)] = labels
    x[np.arange(T), path] += np.float32(gain)
    return x, labels


def masked_case():
    """(12, 60): classes 1, 4, 7, 10 at -inf on every frame of every line; on line 1 also the blank at -inf on every fifth frame; on
    line 2, frame 7 keeps the blank and class 2 alone.  (Seven non-blank classes are finite elsewhere: fewer than K on every frame.)"""
    x, lens = random_case(12, 60, 3, 2.0)
    x[:, :, 1::3] = -np.inf
    x[1, ::5, 0] = -np.inf
    x[2, 7, 3:] = -np.inf
    return x, lens


# ---- the plain beam: name -> (inputs, beams); inputs = ('random', C, T, N, scale) | ('planted', L, C, gain, seed) | ('masked',)
PLAIN = {
    # ctc_beam_walk_kernel<2> (beam <= 16: fold groups of 16, one comparison) and <3> (groups of 8, four), odd beams
    'walk forms': (('random', 11, 24, 5, 2.0), (1, 2, 3, 5, 16, 17, 31, 32)),
    # K = min(beam + 1, C - 1) cut by the class count
    'two classes': (('random', 2, 20, 5, 2.0), (4,)),
    'three classes': (('random', 3, 20, 5, 2.0), (8,)),
    'five classes': (('random', 5, 20, 5, 2.0), (16, 32)),
    # the last class count of the fast path, and the first ones of the exhaustive kernel as production selects it
    '256 classes': (('random', 256, 40, 3, 2.0), (16,)),
    '256 classes, beam 32': (('random', 256, 40, 1, 2.0), (32,)),
    '257 classes': (('random', 257, 24, 2, 2.0), (32,)),
    '300 classes': (('random', 300, 40, 2, 2.0), (16,)),
    # back-pointers: 68 KB of LDS (above the default limit); global memory for beam 32 (T >= 723) and beam 16 (T >= 1366)
    'planted 500': (('planted', 247, 6, 6.0, 0), (32,)),
    'planted 730': (('planted', 362, 6, 6.0, 5), (32,)),
    'planted 1386': (('planted', 690, 6, 6.0, 2), (16,)),
    'masked': (('masked',), (16,)),
}
# the exhaustive kernel selected by hand (COCR_BEAM_REF=1) where production runs the fast path
PLAIN_EXHAUSTIVE = {
    'exhaustive 11': (('random', 11, 40, 5, 2.0), (16,)),
    'exhaustive 33': (('random', 33, 64, 3, 3.5), (32,)),      # (scale 2.0: line 1's closest frame cut is 8.2e-5)
}

# ---- the LM beam: name -> (inputs, beam, classes, order, model seed)
LM = {
    '2048 candidates': (('random', 80, 24, 4, 2.0), 32, 64, 3, 80),
    'beam 17': (('random', 11, 24, 5, 2.0), 17, 8, 3, 11),
    'beam 31': (('random', 11, 24, 5, 2.0), 31, 8, 3, 11),
    'planted 500': (('planted', 247, 6, 6.0, 0), 32, 5, 3, 5),
    'planted 730': (('planted', 362, 6, 6.0, 5), 32, 5, 3, 5),
    'planted 1386': (('planted', 690, 6, 6.0, 2), 16, 5, 3, 5),
    'masked': (('masked',), 16, 8, 3, 12),
}

# ---- n-best: planted lines whose hypotheses lie on both sides of the scorer's seams (S = 2 labels + 1 = 63 | 65, 127 | 129, 255 | 257)
# and of the 255-label limit
NBEST_L = (31, 32, 63, 127, 128, 254, 255)
NBEST_C, NBEST_GAIN, NBEST_BEAM = 6, 4.0, 8

_inputs, _plain, _lm = {}, {}, {}


def inputs(spec):
    """(logits (N, T, C), lens) of an inputs tuple; the same arrays on every call: do not write to them."""
    if spec not in _inputs:
        if spec[0] == 'random':
            _inputs[spec] = random_case(*spec[1:])
        elif spec[0] == 'planted':
            x, _ = planted_line(*spec[1:])
            _inputs[spec] = (x[None], [x.shape[0]])
        else:
            _inputs[spec] = masked_case()
    return _inputs[spec]


def plain_host(spec, beam, dtype=np.float32):
    """Per line (records, (frame gap, final gap)) of oracle/ctc_ref.py::beam_decoder."""
    key = (spec, beam, np.dtype(dtype).name)
    if key not in _plain:
        x, lens = inputs(spec)
        _plain[key] = [ref_beam(x[n, :L].T, beam, return_gap=True, dtype=dtype) for n, L in enumerate(lens)]
    return _plain[key]


def lm_host(name):
    """(model, per line (records, (ctc, lmv), gap)) of lm.beam_decode_host on an LM case."""
    if name not in _lm:
        spec, beam, classes, order, seed = LM[name]
        x, lens = inputs(spec)
        lm = chain_lm(x.shape[2], order, seed)
        _lm[name] = (lm, [beam_decode_host(x[n, :L].T, lm, beam, classes, LM_ALPHA, LM_BETA, return_scores=True, return_gap=True)
                          for n, L in enumerate(lens)])
    return _lm[name]
