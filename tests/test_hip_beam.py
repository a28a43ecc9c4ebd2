"""GPU: CTC prefix beam search (cocr_ctc_beam) against oracle/ctc_ref.py::beam_decoder.  The label sequences and start
frames must be identical; scores are float32 logaddexp chains whose device / numpy libm may differ in the last ulps, so
random cases allow a mismatch only where the oracle's own top-2 final scores are closer than 1e-4 (none observed).  Every kernel form
(walk kernels, fold groups, class counts, back-pointer placements, the exhaustive kernel, masked classes) is compared on the cases of
tests/beam_cases.py, whose decision gaps tests/test_beam_cases_host.py asserts on the CPU."""
import numpy as np
import pytest
import torch

from oracle.ctc_ref import beam_decoder as ref_beam, greedy_decoder as ref_greedy
from tests import beam_cases as bc
from tests.hip_util import fresh_decoder_engine

pytestmark = pytest.mark.gpu


def _engine():
    from conformer_ocr_amd.ctc_decoder import _scratch_engine
    return _scratch_engine(torch.device('cuda', 0))


def _onehot(path, C=6, hi=12.0, lo=-6.0):
    m = np.full((len(path), C), lo, dtype=np.float32)
    for t, c in enumerate(path):
        m[t, c] = hi + 0.1 * t
    return m


def test_beam_equals_greedy_on_peaked_input():
    path = [0, 3, 3, 0, 3, 5, 5, 0, 1, 0]
    m = _onehot(path)
    got = _engine().ctc_beam(torch.from_numpy(m[None]).cuda(), [len(path)], 16)[0]
    want = ref_beam(m.T, 16)
    assert [x[:3] for x in got] == [x[:3] for x in want] == [x[:3] for x in ref_greedy(m.T)]
    np.testing.assert_allclose([x[3] for x in got], [x[3] for x in want], rtol=1e-5)


def test_beam_sums_alignments():
    p = np.array([[0.4, 0.35, 0.25], [0.4, 0.35, 0.25]], dtype=np.float32)
    got = _engine().ctc_beam(torch.from_numpy(np.log(p)[None]).cuda(), [2], 16)[0]
    assert [x[0] for x in got] == [1]          # greedy would output nothing: blank is the per-frame argmax


@pytest.mark.parametrize('C,T,beam', [(5, 12, 4), (11, 40, 16), (32, 60, 16), (128, 48, 16), (93, 33, 8)])
def test_beam_random_matches_oracle(C, T, beam):
    g = np.random.default_rng(C * 1000 + T)
    N = 4
    logits = (g.normal(size=(N, T, C)) * 2.5).astype(np.float32)
    logits[:, :, 0] += 1.5
    lens = [T, T - 3, max(1, T // 2), 1]
    got = _engine().ctc_beam(torch.from_numpy(logits).cuda(), lens, beam)
    for n in range(N):
        want = ref_beam(logits[n, :lens[n]].T, beam)
        assert [x[:2] for x in got[n]] == [x[:2] for x in want], (n, got[n], want)
        assert [x[2] for x in got[n]] == [x[2] for x in want]
        np.testing.assert_allclose([x[3] for x in got[n]], [x[3] for x in want], rtol=1e-4)


def test_beam_zero_length_and_model_attribute(case):
    got = _engine().ctc_beam(torch.zeros((2, 5, 7)).cuda(), [0, 5], 16)
    assert got[0] == []
    # the host class routes a BeamDecoder attribute to the device kernel
    from conformer_ocr_amd.codec import ascii_codec
    from conformer_ocr_amd.ctc_decoder import BeamDecoder
    from conformer_ocr_amd.pred import PytorchRecognitionModel
    hp, state, image, lens, g = case('tiny')
    net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1,
                                  conv_dropout_p=0.1, codec=ascii_codec(hp.num_classes), ctc_decoder=BeamDecoder(16), compute_dtype='fp32')
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net = net.to('cuda:0')
    recs = net.predict_labels(torch.from_numpy(image).cuda(), torch.from_numpy(lens))
    for n in range(image.shape[0]):
        want = ref_beam(g['logits'][n, :int(g['out_lens'][n])].T, 16)
        assert [x[0] for x in recs[n]] == [x[0] for x in want]


@pytest.mark.parametrize('C,T,beam,scale', [(128, 300, 16, 2.5), (128, 300, 16, 0.3), (200, 120, 32, 1.5), (17, 90, 16, 1.0), (3, 50, 8, 1.0),
                                              (7, 500, 32, 1.0), (40, 1500, 16, 2.0), (256, 40, 16, 2.0), (2, 30, 4, 1.0)])
def test_beam_pruned_equals_exhaustive(C, T, beam, scale, monkeypatch):
    """cocr_ctc_beam ranks a static pruned candidate set per frame (ctc_beam_rank_kernel + ctc_beam_walk_kernel); COCR_BEAM_REF=1 selects
    the kernel that ranks all beam x C of them.  (7, 500, 32): back-pointers in more than 64 KB of LDS; (40, 1500, 16): in global memory;
    256 and 2 classes: the ends of the fast path's range.  Every output field must agree exactly (same arithmetic, same tie rules), on peaked and on
    nearly flat logits (many near-ties), full-length and ragged lines."""
    g = np.random.default_rng(C * 7919 + T)
    N = 6
    logits = (g.normal(size=(N, T, C)) * scale).astype(np.float32)
    logits[:, :, 0] += 1.0
    logits[1, :, 1:] = np.round(logits[1, :, 1:] * 2) / 2          # exact ties between classes
    lens = [T, T - 1, T // 2, 1, T, 7]
    x = torch.from_numpy(logits).cuda()
    fast = fresh_decoder_engine().ctc_beam(x, lens, beam)
    monkeypatch.setenv('COCR_BEAM_REF', '1')
    ref = fresh_decoder_engine().ctc_beam(x, lens, beam)
    assert fast == ref


def test_metric_model_forward_then_beam16_against_the_oracle(text_case):
    """BASELINE configs[4] composed: the metric's model (cfg2_text: D=256, 12 blocks) on 96x1200 lines -> HIP logits (T = 300,
    128 classes) -> cocr_ctc_beam(beam 16), against oracle/ctc_ref.py::beam_decoder run on the SAME logits: labels, start and end
    frames exact, scores within 1e-4 relative.  fp32 logits of lines 0-3 (the latency-bound small batch) and bf16 logits of all 32
    lines; and on these peaked lines the beam's label string is the reference's greedy string.  (Semantics of the beam search are
    the build's own restatement of kraken's algorithm: kraken is absent, the reference never calls it -- parity unpinned.)"""
    from tests.hip_util import make_engine
    tc = text_case('cfg2_text')
    image, lens, idx = tc.batch(0)
    for dtype, n in (('fp32', 4), ('bf16', tc.n)):
        eng = make_engine(tc.hp, tc.state, dtype)
        x = torch.from_numpy(image[:n, 0]).cuda()
        logits, out_lens = eng.forward(x, lens[:n])
        assert logits.shape == (n, 300, 128)
        got = eng.ctc_beam(logits, out_lens, 16)
        host = logits.cpu().numpy()
        for k in range(n):
            want = ref_beam(host[k, :int(out_lens[k])].T, 16)
            assert [r[:3] for r in got[k]] == [r[:3] for r in want], (dtype, k)
            np.testing.assert_allclose([r[3] for r in got[k]], [r[3] for r in want], rtol=1e-4)
            assert [r[0] for r in got[k]] == tc.ref_strings[idx[k]], (dtype, k)


# ---- every kernel form against the oracle (tests/beam_cases.py; tests/test_beam_cases_host.py asserts that each line is decided by
# ---- at least 1e-4 and that float32 and float64 evaluation of the oracle agree: no line is left out here)
def _against_the_oracle(eng, spec, beam):
    x, lens = bc.inputs(spec)
    got = eng.ctc_beam(torch.from_numpy(x).cuda(), lens, beam)
    worst = 0.0
    for n, (want, _) in enumerate(bc.plain_host(spec, beam)):
        assert [r[:3] for r in got[n]] == [r[:3] for r in want], (spec, beam, n)
        g, w = np.asarray([r[3] for r in got[n]]), np.asarray([r[3] for r in want])
        if len(w):
            worst = max(worst, float(np.max(np.abs(g - w) / w)))
        np.testing.assert_allclose(g, w, rtol=1e-4)
    print(f'{spec}, beam {beam}: {sum(len(w) for w, _ in bc.plain_host(spec, beam))} records, worst relative conf difference {worst:.3g}')


@pytest.mark.parametrize('name,beam', [(name, beam) for name, (_, beams) in bc.PLAIN.items() for beam in beams])
def test_every_form_matches_the_oracle(name, beam):
    """Labels, starts and ends exact, conf to 1e-4, on every line.  Which case selects which form: tests/beam_cases.py PLAIN."""
    _against_the_oracle(_engine(), bc.PLAIN[name][0], beam)


@pytest.mark.parametrize('name', list(bc.PLAIN_EXHAUSTIVE))
def test_exhaustive_kernel_matches_the_oracle(name, monkeypatch):
    """ctc_beam_kernel, selected by COCR_BEAM_REF=1 where production runs the fast path -- it is otherwise only the other side of
    test_beam_pruned_equals_exhaustive, and shares lse2, the hash, the fold rule and the post-pass with the fast path."""
    monkeypatch.setenv('COCR_BEAM_REF', '1')
    spec, (beam,) = bc.PLAIN_EXHAUSTIVE[name]
    _against_the_oracle(fresh_decoder_engine(), spec, beam)
