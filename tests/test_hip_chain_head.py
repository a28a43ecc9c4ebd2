"""GPU: chain A (out-proj + residual + conv-module LayerNorm -> pointwise conv 1 + GLU) as the HEAD of chain B (rowchain.hip.h: the
workgroup computes it for its own rows and one 16-row tile on either side, the GLU values go straight into the depthwise window) against
the two launches it replaces (COCR_NO_A_FUSE=1).  Every row is computed with the same arithmetic in the same order whichever workgroup
computes it, so every comparison here is bit for bit.  The switch is read when a model is created: every leg makes its own engine."""
import numpy as np
import pytest
import torch

from conformer_ocr_amd import synth
from tests.hip_util import make_engine

pytestmark = pytest.mark.gpu

TAPS = ('mhsa', 'glu', 'dw', 'conv')
_cache = {}


def _model(config='cfg2', **kw):
    key = (config, tuple(sorted(kw.items())))
    if key not in _cache:
        hp = synth.hparams(config, num_encoder_layers=2, **kw)
        _cache[key] = (hp, synth.make_state_dict(hp, seed=31, decoder_gain=1.0, style='text'))
    return _cache[key]


def _engines(monkeypatch, hp, state):
    """(fused, two launches)"""
    monkeypatch.delenv('COCR_NO_A_FUSE', raising=False)
    fused = make_engine(hp, state, 'bf16')
    monkeypatch.setenv('COCR_NO_A_FUSE', '1')
    split = make_engine(hp, state, 'bf16')
    monkeypatch.delenv('COCR_NO_A_FUSE')
    return fused, split


def _ragged(n, w, hp, seed=77):
    widths = [max(40, w - 37 * i) for i in range(n)]
    image, lens = synth.make_lines(n, hp.height, w, seed=seed, widths=widths)
    return torch.from_numpy(image[:, 0]).cuda(), lens


def _forward(eng, x, lens, debug=False):
    eng.set_debug(debug)
    lg, _ = eng.forward(x, lens)
    torch.cuda.synchronize()
    out = {'logits': lg.cpu().numpy().copy()}
    if debug:
        for l in range(2):
            for nm in TAPS:
                out[f'l{l}.{nm}'] = eng.tap(f'l{l}.{nm}').copy()
    eng.set_debug(False)
    return out


@pytest.mark.parametrize('shape', ['one_short_line', 'ragged_3x232', 'lines_on_block_boundaries', 'ragged_17x1200'])
def test_head_equals_two_launches_bit_for_bit(shape, monkeypatch):
    """The smallest batches at which the halo can go wrong: a batch shorter than one halo tile (1 line of 10 frames); line ends inside a
    tile and several lines inside one row block (58, 49, 40 frames); line boundaries exactly on row-block boundaries (4 lines of a
    multiple of 64 frames); 5100 rows = a ragged last block at 64 rows and many row blocks per XCD at 48.  Logits of the production
    kernels, then logits and the taps of both blocks from the TAPS instantiations, at 64, 48 and 32 rows per workgroup."""
    hp, state = _model()
    fused, split = _engines(monkeypatch, hp, state)
    if shape == 'one_short_line':
        image, lens = synth.make_lines(1, hp.height, 40, seed=77, widths=[40])
        x = torch.from_numpy(image[:, 0]).cuda()
        assert fused.out_len(40) == 10
    elif shape == 'ragged_3x232':
        x, lens = _ragged(3, 232, hp)
    elif shape == 'lines_on_block_boundaries':
        w = next(w for w in range(200, 600) if fused.out_len(w) % 64 == 0)
        image, lens = synth.make_lines(4, hp.height, w, seed=78, widths=[w] * 4)
        x = torch.from_numpy(image[:, 0]).cuda()
    else:
        x, lens = _ragged(17, 1200, hp)
    for rows in (64, 48, 32):
        fused.set_chain_rows(rows)
        split.set_chain_rows(rows)
        for debug in (False, True):
            a, b = _forward(fused, x, lens, debug), _forward(split, x, lens, debug)
            assert np.isfinite(a['logits']).all()
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f'{shape}, {rows} rows, debug={debug}: {k}')


def test_all_row_forms_equal_with_the_head():
    """The automatic form, 96 rows (two launches: 8 row tiles do not fit the head), 64, 48, 32 (fused): one set of logits."""
    hp = synth.hparams('cfg2', num_encoder_layers=2)
    state = synth.make_state_dict(hp, seed=3, decoder_gain=1.0, style='text')
    image, lens, _, _ = synth.make_text_lines(17, hp.height, 1200, seed=5)
    x = torch.from_numpy(image[:, 0]).cuda()
    eng = make_engine(hp, state, 'bf16')
    out = {}
    for rows in (0, 96, 64, 48, 32):
        eng.set_chain_rows(rows)
        out[rows] = _forward(eng, x, lens)['logits']
    for rows in (96, 64, 48, 32):
        np.testing.assert_array_equal(out[0], out[rows], err_msg=f'{rows} rows')


@pytest.mark.parametrize('model', ['d512', 'conv_kernel_15', 'zero_padded_default'])
def test_forms_without_the_head_and_the_padded_model(model, monkeypatch):
    """encoder_dim 512 and a conv kernel other than 31 keep their two launches whatever the switch says; the reference's default model
    (144 wide, zero-padded to 256: the head's out-proj keeps all 8 k-steps, its pointwise conv skips 3) runs fused."""
    if model == 'd512':
        (hp, state), n, w = _model('cfg4'), 3, 232
    elif model == 'conv_kernel_15':
        (hp, state), n, w = _model('cfg2', conv_kernel_size=15), 3, 232
    else:
        (hp, state), n, w = _model('cfg1'), 9, 500
    fused, split = _engines(monkeypatch, hp, state)
    x, lens = _ragged(n, w, hp)
    for rows in ((0, 64, 32) if model == 'zero_padded_default' else (0,)):
        fused.set_chain_rows(rows)
        split.set_chain_rows(rows)
        a, b = _forward(fused, x, lens), _forward(split, x, lens)
        assert np.isfinite(a['logits']).all()
        np.testing.assert_array_equal(a['logits'], b['logits'], err_msg=f'{model}, {rows} rows')


def test_head_under_graph_replay():
    """Plain, captured, replayed: the stream's two buffers alternate by block, the same way in every forward."""
    hp, state = _model()
    eng = make_engine(hp, state, 'bf16')
    eng.set_chain_rows(64)
    x, lens = _ragged(3, 232, hp)
    plain = _forward(eng, x, lens)['logits']
    eng.set_graph(True)
    for k in range(3):
        lg, _ = eng.forward(x, lens)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(plain, lg.cpu().numpy(), err_msg=f'forward {k} with graphs on')
