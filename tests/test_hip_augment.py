"""cocr_augment_lines (csrc/augment.hip.h) against tests/augment_ref.py, the numpy restatement of DESIGN.md section 7b: bit for bit."""
import numpy as np
import pytest
import torch

from conformer_ocr_amd import augment as aug
from conformer_ocr_amd import synth
from tests import augment_ref

pytestmark = pytest.mark.gpu

ALONE = {
    'geometry': aug.AugmentConfig(p=1.0, p_geometry=1.0, p_elastic=0.0, p_blur=0.0, p_dropout=0.0),
    'elastic': aug.AugmentConfig(p=1.0, p_geometry=0.0, p_elastic=1.0, p_blur=0.0, p_dropout=0.0),
    'blur': aug.AugmentConfig(p=1.0, p_geometry=0.0, p_elastic=0.0, p_blur=1.0, p_dropout=0.0),
    'dropout': aug.AugmentConfig(p=1.0, p_geometry=0.0, p_elastic=0.0, p_blur=0.0, p_dropout=1.0, dropout_pixel=6554),
    'all': aug.AugmentConfig(p=1.0, p_geometry=1.0, p_elastic=1.0, p_blur=1.0, p_dropout=1.0),
    'default': aug.AugmentConfig(),
}


@pytest.fixture(scope='module')
def eng():
    from conformer_ocr_amd.engine import HipRecognizer
    return HipRecognizer(synth.hparams('tiny'), torch.device('cuda:0'), 'fp32')


def _batch(n, h, w, seed):
    """Text-like lines with ragged seq_lens; the columns beyond each seq_len hold noise (not zeros), so that a read or a write
    there shows up."""
    g = np.random.default_rng(seed)
    image, _, _, _ = synth.make_text_lines(n, h, w, seed=seed)
    x = synth.lines_u8(image)[:, 0].copy()
    sl = g.integers(1, w + 1, n)
    sl[0], sl[-1] = w, max(1, w // 3)
    for i in range(n):
        x[i, :, sl[i]:] = g.integers(0, 256, (h, w - sl[i]), dtype=np.uint8)
    return x, sl.astype(np.int32)


def _run(eng, x, sl, params, grid):
    d = torch.from_numpy(x).cuda()
    out = eng.augment(d, sl, params, grid)
    return out.cpu().numpy()


@pytest.mark.parametrize('stage', sorted(ALONE))
@pytest.mark.parametrize('n,h,w', [(64, 96, 1200), (7, 48, 203), (5, 33, 77), (3, 96, 64)])
def test_device_equals_the_restatement(eng, stage, n, h, w):
    x, sl = _batch(n, h, w, seed=n * 1000 + h + w)
    params, grid = aug.draw(aug.line_keys(11, 3, np.arange(n)), sl, h, w, ALONE[stage])
    got = _run(eng, x, sl, params, grid)
    want = augment_ref.augment_batch(x, sl, params, grid)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, f'{stage}: {bad.shape[0]} bytes differ, first at {bad[:4].tolist()}'
    if stage != 'default':
        assert (params[:, aug.F_FLAGS] != 0).all()
        assert (got != x).any()


def test_every_blur_kind_and_direction_is_exercised(eng):
    """Blur alone over 64 lines draws every kind, every motion length and direction; each equals the restatement (above) and differs
    from the input."""
    n, h, w = 64, 96, 1200
    x, sl = _batch(n, h, w, seed=5)
    params, grid = aug.draw(aug.line_keys(0, 0, np.arange(n)), sl, h, w, ALONE['blur'])
    assert set(params[:, aug.F_BLUR]) == {1, 2, 3}
    mot = params[:, aug.F_BLUR] == 3
    assert set(params[mot, aug.F_MLEN]) == {3, 5, 7} and set(params[mot, aug.F_MDIR]) == {0, 1, 2, 3}
    got = _run(eng, x, sl, params, grid)
    assert np.array_equal(got, augment_ref.augment_batch(x, sl, params, grid))


def test_identity_parameters_reproduce_the_input(eng):
    n, h, w = 9, 96, 300
    x, sl = _batch(n, h, w, seed=2)
    params, grid = aug.draw(aug.line_keys(0, 0, np.arange(n)), sl, h, w, ALONE['all'])
    ident = params.copy()
    ident[:, aug.F_FLAGS] = 0
    assert np.array_equal(_run(eng, x, sl, ident, grid), x)
    # the warp stage on with the identity map and a zero grid: every byte resampled, every byte the same
    ident[:, aug.F_FLAGS] = aug.GEOM | aug.ELASTIC
    ident[:, aug.F_A:aug.F_A + 6] = [aug.FIX, 0, 0, 0, aug.FIX, 0]
    assert np.array_equal(_run(eng, x, sl, ident, np.zeros_like(grid)), x)


def test_columns_beyond_seq_len_are_untouched(eng):
    n, h, w = 16, 96, 517
    x, sl = _batch(n, h, w, seed=4)
    params, grid = aug.draw(aug.line_keys(1, 1, np.arange(n)), sl, h, w, ALONE['all'])
    got = _run(eng, x, sl, params, grid)
    for i in range(n):
        assert np.array_equal(got[i, :, sl[i]:], x[i, :, sl[i]:]), i


def test_same_key_same_bytes_whatever_the_batch(eng):
    """A line's bytes depend on its key only: other lines, its position and a wider batch change nothing."""
    n, h, w = 12, 96, 400
    x, sl = _batch(n, h, w, seed=8)
    keys = aug.line_keys(5, 2, np.arange(100, 100 + n))
    cfg = aug.AugmentConfig(p=1.0, p_geometry=0.5, p_elastic=0.5, p_blur=0.5, p_dropout=0.5)
    full = _run(eng, x, sl, *aug.draw(keys, sl, h, w, cfg))
    sub = [7, 2, 11]
    got = _run(eng, np.ascontiguousarray(x[sub]), sl[sub], *aug.draw(keys[sub], sl[sub], h, w, cfg))
    assert np.array_equal(got, full[sub])
    wide = np.zeros((len(sub), h, w + 200), dtype=np.uint8)
    wide[:, :, :w] = x[sub]
    got = _run(eng, wide, sl[sub], *aug.draw(keys[sub], sl[sub], h, w + 200, cfg))
    for j, i in enumerate(sub):
        assert np.array_equal(got[j, :, :sl[i]], full[i, :, :sl[i]])


def test_bad_tables_raise_before_any_launch(eng):
    n, h, w = 4, 96, 256
    x, sl = _batch(n, h, w, seed=1)
    d = torch.from_numpy(x).cuda()
    params, grid = aug.draw(aug.line_keys(0, 0, np.arange(n)), sl, h, w, ALONE['all'])
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        eng.augment(d, np.array([w + 1, 1, 1, 1]), params, grid)                           # seq_len > W
    with pytest.raises(ValueError):
        eng.augment(d, sl, params, grid[:, :aug.grid_cols(w) - 1])                          # grid too small for W
    for field, value in ((aug.F_SEQ, 3), (aug.F_FLAGS, 16), (aug.F_BLUR, 7), (aug.F_DROP, 70000), (aug.F_A, 1 << 40)):
        bad = params.copy()
        bad[:, aug.F_FLAGS] = 15
        bad[1, field] = value
        with pytest.raises(ValueError):
            eng.augment(d, sl, bad, grid)
    bad = params.copy()
    bad[:, aug.F_FLAGS], bad[:, aug.F_BLUR], bad[0, aug.F_MLEN] = 15, 3, 4
    with pytest.raises(ValueError):
        eng.augment(d, sl, bad, grid)                                                      # motion length 4
    with pytest.raises(ValueError):
        eng.augment(d, sl, params.astype(np.int32), grid)                                   # wrong dtype
    with pytest.raises(ValueError):
        eng.augment(torch.zeros((1, 4097, 8), dtype=torch.uint8, device='cuda:0'), [8], params[:1], grid[:1])   # H over the limit
    # the library's own check (below the Python one): seq_len > W
    import ctypes as C
    from conformer_ocr_amd import _lib
    out = torch.empty_like(d)
    bad_sl = np.array([w + 1, 1, 1, 1], dtype=np.int32)
    rc = eng.lib.cocr_augment_lines(eng._h, C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()), n, h, w,
                                    bad_sl.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()),
                                    aug.grid_cols(w), None)
    assert rc == _lib.EINVAL
    rc = eng.lib.cocr_augment_lines(eng._h, C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()), n, h, w,
                                    sl.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()),
                                    aug.grid_cols(w) - 1, None)
    assert rc == _lib.EINVAL
    # and a good call still runs after all of that
    assert np.array_equal(_run(eng, x, sl, params, grid), augment_ref.augment_batch(x, sl, params, grid))
