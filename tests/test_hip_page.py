"""GPU: whole-page recognition.  The extraction kernels (cocr_extract_lines) bit for bit against the CPU
restatement tests/page_ref.py; `recognize_pages` against `recognize_crops` on the restatement's strips; real geometry (straight,
rotated and curved lines pasted into a page) read by the metric's model; the `ocr` command; errors."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conformer_ocr_amd import synth
from conformer_ocr_amd.codec import ascii_codec
from conformer_ocr_amd.engine import HipRecognizer
from conformer_ocr_amd.page import Line, cut_quads, line_geometry, recognize_pages
from conformer_ocr_amd.pred import PytorchRecognitionModel
from tests import page_ref, page_synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPS = dict(input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1)


@pytest.fixture(scope='module')
def eng():
    return HipRecognizer(synth.hparams('tiny'), torch.device('cuda', 0), 'fp32')


def _extract(eng, pages, items, fill):
    """items: (page index, baseline, boundary) -> device strips as numpy arrays, and the restatement's."""
    geoms = [(p, line_geometry(f'l{i}', bl, bd)) for i, (p, bl, bd) in enumerate(items)]
    buf, offs, hs, ws = eng.extract_lines(pages, geoms, fill=fill)
    torch.cuda.synchronize()
    flat = buf.cpu().numpy()
    got = [flat[o:o + h * w].reshape(h, w) for o, h, w in zip(offs, hs, ws)]
    want = [page_ref.strip(pages[p], page_ref.geometry(bl, bd), fill) for p, bl, bd in items]
    return got, want


def _ring(cx, cy, rx, ry, n, wobble=0.0, seed=0):
    a = np.linspace(0, 2 * np.pi, n, endpoint=False)
    r = 1.0 + wobble * np.random.default_rng(seed).uniform(-1, 1, n)
    return np.stack([cx + rx * r * np.cos(a), cy + ry * r * np.sin(a)], -1)


@pytest.mark.parametrize('fill', [0, 255])
def test_strips_equal_the_restatement(eng, fill):
    rng = np.random.default_rng(3 + fill)
    gray = rng.integers(0, 256, (300, 420), dtype=np.uint8)
    rgb = rng.integers(0, 256, (260, 380, 3), dtype=np.uint8)
    small = rng.integers(0, 256, (57, 83), dtype=np.uint8)
    pages = [gray, rgb, small]
    items = [
        (0, [[20.3, 100.7], [300.1, 112.4]], [[15, 60], [305, 70], [310, 118], [14, 109]]),                 # inside, 4 vertices
        (0, [[-40.5, 30.2], [200.0, 25.0]], [[-50, -20], [210, -25], [205, 40], [-45, 45]]),                # crosses top and left edges
        (0, [[250.0, 280.0], [460.7, 290.25]], [[245, 250], [470, 255], [468, 330], [240, 320]]),           # bottom and right edges
        (1, [[30.0, 200.0], [120.0, 150.0], [220.0, 170.0], [360.0, 120.0]],
         [[25, 150], [125, 100], [365, 80], [370, 150], [210, 200], [120, 215], [20, 230]]),                # RGB, curved, concave
        (1, [[100.0, 50.0], [100.0, 200.0]], [[90, 40], [130, 45], [60, 210]]),                              # 90 degrees, triangle
        (1, [[300.0, 100.0], [100.0, 101.5]], _ring(200.0, 100.0, 110.0, 25.0, 4096, 0.2, 1)),              # 180 degrees, 4096 vertices
        (2, [[-10.0, 20.0], [95.0, 35.0]], [[-20, 0], [100, 5], [0, 70], [100, 80], [-15, 60]]),            # self-intersecting, all edges
        (0, [[50.0, 150.0], [350.0, 150.0 + 300 * math.tan(math.radians(15))]],
         _ring(200.0, 190.0, 160.0, 50.0, 97, 0.1, 2)),                                                      # 15 degrees, 97 vertices
    ]
    got, want = _extract(eng, pages, items, fill)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (i, g.shape, w.shape)
        assert np.array_equal(g, w), (i, int((g != w).sum()), np.argwhere(g != w)[:5])


def test_axis_aligned_known_answer(eng):
    """Integer horizontal baseline, rectangle boundary: the strip is the page on x_a <= x < x_b, y_a <= y < y_b and `fill` elsewhere."""
    rng = np.random.default_rng(11)
    page = rng.integers(0, 256, (120, 200), dtype=np.uint8)
    xa, xb, ya, yb, by = 30, 150, 40, 90, 80
    for fill in (0, 255):
        bl = [[20.0, by], [170.0, by]]
        got, want = _extract(eng, [page], [(0, bl, [[xa, ya], [xb, ya], [xb, yb], [xa, yb]])], fill)
        g = got[0]
        T = by - ya
        assert g.shape == (T + (yb - by) + 1, 151)
        ys = np.arange(g.shape[0])[:, None] + by - T
        xs = np.arange(g.shape[1])[None, :] + 20
        inside = (xs >= xa) & (xs < xb) & (ys >= ya) & (ys < yb)
        expect = np.where(inside, page[np.clip(ys, 0, 119), np.clip(xs, 0, 199)], fill)
        assert np.array_equal(g, expect)
        assert np.array_equal(g, want[0])


# ---- recognition on a synthetic page --------------------------------------------------------------------------------------------
KINDS = [('line', 0.0), ('line', 7.0), ('arc', 2600.0, 1), ('line', -7.0), ('line', 15.0), ('line', 0.0), ('line', -15.0),
         ('arc', 2500.0, -1), ('line', 0.0), ('line', 3.0)]
# The fixture lines pasted at those placements: per placement the first line (in fixture order) that the CPU oracle reads correctly
# from tests/page_ref.py's strip, unpadded in a 1200-px bucket (the fixture's own batch form), with a top-1 / top-2 logit margin >= 1 on
# every frame.  The fixture model's decoder was fitted on its 32 lines as they are; resampled, padded by 16 or bucketed at 1400 px, many
# of them sit within the bf16 path's noise of a different reading (test note).
PICK = [3, 4, 14, 7, 11, 12, 16, 22, 23, 6]
FIXTURE_FORM = dict(pad=0, edge=1200)


@pytest.fixture(scope='module')
def text_page(text_case):
    tc = text_case('cfg2_text')
    pick = PICK
    lines = [np.rint(tc.lines[i] * 255.0).astype(np.uint8) for i in pick]
    page, placed = page_synth.text_page(lines, KINDS)
    codec = ascii_codec(tc.hp.num_classes)
    truth = [''.join(codec.l2c[(l,)] for l in tc.texts[i]) for i in pick]
    spans = []
    for i in pick:
        _, _, _, sp = synth.make_text_lines(1, tc.hp.height, tc.widths[i], seed=tc.meta['seed'] + 1000 + i, alphabet=tc.meta['alphabet'],
                                            alphabet_seed=tc.meta['seed'])
        spans.append(sp[0])
    page_lines = [Line(f'line{k}', P, B) for k, (_, P, B) in enumerate(placed)]
    return tc, page, placed, page_lines, truth, spans


def _net(tc, dtype):
    net = PytorchRecognitionModel(**tc.hp.as_dict(), **DROPS, codec=ascii_codec(tc.hp.num_classes), compute_dtype=dtype)
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    return net.to('cuda:0').eval()


def _inside(pt, quad):
    s = []
    for k in range(4):
        a, b = quad[k], quad[(k + 1) % 4]
        s.append((b[0] - a[0]) * (pt[1] - a[1]) - (b[1] - a[1]) * (pt[0] - a[0]))
    return all(v >= 0 for v in s) or all(v <= 0 for v in s)


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_real_geometry_is_read(text_page, dtype):
    tc, page, placed, page_lines, truth, spans = text_page
    for ln in page_lines:
        assert line_geometry(ln.id, ln.baseline, ln.boundary).H_s in (96, 97)
    net = _net(tc, dtype)
    res, = recognize_pages(net, [(page, page_lines)], batch_size=4, **FIXTURE_FORM)
    assert [r['id'] for r in res] == [l.id for l in page_lines]
    assert [r['text'] for r in res] == truth
    from conformer_ocr_amd import _lib
    lib = _lib.load()

    def unit(v):
        n = np.linalg.norm(v)
        return v / n if n > 0 else v
    for (pl, _, _), r, sp, ln in zip(placed, res, spans, page_lines):
        g = line_geometry(ln.id, ln.baseline, ln.boundary)
        w_in = int(lib.cocr_preproc_width(g.H_s, g.W_s, 96, 0))
        fw = w_in / int(lib.cocr_out_len(w_in, 4)) * g.W_s / w_in                 # one frame, in strip columns
        assert len(r['cuts']) == len(sp)
        for (ch, quad, conf), (x0, x1) in zip(r['cuts'], sp):
            centre = pl.forward(np.array([(x0 + x1 - 1) / 2.0]), np.array([47.5]))[0]
            q = np.asarray(quad)
            dl, dr = unit(q[1] - q[0]), unit(q[2] - q[3])
            wide = [q[0] - fw * dl, q[1] + fw * dl, q[2] + fw * dr, q[3] - fw * dr]
            assert _inside(centre, wide), (ln.id, ch, centre, quad)


def test_same_records_as_recognize_crops_on_the_restatement(text_page):
    from conformer_ocr_amd.evaluate import make_batches, recognize_crops
    tc, page, placed, page_lines, truth, spans = text_page
    net = _net(tc, 'bf16')
    rgb = np.repeat(page[:, :, None], 3, axis=2)                # RGB pages through the same path
    got, got_rgb = recognize_pages(net, [(page, page_lines), (rgb, page_lines[::-1])], batch_size=4, edge=200)
    strips = [page_ref.strip(page, page_ref.geometry(l.baseline, l.boundary)) for l in page_lines]
    want = recognize_crops(net, strips, batch_size=4, edge=200)
    assert [r['text'] for r in got] == [want[i] for i in range(len(strips))]
    assert [r['text'] for r in got_rgb] == [want[i] for i in range(len(strips))][::-1]
    # the records themselves, batch by batch as recognize_pages forms them (both pages: each strip twice)
    both = strips + strips[::-1]
    from conformer_ocr_amd import _lib
    lib = _lib.load()
    widths = [int(lib.cocr_preproc_width(s.shape[0], s.shape[1], 96, 16)) for s in both]
    recs = {}
    for width, idx in make_batches(widths, 4, 200):
        im, lens = net.transform_lines([both[i] for i in idx], pad=16, bucket_edge=200)
        assert im.shape[3] == width
        for i, r, L in zip(idx, net.predict(im, lens), lens.tolist()):
            recs[i] = (r, L)
    flat = got + got_rgb
    for i, res in enumerate(flat):
        r, L = recs[i]
        ln = page_lines[i] if i < len(strips) else page_lines[::-1][i - len(strips)]
        g = line_geometry(ln.id, ln.baseline, ln.boundary)
        assert res['cuts'] == cut_quads(g, r, L, int(lib.cocr_out_len(L, 4)), 16)


def test_ocr_command(text_page, tmp_path):
    from PIL import Image
    from conformer_ocr_amd.pred import save_safetensors
    tc, page, placed, page_lines, truth, spans = text_page
    Image.fromarray(page).save(tmp_path / 'scan.png')
    pts = lambda a: ' '.join(f'{x:.3f},{y:.3f}' for x, y in a)
    body = ''.join(f'<TextLine id="{l.id}"><Coords points="{pts(l.boundary)}"/><Baseline points="{pts(l.baseline)}"/></TextLine>\n'
                   for l in page_lines)
    (tmp_path / 'scan.xml').write_text('<?xml version="1.0"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2019-07-15">'
                                       f'<Page imageFilename="scan.png"><TextRegion id="r">{body}</TextRegion></Page></PcGts>\n')
    src = PytorchRecognitionModel(**tc.hp.as_dict(), **DROPS, codec=ascii_codec(tc.hp.num_classes))
    src.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    save_safetensors(src, tmp_path / 'model.tar')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = tmp_path / 'out.txt'
    p = subprocess.run([sys.executable, '-m', 'conformer_ocr_amd.ocr', '-m', str(tmp_path / 'model.tar'), '-f', 'page',
                        '-i', str(tmp_path / 'scan.xml'), str(out), '--pad', '0', '--edge', '1200'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert out.read_text(encoding='utf-8').split('\n')[:-1] == truth


def test_errors_are_value_errors(eng, text_case):
    import dataclasses
    tc = text_case('cfg2_text')
    net = _net(tc, 'bf16')
    page = np.zeros((100, 200), dtype=np.uint8)
    box = [[0, 0], [100, 0], [100, 50], [0, 50]]
    with pytest.raises(ValueError, match='strip'):
        recognize_pages(net, [(page, [Line('tall', [[0, 0], [100, 0]], [[0, -3000], [100, -3000], [100, 3000], [0, 3000]])])])
    with pytest.raises(ValueError, match="'bad'"):
        recognize_pages(net, [(page, [Line('bad', [[5, 5], [5, 5]], box)])])
    with pytest.raises(ValueError, match='empty page'):
        recognize_pages(net, [(np.zeros((0, 200), dtype=np.uint8), [Line('a', [[0, 10], [50, 10]], box)])])
    assert recognize_pages(net, [(page, [])]) == [[]]
    # the library refuses out-of-limit descriptors itself (no device fault), naming the line
    g = line_geometry('ok', [[0, 10], [50, 10]], box)
    for bad in (dataclasses.replace(g, H_s=5000, T=10), dataclasses.replace(g, T=g.H_s),
                dataclasses.replace(g, verts=np.zeros((2, 2), dtype=np.int32))):
        with pytest.raises(ValueError, match='line 1'):
            eng.extract_lines([page], [(0, g), (0, bad)])
    with pytest.raises(ValueError, match='page'):
        eng.extract_lines([page], [(1, g)])
    # the engine is still usable
    got, want = _extract(eng, [page + 7], [(0, [[0, 10], [50, 10]], box)], 0)
    assert np.array_equal(got[0], want[0])
