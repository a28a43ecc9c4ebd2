"""Host side of whole-page recognition (conformer_ocr_amd/page.py), no GPU involved: the per-line geometry
tables against the CPU restatement (tests/page_ref.py) bit for bit, the limits, the cut mapping, the PAGE and ALTO readers."""
import math
import warnings

import numpy as np
import pytest

from conformer_ocr_amd.page import cut_quads, line_geometry, read_alto, read_page_xml
from tests import page_ref


def _rot(pts, deg, c=(0.0, 0.0)):
    a = math.radians(deg)
    R = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    return (np.asarray(pts, dtype=np.float64) - c) @ R.T + c


def _box(x0, x1, y0, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


def _arc(cx, cy, R, a0, a1, n):
    a = np.linspace(a0, a1, n)
    return np.stack([cx + R * np.sin(a), cy - R * np.cos(a)], -1)


def _cases():
    base = np.array([[100.0, 200.0], [700.0, 200.0]])
    box = _box(95, 705, 160, 210)
    out = {'straight': (base, box)}
    for deg in (7, 15, 90, 180):
        out[f'rot{deg}'] = (_rot(base, deg, (400, 200)), _rot(box, deg, (400, 200)) + 0.3)
    arc = _arc(1000.0, 3000.0, 2600.0, -0.2, 0.2, 25)
    top = _arc(1000.0, 3000.0, 2645.0, -0.21, 0.21, 30)
    bot = _arc(1000.0, 3000.0, 2592.0, 0.21, -0.21, 30)
    out['arc'] = (arc, np.concatenate([top, bot]))
    out['multi'] = (np.array([[10.0, 50.0], [60.5, 58.25], [130.0, 49.0], [131.0, 49.0], [200.0, 70.0]]),
                    np.array([[5, 20], [205, 35], [210, 80], [5, 70]], dtype=np.float64))
    out['duplicates'] = (np.array([[10.0, 50.0], [10.0, 50.0], [60.0, 55.0], [60.0, 55.0], [60.0, 55.0], [120.0, 50.0]]),
                         _box(5, 125, 20, 60))
    out['concave'] = (np.array([[0.0, 100.0], [300.0, 100.0]]),
                      np.array([[0, 60], [100, 60], [150, 90], [200, 60], [300, 60], [300, 110], [150, 80], [0, 110]], dtype=np.float64))
    out['self_intersecting'] = (np.array([[0.0, 100.0], [300.0, 100.0]]),
                                np.array([[0, 60], [300, 110], [300, 60], [0, 110]], dtype=np.float64))
    out['above_only'] = (np.array([[0.0, 100.0], [200.0, 100.0]]), _box(0, 200, 40, 90))
    out['below_only'] = (np.array([[0.0, 100.0], [200.0, 100.0]]), _box(0, 200, 105, 140))
    out['doubling_back'] = (np.array([[0.0, 100.0], [100.0, 100.0], [40.0, 100.0]]), _box(0, 100, 80, 110))
    out['fractional'] = (np.array([[10.37, 20.61], [75.25, 31.9], [160.125, 27.0003]]),
                         np.array([[8.5, 0.49], [161.5, 4.5], [163.2, 40.51], [7.7, 44.5]]))
    return out


@pytest.mark.parametrize('name', sorted(_cases()))
def test_geometry_tables_equal_the_restatement(name):
    bl, bd = _cases()[name]
    g = line_geometry(name, bl, bd)
    r = page_ref.geometry(bl, bd)
    assert (g.T, g.Bt, g.H_s, g.W_s) == (r['T'], r['Bt'], r['H_s'], r['W_s'])
    assert g.top == r['top'] and g.bottom == r['bottom']
    assert np.array_equal(g.points, r['points'])
    assert np.array_equal(g.verts.astype(np.int64), r['verts'])
    assert g.cols.dtype == np.int64 and g.cols.shape == (g.W_s, 4)
    assert np.array_equal(g.cols, r['cols']), np.argwhere(g.cols != r['cols'])[:5]


def test_straight_line_geometry_by_hand():
    g = line_geometry('a', [[10, 50], [110, 50]], _box(5, 120, 20, 53))
    assert (g.T, g.Bt, g.H_s, g.W_s) == (30, 3, 34, 101)
    assert g.cols[0].tolist() == [10 * 65536, 50 * 65536, 0, 65536]
    assert g.cols[100].tolist() == [110 * 65536, 50 * 65536, 0, 65536]
    # 90 degrees: the baseline runs down the page, the normal points to -x
    g = line_geometry('b', [[50, 10], [50, 30]], _box(40, 60, 10, 30))
    assert g.cols[5].tolist() == [50 * 65536, 15 * 65536, -65536, 0]
    assert (g.T, g.Bt) == (10, 10)


def test_duplicate_points_are_dropped():
    g = line_geometry('d', [[0, 0], [0, 0], [10, 0], [10, 0], [20, 0]], _box(0, 20, -5, 5))
    assert g.points.tolist() == [[0, 0], [10, 0], [20, 0]]


@pytest.mark.parametrize('bl', [[[5, 5]], [[5, 5], [5, 5], [5, 5]], []])
def test_baseline_of_fewer_than_two_distinct_points_is_refused(bl):
    with pytest.raises(ValueError, match="line 'x'"):
        line_geometry('x', bl, _box(0, 10, 0, 10))


def test_limits_are_enforced():
    with pytest.raises(ValueError, match='boundary vertices'):
        line_geometry('v', [[0, 0], [10, 0]], [[0, 0], [10, 0]])
    ang = np.linspace(0, 2 * np.pi, 4097, endpoint=False)
    with pytest.raises(ValueError, match='boundary vertices'):
        line_geometry('v', [[0, 0], [10, 0]], np.stack([5 + 4000 * np.cos(ang), 4000 * np.sin(ang)], -1))
    line_geometry('ok', [[0, 0], [10, 0]], np.stack([5 + 4000 * np.cos(ang[:4096]), 2 * np.sin(ang[:4096])], -1))
    with pytest.raises(ValueError, match='strip'):
        line_geometry('h', [[0, 0], [10, 0]], _box(0, 10, -2048, 2048))          # 2048 + 2048 + 1 rows
    line_geometry('h', [[0, 0], [10, 0]], _box(0, 10, -2048, 2047))              # 4096 rows: at the limit
    with pytest.raises(ValueError, match='strip'):
        line_geometry('w', [[0, 0], [65535, 0]], _box(0, 10, -2, 2))             # 65536 columns
    assert line_geometry('w', [[0, 0], [65534, 0]], _box(0, 10, -2, 2)).W_s == 65535
    with pytest.raises(ValueError, match='2\\^24'):
        line_geometry('c', [[0, 0], [1 << 25, 0]], _box(0, 10, -2, 2))
    with pytest.raises(ValueError, match='non-finite'):
        line_geometry('n', [[0, 0], [np.nan, 0]], _box(0, 10, -2, 2))


def test_cut_mapping_by_hand():
    # W_s = 401 (S = 400), T = 20, Bt = 5; seq_len 432 = scaled width 400 + 2 x 16, out_len 108 (4 px per frame)
    g = line_geometry('c', [[100, 300], [500, 300]], _box(100, 500, 280, 305))
    assert (g.T, g.Bt, g.W_s) == (20, 5, 401)
    (lab, quad, conf), = cut_quads(g, [(7, 10, 12, 0.5)], 432, 108, 16)
    # frames 10 .. 12 -> pixels 40 .. 52 of the padded line -> strip columns (40 - 16) * 401 / 400 .. (52 - 16) * 401 / 400
    s0, s1 = 24 * 401 / 400, 36 * 401 / 400
    assert lab == 7 and conf == 0.5
    assert np.allclose(quad, [(100 + s0, 280), (100 + s1, 280), (100 + s1, 305), (100 + s0, 305)], atol=1e-9)
    # clamping to [0, S]: a record in the left padding and one past the end
    (_, q0, _), (_, q1, _) = cut_quads(g, [('a', 0, 2, 1.0), ('b', 100, 107, 1.0)], 432, 108, 16)
    assert q0[0] == (100.0, 280.0) and q0[1] == (100.0, 280.0)
    assert q1[1] == (500.0, 280.0) and q1[2] == (500.0, 305.0)
    # a rotated line: the cut follows the baseline's frame
    g = line_geometry('r', [[0, 0], [0, 200]], _box(-10, 10, 0, 200))          # downwards: normal = -x, top side = +x
    assert (g.T, g.Bt) == (10, 10)
    (_, quad, _), = cut_quads(g, [(1, 4, 4, 1.0)], 232, 58, 16)
    s0, s1 = (16 - 16) * 201 / 200, (20 - 16) * 201 / 200
    assert np.allclose(quad, [(10, s0), (10, s1), (-10, s1), (-10, s0)], atol=1e-9)


PAGE_XML = """<?xml version="1.0" encoding="UTF-8"?>
<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2019-07-15">
  <Page imageFilename="scan_01.png" imageWidth="800" imageHeight="600">
    <TextRegion id="r1">
      <Coords points="0,0 800,0 800,600 0,600"/>
      <TextLine id="l1">
        <Coords points="10,20 400,20 400,60 10,60"/>
        <Baseline points="10,55 200,56 400,55"/>
      </TextLine>
      <TextLine id="l2">
        <Coords points="10,80 400,80 400,120 10,120"/>
      </TextLine>
      <TextLine id="l3">
        <Baseline points="10,150 400,150"/>
        <Coords points="10,120 400,120 400,160 10,160"/>
      </TextLine>
    </TextRegion>
  </Page>
</PcGts>
"""

ALTO_XML = """<?xml version="1.0" encoding="UTF-8"?>
<alto xmlns="http://www.loc.gov/standards/alto/ns-v4#">
  <Description><sourceImageInformation><fileName>page 7.jpg</fileName></sourceImageInformation></Description>
  <Layout><Page WIDTH="800" HEIGHT="600" ID="p"><PrintSpace>
    <TextBlock ID="b">
      <TextLine ID="a1" BASELINE="10,55 200,56 400,55">
        <Shape><Polygon POINTS="10,20 400,20 400,60 10,60"/></Shape>
      </TextLine>
      <TextLine ID="a2" BASELINE="10 150 400 150">
        <Shape><Polygon POINTS="10 120 400 120 400 160 10 160"/></Shape>
      </TextLine>
      <TextLine ID="a3" BASELINE="10,190 400,190"/>
      <TextLine ID="a4"><Shape><Polygon POINTS="1,2 3,4 5,6"/></Shape></TextLine>
    </TextBlock>
  </PrintSpace></Page></Layout>
</alto>
"""


def test_page_xml_reader(tmp_path):
    p = tmp_path / 'p.xml'
    p.write_text(PAGE_XML)
    with pytest.warns(UserWarning, match='l2'):
        page = read_page_xml(p)
    assert page.image == 'scan_01.png'
    assert [l.id for l in page.lines] == ['l1', 'l3']
    assert page.lines[0].baseline.tolist() == [[10, 55], [200, 56], [400, 55]]
    assert page.lines[1].boundary.tolist() == [[10, 120], [400, 120], [400, 160], [10, 160]]


def test_alto_reader_both_baseline_forms(tmp_path):
    p = tmp_path / 'a.xml'
    p.write_text(ALTO_XML)
    with pytest.warns(UserWarning) as rec:
        page = read_alto(p)
    msg = str(rec[0].message)
    assert 'a3' in msg and 'a4' in msg
    assert page.image == 'page 7.jpg'
    assert [l.id for l in page.lines] == ['a1', 'a2']
    assert page.lines[0].baseline.tolist() == [[10, 55], [200, 56], [400, 55]]
    assert page.lines[1].baseline.tolist() == [[10, 150], [400, 150]]
    assert page.lines[1].boundary.tolist() == [[10, 120], [400, 120], [400, 160], [10, 160]]


def test_reader_without_skips_is_silent(tmp_path):
    p = tmp_path / 'p.xml'
    p.write_text(PAGE_XML.replace('<TextLine id="l2">\n        <Coords points="10,80 400,80 400,120 10,120"/>\n      </TextLine>', ''))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert [l.id for l in read_page_xml(p).lines] == ['l1', 'l3']


def test_mask_rule_on_a_rectangle():
    """The restatement's even-odd rule: an axis-aligned rectangle [xa, xb] x [ya, yb] holds xa <= x < xb, ya <= y < yb."""
    ys, xs = np.mgrid[0:20, 0:20]
    m = page_ref.mask(np.array([[3, 4], [12, 4], [12, 15], [3, 15]]), xs, ys)
    want = (xs >= 3) & (xs < 12) & (ys >= 4) & (ys < 15)
    assert np.array_equal(m, want)
