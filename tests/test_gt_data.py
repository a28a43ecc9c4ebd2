"""Ground truth on the host (no GPU): the readers' text, `xml` sniffing, `path` pairing, normalisation, the codec, the batch plan and the
augmentation's parameter draw."""
import os
import warnings

import numpy as np
import pytest

from conformer_ocr_amd import augment as aug
from conformer_ocr_amd import dataset
from conformer_ocr_amd.evaluate import bucket_width
from conformer_ocr_amd.page import Line, read_alto, read_page_xml, read_xml

PAGE = '''<?xml version="1.0" encoding="UTF-8"?>
<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2019-07-15"><Page imageFilename="p.png" imageWidth="400" imageHeight="300">
<TextRegion id="r"><TextEquiv><Unicode>region text</Unicode></TextEquiv>
<TextLine id="l0"><Coords points="10,10 200,10 200,40 10,40"/><Baseline points="10,35 200,35"/>
  <Word id="w0"><TextEquiv><Unicode>WORD</Unicode></TextEquiv></Word>
  <TextEquiv index="2"><Unicode>second</Unicode></TextEquiv><TextEquiv index="1"><Unicode>first</Unicode></TextEquiv></TextLine>
<TextLine id="l1"><Coords points="10,50 200,50 200,80 10,80"/><Baseline points="10,75 200,75"/>
  <TextEquiv><Unicode>plain  text</Unicode></TextEquiv><TextEquiv><Unicode>other</Unicode></TextEquiv></TextLine>
<TextLine id="l2"><Coords points="10,90 200,90 200,120 10,120"/><Baseline points="10,115 200,115"/>
  <Word id="w1"><TextEquiv><Unicode>only a word</Unicode></TextEquiv></Word></TextLine>
<TextLine id="l3"><Coords points="10,130 200,130 200,160 10,160"/></TextLine>
</TextRegion></Page></PcGts>
'''

ALTO = '''<?xml version="1.0" encoding="UTF-8"?>
<alto xmlns="http://www.loc.gov/standards/alto/ns-v4#"><Description><sourceImageInformation><fileName>a.png</fileName>
</sourceImageInformation></Description><Layout><Page ID="p"><PrintSpace><TextBlock ID="b">
<TextLine ID="t0" BASELINE="10 35 200 35"><Shape><Polygon POINTS="10 10 200 10 200 40 10 40"/></Shape>
  <String CONTENT="Hello"/><SP/><String CONTENT="wor"/><HYP CONTENT="-"/></TextLine>
<TextLine ID="t1" BASELINE="10,75 200,75"><Shape><Polygon POINTS="10 50 200 50 200 80 10 80"/></Shape></TextLine>
</TextBlock></PrintSpace></Page></Layout></alto>
'''


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text, encoding='utf-8')
    return str(p)


def test_page_text_by_index_and_line_level_only(tmp_path):
    path = _write(tmp_path, 'p.xml', PAGE)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        page = read_page_xml(path)
    assert [ln.id for ln in page.lines] == ['l0', 'l1', 'l2']                  # l3 (no baseline) skipped as before
    assert [ln.text for ln in page.lines] == ['first', 'plain  text', None]
    assert len(w) == 1 and 'l3' in str(w[0].message) and 'baseline' in str(w[0].message)
    assert page.image == 'p.png'
    np.testing.assert_array_equal(page.lines[0].baseline, [[10, 35], [200, 35]])
    np.testing.assert_array_equal(page.lines[0].boundary, [[10, 10], [200, 10], [200, 40], [10, 40]])


def test_alto_text_joins_string_sp_hyp(tmp_path):
    path = _write(tmp_path, 'a.xml', ALTO)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                                          # a line without text does not warn
        page = read_alto(path)
    assert page.image == 'a.png'
    assert [ln.text for ln in page.lines] == ['Hello wor-', None]
    assert [ln.id for ln in page.lines] == ['t0', 't1']


def test_line_positional_construction_and_default_text():
    ln = Line('x', np.zeros((2, 2)), np.zeros((3, 2)))
    assert ln.text is None


def test_xml_sniffs_the_root_element(tmp_path):
    p = _write(tmp_path, 'p.xml', PAGE)
    a = _write(tmp_path, 'a.xml', ALTO)
    assert read_xml(p).image == 'p.png' and read_xml(a).image == 'a.png'
    assert [ln.text for ln in read_xml(a).lines] == ['Hello wor-', None]
    with pytest.raises(ValueError):
        read_xml(_write(tmp_path, 'x.xml', '<root/>'))


def test_path_pairing_and_skips(tmp_path):
    from PIL import Image
    Image.fromarray(np.zeros((10, 20), dtype=np.uint8)).save(tmp_path / 'foo.png')
    Image.fromarray(np.zeros((10, 20), dtype=np.uint8)).save(tmp_path / 'bar.bin.png')
    assert dataset.gt_text_path(str(tmp_path / 'foo.png')) == str(tmp_path / 'foo.gt.txt')
    assert dataset.gt_text_path(str(tmp_path / 'bar.bin.png')) == str(tmp_path / 'bar.bin.gt.txt')
    _write(tmp_path, 'foo.gt.txt', ' a  b\n')
    _write(tmp_path, 'bar.bin.gt.txt', ' \n')
    with pytest.warns(UserWarning, match='bar.bin.png'):
        gt = dataset.read_ground_truth([str(tmp_path / 'foo.png'), str(tmp_path / 'bar.bin.png')], 'path')
    assert [(g.text, g.geom) for g in gt] == [('a b', None)]


def test_page_lines_without_text_or_geometry_are_skipped_with_one_warning(tmp_path):
    path = _write(tmp_path, 'p.xml', PAGE.replace('<Baseline points="10,75 200,75"/>', '<Baseline points="10,75 10,75"/>'))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        gt = dataset.read_ground_truth([path], 'page')
    assert [g.id for g in gt] == ['l0'] and gt[0].text == 'first'
    mine = [str(x.message) for x in w if 'skipped 2 line' in str(x.message)]
    assert len(mine) == 1 and 'l1' in mine[0] and 'l2' in mine[0]


def test_normalisation_and_whitespace():
    s = 'é \t x  y\n'
    assert dataset.normalize_text(s) == 'é x y'
    assert dataset.normalize_text(s, 'NFC') == 'é x y'
    assert dataset.normalize_text('é', 'NFD') == 'é'
    assert dataset.normalize_text('ﬁ', 'NFKC') == 'fi'
    assert dataset.normalize_text(' a  b ', None, False) == ' a  b '
    with pytest.raises(ValueError):
        dataset.normalize_text('a', 'NFX')


def test_codec_is_deterministic_from_the_alphabet():
    a = dataset.build_codec(['cab', 'b a'])
    b = dataset.build_codec(['a b', 'bca'])
    assert a.c2l == b.c2l == {' ': [1], 'a': [2], 'b': [3], 'c': [4]}
    dataset.check_codec(a, ['abc'])
    with pytest.raises(ValueError, match='xz'):
        dataset.check_codec(a, ['abx', 'z'])


def test_split_is_seeded_and_complete():
    tr, va = dataset.split(50, 0.9, 3)
    assert len(tr) == 45 and len(va) == 5 and sorted(np.concatenate([tr, va]).tolist()) == list(range(50))
    assert np.array_equal(dataset.split(50, 0.9, 3)[1], va) and not np.array_equal(dataset.split(50, 0.9, 4)[1], va)
    assert [len(x) for x in dataset.split(3, 0.9, 0)] == [2, 1]


def test_batch_plan():
    g = np.random.default_rng(0)
    widths = g.integers(100, 2000, 301)
    p0, p1 = dataset.batch_plan(widths, 32, 200, 7, 0), dataset.batch_plan(widths, 32, 200, 7, 1)
    for plan in (p0, p1):
        seen = sorted(i for _, idx in plan for i in idx)
        assert seen == list(range(301))                                         # every line exactly once
        for w, idx in plan:
            assert 1 <= len(idx) <= 32
            assert all(bucket_width(int(widths[i]), 200) == w for i in idx)
    assert p0 == dataset.batch_plan(widths, 32, 200, 7, 0)                     # deterministic per (seed, epoch)
    assert p0 != p1 and p0 != dataset.batch_plan(widths, 32, 200, 8, 0)


def test_parameter_draw():
    n = 10000
    keys = aug.line_keys(0, 0, np.arange(n))
    sl = np.random.default_rng(1).integers(50, 2000, n)
    t, g = aug.draw(keys, sl, 96, 2000)
    t2, g2 = aug.draw(keys, sl, 96, 2000)
    assert np.array_equal(t, t2) and np.array_equal(g, g2)                      # deterministic per key
    t3, _ = aug.draw(keys[::-1], sl[::-1], 96, 2000)
    assert np.array_equal(t3[::-1], t)                                           # a line's draw does not depend on its position
    fl = t[:, aug.F_FLAGS]
    gate = aug._u16(aug.hash64(keys, aug.H_GATE)) < 32768
    assert abs((~gate).mean() - 0.5) < 0.02                                     # the p = 0.5 gate leaves half of the lines alone
    assert (fl[~gate] == 0).all()
    assert abs((fl == 0).mean() - (0.5 + 0.5 * 0.8 ** 4)) < 0.02                # ... and all four stages off: 0.70
    for bit in (aug.GEOM, aug.ELASTIC, aug.BLUR, aug.DROPOUT):
        assert abs(((fl & bit) != 0).mean() - 0.1) < 0.01
    geo = (fl & aug.GEOM) != 0
    A = t[geo, aug.F_A:aug.F_A + 6].astype(np.float64) / aug.FIX
    s = 1.0 / np.hypot(A[:, 0], A[:, 1])
    ang = np.degrees(np.arctan2(A[:, 1], A[:, 0]))
    assert (s > 0.8 - 1e-4).all() and (s < 1.2 + 1e-4).all() and (np.abs(ang) <= 3.0 + 1e-3).all()
    assert (t[~geo, aug.F_A:aug.F_A + 6] == [aug.FIX, 0, 0, 0, aug.FIX, 0]).all()
    # the shift: the line centre maps to within 1/16 of the height / seq_len (scaled) of itself
    cx, cy = (sl[geo] - 1) / 2.0, 47.5
    X = A[:, 0] * cx + A[:, 1] * cy + A[:, 2]
    Y = A[:, 3] * cx + A[:, 4] * cy + A[:, 5]
    sn = np.sin(np.radians(3.0))
    assert (np.abs(X - cx) <= (sl[geo] / 16 + sn * 96 / 16) / 0.8 + 1e-3).all()
    assert (np.abs(Y - cy) <= (96 / 16 + sn * sl[geo] / 16) / 0.8 + 1e-3).all()
    el = (fl & aug.ELASTIC) != 0
    assert (g[~el] == 0).all() and np.abs(g[el]).max() <= 2 * aug.FIX and np.abs(g[el]).max() > 1.9 * aug.FIX
    bl = (fl & aug.BLUR) != 0
    assert set(t[bl, aug.F_BLUR]) == {1, 2, 3} and (t[~bl, aug.F_BLUR] == 0).all()
    assert set(t[bl, aug.F_MLEN]) == {3, 5, 7} and set(t[bl, aug.F_MDIR]) == {0, 1, 2, 3}
    dr = (fl & aug.DROPOUT) != 0
    assert (t[dr, aug.F_DROP] == 655).all() and (t[~dr, aug.F_DROP] == 0).all()
    aug.check_tables(t, g, sl, 96, 2000)
    # keys: different per line, epoch and seed
    assert len(set(keys.tolist())) == n
    assert not np.array_equal(aug.line_keys(0, 1, np.arange(n)), keys) and not np.array_equal(aug.line_keys(1, 0, np.arange(n)), keys)


def test_grid_does_not_depend_on_the_batch_width():
    keys = aug.line_keys(3, 0, np.arange(200))
    cfg = aug.AugmentConfig(p=1.0, p_elastic=1.0)
    _, g1 = aug.draw(keys, np.full(200, 300), 96, 300)
    _, g2 = aug.draw(keys, np.full(200, 300), 96, 1000)
    assert np.array_equal(g2[:, :g1.shape[1]], g1) or not (g1 != 0).any()
    _, g1 = aug.draw(keys, np.full(200, 300), 96, 300, cfg)
    _, g2 = aug.draw(keys, np.full(200, 300), 96, 1000, cfg)
    assert (g1 != 0).any() and np.array_equal(g2[:, :g1.shape[1]], g1)


def test_median_network_matches_a_sort():
    """The restatement's median (np.sort) and the kernel's exchange network select the same element: the network, run here on
    the host over random 9-tuples (including ties), against sorting."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'conformer_ocr_amd', 'csrc', 'augment.hip.h')).read()
    body = src[src.index('aug_median9('):]
    body = body[body.index('{') + 1:body.index('return p4;')]
    import re
    pairs = [(int(a), int(b)) for a, b in re.findall(r'aug_cswap\(p(\d), p(\d)\)', body)]
    assert len(pairs) == 19
    g = np.random.default_rng(0)
    for _ in range(3000):
        p = list(g.integers(0, 4 if _ % 2 else 256, 9))
        want = sorted(p)[4]
        for a, b in pairs:
            if p[a] > p[b]:
                p[a], p[b] = p[b], p[a]
        assert p[4] == want
