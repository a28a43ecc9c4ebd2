"""Synthetic ground truth for the training tests and tools/gt_train_rate.py: `synth.make_text_lines` lines (labels mapped to letters)
pasted into page images by `page_synth.text_page`, written as PNG + PAGE XML or ALTO with each line's text."""
import os
from xml.sax.saxutils import escape, quoteattr

import numpy as np

from conformer_ocr_amd import synth
from tests import page_synth


def letters(labels) -> str:
    """Label 1 -> 'a', 2 -> 'b', ..."""
    return ''.join(chr(ord('a') + int(a) - 1) for a in labels)


def _pts(a, sep):
    return ' '.join(f'{x:.3f}{sep}{y:.3f}' for x, y in np.asarray(a, dtype=np.float64))


def write_page_xml(path, image_name, size, lines):
    """lines: (id, baseline, boundary, text)."""
    h, w = size
    body = ''.join(f'<TextLine id={quoteattr(i)}><Coords points="{_pts(bd, ",")}"/><Baseline points="{_pts(bl, ",")}"/>'
                   f'<TextEquiv><Unicode>{escape(t)}</Unicode></TextEquiv></TextLine>' for i, bl, bd, t in lines)
    with open(path, 'w', encoding='utf-8') as fp:
        fp.write('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2019-07-15">'
                 f'<Page imageFilename={quoteattr(image_name)} imageWidth="{w}" imageHeight="{h}"><TextRegion id="r0">{body}</TextRegion>'
                 '</Page></PcGts>\n')


def write_alto(path, image_name, size, lines):
    body = ''.join(f'<TextLine ID={quoteattr(i)} BASELINE="{_pts(bl, " ")}"><Shape><Polygon POINTS="{_pts(bd, " ")}"/></Shape>'
                   + '<SP/>'.join(f'<String CONTENT={quoteattr(word)}/>' for word in t.split(' ')) + '</TextLine>'
                   for i, bl, bd, t in lines)
    with open(path, 'w', encoding='utf-8') as fp:
        fp.write('<?xml version="1.0" encoding="UTF-8"?>\n<alto xmlns="http://www.loc.gov/standards/alto/ns-v4#"><Description>'
                 f'<sourceImageInformation><fileName>{escape(image_name)}</fileName></sourceImageInformation></Description>'
                 f'<Layout><Page ID="p0"><PrintSpace><TextBlock ID="b0">{body}</TextBlock></PrintSpace></Page></Layout></alto>\n')


def make_pages(directory, formats=('page', 'alto'), lines_per_page=8, width=600, height=96, seed=3, kinds=None):
    """One page per entry of `formats`, lines of `width` px drawn with a shared alphabet.  Returns [(xml path, page image (H, W) u8,
    [page.Line with text])]."""
    from PIL import Image
    from conformer_ocr_amd.page import Line
    kinds = kinds or [('line', 0.0), ('line', 2.0), ('line', -2.0), ('line', 1.0)]
    out = []
    for p, fmt in enumerate(formats):
        image, _, texts, _ = synth.make_text_lines(lines_per_page, height, width, seed=seed + 17 * p, alphabet_seed=seed)
        u8 = synth.lines_u8(image)[:, 0]
        page, placed = page_synth.text_page(list(u8), [kinds[i % len(kinds)] for i in range(lines_per_page)])
        name = f'page_{p}'
        Image.fromarray(page).save(os.path.join(directory, name + '.png'))
        lines = [(f'{name}_l{i}', P, bd, letters(t)) for i, ((_, P, bd), t) in enumerate(zip(placed, texts))]
        xml = os.path.join(directory, name + '.xml')
        (write_page_xml if fmt == 'page' else write_alto)(xml, name + '.png', page.shape, lines)
        out.append((xml, page, [Line(i, P, bd, t) for i, P, bd, t in lines]))
    return out
