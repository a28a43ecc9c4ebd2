"""Whole-page recognition from the command line -- the reference's `cocr ocr -i input output -m model` (README.rst:32-39) on a page
image plus its baseline segmentation:

    python -m conformer_ocr_amd.ocr -m MODEL [-f page|alto] -i IN.xml OUT.txt [-i IN2.xml OUT2.txt ...] [--device cuda:0] [--batch-size 32]
                                    [--pad 16] [--edge 200]

IN is a PAGE XML or ALTO file; the image it names is resolved relative to it.  MODEL is a safetensors archive (`save_safetensors`) or a
Lightning checkpoint.  OUT receives one line of text per TextLine, in document order (the reference's "native" serializer)."""
from __future__ import annotations

import argparse
import os
import sys
import tarfile

import numpy as np


def load_model(path, device='cuda:0', **kw):
    from .pred import PytorchRecognitionModel
    net = PytorchRecognitionModel.load_safetensors(path, **kw) if tarfile.is_tarfile(path) else PytorchRecognitionModel.load_checkpoint(path, **kw)
    return net.to(device).eval()


def load_image(path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ('L', 'RGB'):
            im = im.convert('L' if im.mode in ('1', 'I', 'I;16', 'F') else 'RGB')
        return np.asarray(im, dtype=np.uint8).copy()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog='python -m conformer_ocr_amd.ocr', description=__doc__.split('\n\n')[0])
    ap.add_argument('-m', '--model', required=True, help='safetensors archive or checkpoint')
    ap.add_argument('-f', '--format', choices=('page', 'alto'), default='page', help='segmentation format of the inputs')
    ap.add_argument('-i', '--input', nargs=2, action='append', metavar=('IN', 'OUT'), required=True,
                    help='segmentation file and output text file (repeatable)')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--pad', type=int, default=16, help='zero columns left and right of every scaled line (the model\'s training form)')
    ap.add_argument('--edge', type=int, default=200, help='width bucket edge: lines are padded to a multiple of it')
    args = ap.parse_args(argv)
    from .page import read_alto, read_page_xml, recognize_pages
    reader = read_alto if args.format == 'alto' else read_page_xml
    docs = []
    for src, dst in args.input:
        page = reader(src)
        if not page.image:
            raise SystemExit(f'{src}: names no image file')
        img = load_image(os.path.join(os.path.dirname(os.path.abspath(src)), page.image))
        docs.append((img, page.lines, dst))
    net = load_model(args.model, device=args.device)
    results = recognize_pages(net, [(img, lines) for img, lines, _ in docs], batch_size=args.batch_size, edge=args.edge, pad=args.pad,
                              device=args.device)
    for (_, _, dst), lines in zip(docs, results):
        with open(dst, 'w', encoding='utf-8') as fp:
            for rec in lines:
                fp.write(rec['text'] + '\n')
        print(f'{dst}: {len(lines)} lines', file=sys.stderr)
    return 0


if __name__ == '__main__':
    sys.exit(main())
