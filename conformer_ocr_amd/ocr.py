"""Whole-page recognition from the command line -- the reference's `cocr ocr -i input output -m model` (README.rst:32-39) on a page
image plus its baseline segmentation:

    python -m conformer_ocr_amd.ocr -m MODEL [-f page|alto] -i IN.xml OUT.txt [-i IN2.xml OUT2.txt ...] [--device cuda:0] [--batch-size 32]
                                    [--pad 16] [--edge 200] [--beam N] [--lm FILE [--lm-weight A] [--lm-bonus B] [--lm-classes K]] [--nbest K]

IN is a PAGE XML or ALTO file; the image it names is resolved relative to it.  MODEL is a safetensors archive (`save_safetensors`) or a
Lightning checkpoint.  OUT receives one line of text per TextLine, in document order (the reference's "native" serializer).  With --nbest K (needs --beam or
--lm) OUT.nbest.json also holds, per line id, the K best readings of the beam: [{text, logp, lm_logp, conf: [...]}], logp the exact
CTC log-probability of the reading (null beyond 255 labels), lm_logp the raw n-gram sum, conf the per-character confidences."""
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


def add_decoder_arguments(ap) -> None:
    """--beam / --lm and its weights, shared by the `ocr` and `test` commands."""
    ap.add_argument('--beam', type=int, default=0, help='beam width of the CTC prefix beam search, 1..32; 0 = greedy decoding (default)')
    ap.add_argument('--lm', default=None, metavar='FILE', help='character n-gram language model (python -m conformer_ocr_amd.lm build) mixed into '
                                                               'the beam search; without --beam the beam is 16')
    ap.add_argument('--lm-weight', type=float, default=0.5, help='weight of the language model\'s log-probabilities (default 0.5: a placeholder, '
                                                                 'not tuned on real material; `python -m conformer_ocr_amd.lm tune` finds yours)')
    ap.add_argument('--lm-bonus', type=float, default=0.0, help='bonus per decoded label (default 0: a placeholder, see --lm-weight)')
    ap.add_argument('--lm-classes', type=int, default=8, help='candidate classes per frame of the LM beam search, 1..64 (default 8: a placeholder)')


def add_nbest_argument(ap) -> None:
    """--nbest of the `ocr` and `test` commands (beside `add_decoder_arguments`)."""
    ap.add_argument('--nbest', type=int, default=0, metavar='K', help='also report the K best readings of the beam per line (needs --beam or --lm); '
                                                                      '0 = the best reading only (default)')


def check_nbest(args) -> None:
    """ValueError: --nbest without a beam, negative, or beyond the beam width."""
    if args.nbest < 0 or (args.nbest and not (args.beam or args.lm)):
        raise ValueError('--nbest needs a beam: give --beam or --lm' if args.nbest > 0 else '--nbest must not be negative')
    if args.nbest > (args.beam or 16):
        raise ValueError('--nbest cannot exceed the beam width')


def set_decoder(net, args) -> None:
    """Puts the decoder the arguments of `add_decoder_arguments` select into `net.ctc_decoder`.  ValueError: a beam outside 0..32, or
    a language model whose class count or codec table differs from the model's (naming the first difference)."""
    from .ctc_decoder import BeamDecoder, LMDecoder
    if not 0 <= args.beam <= 32:
        raise ValueError('--beam must be in 0..32')
    if args.lm:
        from .lm import NGramLM
        if not 1 <= args.lm_classes <= 64:
            raise ValueError('--lm-classes must be in 1..64')
        lm = NGramLM.load(args.lm)
        lm.check_codec(net.codec, net.hparams_record.num_classes)
        net.ctc_decoder = LMDecoder(lm, args.beam or 16, args.lm_weight, args.lm_bonus, args.lm_classes)
    elif args.beam:
        net.ctc_decoder = BeamDecoder(args.beam)


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
    add_decoder_arguments(ap)
    add_nbest_argument(ap)
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
    try:
        check_nbest(args)
        set_decoder(net, args)
    except ValueError as e:
        raise SystemExit(f'error: {e}')
    results = recognize_pages(net, [(img, lines) for img, lines, _ in docs], batch_size=args.batch_size, edge=args.edge, pad=args.pad,
                              device=args.device, nbest=args.nbest)
    for (_, _, dst), lines in zip(docs, results):
        with open(dst, 'w', encoding='utf-8') as fp:
            for rec in lines:
                fp.write(rec['text'] + '\n')
        if args.nbest:
            import json
            import math
            doc = {rec['id']: [{'text': text, 'logp': None if math.isnan(logp) else logp, 'lm_logp': lmv, 'conf': [r[3] for r in recs]}
                               for text, logp, lmv, recs in rec['nbest']] for rec in lines}
            with open(dst + '.nbest.json', 'w', encoding='utf-8') as fp:
                json.dump(doc, fp, ensure_ascii=False, indent=1)
                fp.write('\n')
        print(f'{dst}: {len(lines)} lines', file=sys.stderr)
    return 0


if __name__ == '__main__':
    sys.exit(main())
