"""Evaluation of trained models on ground truth from the command line -- the reference's `cocr test` (cli/test.py):

    python -m conformer_ocr_amd.test -m MODEL [-m MODEL2 ...] [-f path|page|alto|xml] [-e LIST ...] [-B 32] [--pad 16] [-u NFD|NFC|NFKD|NFKC]
                                     [--no-normalize-whitespace] [--device cuda:0] [--edge 200] [--scorer device|host]
                                     [--beam N] [--lm FILE [--lm-weight A] [--lm-bonus B] [--lm-classes K]] [--nbest K] FILES...

FILES (globs allowed) and the names listed in the -e manifests (one per line) are PAGE / ALTO documents or, with `-f path`, line images
`foo.png` beside `foo.gt.txt`.  Every line with text and usable geometry is recognized (pages in bounded groups, so a test set larger
than device memory runs) and compared with its ground truth: per model the report of cli/test.py:214-224 (characters, errors, character
and word accuracy, insertions / deletions / substitutions, per-script counts, the most frequent confusions), then the average
accuracies over the models.  The ground truth is not encoded, so the model's alphabet need not cover it.  The alignments behind the
report run on the GPU (`--scorer host`: the Python functions, same output).  With --nbest K (needs --beam or --lm) one more line per
model: `oracle CER in the K-best: x (1-best: y)`, the error rate a perfect ranker would reach on the beam's K best readings.

Not built: `-f binary` (Arrow datasets), `--reorder` / `--base-dir` (python-bidi is absent: text is compared in logical order),
`--workers`, `--threads`."""
from __future__ import annotations

import argparse
import glob
import os
import sys
from typing import Dict, List, Optional, Sequence

PAGE_GROUP = 8          # pages recognized per `recognize_pages` call: bounds the page images held in device memory
CROP_GROUP = 4096       # line images per `recognize_crops` call


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog='python -m conformer_ocr_amd.test', description='Evaluates models on a test set.',
                                 epilog='Not built: -f binary, --reorder / --base-dir (python-bidi is absent: text is compared in logical '
                                        'order), --workers, --threads.')
    ap.add_argument('test_set', nargs='*', help='ground-truth files (globs allowed); added to the -e manifests')
    ap.add_argument('-m', '--model', action='append', default=[], help='model to evaluate: safetensors archive or checkpoint (repeatable)')
    ap.add_argument('-e', '--evaluation-files', action='append', default=[], help='file with paths to evaluation data, one per line (repeatable)')
    ap.add_argument('-f', '--format-type', choices=('path', 'page', 'alto', 'xml'), default='path', help='format of the ground truth')
    ap.add_argument('-B', '--batch-size', type=int, default=32, help='batch sample size')
    ap.add_argument('--pad', type=int, default=16, help='left and right padding around lines')
    ap.add_argument('-u', '--normalization', choices=('NFD', 'NFKD', 'NFC', 'NFKC'), default=None, help='ground truth normalization')
    ap.add_argument('-n', '--normalize-whitespace', dest='normalize_whitespace', action='store_true', default=True,
                    help='normalizes unicode whitespace (default)')
    ap.add_argument('--no-normalize-whitespace', dest='normalize_whitespace', action='store_false')
    ap.add_argument('-d', '--device', default='cuda:0')
    ap.add_argument('--edge', type=int, default=200, help='width bucket edge: lines are padded to a multiple of it')
    ap.add_argument('--scorer', choices=('device', 'host'), default='device', help='where the alignments of the report are computed')
    from .ocr import add_decoder_arguments, add_nbest_argument
    add_decoder_arguments(ap)
    add_nbest_argument(ap)
    return ap


def expand_manifests(manifests: Sequence[str]) -> List[str]:
    """The names listed in the manifest files, one per line (blank lines dropped), in order."""
    out: List[str] = []
    for m in manifests:
        with open(m, encoding='utf-8') as fp:
            out.extend(l.strip() for l in fp if l.strip())
    return out


def expand_globs(entries: Sequence[str]) -> List[str]:
    """Every entry's sorted matches; an entry that matches nothing stays as it is (and fails when it is opened)."""
    out: List[str] = []
    for e in entries:
        out.extend(sorted(glob.glob(e)) or [e])
    return out


def gather_files(args) -> List[str]:
    """The test set of the parsed arguments: the positional files, then the manifests' (cli/test.py:116-119)."""
    return expand_globs(args.test_set) + expand_manifests(args.evaluation_files)


def recognize_ground_truth(net, gt: Sequence, batch_size: int = 32, edge: int = 200, pad: int = 16, device: str = 'cuda:0', nbest: int = 0):
    """The model's string for every `dataset.GTLine` of `gt`, in order: page lines through `page.recognize_pages` in groups of
    PAGE_GROUP pages, line images through `evaluate.recognize_crops` in groups of CROP_GROUP.  nbest > 0: (the strings, per line the
    texts of its `nbest` best readings), through `net.predict_nbest` over the same batches."""
    from .evaluate import make_batches, recognize_crops
    from .ocr import load_image
    from .page import Line, recognize_pages
    out: List[Optional[str]] = [None] * len(gt)
    alts: List[List[str]] = [[] for _ in gt]
    by_page: Dict[str, List[int]] = {}
    crops: List[int] = []
    for i, ln in enumerate(gt):
        if ln.geom is None:
            crops.append(i)
        else:
            by_page.setdefault(ln.image, []).append(i)
    images = list(by_page)
    for k in range(0, len(images), PAGE_GROUP):
        group = images[k:k + PAGE_GROUP]
        pages = [(load_image(image), [Line(gt[i].id, gt[i].geom.points, gt[i].geom.verts) for i in by_page[image]]) for image in group]
        for image, recs in zip(group, recognize_pages(net, pages, batch_size=batch_size, edge=edge, pad=pad, device=device, nbest=nbest)):
            for i, rec in zip(by_page[image], recs):
                out[i] = rec['text']
                alts[i] = [h[0] for h in rec.get('nbest', ())]
    for k in range(0, len(crops), CROP_GROUP):
        group = crops[k:k + CROP_GROUP]
        images = [load_image(gt[i].image) for i in group]
        if not nbest:
            strings = recognize_crops(net, images, batch_size=batch_size, edge=edge, pad=pad, device=device)
            for n, i in enumerate(group):
                out[i] = strings[n]
            continue
        from . import _lib
        lib = _lib.load()
        widths = [int(lib.cocr_preproc_width(int(c.shape[0]), int(c.shape[1]), int(net.height), int(pad))) for c in images]
        for _, idx in make_batches(widths, batch_size, edge):            # `recognize_crops`' batches
            im, lens = net.transform_lines([images[n] for n in idx], pad=pad, bucket_edge=edge, device=device)
            for n, hyps in zip(idx, net.predict_nbest(im, lens, nbest)):
                out[group[n]] = hyps[0][0]
                alts[group[n]] = [h[0] for h in hyps]
    return (out, alts) if nbest else out


def main(argv=None) -> int:
    ap = parser()
    args = ap.parse_args(argv)

    def usage(msg: str) -> int:
        ap.print_usage(sys.stderr)
        print(f'{ap.prog}: error: {msg}', file=sys.stderr)
        return 1
    if not args.model:
        return usage('No model to evaluate given.')
    files = gather_files(args)
    if not files:
        return usage('No evaluation data was provided to the test command. Use `-e` or the `test_set` argument.')
    missing = [f for f in list(args.model) + files if not os.path.exists(f)]
    if missing:
        return usage(f'no such file: {", ".join(missing)}')
    from .dataset import read_ground_truth
    gt = read_ground_truth(files, args.format_type, args.normalization, args.normalize_whitespace)
    if not gt:
        return usage('no usable line in the evaluation data')
    import numpy as np
    from .evaluate import score_strings
    from .ocr import check_nbest, load_model, set_decoder
    truths = [ln.text for ln in gt]
    cer_list, wer_list = [], []
    for model in args.model:
        net = load_model(model, device=args.device)
        try:
            check_nbest(args)
            set_decoder(net, args)
        except ValueError as e:
            return usage(f'{model}: {e}')
        print(f'Evaluating {model}', flush=True)
        preds = recognize_ground_truth(net, gt, args.batch_size, args.edge, args.pad, args.device, args.nbest)
        alts = None
        if args.nbest:
            preds, alts = preds
        res = score_strings(net, preds, truths, report=True, model_name=model, scorer=args.scorer)
        cer_list.append(1.0 - res['cer'])
        wer_list.append(1.0 - res['wer'])
        print(res['report'], flush=True)
        if alts is not None:
            from .nbest import oracle_errors
            chars = max(sum(len(t) for t in truths), 1)
            best = sum(oracle_errors(alts, truths, getattr(net, '_engine', None), args.scorer))
            first = sum(oracle_errors([a[:1] for a in alts], truths, getattr(net, '_engine', None), args.scorer))
            print(f'oracle CER in the {args.nbest}-best: {best / chars:.4f} (1-best: {first / chars:.4f})', flush=True)
    print('Average character accuracy: {:0.2f}%, (stddev: {:0.2f})'.format(np.mean(cer_list) * 100, np.std(cer_list) * 100))
    print('Average word accuracy: {:0.2f}%, (stddev: {:0.2f})'.format(np.mean(wer_list) * 100, np.std(wer_list) * 100))
    return 0


if __name__ == '__main__':
    sys.exit(main())
