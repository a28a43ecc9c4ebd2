"""Ground-truth data for training -- what the reference's `TextLineDataModule` / `TextLineDataset` do for
`cocr train` (reference conformer_ocr/dataset.py), on the GPU:

    files (PAGE / ALTO / xml / path line images) -> normalised text + line geometry (host, once)
    -> one packed device buffer of every line's strip (`extract_lines` per page, line images uploaded as they are; pages dropped)
    -> per batch: `preprocess_device` over a subset of that buffer -> [`augment`] -> the `Trainer` batch dict, all in device memory.

kraken's parsers and `-f path` reader are not installed; the rules below are this build's own: PAGE text is the TextLine's direct
TextEquiv (smallest `index`, else the first), ALTO text joins String@CONTENT, SP and HYP@CONTENT; a line image `foo.png` goes with
`foo.gt.txt` (UTF-8).  Bidi reordering is not applied (python-bidi is absent): right-to-left text trains in logical order."""
from __future__ import annotations

import os
import re
import unicodedata
import warnings
from dataclasses import dataclass
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from .codec import PytorchCodec, resize_codec
from .evaluate import make_batches

FORMATS = ('path', 'page', 'alto', 'xml')
NORMALIZATIONS = ('NFD', 'NFC', 'NFKD', 'NFKC')
_WS = re.compile(r'\s+')


def normalize_text(text: str, normalization: Optional[str] = 'NFD', whitespace: bool = True) -> str:
    """unicodedata.normalize(normalization) (None: unchanged), then every run of Unicode whitespace -> one space, ends stripped."""
    if normalization:
        if normalization not in NORMALIZATIONS:
            raise ValueError(f'normalization must be one of {NORMALIZATIONS}')
        text = unicodedata.normalize(normalization, text)
    if whitespace:
        text = _WS.sub(' ', text).strip()
    return text


@dataclass
class GTLine:
    """One usable ground-truth line: its text (normalised) and where its pixels come from -- a page line (`image` = the page file,
    `geom` its `page.LineGeometry`) or a line image (`image` = the file, `geom` None)."""
    id: str
    text: str
    image: str
    geom: object = None


def gt_text_path(image_path: str) -> str:
    """kraken's `-f path` pairing: foo.png -> foo.gt.txt."""
    return os.path.splitext(image_path)[0] + '.gt.txt'


def read_ground_truth(files: Sequence[str], format_type: str = 'xml', normalization: Optional[str] = 'NFD',
                      normalize_whitespace: bool = True) -> List[GTLine]:
    """Parses `files` (host only).  Lines without text (None or empty after normalisation) or whose geometry raises ValueError are
    skipped, with one warning per file naming them."""
    from .page import READERS, line_geometry
    if format_type not in FORMATS:
        raise ValueError(f'format_type must be one of {FORMATS}')
    out: List[GTLine] = []
    for path in files:
        path = str(path)
        if format_type == 'path':
            with open(gt_text_path(path), encoding='utf-8') as fp:
                text = normalize_text(fp.read(), normalization, normalize_whitespace)
            if text:
                out.append(GTLine(path, text, path))
            else:
                warnings.warn(f'{path}: skipped: empty ground truth')
            continue
        page = READERS[format_type](path)
        image = os.path.join(os.path.dirname(os.path.abspath(path)), page.image)
        skipped = []
        for ln in page.lines:
            text = normalize_text(ln.text, normalization, normalize_whitespace) if ln.text is not None else ''
            if not text:
                skipped.append(f'{ln.id} (no text)')
                continue
            try:
                geom = line_geometry(ln.id, ln.baseline, ln.boundary)
            except ValueError as e:
                skipped.append(f'{ln.id} ({e})')
                continue
            out.append(GTLine(ln.id, text, image, geom))
        if skipped:
            warnings.warn(f'{path}: skipped {len(skipped)} line(s): {", ".join(skipped)}')
    return out


def build_codec(texts: Sequence[str]) -> PytorchCodec:
    """The sorted alphabet of `texts` as labels 1..K."""
    return PytorchCodec(sorted(set(''.join(texts))))


def check_codec(codec: PytorchCodec, texts: Sequence[str]) -> None:
    """ValueError naming the characters of `texts` that `codec` (a loaded model's) cannot encode (`codec.resize_codec` grows it)."""
    resize_codec(codec, texts, 'fail')


def split(n: int, partition: float, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """Seeded random split of n lines: (training indices, validation indices), int(n * partition) for training, at least one on
    each side when n >= 2."""
    perm = np.random.default_rng([int(seed), 0x5EED]).permutation(n)
    k = int(n * float(partition))
    if n >= 2:
        k = min(max(k, 1), n - 1)
    return np.sort(perm[:k]), np.sort(perm[k:])


def batch_plan(widths: Sequence[int], batch_size: int, edge: int, seed: int, epoch: int) -> List[Tuple[int, List[int]]]:
    """An epoch's batches over lines of scaled `widths`: the line order is shuffled, `make_batches` buckets it (fixed edges, at most
    `batch_size` lines), the batch order is shuffled; deterministic per (seed, epoch).  Returns [(bucket width, [line indices])]."""
    rng = np.random.default_rng([int(seed), int(epoch), 0xBA7C])
    order = rng.permutation(len(widths))
    plan = make_batches([int(widths[i]) for i in order], int(batch_size), int(edge))
    return [(w, [int(order[i]) for i in idx]) for w, idx in (plan[b] for b in rng.permutation(len(plan)))]


class GroundTruthDataset:
    """Training and validation lines of `training_files` (and `evaluation_files`, if given: otherwise a seeded `partition` split),
    cached on `device` as one packed strip buffer.

        data = GroundTruthDataset(files, format_type='xml', augment=True)
        for batch in data.batches(epoch): trainer.training_step(batch)
        cer = data.validate(net)

    `codec`: a loaded model's (default: the training alphabet's own, `build_codec`); `resize` ('fail', 'union', 'new') and
    `codec_num_classes` (the rows of that model's output layer) go to `codec.resize_codec`, whose results are `self.codec`,
    `self.row_map` (None without `codec`) and `self.num_classes`."""

    def __init__(self, training_files: Sequence[str], evaluation_files: Optional[Sequence[str]] = None, format_type: str = 'xml',
                 partition: float = 0.9, normalization: Optional[str] = 'NFD', normalize_whitespace: bool = True, height: int = 96,
                 pad: int = 16, batch_size: int = 32, edge: int = 200, seed: int = 0, augment: bool = False, augment_config=None,
                 codec: Optional[PytorchCodec] = None, device: str = 'cuda:0', resize: str = 'fail',
                 codec_num_classes: Optional[int] = None):
        from .augment import AugmentConfig
        train = read_ground_truth(training_files, format_type, normalization, normalize_whitespace)
        if evaluation_files:
            val = read_ground_truth(evaluation_files, format_type, normalization, normalize_whitespace)
        else:
            tr, va = split(len(train), partition, seed)
            train, val = [train[i] for i in tr], [train[i] for i in va]
        if not train:
            raise ValueError('no usable training line')
        if not val:
            raise ValueError('no validation line: give evaluation files or more training lines')
        self.lines = train + val
        self.n_train = len(train)
        self.height, self.pad, self.batch_size, self.edge, self.seed = int(height), int(pad), int(batch_size), int(edge), int(seed)
        self.augment = bool(augment)
        self.augment_config = augment_config or AugmentConfig()
        if codec is None:
            codec = build_codec([ln.text for ln in train])
            self.row_map = None
        else:
            # a loaded model's codec: `resize` 'union' / 'new' adapt it to the training alphabet (codec.resize_codec); `row_map` says
            # which row of the model's output layer (of `codec_num_classes` rows) each class of the new one takes
            codec, self.row_map = resize_codec(codec, [ln.text for ln in train], resize, codec_num_classes)
        self.codec = codec
        self.num_classes = codec.max_label + 1 if self.row_map is None else len(self.row_map)
        self.labels = [np.asarray(codec.encode(ln.text), dtype=np.int32) for ln in train]
        self.device = device
        self._cache()

    # ---- strip cache --------------------------------------------------------------------------------------------------------
    def _cache(self) -> None:
        import torch
        from .engine import HipRecognizer
        from .ocr import load_image
        from .synth import hparams
        # a handle for the pre-processing / extraction / augmentation workspaces only: no weights are loaded into it
        self.engine = eng = HipRecognizer(hparams('tiny'), torch.device(self.device), 'fp32')
        n = len(self.lines)
        parts, offs = [], np.zeros(n, dtype=np.int64)
        hs, ws, ch = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.ones(n, dtype=np.int32)
        at = 0
        by_page: Dict[str, List[int]] = {}
        for i, ln in enumerate(self.lines):
            if ln.geom is None:
                img = load_image(ln.image)
                hs[i], ws[i], ch[i] = img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3
                offs[i] = at
                parts.append(torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).to(eng.device))
                at += img.size
            else:
                by_page.setdefault(ln.image, []).append(i)
        for image, idx in by_page.items():
            page = load_image(image)
            strips, so, sh, sw = eng.extract_lines([page], [(0, self.lines[i].geom) for i in idx])
            offs[idx] = at + so
            hs[idx], ws[idx] = sh, sw
            parts.append(strips)
            at += strips.numel()
        self.buffer = torch.cat(parts) if len(parts) > 1 else parts[0]
        eng._keep_pages = None           # the copies above are stream-ordered behind the extraction: the page images can go
        self.offs, self.hs, self.ws, self.ch = offs, hs, ws, ch
        self.uids = np.arange(n, dtype=np.int64)
        self.widths = np.array([int(eng.lib.cocr_preproc_width(int(h), int(w), self.height, self.pad)) for h, w in zip(hs, ws)],
                               dtype=np.int64)

    def _images(self, idx: Sequence[int], width: int):
        idx = np.asarray(idx, dtype=np.int64)
        return self.engine.preprocess_device(self.buffer, self.offs[idx], self.hs[idx], self.ws[idx], self.ch[idx], height=self.height,
                                             pad=self.pad, width=width)

    # ---- training -----------------------------------------------------------------------------------------------------------
    def plan(self, epoch: int) -> List[Tuple[int, List[int]]]:
        """The batches of `epoch` as (bucket width, training line indices)."""
        return batch_plan(self.widths[:self.n_train], self.batch_size, self.edge, self.seed, epoch)

    def batches(self, epoch: int) -> Iterator[Dict]:
        """The `Trainer` batch dicts of one epoch: image (N, 1, H, W) uint8 on the device (augmented when on), seq_lens, target,
        target_lens."""
        import torch
        from .augment import draw, line_keys
        for width, idx in self.plan(epoch):
            im, lens = self._images(idx, width)
            if self.augment:
                params, grid = draw(line_keys(self.seed, epoch, self.uids[idx]), lens, self.height, width, self.augment_config)
                im = self.engine.augment(im, lens, params, grid)
            labels = [self.labels[i] for i in idx]
            yield {'image': im.unsqueeze(1), 'seq_lens': torch.from_numpy(lens.astype(np.int64)),
                   'target': torch.from_numpy(np.concatenate(labels).astype(np.int64)),
                   'target_lens': torch.tensor([len(t) for t in labels], dtype=torch.int64)}

    # ---- validation ---------------------------------------------------------------------------------------------------------
    def validate(self, net, scorer: Optional[str] = None) -> float:
        """CER of `net.predict_string` on the validation lines (cached strips, no augmentation) against their normalised text; the
        strings are scored in one call at the end (`scorer`: see `evaluate.score_strings`)."""
        import torch
        from . import score as _score
        from .evaluate import ErrorRate
        vi = np.arange(self.n_train, len(self.lines))
        preds: List[str] = []
        refs: List[str] = []
        for width, idx in make_batches([int(self.widths[i]) for i in vi], self.batch_size, self.edge):
            lines = vi[idx]
            im, lens = self._images(lines, width)
            preds.extend(net.predict_string(im.unsqueeze(1), torch.from_numpy(lens.astype(np.int64))))
            refs.extend(self.lines[i].text for i in lines)
        if _score.use_device(scorer, getattr(net, '_engine', None)):
            a, a_offs = _score.pack(refs)
            b, b_offs = _score.pack(preds)
            counts, _, _ = _score.align_pairs(net._engine, a, a_offs, b, b_offs)
            return int(counts[:, 0].sum()) / max(int(a_offs[-1]), 1)
        er = ErrorRate()
        er.update(preds, refs)
        return er.compute()
