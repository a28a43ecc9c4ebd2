"""Device CTC decoders with the call signature of `kraken.lib.ctc_decoder` functions, which is what
the reference stores in `PytorchRecognitionModel.ctc_decoder` (pred.py:42,68,93) and calls per line as
`self.ctc_decoder(seq[:, :seq_len])` on a (C, T) float matrix (pred.py:143,162,177).

The model class recognises these objects and decodes the whole batch in one kernel launch without
moving the logits to the host; called directly with a numpy matrix they decode that one line on the
GPU as well.  Any other callable put into `ctc_decoder` is honoured through the reference's own
per-line host loop."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
import torch

from . import _lib


class _DeviceDecoder:
    """A decoder the engine runs: `decode_async(eng, logits, out_lens)` enqueues the whole batch on `eng`'s device and returns a handle
    for `eng.collect` / `eng.collect_labels`."""
    beam_size = 0

    def decode(self, eng, logits, out_lens):
        return eng.collect(self.decode_async(eng, logits, out_lens))

    def _run(self, outputs: np.ndarray, device=None):
        _lib.load()
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        m = np.ascontiguousarray(np.asarray(outputs, dtype=np.float32).T)           # (T, C)
        T = m.shape[0]
        if T == 0:
            return []
        # a decoder call needs only a device context: borrow a minimal model handle for scratch space
        return self.decode(_scratch_engine(dev), torch.from_numpy(m).to(dev).unsqueeze(0), [T])[0]

    def __call__(self, outputs: np.ndarray) -> List[Tuple[int, int, int, float]]:
        return self._run(outputs)


class GreedyDecoder(_DeviceDecoder):
    """kraken.lib.ctc_decoder.greedy_decoder: argmax, merge runs, drop blank 0."""

    def decode_async(self, eng, logits, out_lens):
        return eng.ctc_greedy_async(logits, out_lens)

    def __repr__(self):
        return 'greedy_decoder<hip>'


class BeamDecoder(_DeviceDecoder):
    """CTC prefix beam search over log-softmax(logits); semantics in include/cocr.h (cocr_ctc_beam)."""

    def __init__(self, beam_size: int = 16):
        self.beam_size = int(beam_size)

    def decode_async(self, eng, logits, out_lens):
        return eng.ctc_beam_async(logits, out_lens, self.beam_size)

    def __repr__(self):
        return f'beam_decoder<hip,{self.beam_size}>'


class LMDecoder(_DeviceDecoder):
    """The beam search with a character n-gram model in the ranking (shallow fusion; DESIGN.md section 7g, include/cocr.h
    cocr_ctc_beam_lm).  `lm`: an `lm.NGramLM` or the path of its file.  alpha weighs the model's log-probabilities, beta is a
    bonus per label, `classes` the candidate classes per frame.  The defaults 0.5 / 0 / 8 are placeholders, not tuned on real
    material: `python -m conformer_ocr_amd.lm tune` finds the values for yours."""

    def __init__(self, lm, beam_size: int = 16, alpha: float = 0.5, beta: float = 0.0, classes: int = 8):
        if isinstance(lm, (str, bytes)) or hasattr(lm, '__fspath__'):
            from .lm import NGramLM
            lm = NGramLM.load(lm)
        self.lm = lm
        self.beam_size, self.alpha, self.beta, self.classes = int(beam_size), float(alpha), float(beta), int(classes)

    def decode_async(self, eng, logits, out_lens):
        """The whole batch in one launch pair on `eng`'s device; a handle for `eng.collect` / `eng.collect_labels`."""
        return eng.ctc_beam_lm_async(logits, out_lens, self.lm, self.beam_size, self.classes, self.alpha, self.beta)

    def __repr__(self):
        return f'lm_beam_decoder<hip,{self.beam_size},order {self.lm.order},alpha {self.alpha:g},beta {self.beta:g},classes {self.classes}>'


_scratch = {}


def _scratch_engine(dev: torch.device):
    from .engine import HipRecognizer
    from .spec import HParams
    key = (dev.type, dev.index)
    if key not in _scratch:
        hp = HParams(num_classes=2, height=16, encoder_dim=16, num_encoder_layers=1, num_attention_heads=1,
                     conv_kernel_size=3, subsampling_conv_channels=8)
        _scratch[key] = HipRecognizer(hp, dev, 'fp32')
    return _scratch[key]


greedy_decoder = GreedyDecoder()


def beam_decoder(outputs: np.ndarray, beam_size: int = 16):
    return BeamDecoder(beam_size)(outputs)
