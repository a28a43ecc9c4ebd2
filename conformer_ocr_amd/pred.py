"""
conformer_ocr_amd.pred
~~~~~~~~~~~~~~~~~~~~~~

Recognition inference: `PytorchRecognitionModel` with the surface of the reference class
(reference conformer_ocr/pred.py:50-210 -- constructor arguments, attributes `nn`, `codec`,
`ctc_decoder`, `height`, `channels`, `width`; methods `forward`, `predict`, `predict_string`,
`predict_labels`, `load_safetensors`, `load_checkpoint`), backed by the gfx950 kernels behind the C
ABI of include/cocr.h.  torch holds the parameters (state-dict compatible with reference
checkpoints) and owns device memory; no layer of the network is evaluated by torch.
"""
from __future__ import annotations

import io
import json
import logging
import tarfile
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import nn

from .codec import PytorchCodec
from .ctc_decoder import BeamDecoder, LMDecoder, _DeviceDecoder, greedy_decoder
from .engine import HipRecognizer
from .spec import HParams, encoder_state_spec

logger = logging.getLogger(__name__)


class _Holder(nn.Module):
    """Parameter container: no forward, only the reference's module tree for its state-dict keys."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('parameters only: the network runs in libcocr_hip.so')


def _build_param_tree(spec) -> nn.Module:
    root = _Holder()
    for name, (shape, kind) in spec.items():
        parts = name.split('.')
        mod = root
        for p in parts[:-1]:
            if not hasattr(mod, p):
                mod.add_module(p, _Holder())
            mod = getattr(mod, p)
        leaf = parts[-1]
        if kind == 'param':
            if len(shape) >= 2:
                t = torch.empty(shape).uniform_(-0.05, 0.05)
            else:
                t = torch.ones(shape) if leaf == 'weight' else torch.zeros(shape)
            mod.register_parameter(leaf, nn.Parameter(t, requires_grad=False))
        elif kind == 'buffer':
            mod.register_buffer(leaf, torch.ones(shape) if leaf == 'running_var' else torch.zeros(shape))
        else:
            mod.register_buffer(leaf, torch.zeros(shape, dtype=torch.long))
    return root


class PytorchRecognitionModel(nn.Module):
    def __init__(self,
                 num_classes: int,
                 height: int,
                 encoder_dim: int,
                 num_encoder_layers: int,
                 num_attention_heads: int,
                 feed_forward_expansion_factor: int,
                 conv_expansion_factor: int,
                 input_dropout_p: float,
                 feed_forward_dropout_p: float,
                 attention_dropout_p: float,
                 conv_dropout_p: float,
                 conv_kernel_size: int,
                 half_step_residual: bool,
                 subsampling_conv_channels: int,
                 subsampling_factor: int,
                 codec: PytorchCodec,
                 ctc_decoder=greedy_decoder,
                 **kwargs):
        """
        Inference version of a conformer_ocr RecognitionModel (pred.py:51-98).  Dropout
        probabilities are accepted and ignored (inference); unknown keyword arguments are ignored
        like in the reference, except `compute_dtype` ('bf16' default, or 'fp32') and `chain_rows`.
        """
        super().__init__()
        self.hparams_record = HParams(num_classes=num_classes, height=height, encoder_dim=encoder_dim,
                                      num_encoder_layers=num_encoder_layers, num_attention_heads=num_attention_heads,
                                      feed_forward_expansion_factor=feed_forward_expansion_factor,
                                      conv_expansion_factor=conv_expansion_factor, conv_kernel_size=conv_kernel_size,
                                      half_step_residual=bool(half_step_residual),
                                      subsampling_conv_channels=subsampling_conv_channels,
                                      subsampling_factor=subsampling_factor)
        encoder = _build_param_tree(encoder_state_spec(self.hparams_record))
        decoder = nn.Linear(encoder_dim, num_classes, bias=True)
        for p in decoder.parameters():
            p.requires_grad_(False)
        self.nn = nn.ModuleDict({'encoder': encoder,
                                 'decoder': decoder})

        self.codec = codec
        self.ctc_decoder = ctc_decoder
        self.height = height
        self.channels = 1
        self.width = 0
        self.compute_dtype = kwargs.get('compute_dtype', 'bf16')
        # the reference's four dropout probabilities: identity at inference, used by conformer_ocr_amd.train.Trainer
        self.dropout_p = (float(input_dropout_p), float(feed_forward_dropout_p), float(attention_dropout_p), float(conv_dropout_p))
        # rows per workgroup of the row-chain kernels (include/cocr.h cocr_set_chain_rows).  This class is called one batch at a time
        # (the reference's loop, cli/test.py:185-199): 48-row blocks give every CU a workgroup at 32 x 300 frames and the shortest
        # forward; a caller that keeps several batches in flight on its own streams (bench.py) passes chain_rows=0.
        self.chain_rows = int(kwargs.get('chain_rows', 48))
        self._engine: Optional[HipRecognizer] = None
        self._engine_sig = None
        self._sig_tensors = None

    # ------------------------------------------------------------------ device model
    def _apply(self, fn, recurse=True):
        """`.to()` / `.cuda()` / `.float()`: parameters get new storage, buffers are replaced -- the cached tensor list is rebuilt."""
        out = super()._apply(fn, recurse)
        self._sig_tensors = None
        return out

    def invalidate_engine(self) -> None:
        """Forces a re-pack of the device model at the next call.  Not needed after any of: in-place writes, `load_state_dict`
        (also with `assign=True`), `.to()`, `p.data = new`, replacing a parameter, a buffer, a sub-module
        (`net.nn.decoder = nn.Linear(...)`) or `net.nn` itself -- `_signature` sees all of these.  What it cannot see: a write
        that bypasses the version counter of a tensor whose address stays the same (raw pointer writes from another library,
        `tensor.data.copy_()` counts and is seen)."""
        self._sig_tensors = None
        self._engine_sig = None

    def _signature(self, device: torch.device):
        """Identity of the weights the packed device model was built from, re-read on EVERY call:
        * which objects hang in the module tree: ids of every module's children, parameters and buffers (a replaced sub-module,
          `load_state_dict(assign=True)`, `del` / re-register) -- read from the modules' own dicts, not through `state_dict()`
          or `parameters()` (1.5 ms / 0.6 ms per call for the 12-block model);
        * where their values live: `data_ptr()` of every tensor (`p.data = new`, `.to()`);
        * whether they were written in place: the sum of the version counters.
        About 0.15 ms for 478 tensors in 539 modules; `forward` runs it AFTER it has enqueued the launch (the GPU is busy for
        0.8 ms or more) and repeats the call in the rare case that the answer is "changed"."""
        ids = None
        if self._sig_tensors is not None and self._sig_tensors[3][0] is self.nn:      # (a replaced `self.nn`: the cached dicts are the old tree's)
            ids = [id(v) for d in self._sig_tensors[1] for v in d.values()]
        if ids is None or ids != self._sig_tensors[2]:
            # first call, or the tree changed.  The cache keeps the modules and tensors it describes alive, so an id in `ids`
            # cannot have been handed to a new object in the meantime; the generation counts the rebuilds.
            mods = list(self.nn.modules())
            dicts = [d for m in mods for d in (m._modules, m._parameters, m._buffers)]
            self._sig_tensors = ([*self.nn.parameters(), *self.nn.buffers()], dicts, [id(v) for d in dicts for v in d.values()], mods)
            self._sig_gen = getattr(self, '_sig_gen', 0) + 1
        ts = self._sig_tensors[0]
        ver, ptrs = 0, []
        for t in ts:
            ver += t._version
            ptrs.append(t.data_ptr())
        return (str(device), self.compute_dtype, self._sig_gen, id(self.nn), tuple(ptrs), ver)

    def _unchanged_at_a_glance(self) -> bool:
        """The cheap part of `_signature` (about 40 us): the same module tree object and the same sum of version counters as when
        the device model was packed.  In-place writes (every optimiser step of a training / validation interleave) show here;
        `forward` then re-packs BEFORE launching instead of running a whole forward on stale weights first."""
        st, sig = self._sig_tensors, self._engine_sig
        if st is None or sig is None or st[3][0] is not self.nn:
            return False
        ver = 0
        for t in st[0]:
            ver += t._version
        return ver == sig[-1]

    def _pack(self, device: torch.device, sig) -> HipRecognizer:
        eng = HipRecognizer(self.hparams_record, device, self.compute_dtype)
        eng.load_state({k: v for k, v in self.nn.state_dict().items()}, strict=True)
        eng.finalize()
        eng.set_chain_rows(self.chain_rows)
        eng.set_graph(True)        # hipGraph replay of the launch sequence, staged for the fresh tensors every call brings
        self._engine, self._engine_sig = eng, sig
        return eng

    def engine(self, device: Optional[torch.device] = None) -> HipRecognizer:
        """The packed device model, (re)built when the parameters or the device changed."""
        if device is None:
            device = next(self.nn.parameters()).device
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('PytorchRecognitionModel (HIP) needs a GPU: move the model / line batch to a cuda device; '
                               'there is no CPU fallback')
        sig = self._signature(device)
        if self._engine is None or sig != self._engine_sig:
            self._pack(device, sig)
        return self._engine

    def engine_pool(self, n: int, device: Optional[torch.device] = None) -> List[HipRecognizer]:
        """`n` packed copies of the device model for callers that keep several batches in flight, one per stream
        (conformer_ocr_amd/evaluate.py `recognize(..., streams=n)`): each has its own workspace and captured launch sequences and reads the
        first engine's weights (`cocr_share_weights`); the
        row-chain kernels run the throughput form the library picks for `n` copies on this process's hardware queues (`cocr_get_chain_rows`:
        96-row blocks when four batches really overlap, 64-row ones when the streams share three queues).  Rebuilt when the parameters
        change, like `engine()`."""
        from . import hw_queues_note
        hw_queues_note(n)
        eng0 = self.engine(device)
        if getattr(self, '_pool_sig', None) != self._engine_sig:
            self._pool, self._pool_sig = [], self._engine_sig
        while len(self._pool) < n:
            eng = HipRecognizer(self.hparams_record, eng0.device, self.compute_dtype)
            eng.share_weights(eng0)        # one set of weights and tables for all copies (they stay in the Infinity Cache; include/cocr.h)
            eng.set_chain_rows(0)
            eng.set_graph(True)
            self._pool.append(eng)
        return self._pool[:n]

    def pool_streams(self, n: int, device: Optional[torch.device] = None) -> List['torch.cuda.Stream']:
        """The streams the copies of `engine_pool` run on: kept, so that repeated loops queue on the same few hardware queues."""
        dev = self.engine(device).device
        if getattr(self, '_pool_streams_dev', None) != dev:
            self._pool_streams_list, self._pool_streams_dev = [], dev
        while len(self._pool_streams_list) < n:
            self._pool_streams_list.append(torch.cuda.Stream(dev))
        return self._pool_streams_list[:n]

    def adopt_engine(self, eng: HipRecognizer) -> None:
        """Use an already packed device model (e.g. one whose weights arrived by RCCL broadcast)."""
        self._engine = eng
        self._engine_sig = self._signature(eng.device)

    # ------------------------------------------------------------------ reference surface
    def forward(self, line: torch.Tensor, lens: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """
        Performs a forward pass on a torch tensor of one or more lines with
        shape (N, C, H, W) and returns the logits (N, W', num_classes) [a torch tensor on the
        line's device, as the reference returns despite its docstring] and the int32 output
        sequence lengths (pred.py:101-122).  `lens` is required, as in the reference
        (calc_length(None) raises there).
        """
        if lens is None:
            raise TypeError('lens is required (the reference raises in calc_length for lens=None)')
        if line.dim() != 4 or line.shape[1] != 1:
            raise ValueError(f'expected a (N,1,H,W) line batch, got {tuple(line.shape)}')
        lens_np = torch.as_tensor(lens).cpu().numpy()
        eng = self._engine
        if eng is None or not line.is_cuda or line.device != eng.device:
            eng = self.engine(line.device if line.is_cuda else None)
            probits, out_lens = eng.forward(line.squeeze(1), lens_np)
        elif not self._unchanged_at_a_glance():
            # version counters moved (or the tree object changed): pack first, then launch -- no forward on stale weights
            eng = self.engine(eng.device)
            probits, out_lens = eng.forward(line.squeeze(1), lens_np)
        else:
            # launch first, walk the whole tree while the GPU works (`_signature`: ids, addresses, versions of 478 tensors -- in front
            # of every launch that was 10 % of a 32-line call); the cheap glance above has already caught in-place writes
            with torch.no_grad():
                probits, out_lens = eng.forward(line.squeeze(1), lens_np)
            sig = self._signature(eng.device)
            if sig != self._engine_sig:                    # a replaced tensor or sub-module: pack again, run again
                torch.cuda.current_stream(eng.device).synchronize()      # (the old engine's launches are still queued on its buffers)
                eng = self._pack(eng.device, sig)
                probits, out_lens = eng.forward(line.squeeze(1), lens_np)
        return probits, torch.from_numpy(out_lens)

    def transform_lines(self, crops, pad: int = 16, bucket_edge: int = 0, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The step kraken's `ImageInputTransforms(1, height, 0, 1, (pad, 0))` performs in the reference's data pipeline
        (dataset.py:89, cli/test.py:156), on the GPU: raw 8-bit line crops ((H, W) or (H, W, 3) numpy arrays of any height) ->
        a `(N, 1, height, W)` uint8 line batch (pixel / 255 = the [0, 1] floats `forward` expects; it ingests uint8 directly)
        and the `seq_lens` (scaled width + 2 pad).  W = the widest line, rounded up to a multiple of `bucket_edge` if given."""
        eng = self.engine(device)
        batch, lens = eng.preprocess(list(crops), height=self.height, pad=pad, bucket_edge=bucket_edge)
        return batch.unsqueeze(1), torch.from_numpy(lens)

    def _label_records(self, line: torch.Tensor, lens: torch.Tensor) -> List[List[Tuple[int, int, int, float]]]:
        kind, h, eng = self.predict_string_async(line, lens)
        return eng.collect(h) if kind == 'device' else h

    def predict(self, line: torch.Tensor, lens: Optional[torch.Tensor] = None) -> List[List[Tuple[str, int, int, float]]]:
        """
        Forward pass + decoding as lists of (string, start, end, confidence) tuples, one list per
        line -- what the reference's docstring promises (pred.py:124-136; its body calls the codec
        object itself, which kraken's codec does not support).
        """
        return [self.codec.decode(locs) for locs in self._label_records(line, lens)]

    def predict_string(self, line: torch.Tensor, lens: Optional[torch.Tensor] = None) -> List[str]:
        """
        Forward pass on a (N, C, H, W) batch; returns one string per line, batch order
        preserved (pred.py:148-164).
        """
        return self.collect_strings(self.predict_string_async(line, lens))

    def predict_nbest(self, line: torch.Tensor, seq_lens: torch.Tensor, nbest: int) -> List[List[Tuple[str, float, float, List[Tuple[int, int, int, float]]]]]:
        """Forward pass + n-best decoding: per line the first `nbest` hypotheses of the beam of `ctc_decoder` (a
        `BeamDecoder`, or an `LMDecoder` with its model and weights), each (text, logp, lm_logp, label records) -- text through the codec
        as `predict_string`'s, logp the exact CTC log-probability of the label sequence (NaN beyond 255 labels), lm_logp the raw
        n-gram sum (0 without a language model).  Entry 0 is the reading `predict_string` returns.  Any other decoder: ValueError."""
        dec = self.ctc_decoder
        if not isinstance(dec, (BeamDecoder, LMDecoder)):
            raise ValueError('n-best output needs a beam: set ctc_decoder to a BeamDecoder or an LMDecoder (--beam / --lm)')
        o, olens = self.forward(line, seq_lens)
        kw = dict(lm=dec.lm, classes=dec.classes, alpha=dec.alpha, beta=dec.beta) if isinstance(dec, LMDecoder) else {}
        hyps = self._engine.ctc_beam_nbest(o, olens.numpy(), dec.beam_size, min(int(nbest), dec.beam_size), **kw)
        return [[(''.join(x[0] for x in self.codec.decode(recs)), logp, lmv, recs) for recs, logp, lmv in hs] for hs in hyps]

    def _codec_lut(self):
        """label -> character table of a 1:1, non-strict codec ('' for labels the codec does not know: skipped, as `decode` skips them;
        last entry: every label beyond the table); None for codecs with multi-label graphemes."""
        c = self.codec
        l2c1 = getattr(c, '_l2c1', None)
        if l2c1 is None or getattr(c, 'strict', False):
            return None
        key = hash(tuple(l2c1.items()))                 # (an in-place edit of the codec's map that keeps its size must rebuild the table)
        if getattr(self, '_lut_of', None) is not c or getattr(self, '_lut_key', None) != key:
            top = max(l2c1, default=0)
            if top > (1 << 20):                         # sparse label ids: no table, `decode()` does it
                self._lut = None
            else:
                width = max((len(v) for v in l2c1.values()), default=1)
                lut = np.zeros(top + 2, dtype=f'<U{max(width, 1)}')
                for k, v in l2c1.items():
                    lut[k] = v
                self._lut = lut
            self._lut_of, self._lut_key = c, key
        return self._lut

    def predict_string_async(self, line: torch.Tensor, lens: torch.Tensor):
        """`predict_string` split in two for pipelined callers (conformer_ocr_amd/evaluate.py): enqueues forward, CTC decode and
        the read-back of the label records on the current stream and returns a handle; `collect_strings(handle)` waits for
        that batch only -- the next batch's upload and forward can be in flight meanwhile."""
        o, olens = self.forward(line, lens)
        eng = self._engine             # the handle carries the engine that owns its pinned records (a re-pack may replace `self._engine` before the collect)
        if isinstance(self.ctc_decoder, _DeviceDecoder):
            return ('device', self.ctc_decoder.decode_async(eng, o, olens.numpy()), eng)
        o = o.transpose(1, 2).cpu().float().numpy()           # a user-supplied decoder: the reference's own host loop (pred.py:158-162)
        return ('host', [self.ctc_decoder(seq[:, :int(seq_len)]) for seq, seq_len in zip(o, olens)], None)

    def collect_strings(self, handle) -> List[str]:
        kind, h, eng = handle
        lut = self._codec_lut() if kind == 'device' else None
        if lut is not None:
            # device decode + a 1:1 codec: label arrays -> characters by one table lookup per line (the record lists of `predict_labels`
            # and the codec's tuple walk cost 0.26 ms per 32 lines on the host, after the GPU had finished: a fifth of the call)
            size = lut.shape[0]
            return [''.join(lut[np.minimum(lab, size - 1)].tolist()) for lab in eng.collect_labels(h)]
        records = eng.collect(h) if kind == 'device' else h
        return [''.join(x[0] for x in self.codec.decode(locs)) for locs in records]

    def step(self, batch: Dict, with_grad: bool = False) -> Dict:
        """The reference's `RecognitionModel._step` (model.py:129-145) on a batch dict {'image' (N,1,H,W), 'seq_lens' (N),
        'target' (sum target_lens,) concatenated labels, 'target_lens' (N)}: forward, then the criterion
        `nn.CTCLoss(reduction='sum', zero_infinity=True)` on `log_softmax(probits)` -- on the device, without materialising the
        log-probabilities.  Returns {'loss' (0-dim device tensor), 'probits', 'output_lens'} like the reference, plus 'nll'
        (per-line terms of the sum) and, with_grad, 'grad_probits' = d loss / d probits: what autograd hands to the decoder's
        backward in `training_step` (model.py:147-152).  Eval-mode forward (BatchNorm running statistics, no dropout): this is the
        reference's `validation_step` forward (model.py:154-156); the encoder's backward is not part of this library yet."""
        probits, out_lens = self.forward(batch['image'], batch['seq_lens'])
        nll, grad = self._engine.ctc_loss(probits, out_lens.numpy(), torch.as_tensor(batch['target']).cpu().numpy(),
                                          torch.as_tensor(batch['target_lens']).cpu().numpy(), with_grad=with_grad)
        out = {'loss': nll.sum(), 'probits': probits, 'output_lens': out_lens, 'nll': nll}
        if with_grad:
            out['grad_probits'] = grad
        return out

    def training_step(self, batch: Dict, batch_idx: int = 0) -> torch.Tensor:
        """The reference's `RecognitionModel.training_step` (model.py:147-152): train-mode forward (BatchNorm batch statistics, dropout
        with the constructor's probabilities), summed CTC loss -- returned as a DIFFERENTIABLE 0-dim device tensor: `loss.backward()`
        leaves `.grad` on every parameter of `self.nn` that requires grad, and any torch optimizer / Lightning loop drives the step
        (model.py:283-289).  Forward and backward run in libcocr_hip.so (conformer_ocr_amd/autograd.py); fp32, or bf16-rounded
        matmul operands with `self.matmul_precision = 'medium'` (the reference's cli/train.py:252)."""
        if not any(p.requires_grad for p in self.nn.parameters()):
            raise RuntimeError('no parameter of net.nn requires grad: call net.nn.requires_grad_(True) (the holders are created frozen for inference)')
        from .autograd import training_step
        return training_step(self, batch)

    def predict_labels(self, line: torch.tensor, lens: torch.Tensor = None) -> List[List[Tuple[int, int, int, float]]]:
        """
        Forward pass on a (N, C, H, W) batch; returns per line a list of tuples
        (class, start, end, max) (pred.py:166-178).
        """
        return self._label_records(line, lens)

    # ------------------------------------------------------------------ forced alignment (conformer_ocr_amd/align.py)
    def _align_labels_async(self, line: torch.Tensor, lens: torch.Tensor, targets, target_lens):
        """Forward + `cocr_ctc_align` enqueued on the current stream.  A line of more than 255 labels (the kernel's bound) is aligned
        by `align.viterbi_align` on its own logits when the handle is collected; the device sees it without labels."""
        from .align import MAX_DEVICE_LABELS
        o, olens = self.forward(line, lens)
        eng = self._engine             # (a re-pack may replace `self._engine` before the collect)
        olens = olens.numpy()
        tl = np.asarray(target_lens, dtype=np.int64).reshape(-1)
        tg = np.asarray(targets, dtype=np.int64).reshape(-1)
        if int(tl.sum()) != tg.shape[0]:
            raise ValueError('targets must hold sum(target_lens) labels')
        offs = np.concatenate([[0], np.cumsum(tl)])
        long_lines = {int(n): tg[offs[n]:offs[n + 1]] for n in np.nonzero(tl > MAX_DEVICE_LABELS)[0]}
        if long_lines:
            keep = np.ones(tg.shape[0], dtype=bool)
            for n in long_lines:
                keep[offs[n]:offs[n + 1]] = False
            tg, tl = tg[keep], np.where(tl > MAX_DEVICE_LABELS, 0, tl)
        return eng, eng.ctc_align_async(o, olens, tg, tl), o, olens, long_lines

    def _collect_align_labels(self, pending):
        from .align import viterbi_align
        eng, handle, o, olens, long_lines = pending
        out = eng.collect_align(handle)
        for n, labels in long_lines.items():
            out[n] = viterbi_align(o[n, :int(olens[n])].transpose(0, 1).cpu().numpy(), labels)
        return out

    def align_labels(self, line: torch.Tensor, lens: torch.Tensor, targets, target_lens):
        """Forced alignment of known label sequences: forward pass on a (N, C, H, W) batch, then per line the best path of its labels
        (`targets`: the batch's concatenated labels, `target_lens` (N)) through the frames.  Returns per line ([(label, start, end,
        conf)] -- one record per label -- or None where the labels do not fit the frames, the path's log-probability)."""
        return self._collect_align_labels(self._align_labels_async(line, lens, targets, target_lens))

    def align_async(self, line: torch.Tensor, lens: torch.Tensor, texts):
        """`align` split in two for pipelined callers (`align.align_pages`): returns a handle for `collect_align`."""
        from .align import encode_text
        enc = [encode_text(self.codec, t) for t in texts]
        labels = [l for lab, _ in enc for l in lab]
        return self._align_labels_async(line, lens, labels, [len(lab) for lab, _ in enc]), [sk for _, sk in enc]

    def collect_align(self, handle) -> List[Dict]:
        from .align import line_result
        pending, skipped = handle
        olens = pending[3]
        return [line_result(self.codec, recs, score, olens[n], skipped[n])
                for n, (recs, score) in enumerate(self._collect_align_labels(pending))]

    def align(self, line: torch.Tensor, lens: torch.Tensor, texts) -> List[Dict]:
        """Forced alignment of transcriptions: `texts` (one string per line) are encoded with `self.codec.encode` and placed on the
        lines' frames.  Returns per line {'chars': [(char, start, end, conf)] or None where the text does not fit the frames,
        'score': the path's log-probability, 'frames': the line's output length, 'skipped': the characters the codec cannot encode}."""
        return self.collect_align(self.align_async(line, lens, texts))

    # ------------------------------------------------------------------ keyword spotting (conformer_ocr_amd/search.py)
    def spot_labels_async(self, line: torch.Tensor, lens: torch.Tensor, queries, hits: int = 1, min_score: float = -np.inf):
        """Forward + `cocr_ctc_spot` enqueued on the current stream; returns a handle for `collect_spot_labels`.  A query of more than
        255 labels (the kernel's bound) is searched by `search.spot_host` on the lines' own logits when the handle is collected."""
        from .search import MAX_DEVICE_HITS, MAX_DEVICE_LABELS
        queries = [[int(l) for l in q] for q in queries]
        if not queries or not all(queries):
            raise ValueError('no query, or an empty one')
        if not 1 <= int(hits) <= MAX_DEVICE_HITS:
            raise ValueError(f'hits must lie in 1..{MAX_DEVICE_HITS}')
        o, olens = self.forward(line, lens)
        eng = self._engine             # (a re-pack may replace `self._engine` before the collect)
        olens = olens.numpy()
        short = [i for i, q in enumerate(queries) if len(q) <= MAX_DEVICE_LABELS]
        handle = eng.ctc_spot_async(o, olens, [queries[i] for i in short], hits, min_score) if short else None
        return eng, handle, o, olens, queries, short, int(hits), float(min_score)

    def collect_spot_labels(self, pending):
        """Waits for a `spot_labels_async` handle: (per line, per query [(start, end, score)], the lines' output lengths)."""
        from .search import spot_host
        eng, handle, o, olens, queries, short, hits, min_score = pending
        out = [[[] for _ in queries] for _ in range(o.shape[0])]
        if handle is not None:
            for n, per_query in enumerate(eng.collect_spot(handle)):
                for i, spots in zip(short, per_query):
                    out[n][i] = spots
        long_queries = sorted(set(range(len(queries))) - set(short))
        if long_queries:
            host = o.cpu().numpy()
            for n in range(o.shape[0]):
                x = host[n, :int(olens[n])].T
                for i in long_queries:
                    out[n][i] = spot_host(x, queries[i], hits, min_score)
        return out, olens

    def spot_labels(self, line: torch.Tensor, lens: torch.Tensor, queries, hits: int = 1, min_score: float = -np.inf):
        """Keyword spotting of label sequences: forward pass on a (N, C, H, W) batch, then per line and per query up to `hits`
        non-overlapping occurrences [(start, end, score)], best first (`search.spot_host` is the definition: score is the log-ratio
        of the query's best path over frames start..end to the unconstrained best path there, 0 when the query is what is read
        there).  `min_score`: occurrences below it are not reported."""
        return self.collect_spot_labels(self.spot_labels_async(line, lens, queries, hits, min_score))[0]

    def spot(self, line: torch.Tensor, lens: torch.Tensor, texts, hits: int = 1, min_score: float = -np.inf) -> Dict:
        """Keyword spotting of strings: `texts` are encoded with `self.codec.encode`.  Returns {'hits': per line, per text
        [(start, end, score)] -- empty for a text that is not searched --, 'frames': the lines' output lengths, 'skipped': per text the
        characters the codec cannot encode ('' where the text was searched; a text with such characters, or one that encodes to
        nothing, is not searched)}."""
        from .align import encode_text
        texts = list(texts)
        enc = [encode_text(self.codec, t) for t in texts]
        searched = [i for i, (lab, sk) in enumerate(enc) if lab and not sk]
        skipped = ['' if lab and not sk else (sk or t) for t, (lab, sk) in zip(texts, enc)]
        if not searched:
            o, olens = self.forward(line, lens)
            return {'hits': [[[] for _ in texts] for _ in range(o.shape[0])], 'frames': [int(l) for l in olens], 'skipped': skipped}
        found, olens = self.collect_spot_labels(self.spot_labels_async(line, lens, [enc[i][0] for i in searched], hits, min_score))
        out = [[[] for _ in texts] for _ in found]
        for n, per_query in enumerate(found):
            for i, spots in zip(searched, per_query):
                out[n][i] = spots
        return {'hits': out, 'frames': [int(l) for l in olens], 'skipped': skipped}

    # ------------------------------------------------------------------ pattern spotting (conformer_ocr_amd/pattern.py)
    def spot_patterns_async(self, line: torch.Tensor, lens: torch.Tensor, patterns, hits: int = 1, min_score: float = -np.inf,
                            ignore_case: bool = False):
        """Forward + the pattern search enqueued on the current stream; returns a handle for `collect_spot_patterns`.  `patterns`:
        regular expressions (compiled with `pattern.compile_pattern` over `self.codec`) or `pattern.PatternGraph`s.  A pattern whose
        graph is a plain chain goes through `cocr_ctc_spot` (the same result, at a string's cost), every other one through
        `cocr_ctc_spot_pattern`.  ValueError: a pattern the codec cannot express, or one `compile_pattern` refuses."""
        from .pattern import PatternGraph, compile_pattern
        from .search import MAX_DEVICE_HITS, MAX_DEVICE_LABELS
        graphs = [p if isinstance(p, PatternGraph) else compile_pattern(p, self.codec, ignore_case) for p in patterns]
        bad = [g.text for g in graphs if g.skipped or not g.P]
        if bad or not graphs:
            raise ValueError(f'patterns the codec cannot express: {bad}' if bad else 'no pattern')
        if not 1 <= int(hits) <= MAX_DEVICE_HITS:
            raise ValueError(f'hits must lie in 1..{MAX_DEVICE_HITS}')
        o, olens = self.forward(line, lens)
        eng = self._engine             # (a re-pack may replace `self._engine` before the collect)
        olens = olens.numpy()
        chains = [i for i, g in enumerate(graphs) if g.is_chain and g.P <= MAX_DEVICE_LABELS]
        rest = [i for i in range(len(graphs)) if i not in set(chains)]
        h_chain = eng.ctc_spot_async(o, olens, [graphs[i].labels for i in chains], hits, min_score) if chains else None
        h_graph = eng.ctc_spot_pattern_async(o, olens, [graphs[i] for i in rest], hits, min_score) if rest else None
        return eng, h_chain, h_graph, o, olens, graphs, chains, rest

    def collect_spot_patterns(self, pending):
        """Waits for a `spot_patterns_async` handle: (per line, per pattern [(start, end, score, labels)] -- `labels`: the label
        sequence the hit matched (`pattern.match_host` on the line's own logits) --, the lines' output lengths, the graphs)."""
        from .pattern import match_host
        eng, h_chain, h_graph, o, olens, graphs, chains, rest = pending
        out = [[[] for _ in graphs] for _ in range(o.shape[0])]
        if h_chain is not None:
            for n, per_query in enumerate(eng.collect_spot(h_chain)):
                for i, spots in zip(chains, per_query):
                    out[n][i] = [(st, en, sc, graphs[i].labels) for st, en, sc in spots]
        if h_graph is not None:
            found = eng.collect_spot_pattern(h_graph)
            host = o.cpu().numpy() if any(spots for per in found for spots in per) else None
            for n, per_pattern in enumerate(found):
                for i, spots in zip(rest, per_pattern):
                    out[n][i] = [(st, en, sc, match_host(host[n, :int(olens[n])].T, graphs[i], st, en, fin)) for st, en, sc, fin in spots]
        return out, olens, graphs

    def spot_patterns(self, line: torch.Tensor, lens: torch.Tensor, patterns, hits: int = 1, min_score: float = -np.inf,
                      ignore_case: bool = False) -> Dict:
        """Pattern spotting: forward pass on a (N, C, H, W) batch, then per line and per pattern up to `hits` non-overlapping matches
        (`pattern.spot_pattern_host` is the definition).  Returns {'hits': per line, per pattern [(start, end, score, matched text)],
        'frames': the lines' output lengths}."""
        from .pattern import labels_text
        found, olens, _ = self.collect_spot_patterns(self.spot_patterns_async(line, lens, patterns, hits, min_score, ignore_case))
        return {'hits': [[[(st, en, sc, labels_text(self.codec, lab)) for st, en, sc, lab in spots] for spots in per] for per in found],
                'frames': [int(l) for l in olens]}

    # ------------------------------------------------------------------ search index (conformer_ocr_amd/index.py)
    def pack_posteriors_async(self, line: torch.Tensor, lens: torch.Tensor, keep: int = 8, step: float = 0.125):
        """Forward + `cocr_posterior_pack` + the read-back into pinned host memory enqueued on the current stream; returns a handle
        for `collect_packed`."""
        o, olens = self.forward(line, lens)
        classes, codes = self._engine.posterior_pack(o, olens.numpy(), keep, step)
        host = (torch.empty(classes.shape, dtype=classes.dtype).pin_memory(), torch.empty(codes.shape, dtype=codes.dtype).pin_memory())
        host[0].copy_(classes, non_blocking=True)
        host[1].copy_(codes, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(o.device))
        return host, ev, olens.numpy(), (o, classes, codes)

    def collect_packed(self, handle):
        """Waits for a `pack_posteriors_async` handle: per line (classes (out_len, keep) uint16, codes (out_len, keep) uint8)."""
        host, ev, olens, _ = handle
        ev.synchronize()
        cls, cod = host[0].numpy(), host[1].numpy()
        return [(cls[n, :int(l)].copy(), cod[n, :int(l)].copy()) for n, l in enumerate(olens)]

    def pack_posteriors(self, line: torch.Tensor, lens: torch.Tensor, keep: int = 8, step: float = 0.125):
        """The pruned, quantised posteriors of a (N, C, H, W) batch (`index.pack_host` is the definition): forward pass, then per
        line (classes, codes) cut to the line's output length.  keep and step are placeholders, not tuned on real material."""
        return self.collect_packed(self.pack_posteriors_async(line, lens, keep, step))

    @classmethod
    def load_safetensors(cls, path, **kwargs):
        """
        Loads a safetensors archive: tar with `metadata.json` {codec, hyper_params} and
        `model.safetensors` = `nn.state_dict()` (pred.py:180-195).
        """
        import safetensors.torch
        with tarfile.open(path, 'r') as tf:
            metadata = json.load(tf.extractfile('metadata.json'))
            if 'codec' not in metadata:
                raise ValueError('No codec in metadata record')
            codec = PytorchCodec(metadata['codec'])
            if 'hyper_params' not in metadata:
                raise ValueError('No hyperparameters in metadata record')
            net = cls(**{**metadata['hyper_params'], **kwargs}, codec=codec)
            weights = safetensors.torch.load(tf.extractfile('model.safetensors').read())
        net.nn.load_state_dict(weights)
        return net.eval()

    @classmethod
    def load_checkpoint(cls, path, **kwargs):
        """
        Loads a lightning checkpoint (pred.py:197-210): `state_dict` (keys `nn.encoder.*`,
        `nn.decoder.*`), `hyper_parameters`, `TextLineDataModule.codec`.
        """
        state_dict = torch.load(path, map_location='cpu', weights_only=True)
        if 'TextLineDataModule' not in state_dict:
            raise ValueError('Checkpoint does not contain data module state.')
        codec = PytorchCodec(state_dict['TextLineDataModule']['codec'])
        if 'hyper_parameters' not in state_dict:
            raise ValueError('No hyperparameters in state_dict')
        net = cls(**{**state_dict['hyper_parameters'], **kwargs}, codec=codec)
        net.load_state_dict(state_dict['state_dict'], strict=False)
        return net.eval()


def save_safetensors(net: PytorchRecognitionModel, path, extra_metadata: Optional[Dict] = None) -> None:
    """Writes the archive format `load_safetensors` reads (the reference's converter, pred.py:213-254,
    does not run: SURVEY A.4)."""
    import safetensors.torch
    hp = net.hparams_record.as_dict()
    hp.update(input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1)
    meta = {'codec': net.codec.c2l, 'hyper_params': hp}
    meta.update(extra_metadata or {})
    blob = safetensors.torch.save({k: v.detach().cpu().contiguous() for k, v in net.nn.state_dict().items()})
    mj = json.dumps(meta).encode()
    with tarfile.open(path, 'w') as tf:
        for name, data in (('model.safetensors', blob), ('metadata.json', mj)):
            ti = tarfile.TarInfo(name)
            ti.size = len(data)
            tf.addfile(ti, io.BytesIO(data))


def resize_output(net: PytorchRecognitionModel, new_codec: PytorchCodec, row_map, seed: int = 0) -> None:
    """Output-layer surgery after `codec.resize_codec`, in place: `net.nn['decoder']` becomes a Linear of `len(row_map)` classes (frozen
    like the constructor's) whose row j is the old layer's row `row_map[j]` bit for bit, or, for row_map[j] == -1, the fresh row
    `synth.output_row(seed, c, encoder_dim)` of the grapheme c that `new_codec` labels j; `net.codec` and `net.hparams_record` follow.
    The device model re-packs at the next call (`_signature` sees the replaced sub-module)."""
    import dataclasses
    from .synth import output_row
    old = net.nn['decoder']
    row_map = np.asarray(row_map, dtype=np.int64).reshape(-1)
    n_old, fan_in = old.weight.shape
    if row_map.shape[0] < 1 or row_map[0] != 0:
        raise ValueError('row_map[0] must be 0: the blank keeps its row')
    if row_map.max() >= n_old or row_map.min() < -1:
        raise ValueError(f'row_map names rows outside the output layer\'s {n_old}')
    if new_codec.max_label >= row_map.shape[0]:
        raise ValueError(f'the codec uses label {new_codec.max_label}, row_map has {row_map.shape[0]} rows')
    w_old, b_old = old.weight.detach().cpu().float().numpy(), old.bias.detach().cpu().float().numpy()
    w, b = np.zeros((row_map.shape[0], fan_in), dtype=np.float32), np.zeros(row_map.shape[0], dtype=np.float32)
    for j, r in enumerate(row_map):
        if r >= 0:
            w[j], b[j] = w_old[r], b_old[r]
            continue
        c = new_codec.l2c.get((j,))
        if c is None:
            raise ValueError(f'row {j} is new, but no grapheme of the codec has the label sequence [{j}]')
        w[j], b[j] = output_row(seed, c, fan_in)
    dec = nn.Linear(fan_in, row_map.shape[0], bias=True)
    with torch.no_grad():
        dec.weight.copy_(torch.from_numpy(w))
        dec.bias.copy_(torch.from_numpy(b))
    dec = dec.to(device=old.weight.device, dtype=old.weight.dtype)
    for p in dec.parameters():
        p.requires_grad_(False)
    net.nn['decoder'] = dec
    net.codec = new_codec
    net.hparams_record = dataclasses.replace(net.hparams_record, num_classes=int(row_map.shape[0]))


def average_checkpoints(paths, num_checkpoints: Optional[int] = None) -> Dict:
    """The reference's `avg_ckpts` (cli/train.py:37-98): element-wise mean of the `state_dict`s of the last `num_checkpoints`
    checkpoints of `paths` (sorted by name like the reference's glob); everything else is taken from the first of them.
    Floating tensors: sum, then in-place division; integer tensors (BatchNorm `num_batches_tracked`): floor division;
    half tensors are summed in float32; a checkpoint whose key list differs raises KeyError.  Returns the averaged checkpoint
    dict (`torch.save` it, or hand `['state_dict']` to `load_state_dict`)."""
    import collections
    ckpts = sorted(str(p) for p in paths)
    if num_checkpoints is not None:
        if num_checkpoints < 2:
            raise ValueError('at least 2 checkpoints are averaged')
        if len(ckpts) < num_checkpoints:
            raise ValueError(f'Less checkpoints found than requested for averaging ({len(ckpts)} < {num_checkpoints})')
        ckpts = ckpts[-num_checkpoints:]
    params, keys, new_state = collections.OrderedDict(), None, None
    for fpath in ckpts:
        state = torch.load(fpath, map_location='cpu', weights_only=True)
        if new_state is None:
            new_state = state
        sd = state['state_dict']
        if keys is None:
            keys = list(sd.keys())
        elif keys != list(sd.keys()):
            raise KeyError(f'For checkpoint {fpath}, expected list of params: {keys}, but found: {list(sd.keys())}')
        for k in keys:
            p = sd[k]
            if p.dtype == torch.float16:
                p = p.float()
            if k not in params:
                params[k] = p.clone()
            else:
                params[k] += p
    for k, v in params.items():
        if v.is_floating_point():
            v.div_(len(ckpts))
        else:
            v //= len(ckpts)
    new_state['state_dict'] = params
    return new_state
