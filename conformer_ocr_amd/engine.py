"""Thin Python handle over a `cocr_model` (include/cocr.h).  torch is used only to own device
memory and streams; every computation is a call through the C ABI."""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .spec import HParams

DTYPES = {'bf16': _lib.BF16, 'bfloat16': _lib.BF16, 'fp32': _lib.F32, 'f32': _lib.F32, 'float32': _lib.F32}
_OPTIMIZER_NAMES = {v: k for k, v in _lib.OPTIMIZERS.items()}


def _stream_ptr(device: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _dp(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device (or pinned host) address of a tensor for a `void *` argument, None -> NULL; the declared argtypes convert the int."""
    return None if t is None else t.data_ptr()


_I32P, _I64P = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
_I32, _F32 = torch.int32, torch.float32


def _hp(a: Optional[np.ndarray], ptr=_I32P):
    """Pointer to a contiguous host array's elements (int32 unless `ptr` names another pointer type), None -> NULL."""
    return None if a is None else a.ctypes.data_as(ptr)


def _i32(values) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(values, dtype=np.int32).reshape(-1))


def _target_arrays(N: int, lens: np.ndarray, targets, label_lens, what: str = 'out_lens'):
    """Beside `HipRecognizer._lattice_args`, for the calls that take a transcription: the contiguous int32 host vectors (label lens,
    labels) of N lines whose `lens` that helper (or `train_step`) has made."""
    tl, tg = _i32(label_lens), _i32(targets)
    if lens.shape[0] != N or tl.shape[0] != N:
        raise ValueError(f'{what} and label_lens need one entry per line')
    if int(tl.sum()) != tg.shape[0]:
        raise ValueError('targets must hold sum(label_lens) labels')
    return tl, tg


def _mem_view(owner, ptr: int, n: int, typestr: str, device: torch.device) -> torch.Tensor:
    """`n` elements of library-owned device memory as a torch view; the view keeps `owner` (the model) alive."""
    class _Mem:
        __cuda_array_interface__ = {'shape': (n,), 'typestr': typestr, 'data': (ptr, False), 'version': 2}
        keep = owner
    return torch.as_tensor(_Mem(), device=device)


class _Handle:
    """An enqueued call whose outputs land in pinned host memory: the pool `key` its buffers `host` go back to, the event `ev` recorded
    behind the call, what must stay alive until then (`keep`), and the values its `collect_*` reads (`meta`).  Indexable in that
    order, for callers that look at the raw buffers."""
    __slots__ = ('key', 'host', 'ev', 'keep', 'meta')

    def __init__(self, key, host, ev, keep, meta):
        self.key, self.host, self.ev, self.keep, self.meta = key, host, ev, keep, meta

    def __getitem__(self, i):
        return getattr(self, self.__slots__[i])


_LAST_WRITER: Dict[int, int] = {}         # logits buffer address -> sequence number of the last `forward` (of any engine) that wrote it


class HipRecognizer:
    """One packed model on one GPU."""
    _WRITE_SEQ = 0

    def __init__(self, hp: HParams, device: torch.device, compute_dtype: str = 'bf16'):
        if compute_dtype not in DTYPES:
            raise ValueError(f'compute_dtype must be one of {sorted(DTYPES)}')
        self.lib = _lib.load()
        self.hp = hp
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('the HIP recognizer runs on a GPU device only (no CPU fallback)')
        self.dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device('cuda', self.dev_index)
        self.compute_dtype = compute_dtype
        chp = _lib.HParamsC(num_classes=hp.num_classes, height=hp.height, encoder_dim=hp.encoder_dim,
                            num_encoder_layers=hp.num_encoder_layers, num_attention_heads=hp.num_attention_heads,
                            feed_forward_expansion_factor=hp.feed_forward_expansion_factor,
                            conv_expansion_factor=hp.conv_expansion_factor, conv_kernel_size=hp.conv_kernel_size,
                            half_step_residual=int(bool(hp.half_step_residual)),
                            subsampling_conv_channels=hp.subsampling_conv_channels,
                            subsampling_factor=hp.subsampling_factor)
        h = C.c_void_p()
        _lib.check(self.lib.cocr_create(C.byref(chp), self.dev_index, C.byref(h)))
        self._h = h
        self.ready = False
        self._pinned = {}

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            try:
                self.lib.cocr_destroy(h)
            except Exception:
                pass

    # ---- weights -------------------------------------------------------------------------------
    def load_state(self, state: Mapping[str, 'np.ndarray | torch.Tensor'], strict: bool = True) -> None:
        """`state`: keys of `nn.state_dict()` (`encoder.*`, `decoder.*`)."""
        for name, val in state.items():
            if name.endswith('num_batches_tracked'):
                continue
            arr = val.detach().cpu().float().numpy() if isinstance(val, torch.Tensor) else np.asarray(val, dtype=np.float32)
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (C.c_int64 * max(arr.ndim, 1))(*arr.shape)
            _lib.check(self.lib.cocr_set_tensor(self._h, name.encode(), _hp(arr, C.c_void_p), _lib.F32, arr.ndim, shape))
        if strict:
            buf = C.create_string_buffer(1 << 16)
            n = self.lib.cocr_missing_tensors(self._h, buf, len(buf))
            if n:
                raise RuntimeError('Missing key(s) in state_dict: ' + ', '.join(buf.value.decode().split()))

    def finalize(self) -> None:
        _lib.check(self.lib.cocr_finalize(self._h, DTYPES[self.compute_dtype]))
        self.ready = True

    def share_weights(self, owner: 'HipRecognizer') -> None:
        """This packed copy reads `owner`'s weights and tables instead of its own (include/cocr.h: cocr_share_weights); keeps `owner` alive."""
        _lib.check(self.lib.cocr_share_weights(self._h, owner._h))
        self._weights_owner = owner
        self.ready = True

    def finalize_empty(self) -> None:
        _lib.check(self.lib.cocr_finalize_empty(self._h, DTYPES[self.compute_dtype]))
        self.ready = True

    def weight_blob(self) -> torch.Tensor:
        """The packed device blob as a uint8 torch view (for an RCCL broadcast through torch.distributed)."""
        return _mem_view(self, *self._blob(), '|u1', self.device)

    def _blob(self) -> Tuple[int, int]:
        p, n = C.c_void_p(), C.c_size_t()
        _lib.check(self.lib.cocr_weight_blob(self._h, C.byref(p), C.byref(n)))
        return p.value, int(n.value)

    def blob_nbytes(self) -> int:
        return self._blob()[1]

    def export_blob(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Packed weights copied into a torch-owned uint8 tensor (the buffer a collective runs on)."""
        n = self.blob_nbytes()
        buf = out if out is not None else torch.empty(n, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_blob_export(self._h, _dp(buf), n, _stream_ptr(self.device)))
        return buf

    def import_blob(self, buf: torch.Tensor) -> None:
        if buf.dtype != torch.uint8 or buf.device != self.device or not buf.is_contiguous():
            raise ValueError('blob buffer must be a contiguous uint8 tensor on the model device')
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_blob_import(self._h, _dp(buf), buf.numel(), _stream_ptr(self.device)))

    # ---- compute -------------------------------------------------------------------------------
    def out_len(self, w: int) -> int:
        return int(self.lib.cocr_out_len(int(w), self.hp.subsampling_factor))

    def reserve(self, n: int, w: int) -> None:
        _lib.check(self.lib.cocr_reserve(self._h, int(n), int(w)))

    def set_graph(self, on: bool) -> None:
        """hipGraph replay of repeated identical forwards (same input / output buffers): see include/cocr.h."""
        _lib.check(self.lib.cocr_set_graph(self._h, int(on)))

    def set_chain_rows(self, rows: int) -> None:
        """Rows per workgroup of the row-chain kernels (0 = automatic): see include/cocr.h."""
        _lib.check(self.lib.cocr_set_chain_rows(self._h, int(rows)))

    def chain_rows(self, n: int, w: int) -> int:
        """Rows per workgroup the next forward of an (n, H, w) batch runs its row-chain launches with: see include/cocr.h."""
        rows = C.c_int()
        _lib.check(self.lib.cocr_get_chain_rows(self._h, int(n), int(w), C.byref(rows)))
        return int(rows.value)

    def forward(self, lines: torch.Tensor, lens: Sequence[int], out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, np.ndarray]:
        """lines: (N,H,W) float32 or uint8 on this device, contiguous.  Returns (logits (N,T,ncls) f32 device, out_lens int32 host).
        `out`: optional preallocated logits buffer (keeps the output address fixed for graph replay)."""
        if not self.ready:
            raise RuntimeError('model not finalized')
        if lines.device != self.device:
            raise RuntimeError(f'line batch lives on {lines.device}, the model on {self.device}')
        if lines.dim() != 3:
            raise ValueError('expected a (N,H,W) batch')
        if lines.dtype == torch.uint8:
            ldt = _lib.U8
        else:
            lines = lines.float()
            ldt = _lib.F32
        lines = lines.contiguous()
        N, H, W = lines.shape
        in_lens = _i32(lens)
        if in_lens.shape[0] != N:
            raise ValueError('lens must have one entry per line')
        out_lens = np.zeros(N, dtype=np.int32)
        T = self.out_len(W)
        logits = out if out is not None else torch.empty((N, T, self.hp.num_classes), dtype=torch.float32, device=self.device)
        if logits.shape != (N, T, self.hp.num_classes) or logits.dtype != torch.float32 or not logits.is_contiguous():
            raise ValueError('out must be a contiguous float32 (N,T,num_classes) tensor')
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_forward(self._h, _dp(lines), ldt, N, H, W, _hp(in_lens), _dp(logits), _hp(out_lens), _stream_ptr(self.device)))
        # The decoder epilogue's per-frame argmax belongs to THESE values: to this tensor object (not to its address: the caching
        # allocator hands a freed address to the next same-sized tensor), at this version, and only while no other engine's forward
        # has written the same buffer since (writes through the C ABI do not bump `_version`: `_LAST_WRITER` records them).
        HipRecognizer._WRITE_SEQ += 1
        if len(_LAST_WRITER) > 4096:
            _LAST_WRITER.clear()
        _LAST_WRITER[logits.data_ptr()] = HipRecognizer._WRITE_SEQ
        self._fresh_logits = (weakref.ref(logits), logits._version, HipRecognizer._WRITE_SEQ)
        return logits, out_lens

    def _argmax_is_fresh(self, logits: torch.Tensor) -> bool:
        ref, ver, seq = getattr(self, '_fresh_logits', None) or (None, -1, -1)
        return ref is not None and ref() is logits and logits._version == ver and _LAST_WRITER.get(logits.data_ptr()) == seq

    # ---- calls on a lattice: one argument check, one path for outputs in pinned host memory ----------
    def _lattice_args(self, logits: torch.Tensor, out_lens=None, name: str = 'logits'):
        """The argument check of every call that takes (N,T,ncls) values and their valid lengths: (contiguous logits, N, T, ncls, int32
        host vector of the lengths -- None without `out_lens`).  RuntimeError for device, dtype or rank, ValueError for the count."""
        if logits.device != self.device or logits.dtype != torch.float32 or logits.dim() != 3:
            raise RuntimeError(f'{name} must be a float32 (N,T,num_classes) tensor on the model device')
        logits = logits.contiguous()
        N, T, ncls = logits.shape
        lens = None if out_lens is None else _i32(out_lens)
        if lens is not None and lens.shape[0] != N:
            raise ValueError('out_lens needs one entry per line')
        return logits, N, T, ncls, lens

    def _enqueue(self, fn, lat, key, shapes, tail, head=(), keep=(), meta=None) -> _Handle:
        """Enqueues `fn(model, *head, logits, N, T, ncls, lens, *tail(*buffers), stream)` on the current stream, `lat` the checked
        arguments of `_lattice_args`, the buffers taken from the pool `key` or allocated as `shapes` says ((shape, dtype) each).  The
        kernels write their outputs STRAIGHT into that pinned host memory (device-visible): no device->host copy is enqueued.  A third
        hipMemcpyAsync D2H in flight (three batches on three streams, each queued behind its forward) blocked the host for a whole
        forward, 5.5 ms at every start of a run.  Returns the handle `_wait` and `_release` take; `meta` is for its `collect_*`."""
        pool = self._pinned.setdefault(key, [])
        with torch.cuda.device(self.device):
            host = pool.pop() if pool else tuple(torch.empty(s, dtype=d).pin_memory() for s, d in shapes)
            try:
                _lib.check(fn(self._h, *head, _dp(lat[0]), *lat[1:4], _hp(lat[4]), *tail(*host), _stream_ptr(self.device)))
            except Exception:
                pool.append(host)                                   # nothing was launched: the buffers go back
                raise
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
        return _Handle(key, host, ev, (lat[0],) + keep, meta)

    def _wait(self, handle: _Handle):
        handle.ev.synchronize()
        return handle.host

    def _release(self, handle: _Handle) -> None:
        self._pinned[handle.key].append(handle.host)

    def _decode_async(self, fn, logits: torch.Tensor, out_lens, extra=(), head=(), keep=()) -> _Handle:
        """Enqueues a decode kernel (greedy or a beam) on the current stream; returns a handle for `collect` / `collect_labels`."""
        fresh = self._argmax_is_fresh(logits)                        # of the caller's tensor: `.contiguous()` may make another
        lat = self._lattice_args(logits, out_lens)
        if not fresh:
            _lib.check(self.lib.cocr_forget_argmax(self._h))          # other logits, or edited in place since the forward: decode from the values
        N, T = lat[1], lat[2]
        return self._enqueue(fn, lat, (N, T), (((3, N, T), _I32), ((N, T), _F32), ((N,), _I32)),
                             lambda ints, conf, counts: (_dp(ints[0]), _dp(ints[1]), _dp(ints[2]), _dp(conf), _dp(counts), T, *extra), head, keep)

    def collect(self, handle) -> List[List[Tuple[int, int, int, float]]]:
        """Waits for a decode handle and builds the per-line (label, start, end, conf) lists."""
        host = self._wait(handle)
        ints_h, conf_h, cnt = host[0].numpy(), host[1].numpy(), host[2].numpy()
        # one conversion per array for the whole batch (per-line slices + tolist: 110 us for 32 lines, after the GPU has finished)
        cl = cnt.tolist()
        mx = max(cl) if cl else 0
        lab, st, en = ints_h[:, :, :mx].tolist()
        cf = conf_h[:, :mx].tolist()
        out = [list(zip(lab[n][:c], st[n][:c], en[n][:c], cf[n][:c])) for n, c in enumerate(cl)]
        self._release(handle)
        return out

    def collect_labels(self, handle) -> List[np.ndarray]:
        """Waits for a decode handle; per line the int32 label array only (copies: the pinned buffers go back to the pool) --
        what `predict_string` needs, without building four Python lists per line."""
        host = self._wait(handle)
        cl = host[2].numpy().tolist()
        mx = max(cl) if cl else 0
        block = host[0].numpy()[0, :, :mx].copy()
        self._release(handle)
        return [block[n, :c] for n, c in enumerate(cl)]

    def ctc_greedy_async(self, logits: torch.Tensor, out_lens) -> _Handle:
        return self._decode_async(self.lib.cocr_ctc_greedy, logits, out_lens)

    def ctc_greedy(self, logits: torch.Tensor, out_lens) -> List[List[Tuple[int, int, int, float]]]:
        return self.collect(self.ctc_greedy_async(logits, out_lens))

    def ctc_beam_async(self, logits: torch.Tensor, out_lens, beam: int = 16) -> _Handle:
        return self._decode_async(self.lib.cocr_ctc_beam, logits, out_lens, (int(beam),))

    def ctc_beam(self, logits: torch.Tensor, out_lens, beam: int = 16) -> List[List[Tuple[int, int, int, float]]]:
        return self.collect(self.ctc_beam_async(logits, out_lens, beam))

    def ctc_beam_lm_async(self, logits: torch.Tensor, out_lens, lm, beam: int = 16, classes: int = 8, alpha: float = 0.5, beta: float = 0.0,
                          score: Optional[torch.Tensor] = None) -> _Handle:
        """`cocr_ctc_beam_lm` (include/cocr.h) enqueued on the current stream: the beam search with the n-gram
        model `lm` (an `lm.NGramLM`; its tables are copied to this device once) in the ranking.  Returns a handle for `collect` /
        `collect_labels`.  `score`: an optional pinned or device float32 (N,2) tensor for (CTC log-probability, lmv) per line."""
        dlm = lm.to_device(self)
        return self._decode_async(self.lib.cocr_ctc_beam_lm, logits, out_lens, (int(beam), int(classes), float(alpha), float(beta), _dp(score)),
                                  head=(dlm.handle,), keep=(dlm, score))

    def ctc_beam_lm(self, logits: torch.Tensor, out_lens, lm, beam: int = 16, classes: int = 8, alpha: float = 0.5, beta: float = 0.0,
                    return_scores: bool = False):
        """Per line [(label, start, end, conf)]; with return_scores also a (N,2) float32 array: the CTC log-probability
        logaddexp(p_b, p_nb) of the returned prefix, and its language-model term lmv."""
        score = torch.empty((logits.shape[0], 2), dtype=torch.float32).pin_memory() if return_scores else None
        recs = self.collect(self.ctc_beam_lm_async(logits, out_lens, lm, beam, classes, alpha, beta, score))
        return (recs, score.numpy().copy()) if return_scores else recs

    def ctc_beam_nbest_async(self, logits: torch.Tensor, out_lens, beam: int = 16, nbest: int = 4, lm=None, classes: int = 8, alpha: float = 0.5,
                             beta: float = 0.0) -> _Handle:
        """`cocr_ctc_beam_nbest` (include/cocr.h) enqueued on the current stream: the first `nbest` prefixes of the
        final beam of `ctc_beam` (or, with `lm`, of `ctc_beam_lm`), each with its exact CTC log-probability and its raw n-gram sum.
        The records and scores land in pinned host memory, like the decoders'.  Returns a handle for `collect_nbest`."""
        lat = self._lattice_args(logits, out_lens)
        N, T, nbest = lat[1], lat[2], int(nbest)
        B = max(nbest, 1)
        dlm = lm.to_device(self) if lm is not None else None
        return self._enqueue(
            self.lib.cocr_ctc_beam_nbest, lat, ('nbest', N, T, B),
            (((3, N, B, T), _I32), ((N, B, T), _F32), ((N, B), _I32), ((N,), _I32), ((N, B, 2), _F32)),
            lambda ints, conf, counts, nhyp, scores: (int(beam), nbest, int(classes), float(alpha), float(beta), _dp(ints[0]), _dp(ints[1]),
                                                      _dp(ints[2]), _dp(conf), _dp(counts), _dp(nhyp), _dp(scores), T),
            head=(dlm.handle if dlm is not None else None,), keep=(dlm,))

    def collect_nbest(self, handle) -> List[List[Tuple[List[Tuple[int, int, int, float]], float, float]]]:
        """Waits for a `ctc_beam_nbest_async` handle; per line its hypotheses in beam order, each (records, logp, lm_logp)."""
        ints, conf, counts, nhyp, scores = (h.numpy() for h in self._wait(handle))
        out = []
        for n, nh in enumerate(nhyp.tolist()):
            hyps = []
            for j in range(nh):
                c = int(counts[n, j])
                lab, st, en = ints[:, n, j, :c].tolist()
                hyps.append((list(zip(lab, st, en, conf[n, j, :c].tolist())), float(scores[n, j, 0]), float(scores[n, j, 1])))
            out.append(hyps)
        self._release(handle)
        return out

    def ctc_beam_nbest(self, logits: torch.Tensor, out_lens, beam: int = 16, nbest: int = 4, lm=None, classes: int = 8, alpha: float = 0.5,
                       beta: float = 0.0):
        """Per line a list of hypotheses (records, logp, lm_logp): `nbest.nbest_host` on the device for the whole batch.  logp is NaN for
        a hypothesis of more than 255 labels."""
        return self.collect_nbest(self.ctc_beam_nbest_async(logits, out_lens, beam, nbest, lm, classes, alpha, beta))

    def ctc_loss(self, probits: torch.Tensor, out_lens, targets, label_lens, with_grad: bool = True):
        """nn.CTCLoss(reduction='sum', zero_infinity=True) on log_softmax(probits) (reference model.py:119,136-142) on the device.
        probits (N,T,ncls) float32 on this device; out_lens (N) valid frames; targets: the batch's concatenated 1-D label vector,
        label_lens (N) its per-line lengths (host sequences).  Returns (per-line nll (N) float32 device tensor -- 0 where no
        alignment exists --, d sum(nll) / d probits (N,T,ncls) or None); the reference's loss is `nll.sum()`.  Stream-ordered."""
        probits, N, T, ncls, lens = self._lattice_args(probits, out_lens, 'probits')
        tl, tg = _target_arrays(N, lens, targets, label_lens)
        nll = torch.empty((N,), dtype=torch.float32, device=self.device)
        grad = torch.empty_like(probits) if with_grad else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_ctc_loss(self._h, _dp(probits), N, T, ncls, _hp(lens), _hp(tg if tg.shape[0] else None), _hp(tl),
                                              _dp(nll), _dp(grad), _stream_ptr(self.device)))
        return nll, grad

    def distill_loss(self, student: torch.Tensor, teacher: torch.Tensor, out_lens, tau: float, grad: Optional[torch.Tensor] = None,
                     ctc_weight: float = 1.0, kd_weight: float = 1.0, with_grad: bool = True):
        """The distillation term of `distill.kd_loss_host` on the device (include/cocr.h: cocr_distill_loss).
        student, teacher (N,T,ncls) float32 logits on this device; out_lens (N) valid frames; tau the temperature.  Returns (per-line
        KD (N) float32 device tensor, gradient (N,T,ncls) or None).  grad=None: a new tensor kd_weight tau (q - p) (with_grad=False:
        the loss only).  grad given (contiguous, float32, the logits' shape): updated IN PLACE to ctc_weight grad + kd_weight tau (q - p)
        -- the two-term criterion on the gradient `ctc_loss` left there -- and returned.  Stream-ordered."""
        for t in (student, teacher):
            if t.device != self.device or t.dtype != torch.float32 or t.dim() != 3:
                raise RuntimeError('student and teacher must be float32 (N,T,num_classes) tensors on the model device')
        if student.shape != teacher.shape:
            raise ValueError(f'student logits are {tuple(student.shape)}, teacher logits {tuple(teacher.shape)}')
        student, teacher = student.contiguous(), teacher.contiguous()
        N, T, ncls = student.shape
        lens = _i32(out_lens)
        if lens.shape[0] != N:
            raise ValueError('out_lens needs one entry per line')
        accumulate = grad is not None
        if accumulate and (grad.device != self.device or grad.dtype != torch.float32 or grad.shape != student.shape or not grad.is_contiguous()):
            raise RuntimeError('grad must be a contiguous float32 tensor of the logits\' shape on the model device')
        if not accumulate and with_grad:
            grad = torch.empty_like(student)
        kd = torch.empty((N,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_distill_loss(self._h, _dp(student), _dp(teacher), N, T, ncls, _hp(lens), float(tau), _dp(kd), _dp(grad),
                                                  float(ctc_weight), float(kd_weight), int(accumulate), _stream_ptr(self.device)))
        return kd, grad

    # ---- forced alignment (include/cocr.h: cocr_ctc_align) ----------
    def ctc_align_async(self, logits: torch.Tensor, out_lens, targets, label_lens) -> _Handle:
        """Enqueues the forced alignment of every line's label sequence on the current stream, its outputs in pinned host memory;
        returns a handle for `collect_align`.  logits (N,T,ncls) float32 on this device; out_lens (N) valid frames; targets: the
        batch's concatenated 1-D label vector, label_lens (N) its per-line lengths (host sequences; at most 255 labels per line).
        Does not touch the forward's per-frame argmax: a `ctc_greedy` on the same logits afterwards still takes its shortcut."""
        lat = self._lattice_args(logits, out_lens)
        N = lat[1]
        tl, tg = _target_arrays(N, lat[4], targets, label_lens)
        cap = max(N, 1) * 255                                       # the kernel's bound on a line's labels
        return self._enqueue(self.lib.cocr_ctc_align, lat, ('align', N), (((2, cap), _I32), ((cap,), _F32), ((N,), _F32), ((N,), _I32)),
                             lambda ints, conf, score, counts: (_hp(tg if tg.shape[0] else None), _hp(tl), _dp(ints[0]), _dp(ints[1]), _dp(conf),
                                                                _dp(score), _dp(counts)), meta=(tg, tl))

    def collect_align(self, handle) -> List[Tuple[Optional[List[Tuple[int, int, int, float]]], float]]:
        """Waits for a `ctc_align_async` handle; per line ([(label, start, end, conf)] -- one record per label, in order -- or None
        where no alignment fits, the path's log-probability)."""
        host, (tg, tl) = self._wait(handle), handle.meta
        total = int(tg.shape[0])
        st, en = host[0].numpy()[:, :total].tolist()
        cf = host[1].numpy()[:total].tolist()
        sc, cnt = host[2].numpy().tolist(), host[3].numpy().tolist()
        lab = tg.tolist()
        out, at = [], 0
        for n, l in enumerate(tl.tolist()):
            out.append((list(zip(lab[at:at + l], st[at:at + l], en[at:at + l], cf[at:at + l])) if cnt[n] >= 0 else None, sc[n]))
            at += l
        self._release(handle)
        return out

    def ctc_align(self, logits: torch.Tensor, out_lens, targets, label_lens):
        return self.collect_align(self.ctc_align_async(logits, out_lens, targets, label_lens))

    # ---- text-to-page alignment (include/cocr.h: cocr_ctc_align_page) ----------
    def ctc_align_page_async(self, logits: torch.Tensor, out_lens, pages, targets, optional=None) -> _Handle:
        """Enqueues the alignment of every page's label sequence to the frames of its lines on the current stream, its outputs in
        pinned host memory; returns a handle for `collect_align_page`.  logits (N,T,ncls) float32 on this device; out_lens (N) valid
        frames; pages: per page the rows of `logits` that are its lines in reading order (a row in at most one page); targets: per
        page its labels (at most 4095); optional: per page one bool per label (None: none may be skipped).  Does not touch the
        forward's per-frame argmax."""
        lat = self._lattice_args(logits, out_lens)
        P = len(pages)
        if len(targets) != P or (optional is not None and len(optional) != P):
            raise ValueError('targets and optional need one entry per page')
        rows = [np.asarray(pg, dtype=np.int32).reshape(-1) for pg in pages]
        labs = [np.asarray(t, dtype=np.int32).reshape(-1) for t in targets]
        opts = [np.zeros(l.shape[0], dtype=np.uint8) if optional is None or optional[p] is None else
                np.asarray(optional[p]).astype(bool).astype(np.uint8).reshape(-1) for p, l in enumerate(labs)]
        if any(o.shape[0] != l.shape[0] for o, l in zip(opts, labs)):
            raise ValueError('optional needs one entry per label')
        i32 = np.int32
        line_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([r.shape[0] for r in rows])]).astype(i32))
        tl = np.ascontiguousarray(np.array([l.shape[0] for l in labs], dtype=i32))
        page_lines = np.ascontiguousarray(np.concatenate(rows + [np.zeros(0, i32)]).astype(i32))
        tg = np.ascontiguousarray(np.concatenate(labs + [np.zeros(0, i32)]).astype(i32))
        op = np.ascontiguousarray(np.concatenate(opts + [np.zeros(0, np.uint8)]).astype(np.uint8))

        def cap(n):
            return 1 << max(int(n) - 1, 0).bit_length()
        ct, cp, cl = cap(tg.shape[0]), cap(P), cap(page_lines.shape[0])
        return self._enqueue(
            self.lib.cocr_ctc_align_page, lat, ('align_page', ct, cp, cl), (((3, ct), _I32), ((ct,), _F32), ((cp,), _F32), ((cp,), _I32), ((cl,), _F32)),
            lambda ints, conf, score, counts, line_score: (P, _hp(line_off), _hp(page_lines), _hp(tg), _hp(tl), _hp(op, C.POINTER(C.c_uint8)),
                                                           _dp(ints[0]), _dp(ints[1]), _dp(ints[2]), _dp(conf), _dp(score), _dp(counts), _dp(line_score)),
            meta=(tg, tl, line_off))

    def collect_align_page(self, handle):
        """Waits for a `ctc_align_page_async` handle; per page ([(label, line, start, end, conf)] -- one record per label, a skipped
        optional label with line = start = end = -1 and conf 0 --, the page's score, the per-line scores as a float32 array), or
        (None, -inf, None) where the text does not fit: the returns of `align.viterbi_align_page`."""
        host, (tg, tl, line_off) = self._wait(handle), handle.meta
        total = int(tg.shape[0])
        ln, st, en = host[0].numpy()[:, :total].tolist()
        cf = host[1].numpy()[:total].tolist()
        sc, cnt = host[2].numpy().tolist(), host[3].numpy().tolist()
        ls = host[4].numpy()
        lab = tg.tolist()
        out, at = [], 0
        for p, l in enumerate(tl.tolist()):
            if cnt[p] >= 0:
                out.append((list(zip(lab[at:at + l], ln[at:at + l], st[at:at + l], en[at:at + l], cf[at:at + l])), sc[p],
                            ls[line_off[p]:line_off[p + 1]].copy()))
            else:
                out.append((None, sc[p], None))
            at += l
        self._release(handle)
        return out

    def ctc_align_page(self, logits: torch.Tensor, out_lens, pages, targets, optional=None):
        return self.collect_align_page(self.ctc_align_page_async(logits, out_lens, pages, targets, optional))

    # ---- keyword spotting (include/cocr.h: cocr_ctc_spot) ----------
    def ctc_spot_async(self, logits: torch.Tensor, out_lens, queries, hits: int = 1, min_score: float = -np.inf) -> _Handle:
        """Enqueues the search for every query in every line on the current stream, its outputs in pinned host memory; returns a
        handle for `collect_spot`.  logits (N,T,ncls) float32 on this device; out_lens (N) valid frames; queries: Q label sequences
        (1..255 labels each); hits: 1..8 per (line, query); min_score: the selection stops below it.  Does not touch the forward's
        per-frame argmax: a `ctc_greedy` on the same logits afterwards still takes its shortcut."""
        lat = self._lattice_args(logits, out_lens)
        qs = [np.asarray(q, dtype=np.int32).reshape(-1) for q in queries]
        N, Q, K = lat[1], len(qs), int(hits)
        ql = _i32([q.shape[0] for q in qs])
        qv = np.ascontiguousarray(np.concatenate(qs + [np.zeros(0, dtype=np.int32)]), dtype=np.int32)
        cells = max(N * Q, 1)
        cap = cells * min(max(K, 1), 8)
        return self._enqueue(self.lib.cocr_ctc_spot, lat, ('spot', cap, cells), (((2, cap), _I32), ((cap,), _F32), ((cells,), _I32)),
                             lambda ints, score, counts: (_hp(qv), _hp(ql), Q, K, float(min_score), _dp(ints[0]), _dp(ints[1]), _dp(score), _dp(counts)),
                             meta=(N, Q, K))

    def collect_spot(self, handle) -> List[List[List[Tuple[int, int, float]]]]:
        """Waits for a `ctc_spot_async` handle; per line, per query [(start, end, score)], best first."""
        host, (N, Q, K) = self._wait(handle), handle.meta
        st, en = host[0].numpy()[:, :N * Q * K].reshape(2, N, Q, K).tolist()
        sc = host[1].numpy()[:N * Q * K].reshape(N, Q, K).tolist()
        cnt = host[2].numpy()[:N * Q].reshape(N, Q).tolist()
        out = [[list(zip(st[n][q][:cnt[n][q]], en[n][q][:cnt[n][q]], sc[n][q][:cnt[n][q]])) for q in range(Q)] for n in range(N)]
        self._release(handle)
        return out

    def ctc_spot(self, logits: torch.Tensor, out_lens, queries, hits: int = 1, min_score: float = -np.inf):
        return self.collect_spot(self.ctc_spot_async(logits, out_lens, queries, hits, min_score))

    # ---- pattern spotting (include/cocr.h: cocr_ctc_spot_pattern) ----------
    def ctc_spot_pattern_async(self, logits: torch.Tensor, out_lens, graphs, hits: int = 1, min_score: float = -np.inf) -> _Handle:
        """Enqueues the search for every pattern in every line on the current stream, its outputs in pinned host memory; returns a
        handle for `collect_spot_pattern`.  logits (N,T,ncls) float32 on this device; out_lens (N) valid frames; graphs: Q
        `pattern.PatternGraph`s (1..256 label states, at most 4096 edges each; a chain is run as a graph like any other); hits: 1..8
        per (line, pattern); min_score: the selection stops below it.  Does not touch the forward's per-frame argmax."""
        lat = self._lattice_args(logits, out_lens)
        tabs = [g.tables() for g in graphs]
        N, Q, K = lat[1], len(tabs), int(hits)
        states = _i32([t[0].shape[0] for t in tabs])
        cls, flags, off, preds = (np.ascontiguousarray(np.concatenate([t[i] for t in tabs] + [np.zeros(0, dtype=np.int32)]), dtype=np.int32)
                                  for i in range(4))
        cells = max(N * Q, 1)
        cap = cells * min(max(K, 1), 8)
        return self._enqueue(self.lib.cocr_ctc_spot_pattern, lat, ('spot_pattern', cap, cells), (((3, cap), _I32), ((cap,), _F32), ((cells,), _I32)),
                             lambda ints, score, counts: (_hp(states), _hp(cls), _hp(flags), _hp(off), _hp(preds), Q, K, float(min_score),
                                                          _dp(ints[0]), _dp(ints[1]), _dp(score), _dp(ints[2]), _dp(counts)), meta=(N, Q, K))

    def collect_spot_pattern(self, handle, raw: bool = False):
        """Waits for a `ctc_spot_pattern_async` handle; per line, per pattern [(start, end, score, final state)], best first.  `raw`:
        the output arrays themselves, copies of (starts, ends, scores, finals (N,Q,hits), counts (N,Q))."""
        host, (N, Q, K) = self._wait(handle), handle.meta
        ints = host[0].numpy()[:, :N * Q * K].reshape(3, N, Q, K).copy()
        score = host[1].numpy()[:N * Q * K].reshape(N, Q, K).copy()
        counts = host[2].numpy()[:N * Q].reshape(N, Q).copy()
        self._release(handle)
        if raw:
            return ints[0], ints[1], score, ints[2], counts
        st, en, fi = ints.tolist()
        sc, cnt = score.tolist(), counts.tolist()
        return [[list(zip(st[n][q][:cnt[n][q]], en[n][q][:cnt[n][q]], sc[n][q][:cnt[n][q]], fi[n][q][:cnt[n][q]])) for q in range(Q)] for n in range(N)]

    def ctc_spot_pattern(self, logits: torch.Tensor, out_lens, graphs, hits: int = 1, min_score: float = -np.inf):
        return self.collect_spot_pattern(self.ctc_spot_pattern_async(logits, out_lens, graphs, hits, min_score))

    # ---- search index (include/cocr.h: cocr_posterior_pack / cocr_posterior_unpack) ----------
    def posterior_pack(self, logits: torch.Tensor, out_lens, keep: int = 8, step: float = 0.125) -> Tuple[torch.Tensor, torch.Tensor]:
        """Enqueues `index.pack_host` of every line on the current stream: (classes uint16, codes uint8), device tensors (N,T,keep);
        frames at or beyond out_lens[n] hold class 0 / code 255.  logits (N,T,ncls) float32 on this device.  Does not touch the
        forward's per-frame argmax."""
        from .index import inv_step
        cont, N, T, ncls, lens = self._lattice_args(logits, out_lens)
        inv = float(inv_step(step))
        K = max(int(keep), 0)
        classes = torch.empty((N, T, K), dtype=torch.uint16, device=self.device)
        codes = torch.empty((N, T, K), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_posterior_pack(self._h, _dp(cont), N, T, ncls, _hp(lens), int(keep), inv, _dp(classes), _dp(codes),
                                                    _stream_ptr(self.device)))
        return classes, codes

    def posterior_unpack(self, classes: torch.Tensor, codes: torch.Tensor, ncls: int, step: float = 0.125) -> torch.Tensor:
        """Enqueues `index.expand_host` on the current stream: packed (N,T,keep) device tensors -> the (N,T,ncls) float32 table
        `ctc_spot` takes.  An entry whose class is >= ncls is ignored."""
        if classes.device != self.device or codes.device != self.device or classes.dtype != torch.uint16 or codes.dtype != torch.uint8:
            raise RuntimeError('classes (uint16) and codes (uint8) must be tensors on the model device')
        if classes.dim() != 3 or classes.shape != codes.shape:
            raise ValueError('classes and codes must be (N,T,keep) tensors of one shape')
        classes, codes = classes.contiguous(), codes.contiguous()
        N, T, K = classes.shape
        step32 = float(np.float32(step))
        out = torch.empty((N, T, max(int(ncls), 0)), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_posterior_unpack(self._h, _dp(classes), _dp(codes), N, T, K, int(ncls), step32, _dp(out), _stream_ptr(self.device)))
        return out

    # ---- output-layer training step (include/cocr.h: cocr_decoder_backward / cocr_decoder_adamw) ----------
    def decoder_backward(self, grad_probits: torch.Tensor, with_input_grad: bool = False):
        """Gradients of the decoder `nn.Linear` for the LAST forward on this engine: (grad_weight (ncls, D), grad_bias (ncls),
        grad_output (N, T, D) or None), float32 device tensors."""
        grad_probits, N, T, ncls, _ = self._lattice_args(grad_probits, name='grad_probits')
        if ncls != self.hp.num_classes:
            raise ValueError('grad_probits has the wrong number of classes')
        D = self.hp.encoder_dim
        gw = torch.empty((ncls, D), dtype=torch.float32, device=self.device)
        gb = torch.empty((ncls,), dtype=torch.float32, device=self.device)
        gy = torch.empty((N, T, D), dtype=torch.float32, device=self.device) if with_input_grad else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_decoder_backward(self._h, _dp(grad_probits), N, T, _dp(gw), _dp(gb), _dp(gy), _stream_ptr(self.device)))
        return gw, gb, gy

    def decoder_adamw(self, grad_weight: torch.Tensor, grad_bias: torch.Tensor, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                      weight_decay: float = 1e-2) -> None:
        """One torch.optim.AdamW step on the decoder (state kept inside the engine); defaults are torch's."""
        self._check_decoder_grads(grad_weight, grad_bias)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_decoder_adamw(self._h, _dp(grad_weight), _dp(grad_bias), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                                   float(weight_decay), _stream_ptr(self.device)))

    def _check_decoder_grads(self, grad_weight: torch.Tensor, grad_bias: torch.Tensor) -> None:
        for g in (grad_weight, grad_bias):
            if g.device != self.device or g.dtype != torch.float32 or not g.is_contiguous():
                raise RuntimeError('gradients must be contiguous float32 tensors on the model device')
        if grad_weight.shape != (self.hp.num_classes, self.hp.encoder_dim) or grad_bias.shape != (self.hp.num_classes,):
            raise ValueError('gradient shapes do not match the decoder')

    @staticmethod
    def _optim(kind: str, lr: float, weight_decay: float, betas, eps: float, momentum: float, alpha: float) -> '_lib.OptimC':
        if kind not in _lib.OPTIMIZERS:
            raise ValueError(f'unknown optimizer {kind!r}: one of {", ".join(_lib.OPTIMIZERS)}')
        return _lib.OptimC(_lib.OPTIMIZERS[kind], float(lr), float(weight_decay), float(betas[0]), float(betas[1]), float(eps), float(momentum), float(alpha))

    def decoder_optim_step(self, kind: str, grad_weight: torch.Tensor, grad_bias: torch.Tensor, lr: float, weight_decay: float = 0.0,
                           betas=(0.9, 0.999), eps: float = 1e-8, momentum: float = 0.0, alpha: float = 0.99) -> None:
        """One step of torch.optim.{AdamW, Adam, SGD, RMSprop} (`kind`) on the decoder, state kept inside the engine; betas / eps
        reach the Adam kinds, momentum SGD and RMSprop, alpha / eps RMSprop.  The first step fixes the kind."""
        self._check_decoder_grads(grad_weight, grad_bias)
        o = self._optim(kind, lr, weight_decay, betas, eps, momentum, alpha)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_decoder_optim_step(self._h, _dp(grad_weight), _dp(grad_bias), C.byref(o), _stream_ptr(self.device)))

    def decoder_optim_state(self) -> Dict:
        """The output layer's optimizer state: {'kind': name or None, 'step', 'state': float32 torch view of the library's
        [master copy | slot 0 | slot 1] vector, or None before the first step}."""
        kind, step, p, n = C.c_int(), C.c_int64(), C.c_void_p(), C.c_size_t()
        _lib.check(self.lib.cocr_decoder_optim_state(self._h, C.byref(kind), C.byref(step), C.byref(p), C.byref(n)))
        return {'kind': _OPTIMIZER_NAMES.get(kind.value), 'step': int(step.value), 'state': self._device_view(p.value, n.value) if p.value else None}

    def decoder_optim_restore(self, kind: Optional[str], step: int, state: torch.Tensor) -> None:
        """Puts a `decoder_optim_state` back: the vector (float32, this device), the kind and the step count; the serving copy of
        the output layer follows the master copy."""
        if state.device != self.device or state.dtype != torch.float32 or not state.is_contiguous() or state.dim() != 1:
            raise RuntimeError('the state must be a contiguous float32 vector on the model device')
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_decoder_optim_restore(self._h, -1 if kind is None else _lib.OPTIMIZERS[kind], int(step), _dp(state), state.numel(),
                                                           _stream_ptr(self.device)))

    def decoder_state(self) -> Dict[str, np.ndarray]:
        """{'decoder.weight', 'decoder.bias'}: float32 host copies of the (trained) output layer."""
        out = {}
        for name, shape in (('decoder.weight', (self.hp.num_classes, self.hp.encoder_dim)), ('decoder.bias', (self.hp.num_classes,))):
            a = np.empty(shape, dtype=np.float32)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.cocr_get_tensor(self._h, name.encode(), _hp(a, C.c_void_p), a.size, _stream_ptr(self.device)))
            out[name] = a
        return out

    # ---- training step of the whole network (include/cocr.h: cocr_train_*) ------------------------------
    def train_begin(self, matmul_precision: str = 'highest') -> None:
        """fp32 master copy of the loaded state (`load_state`) on the device, zeroed AdamW moments.  matmul_precision: 'highest' (exact
        fp32 products) or 'medium' (bf16-rounded operands, fp32 accumulation: torch.set_float32_matmul_precision('medium'), what the
        reference's cli/train.py:252 sets)."""
        if matmul_precision not in ('highest', 'medium'):
            raise ValueError("matmul_precision must be 'highest' or 'medium'")
        _lib.check(self.lib.cocr_train_begin(self._h))
        _lib.check(self.lib.cocr_train_set_matmul(self._h, int(matmul_precision == 'medium')))

    def train_step(self, lines: torch.Tensor, lens, targets, label_lens, dropout=(0.0, 0.0, 0.0, 0.0), seed: int = 0,
                   teacher_logits: Optional[torch.Tensor] = None, tau: float = 1.0, distill_weight: float = 0.0):
        """`RecognitionModel.training_step` without the optimizer (reference model.py:129-152): train-mode forward, summed CTC loss,
        backward through decoder and encoder.  lines (N,H,W) float32 / uint8 on this device; lens pixel widths; targets the
        concatenated labels, label_lens their per-line counts; dropout = (input, feed_forward, attention, conv) probabilities.
        Returns the loss; the gradients stay on the device (`train_grad`, `train_optim_step`).
        teacher_logits (N,T,ncls) float32 on this device, T = out_len(W): the step with the distillation term,
        criterion (1 - distill_weight) CTC + distill_weight KD at temperature tau; returns (summed CTC, summed KD), both unweighted."""
        if lines.device != self.device or lines.dim() != 3:
            raise ValueError('expected a (N,H,W) batch on the model device')
        ldt = _lib.U8 if lines.dtype == torch.uint8 else _lib.F32
        lines = (lines if ldt == _lib.U8 else lines.float()).contiguous()
        N, H, W = lines.shape
        il = _i32(lens)
        tl, tg = _target_arrays(N, il, targets, label_lens, 'lens')
        labels = (_hp(tg if tg.shape[0] else None), _hp(tl))
        dp = (C.c_float * 4)(*[float(x) for x in dropout])
        if teacher_logits is not None:
            tz = teacher_logits
            if tz.device != self.device or tz.dtype != torch.float32 or tuple(tz.shape) != (N, self.out_len(W), self.hp.num_classes):
                raise ValueError(f'teacher_logits must be a float32 {(N, self.out_len(W), self.hp.num_classes)} tensor on the model device')
            tz = tz.contiguous()
            both = (C.c_float * 2)()
            with torch.cuda.device(self.device):
                _lib.check(self.lib.cocr_train_step_distill(self._h, _dp(lines), ldt, N, H, W, _hp(il), *labels, dp, C.c_uint64(int(seed)), _dp(tz),
                                                            float(tau), float(distill_weight), both, _stream_ptr(self.device)))
            return float(both[0]), float(both[1])
        loss = C.c_float()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_train_step(self._h, _dp(lines), ldt, N, H, W, _hp(il), *labels, dp, C.c_uint64(int(seed)), C.byref(loss),
                                                _stream_ptr(self.device)))
        return float(loss.value)

    def _train_get(self, name: str, kind: int) -> np.ndarray:
        from .spec import model_state_spec
        shape = model_state_spec(self.hp)[name][0]
        a = np.empty(shape, dtype=np.float32)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_train_get(self._h, name.encode(), kind, _hp(a, C.c_void_p), a.size, _stream_ptr(self.device)))
        return a

    def train_grad(self, name: str) -> np.ndarray:
        """d loss / d `name` of the last `train_step` (reference state-dict name, e.g. 'encoder.layers.0.sequential.1.module.attention.u_bias')."""
        return self._train_get(name, 1)

    def train_value(self, name: str) -> np.ndarray:
        """Current value of a parameter or buffer (BatchNorm running statistics) of the training state."""
        return self._train_get(name, 0)

    def train_adamw(self, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2) -> None:
        """One torch.optim.AdamW step on all parameters with the gradients of the last `train_step` (defaults are torch's)."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_train_adamw(self._h, float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), _stream_ptr(self.device)))

    def train_adopt_decoder(self, src: 'HipRecognizer') -> None:
        """The output layer of `src` as its decoder steps left it (fp32 master copy, both slots, step count k) into this engine's
        training state, device to device on the current stream; the optimizer step continues that layer at step k + 1 and every
        other parameter at its own count."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_train_adopt_decoder(self._h, src._h, _stream_ptr(self.device)))

    def _device_view(self, ptr: int, n: int) -> torch.Tensor:
        """`n` floats of library-owned device memory as a float32 torch view."""
        return _mem_view(self, ptr, n, '<f4', self.device)

    def train_grad_buffer(self) -> torch.Tensor:
        """The flat gradient vector of all parameters as a float32 torch view of library-owned memory (for an all-reduce)."""
        p, n = C.c_void_p(), C.c_size_t()
        _lib.check(self.lib.cocr_train_grad_buffer(self._h, C.byref(p), C.byref(n)))
        return self._device_view(p.value, n.value)

    def train_value_buffer(self) -> torch.Tensor:
        """The flat value vector (all parameters in the gradient vector's layout, then the BatchNorm running statistics) as a float32
        torch view of library-owned memory."""
        p, n, npar = C.c_void_p(), C.c_size_t(), C.c_size_t()
        _lib.check(self.lib.cocr_train_param_buffer(self._h, C.byref(p), C.byref(n), C.byref(npar)))
        return self._device_view(p.value, n.value)

    def train_optim_step(self, kind: str, lr: float, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, momentum: float = 0.0,
                         alpha: float = 0.99, grad: Optional[torch.Tensor] = None, grad_scale: float = 1.0) -> None:
        """One step of torch.optim.{AdamW, Adam, SGD, RMSprop} (`kind`) on all parameters with the gradients of the last `train_step`;
        betas / eps reach the Adam kinds, momentum SGD and RMSprop, alpha / eps RMSprop (defaults are torch's).  The first step
        fixes the kind: another kind afterwards raises.  grad: another gradient vector in `train_grad_buffer()`'s layout (an
        accumulation window); grad_scale: every gradient element enters the step as fl(grad_scale * g) (the clip coefficient)."""
        o = self._optim(kind, lr, weight_decay, betas, eps, momentum, alpha)
        if grad is None and float(grad_scale) == 1.0:
            with torch.cuda.device(self.device):
                _lib.check(self.lib.cocr_train_optim_step(self._h, C.byref(o), _stream_ptr(self.device)))
            return
        if grad is not None:
            self._check_flat(grad)
            if grad.numel() != self.train_grad_buffer().numel():
                raise ValueError(f'grad has {grad.numel()} floats, the gradient vector {self.train_grad_buffer().numel()}')
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_train_optim_step_ex(self._h, C.byref(o), _dp(grad), float(grad_scale), _stream_ptr(self.device)))

    # ---- the gradient window on flat vectors (include/cocr.h: cocr_grad_accumulate / cocr_grad_norm) ------
    def _check_flat(self, t: torch.Tensor) -> None:
        if t.device != self.device or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
            raise RuntimeError('expected a contiguous float32 vector on the model device')

    def grad_accumulate(self, dst: torch.Tensor, src: torch.Tensor, scale: float, overwrite: bool = False) -> None:
        """dst += fl(scale * src), or dst = fl(scale * src) with `overwrite` (then dst may be src: the in-place scale); float32 vectors
        of one length on this device, stream-ordered.  Bit for bit torch's `dst.add_(src * scale)`."""
        self._check_flat(dst)
        self._check_flat(src)
        if dst.numel() != src.numel():
            raise ValueError(f'dst has {dst.numel()} floats, src {src.numel()}')
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_grad_accumulate(_dp(dst), _dp(src), dst.numel(), float(scale), int(bool(overwrite)), self.device.index or 0,
                                                     _stream_ptr(self.device)))

    def grad_norm(self, t: torch.Tensor) -> float:
        """The L2 norm of a float32 vector on this device, squares and sums in double, the same bits on every call; waits for the stream."""
        self._check_flat(t)
        out = C.c_double()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_grad_norm(_dp(t), t.numel(), self.device.index or 0, C.byref(out), _stream_ptr(self.device)))
        return float(out.value)

    def train_optim_state(self) -> Dict:
        """The whole-network optimizer state: {'kind': name or None before the first step, 'step', 'dec_steps', 'slot0', 'slot1'}; the
        slots are float32 torch views of the library's two state vectors (the gradient vector's layout; their meaning per kind:
        include/cocr.h)."""
        kind, step, dec, p0, p1, n = C.c_int(), C.c_int64(), C.c_int64(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        _lib.check(self.lib.cocr_train_optim_state(self._h, C.byref(kind), C.byref(step), C.byref(dec), C.byref(p0), C.byref(p1), C.byref(n)))
        return {'kind': _OPTIMIZER_NAMES.get(kind.value), 'step': int(step.value), 'dec_steps': int(dec.value),
                'slot0': self._device_view(p0.value, n.value), 'slot1': self._device_view(p1.value, n.value)}

    def train_optim_restore(self, kind: Optional[str], step: int, dec_steps: int = 0) -> None:
        """The counters of a restored state, after the caller has written `train_value_buffer()` and the two slots."""
        _lib.check(self.lib.cocr_train_optim_restore(self._h, -1 if kind is None else _lib.OPTIMIZERS[kind], int(step), int(dec_steps)))

    def train_end(self) -> None:
        """Trained values back into the model's state; `finalize()` again to serve them."""
        _lib.check(self.lib.cocr_train_end(self._h))

    # ---- line pre-processing (include/cocr.h: cocr_preproc_lines) --------------------------------------
    def preprocess(self, lines: Sequence[np.ndarray], height: Optional[int] = None, pad: int = 16, width: int = 0,
                   bucket_edge: int = 0) -> Tuple[torch.Tensor, np.ndarray]:
        """Raw 8-bit line crops ((H, W) grayscale or (H, W, 3) RGB numpy arrays, any height) -> the (N, height, Wb) uint8 device
        batch `forward` ingests, and the lines' widths after scaling and padding (the batch's `seq_lens`).  Grayscale, Pillow
        LANCZOS scaling to `height` (default: the model's), `pad` zero columns left and right, right-zero-filled to Wb = `width`,
        or the widest line rounded up to a multiple of `bucket_edge`, or the widest line."""
        if len(lines) < 1:
            raise ValueError('empty batch')
        hs = np.array([x.shape[0] for x in lines], dtype=np.int32)
        ws = np.array([x.shape[1] for x in lines], dtype=np.int32)
        ch = np.array([1 if x.ndim == 2 else x.shape[2] for x in lines], dtype=np.int32)
        for x in lines:
            if x.dtype != np.uint8 or x.ndim not in (2, 3):
                raise ValueError('line crops are (H, W) or (H, W, 3) uint8 arrays')
        sizes = hs.astype(np.int64) * ws * ch
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        flat = np.concatenate([np.ascontiguousarray(x).reshape(-1) for x in lines])
        self._keep = px = torch.from_numpy(flat).to(self.device)            # the kernels read it asynchronously on the current stream
        return self.preprocess_device(px, offs, hs, ws, ch, height, pad, width, bucket_edge)

    def preprocess_device(self, pixels: torch.Tensor, offsets, heights, widths, channels=None, height: Optional[int] = None,
                          pad: int = 16, width: int = 0, bucket_edge: int = 0) -> Tuple[torch.Tensor, np.ndarray]:
        """`preprocess` on lines already in device memory: `pixels` a uint8 device buffer holding line i at byte offsets[i] as
        heights[i] x widths[i] pixels of channels[i] (None: all 1) bytes -- e.g. the strips of `extract_lines`.  Same output."""
        height = int(height or self.hp.height)
        if pixels.device != self.device or pixels.dtype != torch.uint8 or not pixels.is_contiguous():
            raise ValueError('pixels must be a contiguous uint8 buffer on the model device')
        offs = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        hs, ws = _i32(heights), _i32(widths)
        n = offs.shape[0]
        ch = np.ones(n, dtype=np.int32) if channels is None else _i32(channels)
        if n < 1:
            raise ValueError('empty batch')
        if hs.shape[0] != n or ws.shape[0] != n or ch.shape[0] != n:
            raise ValueError('offsets, heights, widths and channels need one entry per line')
        ends = offs + hs.astype(np.int64) * ws * ch
        if offs.min() < 0 or ends.max() > pixels.numel():
            raise ValueError('a line reaches outside the pixel buffer')
        wl = [int(self.lib.cocr_preproc_width(int(h), int(w), height, int(pad))) for h, w in zip(hs, ws)]
        wb = int(width) if width else max(wl)
        if not width and bucket_edge:
            wb = -(-wb // int(bucket_edge)) * int(bucket_edge)
        out = torch.empty((n, height, wb), dtype=torch.uint8, device=self.device)
        lens = np.zeros(n, dtype=np.int32)
        _lib.check(self.lib.cocr_preproc_lines(self._h, _dp(pixels), _hp(offs, _I64P), _hp(hs), _hp(ws), _hp(ch), n, height, int(pad), wb, _dp(out),
                                               _hp(lens), _stream_ptr(self.device)))
        return out, lens

    # ---- training augmentation (include/cocr.h: cocr_augment_lines) -----------------------------------------------------------
    def augment(self, lines: torch.Tensor, seq_lens, params: np.ndarray, grid: np.ndarray, out: Optional[torch.Tensor] = None
                ) -> torch.Tensor:
        """Augmented copy of the (N, H, W) uint8 device batch `lines` with the host tables of `augment.draw`.
        The tables are checked here (ValueError before any launch), staged in pinned memory and uploaded with non-blocking copies;
        nothing synchronises the stream."""
        from . import augment as _aug
        if lines.device != self.device or lines.dtype != torch.uint8 or lines.dim() != 3 or not lines.is_contiguous():
            raise ValueError('expected a contiguous (N, H, W) uint8 batch on the model device')
        N, H, W = lines.shape
        sl = _i32(seq_lens)
        if sl.shape[0] != N:
            raise ValueError('one seq_len per line')
        if H > _aug.MAX_H or W > _aug.MAX_W or sl.min() < 0 or sl.max() > W:
            raise ValueError(f'batch of {H} x {W} px with seq_lens in [{sl.min()}, {sl.max()}] (limits {_aug.MAX_H} x {_aug.MAX_W}, 0 <= seq_len <= W)')
        params, grid = np.asarray(params), np.asarray(grid)
        _aug.check_tables(params, grid, sl, H, W)
        if out is None:
            out = torch.empty_like(lines)
        elif out.shape != lines.shape or out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous() \
                or out.data_ptr() == lines.data_ptr():
            raise ValueError('out must be a separate contiguous uint8 buffer of the batch\'s shape on the model device')
        # torch's pinned-memory allocator keeps the staging blocks alive until the copies that read them have run
        d_params = torch.from_numpy(np.ascontiguousarray(params)).pin_memory().to(self.device, non_blocking=True)
        d_grid = torch.from_numpy(np.ascontiguousarray(grid)).pin_memory().to(self.device, non_blocking=True)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_augment_lines(self._h, _dp(lines), _dp(out), N, H, W, _hp(sl), _dp(d_params), _dp(d_grid), int(grid.shape[1]),
                                                   _stream_ptr(self.device)))
        return out

    # ---- scoring (include/cocr.h: cocr_edit_align) ---------------------------------------------------------------------------
    def edit_align_lds(self, len_a: int, len_b: int) -> int:
        """Bytes of LDS a pair of these lengths takes when its op-code table lives in LDS; 0: the table goes to the global workspace."""
        return int(_lib.check(self.lib.cocr_edit_align_lds(self._h, int(len_a), int(len_b))))

    def _score_pinned(self, name: str, nbytes: int) -> torch.Tensor:
        buf = self._pinned.get(name)
        if buf is None or buf.numel() < nbytes:
            buf = self._pinned[name] = torch.empty(max(1 << 16, nbytes + nbytes // 2), dtype=torch.uint8).pin_memory()
        return buf

    def edit_align(self, a: np.ndarray, a_offs: np.ndarray, b: np.ndarray, b_offs: np.ndarray, want_ops: bool = False
                   ) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:
        """Edit-distance alignment of P packed pairs of int32 symbol sequences (a = ground truth, b = prediction; `*_offs` P + 1 int64
        offsets starting at 0) with `evaluate.global_align`'s definition.  Returns counts (P, 4) int32 = (distance, insertions,
        deletions, substitutions) and, with `want_ops`, the raw op buffer (sum of len_a + len_b bytes) and ops_len (P): pair p's
        alignment (0 equal, 1 substitution, 2 deletion, 3 insertion, forward order) is the LAST ops_len[p] bytes of its slot
        [a_offs[p] + b_offs[p], a_offs[p+1] + b_offs[p+1]).  The packed sequences go up through pinned staging with non-blocking
        copies, the results come back the same way; the call returns when they have arrived.  ValueError before any launch for a
        sequence of more than 4096 symbols or malformed offsets."""
        ao = np.ascontiguousarray(np.asarray(a_offs, dtype=np.int64).reshape(-1))
        bo = np.ascontiguousarray(np.asarray(b_offs, dtype=np.int64).reshape(-1))
        if ao.shape[0] < 1 or ao.shape != bo.shape or ao[0] != 0 or bo[0] != 0:
            raise ValueError('a_offs and b_offs hold P + 1 offsets each, starting at 0')
        P = ao.shape[0] - 1
        a = _i32(a)
        b = _i32(b)
        if a.shape[0] != ao[-1] or b.shape[0] != bo[-1]:
            raise ValueError('the last offsets must equal the lengths of a and b')
        if P == 0:
            return np.zeros((0, 4), dtype=np.int32), (np.zeros(0, dtype=np.uint8) if want_ops else None), \
                (np.zeros(0, dtype=np.int32) if want_ops else None)
        na, nb = a.shape[0], b.shape[0]
        nops = (na + nb) if want_ops else 0
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            h_in = self._score_pinned('score_in', (na + nb) * 4 + 16)
            sym = h_in[:(na + nb) * 4].view(torch.int32).numpy()
            sym[:na] = a
            sym[na:] = b
            d_in = h_in[:(na + nb) * 4 + 16].to(self.device, non_blocking=True)
            # [counts (P, 4) | ops_len (P) | ops]: one buffer, one copy back
            out_bytes = 20 * P + nops
            d_out = torch.empty(out_bytes + 16, dtype=torch.uint8, device=self.device)
            base = d_out.data_ptr()
            _lib.check(self.lib.cocr_edit_align(self._h, _dp(d_in), _hp(ao, _I64P), _dp(d_in) + 4 * na, _hp(bo, _I64P), P, base,
                                                base + 20 * P if want_ops else None, base + 16 * P if want_ops else None, _stream_ptr(self.device)))
            h_out = self._score_pinned('score_out', out_bytes)
            h_out[:out_bytes].copy_(d_out[:out_bytes], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
            ev.synchronize()
        res = h_out[:out_bytes].numpy()
        counts = res[:16 * P].view(np.int32).reshape(P, 4).copy()
        if not want_ops:
            return counts, None, None
        return counts, res[20 * P:].copy(), res[16 * P:20 * P].view(np.int32).copy()

    # ---- baseline line extraction (include/cocr.h: cocr_extract_lines) -------------------------------------------------------
    def extract_lines(self, pages: Sequence['np.ndarray | torch.Tensor'], geoms: Sequence, fill: int = 0
                      ) -> Tuple[torch.Tensor, np.ndarray, np.ndarray, np.ndarray]:
        """Cuts and straightens text lines out of page images on the GPU.  `pages`: (H, W) or (H, W, 3) uint8
        images, numpy (uploaded here) or tensors on this device; `geoms`: (page index, `page.LineGeometry`) pairs.  Returns the packed
        uint8 strip buffer (device) and per line its byte offset, rows H_s and columns W_s: the input of `preprocess_device`."""
        if len(geoms) < 1:
            raise ValueError('no lines to extract')
        dp = []
        for a in pages:
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
            if t.dtype != torch.uint8 or not (t.dim() == 2 or (t.dim() == 3 and t.shape[2] == 3)) or t.numel() == 0:
                raise ValueError('a page is a non-empty (H, W) or (H, W, 3) uint8 image')
            dp.append(t.to(self.device).contiguous())
        P = len(dp)
        page_dims = np.array([[t.shape[0], t.shape[1], 1 if t.dim() == 2 else 3] for t in dp], dtype=np.int32)
        page_ptrs = (C.c_void_p * P)(*[t.data_ptr() for t in dp])
        lp = np.array([int(p) for p, _ in geoms], dtype=np.int32)
        gs = [g for _, g in geoms]
        dims = np.ascontiguousarray(np.array([[g.H_s, g.W_s, g.T] for g in gs], dtype=np.int32))
        cols = np.ascontiguousarray(np.concatenate([g.cols for g in gs]).astype(np.int64))
        verts = np.ascontiguousarray(np.concatenate([g.verts for g in gs]).astype(np.int32))
        nv = np.array([g.verts.shape[0] for g in gs], dtype=np.int32)
        hs, ws = dims[:, 0].copy(), dims[:, 1].copy()
        sizes = hs.astype(np.int64) * ws
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        out = torch.empty((int(sizes.sum()),), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_extract_lines(self._h, page_ptrs, _hp(page_dims), P, _hp(lp), _hp(dims), _hp(cols, _I64P), _hp(verts), _hp(nv),
                                                   len(gs), int(fill), _dp(out), _hp(offs, _I64P), _stream_ptr(self.device)))
        self._keep_pages = dp          # the sampler reads them asynchronously on the current stream
        return out, offs, hs, ws

    # ---- test / measurement hooks ---------------------------------------------------------------
    def set_debug(self, on: bool) -> None:
        _lib.check(self.lib.cocr_set_debug(self._h, int(on)))

    def tap(self, name: str) -> np.ndarray:
        n = C.c_int64()
        _lib.check(self.lib.cocr_debug_tap(self._h, name.encode(), None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.float32)
        _lib.check(self.lib.cocr_debug_tap(self._h, name.encode(), _hp(out, C.c_void_p), n.value, C.byref(n)))
        return out

    def attention_layout(self, n: int, T: int) -> Tuple[int, int, int, int]:
        """(heads, dh, dhp, Tp) of `attention_core`'s tensors for n lines of T frames: the engine's d_head (a zero-padded narrow model:
        its slot), that rounded up to 32, T rounded up to 64."""
        dims = np.zeros(4, dtype=np.int32)
        _lib.check(self.lib.cocr_debug_attention(self._h, 0, int(n), int(T), None, None, None, 0, None, 0, _hp(dims), None))
        return tuple(int(d) for d in dims)

    def attention_core(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, layer: int, T: int) -> torch.Tensor:
        """Block `layer`'s attention core alone (include/cocr.h: cocr_debug_attention) on q, k, v of shape (N, heads, Tp, dhp) in the compute
        dtype on this device, zero beyond T and beyond d_head.  Returns ctx (N, T, heads * dh) in the compute dtype."""
        want = torch.bfloat16 if DTYPES[self.compute_dtype] == _lib.BF16 else torch.float32
        for t in (q, k, v):
            if t.device != self.device or t.dtype != want or t.dim() != 4 or t.shape != q.shape or not t.is_contiguous():
                raise ValueError(f'q, k, v must be contiguous (N, heads, Tp, dhp) {want} tensors of one shape on {self.device}')
        N = int(q.shape[0])
        heads, dh, _, _ = self.attention_layout(N, T)
        ctx = torch.empty((N, int(T), heads * dh), dtype=want, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.cocr_debug_attention(self._h, int(layer), N, int(T), _dp(q), _dp(k), _dp(v), q.numel(), _dp(ctx), ctx.numel(), None,
                                                     _stream_ptr(self.device)))
        return ctx

    def profile(self, on: bool) -> None:
        _lib.check(self.lib.cocr_profile(self._h, int(on)))

    def profile_read(self) -> Dict[str, Tuple[float, int]]:
        names = C.create_string_buffer(4096)
        ms = (C.c_double * 64)()
        cnt = (C.c_int64 * 64)()
        n = _lib.check(self.lib.cocr_profile_read(self._h, names, len(names), ms, cnt, 64))
        keys = names.value.decode().split('\n')[:n]
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(keys)}
