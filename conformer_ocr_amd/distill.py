"""Knowledge distillation: a small model learns from a large one's per-frame posteriors.

The definition, on student logits zS and teacher logits zT, both (N, T, ncls), with out_len[n] valid frames per line, a temperature
tau > 0 and a weight lambda in [0, 1]:

    p = softmax(zT / tau),  q = softmax(zS / tau)                         (over the classes of a frame)
    KD[n] = tau^2 sum_{t < out_len[n]} sum_c p(c) (log p(c) - log q(c))
          = tau^2 F.kl_div(log_softmax(zS / tau), log_softmax(zT / tau), reduction='sum', log_target=True) on the line's valid frames
    total = (1 - lambda) sum_n CTC[n] + lambda sum_n KD[n]
    d total / d zS[n, t, :] = (1 - lambda) dCTC + lambda tau (q - p)      for t < out_len[n], 0 behind it

Sum reduction, like the criterion's `reduction='sum'`; the tau^2 factor keeps the gradient's scale independent of tau.
`kd_loss_host` is this definition in torch on the CPU: what the kernel behind `cocr_distill_loss` (include/cocr.h) is tested against.
`check_teacher` is the host check `train.Trainer` runs on a (student, teacher) pair."""
from __future__ import annotations

from typing import Tuple

import torch


def kd_loss_host(student: torch.Tensor, teacher: torch.Tensor, out_lens, tau: float, dtype: torch.dtype = torch.float64) -> Tuple[torch.Tensor, torch.Tensor]:
    """(KD (N), d sum(KD) / d student (N, T, ncls)) in `dtype` on the CPU.  The log-probabilities come from log-softmax (maximum
    subtracted), never from log(p): a teacher probability that underflows to 0 contributes exactly 0, not NaN.  The logits must be
    finite; anything else is unspecified."""
    if not float(tau) > 0.0:
        raise ValueError(f'the temperature must be positive, not {tau}')
    zs, zt = student.detach().cpu().to(dtype), teacher.detach().cpu().to(dtype)
    if zs.dim() != 3 or zs.shape != zt.shape:
        raise ValueError('student and teacher logits are (N, T, ncls) tensors of one shape')
    N, T, _ = zs.shape
    lens = torch.as_tensor(out_lens).reshape(-1).to(torch.int64)
    if lens.shape[0] != N or int(lens.min()) < 0 or int(lens.max()) > T:
        raise ValueError('out_lens needs one entry in [0, T] per line')
    t = torch.as_tensor(float(tau), dtype=dtype)
    lq, lp = torch.log_softmax(zs / t, dim=-1), torch.log_softmax(zt / t, dim=-1)
    q, p = lq.exp(), lp.exp()
    valid = (torch.arange(T)[None, :] < lens[:, None]).to(dtype)                       # (N, T)
    kd = t * t * ((p * (lp - lq)).sum(-1) * valid).sum(-1)
    grad = t * (q - p) * valid[:, :, None]
    return kd, grad


def check_teacher(net, teacher) -> None:
    """ValueError naming the first difference between the student `net` and `teacher` that rules distillation out: the two must have
    the same num_classes, height and subsampling_factor and equal codec tables, label <-> grapheme (distilling between alphabets is
    not built)."""
    a, b = net.hparams_record, teacher.hparams_record
    for k in ('num_classes', 'height', 'subsampling_factor'):
        if getattr(a, k) != getattr(b, k):
            raise ValueError(f'the teacher does not fit the model: {k} is {getattr(b, k)!r}, the model\'s {getattr(a, k)!r}')
    for name in ('c2l', 'l2c'):
        ta, tb = getattr(net.codec, name, None), getattr(teacher.codec, name, None)
        if _table(ta) != _table(tb):
            raise ValueError(f'the teacher does not fit the model: the codecs differ ({name})')


def _table(t):
    return None if t is None else {k: list(v) if isinstance(v, (list, tuple)) else v for k, v in dict(t).items()}
