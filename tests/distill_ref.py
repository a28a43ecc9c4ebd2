"""TEST INFRASTRUCTURE ONLY: what the distillation tests compare the device with.  Plain torch on the CPU, no GPU.

1. `kernel_cases` / `case_reference`: the inputs of the kernel tests and, per case, the float64 definition (`distill.kd_loss_host`), the
   float32 evaluation's own error e32 and the bounds derived from it.
2. `distill_train_grads`: the float64 training step with the distillation term -- `Oracle.forward_train`, the criterion and the KD term
   through torch autograd, modelled on `train_ref.train_grads`."""
from __future__ import annotations

import functools

import numpy as np
import torch

from conformer_ocr_amd.distill import kd_loss_host
from oracle.conformer_ref import Oracle

N, T, LENS = 3, 19, (19, 0, 7)
NCLS = (2, 11, 64, 65, 97, 256, 260, 1100)      # one lane group, a partial one, 16-byte and scalar accesses, rows wider than the registers
TAUS = (0.5, 1.0, 2.0, 4.0)
SCALES = (1.0, 8.0, 20.0)                       # sigma of the normal draw: logits up to about +-60
MARGIN = 8.0                                    # the GPU's exp / log and summation order differ from torch's


@functools.lru_cache(maxsize=None)
def logits(ncls: int, scale: float):
    """(student, teacher) float32 (N, T, ncls), seeded by the shape and the scale."""
    g = torch.Generator().manual_seed(1000 * ncls + int(scale))
    zs = torch.randn((N, T, ncls), generator=g, dtype=torch.float32) * scale
    zt = torch.randn((N, T, ncls), generator=g, dtype=torch.float32) * scale
    return zs, zt


@functools.lru_cache(maxsize=None)
def case_reference(ncls: int, scale: float, tau: float):
    """kd64 (N), grad64 (N, T, ncls), and the bounds: kd_tol (N) = max(8 e32, 2^-18 A_n), A_n = tau^2 sum p |log p - log q| in float64;
    grad_tol (scalar) = max(8 e32, 2^-20 tau) -- 8 ulp of a probability <= 1, times tau -- with e32 the error of the definition evaluated
    in float32 on the CPU against float64 (per line for KD, the largest element for the gradient)."""
    zs, zt = logits(ncls, scale)
    kd64, g64 = kd_loss_host(zs, zt, LENS, tau, torch.float64)
    kd32, g32 = kd_loss_host(zs, zt, LENS, tau, torch.float32)
    t = torch.tensor(tau, dtype=torch.float64)
    lq, lp = torch.log_softmax(zs.double() / t, -1), torch.log_softmax(zt.double() / t, -1)
    valid = (torch.arange(T)[None, :] < torch.tensor(LENS)[:, None]).double()
    A = t * t * ((lp.exp() * (lp - lq).abs()).sum(-1) * valid).sum(-1)
    e_kd = (kd32.double() - kd64).abs()
    e_g = float((g32.double() - g64).abs().max())
    kd_tol = torch.maximum(MARGIN * e_kd, 2.0 ** -18 * A)
    grad_tol = max(MARGIN * e_g, 2.0 ** -20 * tau)
    return kd64, g64, kd_tol, grad_tol


def distill_train_grads(hp, state, image, lens, targets, teacher_logits, tau: float, lam: float, dtype=torch.float64):
    """(ctc, kd, probits, d total / d parameter, BatchNorm batch statistics) of the step with a teacher in `dtype`: total =
    (1 - lam) CTC + lam KD, KD = tau^2 kl_div(log_softmax(zS / tau), log_softmax(zT / tau), 'sum', log_target=True) on the valid frames."""
    o = Oracle(hp, state, dtype)
    params = {k: v for k, v in o.w.items() if v.is_floating_point() and 'running_' not in k}
    for v in params.values():
        v.requires_grad_(True)
    probits, ol = o.forward_train(torch.from_numpy(image).to(dtype), torch.from_numpy(np.asarray(lens)))
    target = torch.tensor([c for s in targets for c in s], dtype=torch.long)
    tl = torch.tensor([len(s) for s in targets], dtype=torch.long)
    F = torch.nn.functional
    ctc = F.ctc_loss(F.log_softmax(probits, -1).transpose(0, 1), target, ol.long(), tl, reduction='sum', zero_infinity=True)
    zt = torch.as_tensor(teacher_logits).to(dtype)
    kd = probits.new_zeros(())
    for n in range(probits.shape[0]):
        L = int(ol[n])
        if L:
            kd = kd + tau * tau * F.kl_div(F.log_softmax(probits[n, :L] / tau, -1), F.log_softmax(zt[n, :L] / tau, -1), reduction='sum', log_target=True)
    ((1.0 - lam) * ctc + lam * kd).backward()
    return float(ctc.detach()), float(kd.detach()), probits.detach().numpy(), {k: v.grad.numpy() for k, v in params.items()}, o.bn_batch_stats
