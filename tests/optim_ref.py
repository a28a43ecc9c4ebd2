"""The four optimizer steps of include/cocr.h (cocr_train_optim_step) stated in numpy, in the dtype of the arrays given: what
tests/test_optim_host.py pins on torch.optim in float64 and what the kernel k_optim_flat computes per element in fp32.

    state = new_state(p)                      # both slots zero, step 0
    p = step(kind, p, g, state, lr=..., weight_decay=..., momentum=...)

Slots: AdamW / Adam (exp_avg, exp_avg_sq); SGD (momentum buffer, unused); RMSprop (square_avg, momentum buffer)."""
import numpy as np

KINDS = ('AdamW', 'Adam', 'SGD', 'RMSprop')


def new_state(p):
    return {'slot0': np.zeros_like(p), 'slot1': np.zeros_like(p), 'step': 0}


def step(kind, p, g, state, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, momentum=0.0, alpha=0.99):
    """One step on the array `p` with the gradient `g`; `state` is updated in place, the new `p` returned."""
    s0, s1 = state['slot0'], state['slot1']
    state['step'] += 1
    t = state['step']
    if kind in ('AdamW', 'Adam'):
        b1, b2 = betas
        if kind == 'AdamW':
            p = p * (1 - lr * weight_decay)                      # decoupled decay
        else:
            g = g + weight_decay * p                             # L2 decay folded into the gradient
        s0[...] = b1 * s0 + (1 - b1) * g
        s1[...] = b2 * s1 + (1 - b2) * g * g
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        return p - lr / bc1 * s0 / (np.sqrt(s1) / np.sqrt(bc2) + eps)
    g = g + weight_decay * p
    if kind == 'SGD':                                            # dampening 0, no Nesterov
        if momentum == 0:
            return p - lr * g                                    # the slot is not touched
        s0[...] = momentum * s0 + g                              # zero slot: buf = g' on the first step, as torch sets it
        return p - lr * s0
    if kind == 'RMSprop':                                        # not centered
        s0[...] = alpha * s0 + (1 - alpha) * g * g
        a = np.sqrt(s0) + eps
        if momentum > 0:
            s1[...] = momentum * s1 + g / a
            return p - lr * s1
        return p - lr * g / a
    raise ValueError(kind)
