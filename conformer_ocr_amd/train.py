"""Training step of the output layer on a frozen backbone -- the first slice of the reference's training loop
(`RecognitionModel.training_step` / `configure_optimizers`, reference conformer_ocr/model.py:147-152,238-250,267-290) on the GPU:

    forward (eval-mode encoder) -> CTC criterion + d loss / d probits (cocr_ctc_loss) -> decoder backward (cocr_decoder_backward)
    -> [all-reduce of the two gradients across ranks] -> the optimizer step (cocr_decoder_adamw; Adam / SGD / RMSprop: cocr_decoder_optim_step)

This is what the reference's `freeze_backbone` asks for (cli/train.py:154-155: "keep the backbone (everything but the last layer)
frozen") and what adapts a model to a new alphabet.  `DecoderTrainer` is that step alone; `Trainer(freeze_backbone=N)` runs it for
the first N samples and then hands the output layer and its optimizer state over to the whole-network step.

Data-parallel training: one process per GPU; each rank computes its batch's gradients, `torch.distributed.all_reduce` (backend
"nccl" = RCCL over xGMI; two tensors, (ncls x D + ncls) x 4 bytes -- ~100 KB) combines them, every rank applies the same update: the
replicas stay bit-identical without a weight broadcast.  The gradients are AVERAGED over the ranks: the reference trains through
Lightning's `Trainer(devices=...)`, i.e. torch DDP, which divides the all-reduced gradients by the world size whatever the loss's
own reduction is (each rank's loss is the sum over ITS lines, `reduction='sum'`)."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .pred import PytorchRecognitionModel


OPTIMIZERS = ('AdamW', 'Adam', 'SGD', 'RMSprop')                      # the reference's `--optimizer` choices (cli/train.py:140-147)


def _momentum_of(optimizer: str, momentum: float) -> float:
    """`momentum` reaches SGD and RMSprop only (model.py:283-289)."""
    return float(momentum) if optimizer in ('SGD', 'RMSprop') else 0.0


class DecoderTrainer:
    """Training of `net.nn['decoder']` with the rest of `net` frozen, AdamW by default.

    Hyper-parameter names and defaults follow the reference (`lrate`, `weight_decay`, `optimizer`, `momentum`: model.py:47-50; betas /
    eps / alpha are torch's defaults, as the reference passes none; `momentum` reaches SGD and RMSprop only)."""

    def __init__(self, net: PytorchRecognitionModel, lrate: float = 1e-3, weight_decay: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 process_group=None, distributed: Optional[bool] = None, optimizer: str = 'AdamW', momentum: float = 0.9):
        if optimizer not in OPTIMIZERS:
            raise ValueError(f'unknown optimizer {optimizer!r}: one of {", ".join(OPTIMIZERS)}')
        self.net = net
        self.optimizer, self.momentum = optimizer, float(momentum)
        self.lrate, self.weight_decay, self.betas, self.eps = float(lrate), float(weight_decay), tuple(betas), float(eps)
        self.process_group = process_group
        if distributed is None:
            distributed = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size(process_group) > 1
        self.distributed = bool(distributed)
        self.global_step = 0

    def training_step(self, batch: Dict) -> torch.Tensor:
        """One optimizer step on `batch` (the reference's batch dict: image, seq_lens, target, target_lens); returns the batch loss
        (0-dim device tensor, this rank's lines only, like the reference logs `train_loss`)."""
        o = self.net.step(batch, with_grad=True)
        eng = self.net._engine
        gw, gb, _ = eng.decoder_backward(o['grad_probits'])
        if self.distributed:
            reduce_gradients((gw, gb), self.process_group)
        if self.optimizer == 'AdamW':
            eng.decoder_adamw(gw, gb, self.lrate, self.betas, self.eps, self.weight_decay)
        else:
            eng.decoder_optim_step(self.optimizer, gw, gb, self.lrate, weight_decay=self.weight_decay, betas=self.betas, eps=self.eps,
                                   momentum=_momentum_of(self.optimizer, self.momentum))
        self.global_step += 1
        return o['loss']

    def sync_module(self) -> None:
        """Copies the trained output layer back into `net.nn['decoder']` (so `save_safetensors` / `state_dict()` see it)."""
        _sync_decoder(self.net)


def _sync_decoder(net: PytorchRecognitionModel) -> None:
    st = net._engine.decoder_state()
    dec = net.nn['decoder']
    with torch.no_grad():
        dec.weight.copy_(torch.from_numpy(st['decoder.weight']))
        dec.bias.copy_(torch.from_numpy(st['decoder.bias']))
    # the module now equals the engine's weights: keep the engine (and its optimizer state) instead of re-packing on the next forward
    net._engine_sig = net._signature(net._engine.device)


def reduce_gradients(tensors, group=None) -> None:
    """Mean of each gradient tensor over the ranks (torch DDP's semantics), in place: ONE collective on a flat bucket (the tensors
    are small; two launches of a ring all-reduce would cost two latencies over xGMI).  Sum + division: gloo has no AVG op."""
    flat = torch.cat([t.reshape(-1) for t in tensors])
    torch.distributed.all_reduce(flat, op=torch.distributed.ReduceOp.SUM, group=group)
    flat.div_(torch.distributed.get_world_size(group))
    off = 0
    for t in tensors:
        t.copy_(flat[off:off + t.numel()].view_as(t))
        off += t.numel()


def clip_coef(norm: float, max_norm: float) -> float:
    """The factor `torch.nn.utils.clip_grad_norm_(max_norm)` applies to a gradient of L2 norm `norm`, computed in float32 like torch's:
    min(1, f32(max_norm) / (f32(norm) + f32(1e-6)))."""
    import numpy as np
    with np.errstate(over='ignore', invalid='ignore'):
        c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
        return float(np.minimum(np.float32(1.0), c))                                                # (a NaN norm gives NaN, as torch's clamp does)


# what a state written before the gradient window existed lacks, with the values that describe such a run
WINDOW_HYPER = {'accumulate_grad_batches': 1, 'gradient_clip_val': None, 'skip_nonfinite': False}


def upgrade_state(sd: Dict) -> Dict:
    """`sd` (a `Trainer.state_dict()`, or the tensors and records of a state file) with the keys of the gradient window filled in where
    an older writer left them out: the three arguments at their defaults, no skipped step, no open window, and -- every call having
    been an optimizer step -- batches_seen = global_step, frozen_batches = frozen_steps; and 'distill' = None (no teacher) where a
    writer from before distillation left it out.  `sd` itself is not changed."""
    out = dict(sd)
    out['hyper'] = dict(WINDOW_HYPER, **sd['hyper'])
    c = sd['counters']
    out['counters'] = dict({'batches_seen': c['global_step'], 'frozen_batches': c['frozen_steps'], 'skipped_steps': 0, '_window': 0,
                            '_window_frozen': False}, **c)
    out['distill'] = sd.get('distill')                    # (a state without the key was written without a teacher)
    return out


class Trainer:
    """Training of the WHOLE network on the GPU: the reference's `training_step` + `configure_optimizers` + `optimizer_step` /
    `lr_scheduler_step` (reference conformer_ocr/model.py:147-152,238-321) behind one object.

        trainer = Trainer(net, lr=1e-3, weight_decay=1e-2, warmup=100, schedule='cosine', cos_t_max=50)
        for batch in loader: loss = trainer.training_step(batch)      # batch: image (N,1,H,W), seq_lens, target, target_lens
        trainer.end_epoch(val_accuracy)                               # epoch-wise schedulers
        trainer.sync_module()                                         # trained values into net.nn (state_dict / save_safetensors / predict_*)

    Forward in train mode (BatchNorm batch statistics + running-statistics update, dropout with the probabilities the model was
    constructed with), summed CTC loss, backward through decoder and encoder, AdamW -- all in libcocr_hip.so (include/cocr.h
    cocr_train_*; fp32).  Optimizer: `optimizer` = 'AdamW' (default), 'Adam', 'SGD' or 'RMSprop' with the arguments the reference
    passes them (model.py:283-289: `lr`, `weight_decay`, and `momentum` for SGD and RMSprop only; betas / eps / alpha torch's defaults).
    Learning rate: linear warm-up over `warmup` steps exactly as `optimizer_step` applies it (the step itself runs at the rate
    set by the previous one; after step g the rate becomes min(1, (g + 1) / warmup) lr while g < warmup), then the epoch-wise schedule.
    Data parallel: one process per GPU, the flat gradient vector is averaged by ONE all-reduce per step (torch DDP's semantics).

    `freeze_backbone` (the reference's hyper-parameter; samples = this rank's lines): while `samples_seen < freeze_backbone` at the
    start of a step, the step is the FROZEN step -- `DecoderTrainer.training_step` on `net`'s own serving engine (eval-mode forward
    in the model's `compute_dtype`, CTC gradient, decoder backward, AdamW on the output layer at the current `lr` / weight decay);
    no encoder parameter or BatchNorm statistic moves, `sync_module` copies the output layer only and keeps that engine and its
    AdamW state.
    Before the first unfrozen step the output layer's fp32 master copy, moments and step count move into the whole-network state on
    the device (`cocr_train_adopt_decoder`); AdamW's step counts are per tensor from there on.  `global_step` and the warm-up run
    on across both phases.  The frozen step and the hand-over work for every optimizer kind.

    `state_dict()` / `load_state_dict()` hold everything a step or an epoch end reads: `fit(save_state=True)` writes
    them to a file, `fit(resume=...)` continues from one.

    The gradient window (the names are Lightning's, under whose `Trainer` the reference trains).  With all three at
    their defaults the step launches what it always launched: no norm, no extra wait.
    `accumulate_grad_batches` = k > 1: `training_step` is still called once per batch and returns that batch's loss; each call adds
    fl(1/k) g (1/k in float32) to an accumulation vector A, the k-th call takes the optimizer step on A and zeroes it.  `flush()` takes
    the step on an incomplete window, still at 1/k (as Lightning steps on an epoch's last batch); `end_epoch` and `fit` call it.  This
    is NOT one k-times larger batch: BatchNorm takes and updates its statistics per call, as torch does under accumulation.
    `global_step`, the warm-up and `lr` count optimizer steps, `samples_seen` lines per call, `batches_seen` calls (the dropout seed
    is seed * 1000003 + batches_seen).  Whether a window is frozen is decided at its start: the hand-over never splits one.  Data
    parallel: ONE all-reduce per optimizer step, on A; every rank then holds the same bits, hence the same norm, coefficient and skip.
    `gradient_clip_val`: the vector the step uses (A, or the gradient vector when k = 1; after the all-reduce) is clipped to that global
    L2 norm: its norm is taken in double on the device (`last_grad_norm`; None while no norm is taken), `clip_coef` of it scales
    every element on its way into the optimizer kernel (the frozen phase: in place, before its own step).
    `skip_nonfinite`: a window whose norm is not finite takes no optimizer step -- no parameter, slot, step count or `global_step`
    moves, A is zeroed, `skipped_steps` counts it, `log` gets a line.  Without it, with clipping on, such a window raises
    FloatingPointError (the window is dropped, nothing else moves): a NaN coefficient never reaches the kernel.  With neither, the
    gradient is used as it is.

    `teacher`: a `PytorchRecognitionModel` on the same device with the same classes, height, subsampling and
    codec (`distill.check_teacher`).  Every `training_step` runs its eval-mode forward (its own `compute_dtype`, no gradient) on the very
    batch the student sees and hands the logits to the step: the criterion becomes (1 - distill_weight) CTC + distill_weight KD at
    `distill_temperature` -- in the whole-network step inside `cocr_train_step_distill`, in the frozen phase by `cocr_distill_loss` on
    the serving engine's CTC gradient ahead of the decoder backward.  `training_step` returns that weighted total; `last_ctc_loss` and
    `last_kd_loss` keep the two sums.  The defaults 0.5 / 2.0 are placeholders, not tuned on real material.  Accumulation, clipping,
    `skip_nonfinite` and the all-reduce work on the flat gradient and do not change; with teacher=None nothing new is launched."""

    SCHEDULES = ('constant', 'exponential', 'cosine', 'step', 'reduceonplateau')

    def __init__(self, net: PytorchRecognitionModel, lr: float = 1e-3, weight_decay: float = 1e-3, optimizer: str = 'AdamW', warmup: int = 0,
                 schedule: str = 'constant', gamma: float = 0.1, cos_t_max: int = 50, cos_min_lr: float = 1e-4, step_size: int = 10,
                 rop_factor: float = 0.1, rop_patience: int = 5, completed_epochs: int = 0, seed: int = 0, process_group=None,
                 distributed: Optional[bool] = None, matmul_precision: str = 'highest', freeze_backbone: int = 0, log=None,
                 momentum: float = 0.9, accumulate_grad_batches: int = 1, gradient_clip_val: Optional[float] = None,
                 skip_nonfinite: bool = False, teacher: Optional[PytorchRecognitionModel] = None, distill_weight: float = 0.5,
                 distill_temperature: float = 2.0):
        if optimizer not in OPTIMIZERS:
            raise ValueError(f'unknown optimizer {optimizer!r}: one of {", ".join(OPTIMIZERS)}')
        if int(accumulate_grad_batches) < 1:
            raise ValueError(f'accumulate_grad_batches must be at least 1, not {accumulate_grad_batches}')
        if gradient_clip_val is not None and not float(gradient_clip_val) > 0.0:
            raise ValueError(f'gradient_clip_val must be positive, not {gradient_clip_val}')
        if schedule not in self.SCHEDULES:
            raise ValueError(f'Unsupported learning rate scheduler {schedule}.')                      # model.py:309
        if not float(momentum) >= 0.0:
            raise ValueError(f'Invalid momentum value: {momentum}')                                   # torch.optim.SGD / RMSprop
        self.teacher = teacher
        self.distill_weight, self.distill_temperature = float(distill_weight), float(distill_temperature)
        self.last_ctc_loss: Optional[float] = None
        self.last_kd_loss: Optional[float] = None
        if teacher is not None:
            from .distill import check_teacher
            if not 0.0 <= self.distill_weight <= 1.0:
                raise ValueError(f'distill_weight must lie in [0, 1], not {distill_weight}')
            if not self.distill_temperature > 0.0 or self.distill_temperature == float('inf'):
                raise ValueError(f'distill_temperature must be positive and finite, not {distill_temperature}')
            check_teacher(net, teacher)
        self.net = net
        self.optimizer, self.momentum, self.matmul_precision = optimizer, float(momentum), matmul_precision
        self.base_lr = self.lr = float(lr)
        self.weight_decay, self.warmup, self.schedule = float(weight_decay), int(warmup), schedule
        self.gamma, self.cos_t_max, self.cos_min_lr, self.step_size = float(gamma), int(cos_t_max), float(cos_min_lr), int(step_size)
        self.rop_factor, self.rop_patience = float(rop_factor), int(rop_patience)
        self.epoch = int(completed_epochs)
        self._sched_lr = self._lr_at_epoch(self.epoch)
        self.lr = self._sched_lr
        self._best, self._bad = None, 0
        self.global_step = 0
        self.freeze_backbone, self.samples_seen, self.frozen_steps = int(freeze_backbone), 0, 0
        self._adopted = False                  # the frozen phase's output layer has moved into the whole-network state
        self.accumulate_grad_batches = int(accumulate_grad_batches)
        self.gradient_clip_val = None if gradient_clip_val is None else float(gradient_clip_val)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.batches_seen, self.frozen_batches, self.skipped_steps = 0, 0, 0       # calls; calls of frozen windows; windows without a step
        self._window, self._window_frozen = 0, False                                # calls in the open window; whether it is a frozen one
        self._accum: Optional[torch.Tensor] = None                                  # A: the open window's accumulated gradient (k > 1)
        self._pending = None                                                        # k = 1: the call's own gradient on its way to the step
        self.last_grad_norm: Optional[float] = None
        self.log = log
        self.seed = int(seed)
        self.process_group = process_group
        if distributed is None:
            distributed = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size(process_group) > 1
        self.distributed = bool(distributed)
        dev = next(net.nn.parameters()).device
        if teacher is not None and next(teacher.nn.parameters()).device != dev:
            raise ValueError(f'the teacher lives on {next(teacher.nn.parameters()).device}, the model on {dev}')
        from .engine import HipRecognizer
        self.engine = HipRecognizer(net.hparams_record, dev, 'fp32')
        self.engine.load_state({k: v for k, v in net.nn.state_dict().items()}, strict=True)
        # 'medium' = torch.set_float32_matmul_precision('medium') of the reference's cli/train.py:252 (bf16-rounded matmul operands);
        # 'highest' (default) = exact fp32 products, what the gradient-parity tests are stated for
        self.engine.train_begin(matmul_precision)

    def _lr_at_epoch(self, e: int) -> float:
        import math
        if self.schedule == 'exponential':
            return self.base_lr * self.gamma ** e                                                     # lr_scheduler.ExponentialLR
        if self.schedule == 'cosine':                                                                 # CosineAnnealingLR, closed form
            return self.cos_min_lr + (self.base_lr - self.cos_min_lr) * (1 + math.cos(math.pi * e / self.cos_t_max)) / 2
        if self.schedule == 'step':
            return self.base_lr * self.gamma ** (e // self.step_size)                                 # StepLR
        return self.base_lr

    @property
    def frozen(self) -> bool:
        """Whether the next step is the frozen step."""
        return self.samples_seen < self.freeze_backbone

    def _unfreeze(self) -> None:
        """The hand-over: the serving engine's output layer (fp32 master copy, moments, step count) into the whole-network state."""
        self.engine.train_adopt_decoder(self.net._engine)
        self._adopted = True
        if self.log is not None:
            self.log(f'backbone unfrozen after {self.samples_seen} samples ({self.frozen_steps} steps): training the whole network')

    @property
    def _norm_wanted(self) -> bool:
        return self.gradient_clip_val is not None or self.skip_nonfinite

    def _accumulate(self, parts) -> None:
        """A += fl(1/k) g for the flat gradient pieces `parts`, which lie one behind the other in A."""
        import numpy as np
        n = sum(p.numel() for p in parts)
        if self._accum is None or self._accum.numel() != n:
            self._accum = torch.zeros(n, dtype=torch.float32, device=self.engine.device)
        inv_k, off = float(np.float32(1.0) / np.float32(self.accumulate_grad_batches)), 0
        for p in parts:
            self.engine.grad_accumulate(self._accum[off:off + p.numel()], p, inv_k)
            off += p.numel()

    def training_step(self, batch: Dict) -> float:
        """One call of the step on `batch`: its gradient joins the open window, and the call that completes the window takes the
        optimizer step (every call, at accumulate_grad_batches = 1); returns the batch's summed CTC loss (this rank's lines) -- with a
        teacher the weighted total (1 - distill_weight) CTC + distill_weight KD of the two sums in `last_ctc_loss` / `last_kd_loss`."""
        image = batch['image']
        if image.dim() != 4 or image.shape[1] != 1:
            raise ValueError(f'expected a (N,1,H,W) line batch, got {tuple(image.shape)}')
        if self._window == 0:                             # (decided at the start of a window: neither a batch nor a window is split)
            self._window_frozen = self.frozen
            if not self._window_frozen and self.frozen_steps and not self._adopted:
                self._unfreeze()
        self.samples_seen += int(image.shape[0])
        k = self.accumulate_grad_batches
        lam, tau, kd, tz = self.distill_weight, self.distill_temperature, None, None
        if self.teacher is not None:
            with torch.no_grad():                         # the teacher's eval-mode forward on the batch the student sees
                tz, _ = self.teacher.forward(image.to(self.engine.device), batch['seq_lens'])
        if self._window_frozen:
            # `DecoderTrainer.training_step` at this Trainer's rate: only the output layer moves, on the serving engine
            o = self.net.step(dict(batch, image=image.to(self.engine.device)), with_grad=True)
            if tz is not None:                            # (1 - lambda) dCTC + lambda tau (q - p), in place, ahead of the decoder backward
                kdv, _ = self.net._engine.distill_loss(o['probits'], tz, o['output_lens'].numpy(), tau, grad=o['grad_probits'], ctc_weight=1.0 - lam,
                                                       kd_weight=lam)
                kd = float(kdv.sum())
            gw, gb, _ = self.net._engine.decoder_backward(o['grad_probits'])
            loss = float(o['loss'])
            self.frozen_batches += 1
            if k > 1:
                self._accumulate((gw.reshape(-1), gb))
            else:
                self._pending = (gw, gb)
        else:
            x = image.squeeze(1).to(self.engine.device)
            loss = self.engine.train_step(x, torch.as_tensor(batch['seq_lens']).cpu().numpy(), torch.as_tensor(batch['target']).cpu().numpy(),
                                          torch.as_tensor(batch['target_lens']).cpu().numpy(), dropout=self.net.dropout_p,
                                          seed=self.seed * 1000003 + self.batches_seen, teacher_logits=tz, tau=tau, distill_weight=lam)
            if tz is not None:
                loss, kd = loss
            if k > 1:
                self._accumulate((self.engine.train_grad_buffer(),))
        self.batches_seen += 1
        self._window += 1
        if self._window >= k:
            self._optimizer_step()
        self.last_ctc_loss, self.last_kd_loss = loss, kd
        return loss if kd is None else (1.0 - lam) * loss + lam * kd

    def flush(self) -> None:
        """The optimizer step on an incomplete window (its gradients still scaled by 1/k); nothing on an empty one."""
        if self._window:
            self._optimizer_step()

    def _close_window(self) -> None:
        if self._accum is not None:
            self._accum.zero_()
        self._window, self._pending = 0, None

    def _optimizer_step(self) -> None:
        """All-reduce, norm, clip or skip, and the optimizer step on the open window's gradient; closes the window."""
        k, frozen = self.accumulate_grad_batches, self._window_frozen
        eng = self.net._engine if frozen else self.engine
        # ---- the vector the step uses, averaged over the ranks by one collective
        if k > 1:
            vec = self._accum
            if self.distributed:
                torch.distributed.all_reduce(vec, op=torch.distributed.ReduceOp.SUM, group=self.process_group)
                vec.div_(torch.distributed.get_world_size(self.process_group))
        elif frozen:
            gw, gb = self._pending
            if self.distributed:
                reduce_gradients((gw, gb), self.process_group)
            vec = torch.cat([gw.reshape(-1), gb]) if self._norm_wanted else None
        else:
            vec = self.engine.train_grad_buffer()
            if self.distributed:
                torch.distributed.all_reduce(vec, op=torch.distributed.ReduceOp.SUM, group=self.process_group)
                vec.div_(torch.distributed.get_world_size(self.process_group))
        # ---- norm, skip, coefficient
        coef = 1.0
        self.last_grad_norm = None
        if self._norm_wanted:
            import math
            norm = self.last_grad_norm = self.engine.grad_norm(vec)
            if not math.isfinite(norm):
                self._close_window()
                if not self.skip_nonfinite:
                    raise FloatingPointError(f'the gradient norm of optimizer step {self.global_step} is {norm}: no step was taken '
                                             '(skip_nonfinite=True skips such a window instead)')
                self.skipped_steps += 1
                if self.log is not None:
                    self.log(f'optimizer step {self.global_step} skipped: the gradient norm is {norm} ({self.skipped_steps} skipped so far)')
                return
            if self.gradient_clip_val is not None:
                coef = clip_coef(norm, self.gradient_clip_val)
        # ---- the step
        mom = _momentum_of(self.optimizer, self.momentum)
        if frozen:
            if vec is not None:
                if coef != 1.0:
                    eng.grad_accumulate(vec, vec, coef, overwrite=True)               # (ncls x D floats: the extra pass costs nothing)
                nw = eng.hp.num_classes * eng.hp.encoder_dim
                gw, gb = vec[:nw].view(eng.hp.num_classes, eng.hp.encoder_dim), vec[nw:]
            if self.optimizer == 'AdamW':
                eng.decoder_adamw(gw, gb, self.lr, weight_decay=self.weight_decay)
            else:
                eng.decoder_optim_step(self.optimizer, gw, gb, self.lr, weight_decay=self.weight_decay, momentum=mom)
            self.frozen_steps += 1
        elif k == 1 and coef == 1.0:
            if self.optimizer == 'AdamW':
                self.engine.train_adamw(self.lr, weight_decay=self.weight_decay)
            else:
                self.engine.train_optim_step(self.optimizer, self.lr, weight_decay=self.weight_decay, momentum=mom)
        else:
            # (AdamW through the general kernel: bit for bit cocr_train_adamw's step, with the scale fused in)
            self.engine.train_optim_step(self.optimizer, self.lr, weight_decay=self.weight_decay, momentum=mom, grad=vec if k > 1 else None,
                                         grad_scale=coef)
        self._close_window()
        self._after_step()

    def _after_step(self) -> None:
        if self.warmup and self.global_step < self.warmup:                                            # model.py:246-252
            self.lr = min(1.0, float(self.global_step + 1) / self.warmup) * self.base_lr
        elif self.warmup and self.global_step == self.warmup:
            self.lr = self._sched_lr
        self.global_step += 1

    def end_epoch(self, metric: Optional[float] = None) -> float:
        """Epoch-wise scheduler step (model.py:254-265; not during warm-up); `metric` (validation accuracy, larger is better) drives
        'reduceonplateau'.  Returns the learning rate of the next epoch.  An open accumulation window takes its step first."""
        self.flush()
        self.epoch += 1
        if self.warmup and self.global_step < self.warmup:
            return self.lr
        if self.schedule == 'reduceonplateau':
            if metric is not None:
                if self._best is None or metric > self._best:
                    self._best, self._bad = metric, 0
                else:
                    self._bad += 1
                    if self._bad > self.rop_patience:
                        self._sched_lr *= self.rop_factor
                        self._bad = 0
        else:
            self._sched_lr = self._lr_at_epoch(self.epoch)
        self.lr = self._sched_lr
        return self.lr

    def sync_module(self) -> None:
        """Copies every trained parameter and BatchNorm running statistic into `net.nn` (so `state_dict()`, `save_safetensors` and the
        inference path -- re-packed on its next call -- see them).  Training can continue afterwards.  While the backbone is frozen only
        the output layer has moved: it alone is copied, and the serving engine that trains it (with its AdamW state) is kept, not
        re-packed."""
        if self.frozen_steps and not self._adopted:
            _sync_decoder(self.net)
            return
        self._sync_all()

    def _sync_all(self) -> None:
        sd = self.net.nn.state_dict()
        with torch.no_grad():
            for k, v in sd.items():
                if k.endswith('num_batches_tracked'):
                    v.add_(self.batches_seen - self.frozen_batches - int(v))                           # (train-mode forwards only)
                    continue
                v.copy_(torch.from_numpy(self.engine.train_value(k)).to(v.device).reshape(v.shape))

    # ---- everything a step or an epoch end reads, out and back in ------------------------------------------------
    HYPER = ('base_lr', 'weight_decay', 'optimizer', 'momentum', 'warmup', 'schedule', 'gamma', 'cos_t_max', 'cos_min_lr', 'step_size',
             'rop_factor', 'rop_patience', 'seed', 'matmul_precision', 'freeze_backbone', 'accumulate_grad_batches', 'gradient_clip_val',
             'skip_nonfinite')
    COUNTERS = ('epoch', 'global_step', 'samples_seen', 'frozen_steps', '_adopted', 'lr', '_sched_lr', '_best', '_bad', 'batches_seen',
                'frozen_batches', 'skipped_steps', '_window', '_window_frozen')

    def state_dict(self) -> Dict:
        """{'values': the flat value vector (parameters, then BatchNorm statistics), 'slot0', 'slot1': the optimizer's two state vectors
        (device copies), 'optim': {kind, step, dec_steps}, 'counters', 'hyper'} and, while the frozen phase's output layer has not moved
        into the whole-network state, 'decoder_state' ([master | slot 0 | slot 1] of the serving engine) with 'decoder_optim'
        {kind, step}.  While an accumulation window is open (counters['_window'] calls in): 'accum', the vector A.  'distill': None
        without a teacher, else {'weight', 'temperature', 'teacher': the teacher's hyper-parameters, codec and compute_dtype}."""
        st = self.engine.train_optim_state()
        out = {'values': self.engine.train_value_buffer().clone(), 'slot0': st['slot0'].clone(), 'slot1': st['slot1'].clone(),
               'optim': {'kind': st['kind'], 'step': st['step'], 'dec_steps': st['dec_steps']},
               'counters': {k: getattr(self, k) for k in self.COUNTERS}, 'hyper': {k: getattr(self, k) for k in self.HYPER}}
        if self.frozen_steps and not self._adopted:
            d = self.net._engine.decoder_optim_state()
            out['decoder_state'] = d['state'].clone()
            out['decoder_optim'] = {'kind': d['kind'], 'step': d['step']}
        if self._window and self.accumulate_grad_batches > 1:
            out['accum'] = self._accum.clone()
        out['distill'] = self._distill_record()
        return out

    def _distill_record(self) -> Optional[Dict]:
        if self.teacher is None:
            return None
        import json
        return {'weight': self.distill_weight, 'temperature': self.distill_temperature, 'teacher': json.loads(json.dumps(_model_record(self.teacher)))}

    def load_state_dict(self, sd: Dict) -> None:
        """Puts a `state_dict()` back into this trainer, its engine and `net.nn`; the model layout must be the one it was taken from.
        A state from before the gradient window loads as `upgrade_state` describes."""
        sd = upgrade_state(sd)
        was, now = sd['distill'], self._distill_record()
        if (was is None) != (now is None):
            raise ValueError('the state was written ' + ('with a teacher: give the teacher again' if now is None else 'without a teacher'))
        for k in (() if was is None else ('weight', 'temperature', 'teacher')):
            if was[k] != now[k]:
                raise ValueError(f'the distillation is not the one the state was written with: {k} ' +
                                 ('differs' if k == 'teacher' else f'is {now[k]!r}, was {was[k]!r}'))
        values, st = self.engine.train_value_buffer(), self.engine.train_optim_state()
        for name, have in (('values', values), ('slot0', st['slot0']), ('slot1', st['slot1'])):
            if tuple(sd[name].shape) != tuple(have.shape):
                raise ValueError(f'the state does not fit this model\'s layout: {name} has {sd[name].numel()} floats, the model {have.numel()}')
        for k in self.HYPER:
            setattr(self, k, sd['hyper'][k])
        for k in self.COUNTERS:
            setattr(self, k, sd['counters'][k])
        values.copy_(sd['values'].to(values.device))
        st['slot0'].copy_(sd['slot0'].to(values.device))
        st['slot1'].copy_(sd['slot1'].to(values.device))
        self.engine.train_optim_restore(sd['optim']['kind'], sd['optim']['step'], sd['optim']['dec_steps'])
        self._accum, self._pending, self.last_grad_norm = None, None, None
        if self._window:
            if self.accumulate_grad_batches < 2 or 'accum' not in sd:
                raise ValueError('the state has an open accumulation window but no accumulated gradient')
            self._accum = sd['accum'].to(values.device, torch.float32).contiguous().clone()
        self._sync_all()
        if 'decoder_state' in sd:
            # still in (or just out of) the frozen phase: the output layer and its optimizer state live on the serving engine
            eng = self.net.engine(self.engine.device)
            state = sd['decoder_state'].to(self.engine.device).contiguous()
            eng.decoder_optim_restore(sd['decoder_optim']['kind'], sd['decoder_optim']['step'], state)      # (a vector of another size: ValueError)
            _sync_decoder(self.net)


# ---- the state file of `fit(save_state=True)` ---------------------------------------------------------------------------------------
STATE_TENSORS = ('values', 'slot0', 'slot1', 'decoder_state', 'accum')
FINGERPRINT = ('n_train', 'n_val', 'seed', 'batch_size', 'edge', 'augment', 'height', 'pad')


def write_state_file(path: str, tensors: Dict[str, torch.Tensor], meta: Dict) -> None:
    """One safetensors file: `tensors` and, in its JSON header's `__metadata__`, `meta` as a JSON string under 'fit_state'.  Written
    beside `path` and moved over it, so that a cut never leaves half a file under the name."""
    import json
    import os
    import safetensors.torch
    blob = safetensors.torch.save({k: v.detach().cpu().contiguous() for k, v in tensors.items()}, metadata={'fit_state': json.dumps(meta)})
    tmp = f'{path}.tmp'
    with open(tmp, 'wb') as fp:
        fp.write(blob)
    os.replace(tmp, path)


def read_state_file(path: str, tensors: bool = True):
    """(tensors {name: CPU tensor}, meta) of a `write_state_file`; tensors=False reads the header only."""
    import json
    import struct
    import safetensors.torch
    with open(path, 'rb') as fp:
        data = fp.read() if tensors else None
        if data is None:
            n = struct.unpack('<Q', fp.read(8))[0]
            header = json.loads(fp.read(n))
        else:
            header = json.loads(data[8:8 + struct.unpack('<Q', data[:8])[0]])
    meta = (header.get('__metadata__') or {}).get('fit_state')
    if meta is None:
        raise ValueError(f'{path} is not a training state file (no fit_state record)')
    return (safetensors.torch.load(data) if tensors else None), json.loads(meta)


def data_fingerprint(data) -> Dict:
    """What decides the batches of an epoch: a state file continues on the data set it was written with."""
    return {'n_train': int(data.n_train), 'n_val': len(data.lines) - int(data.n_train), 'seed': int(data.seed), 'batch_size': int(data.batch_size),
            'edge': int(data.edge), 'augment': bool(data.augment), 'height': int(data.height), 'pad': int(data.pad)}


def check_fingerprint(saved: Dict, now: Dict) -> None:
    for k in FINGERPRINT:
        if saved.get(k) != now.get(k):
            raise ValueError(f'the data set is not the one the state was written with: {k} is {now.get(k)!r}, was {saved.get(k)!r}')


def _model_record(net: PytorchRecognitionModel) -> Dict:
    """hyper_params and codec as `save_safetensors` records them (with the dropout probabilities the model trains with)."""
    hp = net.hparams_record.as_dict()
    hp.update(zip(('input_dropout_p', 'feed_forward_dropout_p', 'attention_dropout_p', 'conv_dropout_p'), net.dropout_p))
    return {'hyper_params': hp, 'codec': net.codec.c2l, 'compute_dtype': net.compute_dtype}


def _save_fit_state(path: str, net, data, trainer: 'Trainer', progress: Dict) -> None:
    sd = trainer.state_dict()
    meta = dict(_model_record(net), format=1, data=data_fingerprint(data), fit=progress,
                trainer={k: sd[k] for k in ('optim', 'counters', 'hyper', 'decoder_optim') if k in sd})
    if sd['distill'] is not None:
        meta['distill'] = sd['distill']
    write_state_file(path, {k: sd[k] for k in STATE_TENSORS if k in sd}, meta)


def _resume_fit(path: str, net, data, log, **trainer_kw):
    """(net, trainer, progress) of the state file `path`: the model it describes (or `net`, if given and of that layout), a Trainer in
    the state it was written in."""
    import json
    from .codec import PytorchCodec
    tensors, meta = read_state_file(path)
    check_fingerprint(meta['data'], data_fingerprint(data))
    rec = meta['hyper_params']
    if net is None:
        net = PytorchRecognitionModel(**rec, codec=PytorchCodec(meta['codec']), compute_dtype=meta['compute_dtype'])
        net = net.to(data.device).eval()
    else:
        have = _model_record(net)
        for k, v in rec.items():
            if have['hyper_params'].get(k) != v:
                raise ValueError(f'the model is not the one the state was written with: {k} is {have["hyper_params"].get(k)!r}, was {v!r}')
        if json.loads(json.dumps(have['codec'])) != meta['codec']:
            raise ValueError('the model is not the one the state was written with: the codecs differ')
    meta['trainer'] = upgrade_state(dict(meta['trainer'], distill=meta.get('distill')))
    hyper = dict(meta['trainer']['hyper'])
    hyper['lr'] = hyper.pop('base_lr')
    was = meta['trainer']['distill']
    if was is not None:                                   # the two numbers come from the state unless given (then they must agree)
        if trainer_kw.get('teacher') is None:
            raise ValueError('the state was written with a teacher: give the teacher again')
        for kw, k in (('distill_weight', 'weight'), ('distill_temperature', 'temperature')):
            if trainer_kw.get(kw) is None:
                trainer_kw[kw] = was[k]
    trainer_kw = {k: v for k, v in trainer_kw.items() if v is not None}
    trainer = Trainer(net, log=log, **hyper, **trainer_kw)
    trainer.load_state_dict(dict(tensors, **meta['trainer']))
    return net, trainer, meta['fit']


# ---- the fit loop and `python -m conformer_ocr_amd.train` (the reference's `cocr train`, cli/train.py:100-380) ----------------------
def fit(net: Optional[PytorchRecognitionModel], data, trainer: Optional[Trainer] = None, epochs: int = 100, quit: str = 'fixed', min_epochs: int = 0,
        lag: int = 10, output: Optional[str] = 'model', log=print, save_state: bool = False, resume: Optional[str] = None, **trainer_kw) -> Dict:
    """Trains `net` on `data` (a `dataset.GroundTruthDataset`).  Per epoch: `training_step` on every batch of `data.batches(epoch)`,
    `sync_module`, validation CER (`data.validate`), `end_epoch(1 - CER)`, `{output}_{epoch}.safetensors` and, when the CER is the best
    so far, `{output}_best.safetensors` (no files with output=None); one log line with the summed loss (with a teacher: the weighted
    total and its CTC and KD parts), lines/s and the CER.
    quit 'fixed': `epochs` epochs; 'early': stops once `lag` epochs in a row did not improve the best CER and at least `min_epochs`
    ran (`epochs` still bounds the run).  Returns {'best_epoch', 'best_cer', 'history': [(loss, lines/s, cer), ...], 'net', 'trainer'}.

    save_state: after each epoch's checkpoint, `{output}_state.safetensors` -- the trainer's `state_dict()`, the loop's own bookkeeping,
    the model's hyper-parameters and codec and a fingerprint of `data`.  resume: such a file; the model (built
    from the file when `net` is None) and a new trainer take its state and the loop continues at the next epoch, `epochs` staying the
    total count.  A data set with another fingerprint or a model of another layout is refused (ValueError)."""
    import shutil
    import time
    from .pred import save_safetensors
    if quit not in ('fixed', 'early'):
        raise ValueError("quit must be 'fixed' or 'early'")
    if save_state and output is None:
        raise ValueError('save_state needs an output prefix')
    first = 0
    if resume is not None:
        if trainer is not None:
            raise ValueError('resume builds its own trainer from the state file')
        net, trainer, progress = _resume_fit(resume, net, data, log, **trainer_kw)
        best_epoch, best_cer, bad = progress['best_epoch'], progress['best_cer'], progress['bad']
        history = [tuple(h) for h in progress['history']]
        first = len(history)
    else:
        trainer = trainer or Trainer(net, **trainer_kw)
        best_epoch, best_cer, bad, history = -1, None, 0, []
    dev = trainer.engine.device
    for epoch in range(first, int(epochs)):
        t0, loss, lines, skipped0 = time.perf_counter(), 0.0, 0, trainer.skipped_steps
        ctc, kd = 0.0, 0.0
        for batch in data.batches(epoch):
            loss += trainer.training_step(batch)
            lines += int(batch['image'].shape[0])
            if trainer.teacher is not None:
                ctc, kd = ctc + trainer.last_ctc_loss, kd + trainer.last_kd_loss
        trainer.flush()                                   # (an epoch's last window may be incomplete)
        torch.cuda.synchronize(dev)
        rate = lines / max(time.perf_counter() - t0, 1e-9)
        trainer.sync_module()
        cer = float(data.validate(net))
        trainer.end_epoch(1.0 - cer)
        improved = best_cer is None or cer < best_cer
        if improved:
            best_epoch, best_cer, bad = epoch, cer, 0
        else:
            bad += 1
        if output is not None:
            path = f'{output}_{epoch}.safetensors'
            save_safetensors(net, path)
            if improved:
                shutil.copyfile(path, f'{output}_best.safetensors')
        history.append((loss, rate, cer))
        if save_state:
            _save_fit_state(f'{output}_state.safetensors', net, data, trainer,
                            {'best_epoch': best_epoch, 'best_cer': best_cer, 'bad': bad, 'history': [list(h) for h in history]})
        if log is not None:
            skipped = trainer.skipped_steps - skipped0
            parts = f' (CTC {ctc:.4f}, KD {kd:.4f})' if trainer.teacher is not None else ''
            log(f'epoch {epoch}: loss {loss:.4f}{parts}  {rate:.1f} lines/s  val CER {cer:.4f}{f"  {skipped} steps skipped" if skipped else ""}'
                f'{"  (best)" if improved else ""}')
        if quit == 'early' and bad >= int(lag) and epoch + 1 >= int(min_epochs):
            break
    return {'best_epoch': best_epoch, 'best_cer': best_cer, 'history': history, 'net': net, 'trainer': trainer}


# the reference's RECOGNITION_HYPER_PARAMS (default_specs.py): model shape and the training defaults the command exposes
MODEL_DEFAULTS = dict(encoder_dim=144, num_encoder_layers=16, num_attention_heads=4, feed_forward_expansion_factor=4, conv_expansion_factor=2,
                      input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1, conv_kernel_size=31,
                      half_step_residual=True, subsampling_conv_channels=32, subsampling_factor=4)


def load_codec_file(path: str):
    """The codec file of `-c/--codec`: JSON {grapheme: [labels]}, as the reference loads it (cli/train.py:296-298)."""
    import json
    from .codec import PytorchCodec
    with open(path, encoding='utf-8') as fp:
        c2l = json.load(fp)
    if not isinstance(c2l, dict) or not c2l or not all(isinstance(k, str) and k and isinstance(v, list) and v and all(isinstance(x, int) for x in v)
                                                       for k, v in c2l.items()):
        raise ValueError(f'{path}: a codec file is a JSON object of grapheme -> list of integer labels')
    return PytorchCodec(c2l)


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(prog='python -m conformer_ocr_amd.train',
                                 description='Trains a recognition model from PAGE / ALTO / line-image ground truth on the GPU.')
    ap.add_argument('ground_truth', nargs='*', help='training files (added to -t)')
    ap.add_argument('-t', '--training-files', action='append', default=[], help='file of training file names, one per line, or a glob')
    ap.add_argument('-e', '--evaluation-files', action='append', default=[], help='file of evaluation file names, one per line, or a glob')
    ap.add_argument('-f', '--format-type', choices=('path', 'page', 'alto', 'xml'), default='path')
    ap.add_argument('-p', '--partition', type=float, default=0.9, help='training share of the lines without -e')
    ap.add_argument('-B', '--batch-size', type=int, default=32)
    ap.add_argument('--pad', type=int, default=16)
    ap.add_argument('--line-height', type=int, default=96)
    ap.add_argument('--edge', type=int, default=200, help='width bucket edge of the batches')
    ap.add_argument('--optimizer', choices=OPTIMIZERS, default='AdamW', help='Select optimizer')
    ap.add_argument('-m', '--momentum', type=float, default=0.9, help='Momentum (SGD and RMSprop)')
    ap.add_argument('-r', '--lrate', type=float, default=3e-4)
    ap.add_argument('-w', '--weight-decay', type=float, default=1e-5)
    ap.add_argument('--warmup', type=int, default=35000)
    ap.add_argument('--schedule', choices=Trainer.SCHEDULES, default='cosine')
    ap.add_argument('-g', '--gamma', type=float, default=0.1, help='Decay factor of the exponential and step schedules')
    ap.add_argument('-ss', '--step-size', type=int, default=10, help='Number of epochs between two decays of the step schedule')
    ap.add_argument('--sched-patience', type=int, default=5, help='Epochs without improvement before reduceonplateau lowers the rate')
    ap.add_argument('--cos-max', type=int, default=100)
    ap.add_argument('--cos-min-lr', type=float, default=3e-5)
    ap.add_argument('-q', '--quit', choices=('fixed', 'early'), default='fixed')
    ap.add_argument('-N', '--epochs', type=int, default=100)
    ap.add_argument('--min-epochs', type=int, default=10)
    ap.add_argument('--lag', type=int, default=10)
    ap.add_argument('-u', '--normalization', choices=('NFD', 'NFKD', 'NFC', 'NFKC'), default='NFD')
    ap.add_argument('--normalize-whitespace', dest='normalize_whitespace', action='store_true', default=True)
    ap.add_argument('--no-normalize-whitespace', dest='normalize_whitespace', action='store_false')
    ap.add_argument('--augment', dest='augment', action='store_true', default=True)
    ap.add_argument('--no-augment', dest='augment', action='store_false')
    ap.add_argument('-i', '--load', default=None, help='safetensors archive or checkpoint to continue training')
    ap.add_argument('--resize', choices=('fail', 'union', 'new'), default='fail',
                    help='with --load, when the training alphabet has characters the model does not know: fail, add them to the codec and '
                         'the output layer (union), or make the codec exactly the training alphabet (new)')
    ap.add_argument('--freeze-backbone', type=int, default=0, help='number of samples to keep the backbone (everything but last layer) frozen')
    ap.add_argument('-c', '--codec', default=None, help='JSON codec file {grapheme: [labels]} for a new model, instead of the training alphabet')
    ap.add_argument('--accumulate', type=int, default=1, metavar='K', help='optimizer step on the gradients of K batches (accumulate_grad_batches)')
    ap.add_argument('--clip-norm', type=float, default=None, metavar='X', help='clip the gradient to this global L2 norm (gradient_clip_val)')
    ap.add_argument('--skip-nonfinite', action='store_true', help='take no optimizer step on a gradient whose norm is Inf or NaN')
    ap.add_argument('--teacher', default=None, metavar='FILE',
                    help='safetensors archive or checkpoint of a (larger) model of the same alphabet to distill from: the loss becomes '
                         '(1 - weight) CTC + weight KD against its per-frame posteriors')
    ap.add_argument('--distill-weight', type=float, default=None, metavar='L',
                    help='weight of the distillation term, in [0, 1] (default 0.5: a placeholder, not tuned on real material)')
    ap.add_argument('--distill-temperature', type=float, default=None, metavar='TAU',
                    help='temperature both posteriors are softened with (default 2.0: a placeholder, not tuned on real material)')
    ap.add_argument('-o', '--output', default='model', help='prefix of the written models')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--precision', choices=('medium', 'highest'), default='medium', help='matmul precision of the training step')
    ap.add_argument('--hyper-params', default=None, help='JSON object overriding the model hyper-parameters of a new model')
    ap.add_argument('--save-state', action='store_true', help='after every epoch, write {output}_state.safetensors: what --resume continues from')
    ap.add_argument('--resume', default=None, metavar='FILE',
                    help='continue the run that wrote this state file (model, optimizer, schedule and counters come from it; -N stays the '
                         'total epoch count; implies --save-state)')
    return ap


def check_args(ap, args) -> None:
    """The exclusions between the command's options (`ap.error`: exit status 2)."""
    if args.codec and args.load:
        ap.error('-c/--codec describes a new model: a loaded model brings its codec (--resize adapts it)')
    if args.resize != 'fail' and not args.load:
        ap.error('--resize adapts a loaded model: give -i/--load')
    if args.freeze_backbone < 0:
        ap.error('--freeze-backbone is a number of samples')
    if args.momentum < 0:
        ap.error('-m/--momentum must not be negative')
    if args.accumulate < 1:
        ap.error('--accumulate is a number of batches, at least 1')
    if args.clip_norm is not None and not args.clip_norm > 0:
        ap.error('--clip-norm must be positive')
    if not args.teacher and (args.distill_weight is not None or args.distill_temperature is not None):
        ap.error('--distill-weight and --distill-temperature describe the distillation: give --teacher')
    if args.distill_weight is not None and not 0.0 <= args.distill_weight <= 1.0:
        ap.error('--distill-weight must lie in [0, 1]')
    if args.distill_temperature is not None and not (args.distill_temperature > 0 and args.distill_temperature != float('inf')):
        ap.error('--distill-temperature must be positive')
    if args.resume:
        for flag, given in (('-i/--load', args.load), ('-c/--codec', args.codec), ('--resize', args.resize != 'fail')):
            if given:
                ap.error(f'--resume continues the model of the state file: {flag} cannot be given with it')
        args.save_state = True


def main(argv=None) -> int:
    import glob
    import json
    import os
    import numpy as np
    ap = build_parser()
    args = ap.parse_args(argv)
    check_args(ap, args)

    def expand(entries):
        out = []
        for e in entries:
            if os.path.isfile(e) and not e.lower().endswith(('.xml', '.png', '.jpg', '.jpeg', '.tif', '.tiff')):
                with open(e, encoding='utf-8') as fp:
                    out.extend(l.strip() for l in fp if l.strip())
            else:
                out.extend(sorted(glob.glob(e)) or [e])
        return out
    from .dataset import GroundTruthDataset
    from .ocr import load_model
    from .synth import make_state_dict
    from .spec import HParams
    train_files = expand(args.training_files) + list(args.ground_truth)
    if not train_files:
        ap.error('no training data: give files or -t')
    codec, net, old_classes = None, None, None
    if args.resume:
        from .codec import PytorchCodec
        _, meta = read_state_file(args.resume, tensors=False)
        codec, old_classes = PytorchCodec(meta['codec']), int(meta['hyper_params']['num_classes'])
    if args.codec:
        codec = load_codec_file(args.codec)
    if args.load:
        net = load_model(args.load, device=args.device)
        codec, old_classes = net.codec, net.hparams_record.num_classes
    try:
        data = GroundTruthDataset(train_files, expand(args.evaluation_files) or None, format_type=args.format_type, partition=args.partition,
                                  normalization=args.normalization, normalize_whitespace=args.normalize_whitespace, height=args.line_height,
                                  pad=args.pad, batch_size=args.batch_size, edge=args.edge, seed=args.seed, augment=args.augment, codec=codec,
                                  device=args.device, resize=args.resize, codec_num_classes=old_classes)
    except ValueError as e:
        if args.codec and str(e).startswith('the model\'s codec does not cover'):
            raise ValueError(str(e).replace('the model\'s codec', f'the codec of {args.codec}', 1)) from None
        raise
    if net is not None and args.resize != 'fail':
        from .pred import resize_output
        was, now = set(codec.c2l), set(data.codec.c2l)
        resize_output(net, data.codec, data.row_map, seed=args.seed)
        print(f'resize {args.resize}: {old_classes} -> {data.num_classes} classes; kept {len(was & now)}, added {len(now - was)} '
              f'({"".join(sorted(now - was))!r}), dropped {len(was - now)} characters')
    teacher = load_model(args.teacher, device=args.device) if args.teacher else None
    if args.resume:
        res = fit(None, data, epochs=args.epochs, quit=args.quit, min_epochs=args.min_epochs, lag=args.lag, output=args.output, save_state=True,
                  resume=args.resume, teacher=teacher, distill_weight=args.distill_weight, distill_temperature=args.distill_temperature)
        return _report(res, args.output)
    if net is None:
        from .pred import PytorchRecognitionModel
        hp = dict(MODEL_DEFAULTS, **json.loads(args.hyper_params or '{}'))
        hp.update(height=args.line_height, num_classes=data.codec.max_label + 1)
        net = PytorchRecognitionModel(**hp, codec=data.codec)
        shape = HParams.from_kwargs(**{k: v for k, v in hp.items() if not k.endswith('dropout_p')})
        state = make_state_dict(shape, seed=args.seed)
        net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
        net = net.to(args.device).eval()
    elif net.height != args.line_height:
        ap.error(f'the loaded model takes lines of {net.height} rows, not {args.line_height}')
    trainer = Trainer(net, lr=args.lrate, weight_decay=args.weight_decay, optimizer=args.optimizer, momentum=args.momentum, warmup=args.warmup,
                      schedule=args.schedule, gamma=args.gamma, step_size=args.step_size, rop_patience=args.sched_patience,
                      cos_t_max=args.cos_max, cos_min_lr=args.cos_min_lr, seed=args.seed, matmul_precision=args.precision,
                      freeze_backbone=args.freeze_backbone, log=print, accumulate_grad_batches=args.accumulate,
                      gradient_clip_val=args.clip_norm, skip_nonfinite=args.skip_nonfinite, teacher=teacher,
                      distill_weight=0.5 if args.distill_weight is None else args.distill_weight,
                      distill_temperature=2.0 if args.distill_temperature is None else args.distill_temperature)
    res = fit(net, data, trainer, epochs=args.epochs, quit=args.quit, min_epochs=args.min_epochs, lag=args.lag, output=args.output,
              save_state=args.save_state)
    return _report(res, args.output)


def _report(res: Dict, output: str) -> int:
    if res['best_epoch'] < 0:
        print('Model did not improve during training.')
        return 1
    print(f'Best model {output}_best.safetensors (epoch {res["best_epoch"]}, val CER {res["best_cer"]:.4f})')
    return 0


if __name__ == '__main__':
    import sys
    sys.exit(main())
