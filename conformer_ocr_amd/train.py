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
    them to a file, `fit(resume=...)` continues from one."""

    SCHEDULES = ('constant', 'exponential', 'cosine', 'step', 'reduceonplateau')

    def __init__(self, net: PytorchRecognitionModel, lr: float = 1e-3, weight_decay: float = 1e-3, optimizer: str = 'AdamW', warmup: int = 0,
                 schedule: str = 'constant', gamma: float = 0.1, cos_t_max: int = 50, cos_min_lr: float = 1e-4, step_size: int = 10,
                 rop_factor: float = 0.1, rop_patience: int = 5, completed_epochs: int = 0, seed: int = 0, process_group=None,
                 distributed: Optional[bool] = None, matmul_precision: str = 'highest', freeze_backbone: int = 0, log=None,
                 momentum: float = 0.9):
        if optimizer not in OPTIMIZERS:
            raise ValueError(f'unknown optimizer {optimizer!r}: one of {", ".join(OPTIMIZERS)}')
        if schedule not in self.SCHEDULES:
            raise ValueError(f'Unsupported learning rate scheduler {schedule}.')                      # model.py:309
        if not float(momentum) >= 0.0:
            raise ValueError(f'Invalid momentum value: {momentum}')                                   # torch.optim.SGD / RMSprop
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
        self.log = log
        self.seed = int(seed)
        self.process_group = process_group
        if distributed is None:
            distributed = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size(process_group) > 1
        self.distributed = bool(distributed)
        dev = next(net.nn.parameters()).device
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

    def _frozen_step(self, batch: Dict) -> float:
        """`DecoderTrainer.training_step` at this Trainer's rate: only the output layer moves, on the serving engine."""
        o = self.net.step(dict(batch, image=batch['image'].to(self.engine.device)), with_grad=True)
        eng = self.net._engine
        gw, gb, _ = eng.decoder_backward(o['grad_probits'])
        if self.distributed:
            reduce_gradients((gw, gb), self.process_group)
        if self.optimizer == 'AdamW':
            eng.decoder_adamw(gw, gb, self.lr, weight_decay=self.weight_decay)
        else:
            eng.decoder_optim_step(self.optimizer, gw, gb, self.lr, weight_decay=self.weight_decay, momentum=_momentum_of(self.optimizer, self.momentum))
        self.frozen_steps += 1
        return float(o['loss'])

    def _unfreeze(self) -> None:
        """The hand-over: the serving engine's output layer (fp32 master copy, moments, step count) into the whole-network state."""
        self.engine.train_adopt_decoder(self.net._engine)
        self._adopted = True
        if self.log is not None:
            self.log(f'backbone unfrozen after {self.samples_seen} samples ({self.frozen_steps} steps): training the whole network')

    def training_step(self, batch: Dict) -> float:
        """One optimizer step on `batch`; returns the batch's summed CTC loss (this rank's lines)."""
        image = batch['image']
        if image.dim() != 4 or image.shape[1] != 1:
            raise ValueError(f'expected a (N,1,H,W) line batch, got {tuple(image.shape)}')
        if self.frozen:                                   # (tested at the start of a step: a batch is never split)
            self.samples_seen += int(image.shape[0])
            loss = self._frozen_step(batch)
            self._after_step()
            return loss
        if self.frozen_steps and not self._adopted:
            self._unfreeze()
        self.samples_seen += int(image.shape[0])
        x = image.squeeze(1).to(self.engine.device)
        loss = self.engine.train_step(x, torch.as_tensor(batch['seq_lens']).cpu().numpy(), torch.as_tensor(batch['target']).cpu().numpy(),
                                      torch.as_tensor(batch['target_lens']).cpu().numpy(), dropout=self.net.dropout_p,
                                      seed=self.seed * 1000003 + self.global_step)
        if self.distributed:
            g = self.engine.train_grad_buffer()
            torch.distributed.all_reduce(g, op=torch.distributed.ReduceOp.SUM, group=self.process_group)
            g.div_(torch.distributed.get_world_size(self.process_group))
        if self.optimizer == 'AdamW':
            self.engine.train_adamw(self.lr, weight_decay=self.weight_decay)
        else:
            self.engine.train_optim_step(self.optimizer, self.lr, weight_decay=self.weight_decay, momentum=_momentum_of(self.optimizer, self.momentum))
        self._after_step()
        return loss

    def _after_step(self) -> None:
        if self.warmup and self.global_step < self.warmup:                                            # model.py:246-252
            self.lr = min(1.0, float(self.global_step + 1) / self.warmup) * self.base_lr
        elif self.warmup and self.global_step == self.warmup:
            self.lr = self._sched_lr
        self.global_step += 1

    def end_epoch(self, metric: Optional[float] = None) -> float:
        """Epoch-wise scheduler step (model.py:254-265; not during warm-up); `metric` (validation accuracy, larger is better) drives
        'reduceonplateau'.  Returns the learning rate of the next epoch."""
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
                    v.add_(self.global_step - self.frozen_steps - int(v))                              # (train-mode forwards only)
                    continue
                v.copy_(torch.from_numpy(self.engine.train_value(k)).to(v.device).reshape(v.shape))

    # ---- everything a step or an epoch end reads, out and back in ------------------------------------------------
    HYPER = ('base_lr', 'weight_decay', 'optimizer', 'momentum', 'warmup', 'schedule', 'gamma', 'cos_t_max', 'cos_min_lr', 'step_size',
             'rop_factor', 'rop_patience', 'seed', 'matmul_precision', 'freeze_backbone')
    COUNTERS = ('epoch', 'global_step', 'samples_seen', 'frozen_steps', '_adopted', 'lr', '_sched_lr', '_best', '_bad')

    def state_dict(self) -> Dict:
        """{'values': the flat value vector (parameters, then BatchNorm statistics), 'slot0', 'slot1': the optimizer's two state vectors
        (device copies), 'optim': {kind, step, dec_steps}, 'counters', 'hyper'} and, while the frozen phase's output layer has not moved
        into the whole-network state, 'decoder_state' ([master | slot 0 | slot 1] of the serving engine) with 'decoder_optim'
        {kind, step}."""
        st = self.engine.train_optim_state()
        out = {'values': self.engine.train_value_buffer().clone(), 'slot0': st['slot0'].clone(), 'slot1': st['slot1'].clone(),
               'optim': {'kind': st['kind'], 'step': st['step'], 'dec_steps': st['dec_steps']},
               'counters': {k: getattr(self, k) for k in self.COUNTERS}, 'hyper': {k: getattr(self, k) for k in self.HYPER}}
        if self.frozen_steps and not self._adopted:
            d = self.net._engine.decoder_optim_state()
            out['decoder_state'] = d['state'].clone()
            out['decoder_optim'] = {'kind': d['kind'], 'step': d['step']}
        return out

    def load_state_dict(self, sd: Dict) -> None:
        """Puts a `state_dict()` back into this trainer, its engine and `net.nn`; the model layout must be the one it was taken from."""
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
        self._sync_all()
        if 'decoder_state' in sd:
            # still in (or just out of) the frozen phase: the output layer and its optimizer state live on the serving engine
            eng = self.net.engine(self.engine.device)
            state = sd['decoder_state'].to(self.engine.device).contiguous()
            eng.decoder_optim_restore(sd['decoder_optim']['kind'], sd['decoder_optim']['step'], state)      # (a vector of another size: ValueError)
            _sync_decoder(self.net)


# ---- the state file of `fit(save_state=True)` ---------------------------------------------------------------------------------------
STATE_TENSORS = ('values', 'slot0', 'slot1', 'decoder_state')
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
    hyper = dict(meta['trainer']['hyper'])
    hyper['lr'] = hyper.pop('base_lr')
    trainer = Trainer(net, log=log, **hyper, **trainer_kw)
    trainer.load_state_dict(dict(tensors, **meta['trainer']))
    return net, trainer, meta['fit']


# ---- the fit loop and `python -m conformer_ocr_amd.train` (the reference's `cocr train`, cli/train.py:100-380) ----------------------
def fit(net: Optional[PytorchRecognitionModel], data, trainer: Optional[Trainer] = None, epochs: int = 100, quit: str = 'fixed', min_epochs: int = 0,
        lag: int = 10, output: Optional[str] = 'model', log=print, save_state: bool = False, resume: Optional[str] = None, **trainer_kw) -> Dict:
    """Trains `net` on `data` (a `dataset.GroundTruthDataset`).  Per epoch: `training_step` on every batch of `data.batches(epoch)`,
    `sync_module`, validation CER (`data.validate`), `end_epoch(1 - CER)`, `{output}_{epoch}.safetensors` and, when the CER is the best
    so far, `{output}_best.safetensors` (no files with output=None); one log line with the summed loss, lines/s and the CER.
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
        t0, loss, lines = time.perf_counter(), 0.0, 0
        for batch in data.batches(epoch):
            loss += trainer.training_step(batch)
            lines += int(batch['image'].shape[0])
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
            log(f'epoch {epoch}: loss {loss:.4f}  {rate:.1f} lines/s  val CER {cer:.4f}{"  (best)" if improved else ""}')
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
    if args.resume:
        res = fit(None, data, epochs=args.epochs, quit=args.quit, min_epochs=args.min_epochs, lag=args.lag, output=args.output, save_state=True,
                  resume=args.resume)
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
                      freeze_backbone=args.freeze_backbone, log=print)
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
