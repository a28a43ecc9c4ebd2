#!/usr/bin/env python3
"""
Golden fixture of the TRAINING step (tests/golden/tiny_train.npz), made by running THE REFERENCE ITSELF in train mode:
`/root/reference/conformer_ocr/conformer/encoder.py::ConformerEncoder` with `.train()` (BatchNorm batch statistics; all dropout
probabilities 0 so that the step is deterministic), the `nn.Linear` decoder and the two loss lines of `RecognitionModel._step`
(model.py:119,136-142), float64, followed by `loss.backward()`.  Stored: loss, probits, the gradient of every parameter, the
BatchNorm running statistics after the step.  Run in the authoring container only:   python tests/golden/make_train_golden.py

`tiny_train_drop` is the same step WITH dropout: every `nn.Dropout` instance of the reference encoder is given, by its module path, a forward
that multiplies by the mask the HIP step generates for that site (tests/train_ref.py: `drop_keep`, `drop_site`, scale 1 / (1 - p) in float32).
Four distinct probabilities, so that two sites taking each other's probability cannot cancel.  The fixture pins WHERE each mask acts and over
which index; the mask generator itself is the restatement's.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, '/root/reference')

from conformer_ocr.conformer.encoder import ConformerEncoder  # noqa: E402  (the reference)

from conformer_ocr_amd import synth  # noqa: E402

TARGETS = {'tiny_train': dict(config='tiny', seed=4321, n=3, W=64, widths=[64, 37, 50], targets=[[3, 1, 4], [1, 5], [9, 2, 6, 5]]),
           # the 'tiny' case with the device's dropout masks at the reference's own nn.Dropout modules
           'tiny_train_drop': dict(config='tiny', seed=4321, n=3, W=64, widths=[64, 37, 50], targets=[[3, 1, 4], [1, 5], [9, 2, 6, 5]],
                                   dropout=(0.1, 0.2, 0.3, 0.4), drop_seed=20240229),
           # round 4: the metric model's shapes (D = 256, 4 heads of 64, 256 conv channels, kernel 31), two blocks, short ragged lines.  4.8 M
           # parameters: per tensor the fixture holds 64 SAMPLED gradient entries (seeded indices) and its sum / sum of magnitudes / L2 norm /
           # largest magnitude instead of the whole gradient.
           'cfg2x2_train': dict(config='cfg2', over=dict(num_encoder_layers=2), seed=5, n=2, W=120, widths=[120, 77], targets=[[5, 9, 9, 3], [17]], sampled=64)}


# nn.Dropout instances of a conformer block by (index in the block's Sequential, path below `.module.`): (site, which feed-forward module,
# tensor layout at that point)
BLOCK_DROPOUTS = {(0, 'sequential.3'): ('ff_hidden', 0, 'btd'), (0, 'sequential.5'): ('ff_out', 0, 'btd'),
                  (1, 'attention.dropout'): ('attn_weights', 0, 'bhtt'), (1, 'dropout'): ('attn_out', 0, 'btd'),
                  (2, 'sequential.8'): ('conv_out', 0, 'bdt'),
                  (3, 'sequential.3'): ('ff_hidden', 1, 'btd'), (3, 'sequential.5'): ('ff_out', 1, 'btd')}


def install_masks(enc, p4, seed):
    """Every nn.Dropout of the reference encoder -> a forward applying the restated mask of its site.  Returns the number installed."""
    import re
    from tests.train_ref import drop_factor, site_of, site_p

    def forward_of(site, l, which, layout):
        def forward(x):
            p = site_p(site, p4)
            if layout == 'bdt':          # the conv module's dropout sees (B, D, T); the device's index runs over (line, frame, channel)
                b, d, t = x.shape
                return x * drop_factor((b, t, d), seed, site_of(site, l, which), p, x.dtype).permute(0, 2, 1)
            return x * drop_factor(x.shape, seed, site_of(site, l, which), p, x.dtype)
        return forward
    n = 0
    for path, mod in enc.named_modules():
        if not isinstance(mod, torch.nn.Dropout):
            continue
        if path == 'conv_subsample.out.1':
            mod.forward = forward_of('input', 0, 0, 'btd')
        else:
            m = re.fullmatch(r'layers\.(\d+)\.sequential\.(\d+)\.module\.(.+)', path)
            site, which, layout = BLOCK_DROPOUTS[(int(m.group(2)), m.group(3))]          # (KeyError: a Dropout this table does not know)
            mod.forward = forward_of(site, int(m.group(1)), which, layout)
        n += 1
    return n


def main(only=None):
    torch.manual_seed(0)
    for name, t in TARGETS.items():
        if only and name not in only:
            continue
        hp = synth.hparams(t['config'], **t.get('over', {}))
        state = synth.make_state_dict(hp, seed=t['seed'], decoder_gain=1.0)
        image, lens = synth.make_lines(t['n'], hp.height, t['W'], seed=t['seed'], widths=t['widths'])
        enc = ConformerEncoder(in_channels=1, input_dim=hp.height, encoder_dim=hp.encoder_dim, num_layers=hp.num_encoder_layers,
                               num_attention_heads=hp.num_attention_heads, feed_forward_expansion_factor=hp.feed_forward_expansion_factor,
                               conv_expansion_factor=hp.conv_expansion_factor, input_dropout_p=0.0, feed_forward_dropout_p=0.0,
                               attention_dropout_p=0.0, conv_dropout_p=0.0, conv_kernel_size=hp.conv_kernel_size,
                               half_step_residual=hp.half_step_residual, subsampling_conv_channels=hp.subsampling_conv_channels,
                               subsampling_factor=hp.subsampling_factor).double()
        dec = torch.nn.Linear(hp.encoder_dim, hp.num_classes, bias=True).double()
        enc.load_state_dict({k[len('encoder.'):]: torch.from_numpy(np.asarray(v)).double() if np.asarray(v).dtype.kind == 'f' else torch.from_numpy(np.asarray(v))
                             for k, v in state.items() if k.startswith('encoder.')})
        dec.load_state_dict({'weight': torch.from_numpy(state['decoder.weight']).double(), 'bias': torch.from_numpy(state['decoder.bias']).double()})
        enc.train()
        dec.train()
        if t.get('dropout'):
            assert install_masks(enc, t['dropout'], t['drop_seed']) == 1 + 7 * hp.num_encoder_layers
        x = torch.from_numpy(image).double().squeeze(1).transpose(1, 2)             # model.py:132
        eo, el = enc(x, torch.from_numpy(lens))                                     # model.py:134
        probits = dec(eo)
        logits = torch.nn.functional.log_softmax(probits, dim=-1)                   # model.py:136
        target = torch.tensor([c for s in t['targets'] for c in s], dtype=torch.long)
        tl = torch.tensor([len(s) for s in t['targets']], dtype=torch.long)
        crit = torch.nn.CTCLoss(reduction='sum', zero_infinity=True)                # model.py:119
        loss = crit(logits.transpose(0, 1), target, el.long(), tl)                  # model.py:139-142
        loss.backward()
        out = {'loss': np.float64(loss.item()), 'probits': probits.detach().numpy(), 'out_lens': el.numpy(), 'target': target.numpy(),
               'target_lens': tl.numpy()}
        if t.get('dropout'):
            out['dropout'], out['drop_seed'] = np.asarray(t['dropout'], dtype=np.float64), np.int64(t['drop_seed'])
        named = [('encoder.' + k, p) for k, p in enc.named_parameters()] + [('decoder.' + k, p) for k, p in dec.named_parameters()]
        if t.get('sampled'):
            out['probits'] = out['probits'].astype(np.float32)
            rng = np.random.default_rng(t['seed'])
            for k, p in named:
                gflat = p.grad.numpy().reshape(-1)
                idx = np.sort(rng.choice(gflat.size, size=min(t['sampled'], gflat.size), replace=False)).astype(np.int64)
                out['gi:' + k], out['gs:' + k] = idx, gflat[idx]
                out['gn:' + k] = np.array([gflat.sum(), np.abs(gflat).sum(), np.sqrt((gflat ** 2).sum()), np.abs(gflat).max()])
        else:
            for k, p in named:
                out['grad:' + k] = p.grad.numpy()
        for k, b in enc.named_buffers():
            if 'running_' in k or 'num_batches' in k:
                out['buf:encoder.' + k] = b.detach().numpy()
        np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
        print(name, 'loss', loss.item(), 'entries', len(out), os.path.getsize(os.path.join(HERE, name + '.npz')))


if __name__ == '__main__':
    main(sys.argv[1:])          # (no arguments: every target; else the named ones)
