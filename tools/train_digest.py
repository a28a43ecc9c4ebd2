#!/usr/bin/env python3
"""Digests of the training step, for comparing two builds of the library bit for bit:   python tools/train_digest.py [--out FILE]
(the library is the tree's, or the one COCR_LIB_PATH names).  The step has no floating-point atomics, so two builds that launch the same
kernels on the same data print the same JSON.

Per case: one `train_step` and one AdamW step on a fresh engine; the loss's bit pattern, the sha256 of the gradient vector after the step
and of the value vector (parameters, then BatchNorm running statistics) after the optimizer.  Cases: the four of
tests/test_hip_train_full.py (factor 2 / 4 / 8 frontends, both attention forms, a class count that is no multiple of 4, split-K and
single-split weight gradients), each in 'highest' and 'medium', with dropout (0.1 x 4, seed 1234) and without; cfg2x2 again with
COCR_TRAIN_ATTN_NAIVE=1, and in 'medium' with COCR_TRAIN_NO_TN=1.  The `shapes` leg adds the kernel forms those four do not select: every
case of tests/train_ref.py's SHAPE_CASES in 'highest', MEDIUM_SHAPE_CASES in 'medium' and the 'rows' case of tests/test_hip_train_pin.py in
both (scalar column sums and k_pad_cols: nohalf97ff2; 2 and 4 column blocks: d512k7, widest; the splits == 1 store: widest; the flat
depthwise finals: k33; 66 chunks and the 64- / 256-row chunk forms: rows), with and without dropout like the others.  Each leg runs in a
process of its own (the switches are read at different times); this process only starts them and does not open the GPU."""
import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {'default': {}, 'attn_naive': {'COCR_TRAIN_ATTN_NAIVE': '1'}, 'no_tn': {'COCR_TRAIN_NO_TN': '1'}, 'shapes': {}}
LEG_TIMEOUT = {'shapes': 120}      # seconds; the others 300.  The shapes leg's 32 steps take 5 s on an idle MI355X (the other legs 2 - 3 s)
SEED = 1234


def run_leg(leg):
    sys.path.insert(0, ROOT)
    import torch
    from conformer_ocr_amd import synth
    from conformer_ocr_amd.engine import HipRecognizer
    from tests import train_ref
    from tests.test_hip_train_full import CASES

    def sha(t):
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    if leg == 'shapes':                   # (case, modes); the inputs are those of the tests that pin these cases
        runs = [(n, ['highest', 'medium'] if n in train_ref.MEDIUM_SHAPE_CASES else ['highest']) for n in train_ref.SHAPE_CASES] + [('rows', ['highest', 'medium'])]
    else:
        runs = [(n, ['medium'] if leg == 'no_tn' else ['highest', 'medium']) for n in (list(CASES) if leg == 'default' else ['cfg2x2'])]
    out = {}
    for name, modes in runs:
        if leg == 'shapes':
            hp, state, image, lens, targets = train_ref.inputs(name)
        else:
            c = CASES[name]
            hp = c['hp']()
            state = synth.make_state_dict(hp, seed=c['seed'], decoder_gain=c['gain'])
            image, lens = synth.make_lines(c['n'], hp.height, c['W'], seed=c['seed'], widths=c['widths'])
            targets = c['targets']
        x = torch.from_numpy(image[:, 0]).cuda()
        tg, tl = [v for s in targets for v in s], [len(s) for s in targets]
        for mode in modes:
            for drop in ((0.1, 0.1, 0.1, 0.1), (0.0, 0.0, 0.0, 0.0)):
                eng = HipRecognizer(hp, torch.device('cuda', 0), 'fp32')
                eng.load_state(state)
                eng.train_begin(mode)
                loss = eng.train_step(x, lens, tg, tl, dropout=drop, seed=SEED)
                grads = sha(eng.train_grad_buffer())
                eng.train_adamw(1e-3, weight_decay=1e-2)
                torch.cuda.synchronize()
                out[f'{leg}/{name}/{mode}/{"drop" if drop[0] else "nodrop"}'] = {
                    'loss_bits': struct.pack('<f', loss).hex(), 'loss': loss, 'grads': grads, 'values': sha(eng.train_value_buffer())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=sorted(LEGS))
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(run_leg(args.leg)))
        return 0
    out = {}
    for leg, env in LEGS.items():
        t0 = time.monotonic()
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', leg], env={**os.environ, **env}, stdout=subprocess.PIPE, text=True,
                           timeout=LEG_TIMEOUT.get(leg, 300))
        if r.returncode != 0:
            print(f'leg {leg} ended with status {r.returncode}', file=sys.stderr)
            return r.returncode or 1
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
        print(f'leg {leg}: {time.monotonic() - t0:.0f} s', file=sys.stderr)
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(text + '\n')
    print(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
