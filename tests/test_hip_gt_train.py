"""Training from page ground truth end to end: PAGE + ALTO files -> GroundTruthDataset (strip cache, GPU augmentation) -> train.fit ->
a model that reads those pages through recognize_pages; and the command line (`python -m conformer_ocr_amd.train`)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conformer_ocr_amd import synth
from tests import gt_synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cer(net, pages):
    from conformer_ocr_amd.evaluate import ErrorRate
    from conformer_ocr_amd.page import recognize_pages
    res = recognize_pages(net, [(img, lines) for _, img, lines in pages])
    er = ErrorRate()
    for (_, _, lines), recs in zip(pages, res):
        er.update([r['text'] for r in recs], [ln.text for ln in lines])
    return er.compute()


@pytest.mark.timeout(600)
def test_fit_from_page_ground_truth_learns_to_read_the_pages(tmp_path):
    """A 2-block model of the metric's shapes from random weights, 16 lines on two pages (one PAGE, one ALTO), augmentation on,
    batches of 8 (two steps per epoch), lr 1e-3 with a 10-step warm-up, exact fp32 products.  Calibrated once: 150 epochs = 300 steps
    (the step count of tests/test_hip_train_full.py's run on plain batches) take the CER on the pages, read through recognize_pages,
    from >= 0.9 to <= 0.05."""
    from conformer_ocr_amd.dataset import GroundTruthDataset
    from conformer_ocr_amd.pred import PytorchRecognitionModel
    from conformer_ocr_amd.train import Trainer, fit
    pages = gt_synth.make_pages(str(tmp_path))
    files = [x for x, _, _ in pages]
    data = GroundTruthDataset(files, evaluation_files=files, format_type='xml', batch_size=8, augment=True, seed=1)
    assert data.n_train == 16
    hp = synth.hparams('cfg2', num_encoder_layers=2, num_classes=data.codec.max_label + 1)
    net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1,
                                  codec=data.codec, compute_dtype='bf16')
    state = synth.make_state_dict(hp, seed=1, decoder_gain=1.0)
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    net = net.to('cuda:0').eval()
    assert _cer(net, pages) >= 0.9
    tr = Trainer(net, lr=1e-3, weight_decay=1e-2, warmup=10)
    res = fit(net, data, tr, epochs=150, output=None, log=None)
    losses = [h[0] for h in res['history']]
    assert losses[-1] < 0.05 * losses[0]
    cer = _cer(net, pages)
    assert cer <= 0.05, (cer, res['history'][-5:])
    assert res['best_cer'] <= 0.05


@pytest.mark.timeout(600)
def test_train_command_writes_a_model_the_ocr_command_reads(tmp_path):
    from conformer_ocr_amd.pred import PytorchRecognitionModel
    pages = gt_synth.make_pages(str(tmp_path), lines_per_page=6)
    hp = synth.hparams('cfg2', num_encoder_layers=2).as_dict()
    for k in ('num_classes', 'height'):
        hp.pop(k)
    out = str(tmp_path / 'm')
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, '-m', 'conformer_ocr_amd.train', '-f', 'xml', '-N', '2', '-B', '4', '--warmup', '5', '-r', '1e-3', '-o', out,
           '--hyper-params', json.dumps(hp), '-t', str(tmp_path / 'page_*.xml')]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert 'epoch 1:' in r.stdout, r.stdout + r.stderr[-3000:]
    for f in ('m_0.safetensors', 'm_1.safetensors', 'm_best.safetensors'):
        assert os.path.exists(tmp_path / f), f
    net = PytorchRecognitionModel.load_safetensors(out + '_best.safetensors')
    assert net.hparams_record.num_encoder_layers == 2 and len(net.codec) > 0
    xml = pages[0][0]
    txt = str(tmp_path / 'page_0.txt')
    r = subprocess.run([sys.executable, '-m', 'conformer_ocr_amd.ocr', '-m', out + '_best.safetensors', '-i', xml, txt], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(txt, encoding='utf-8') as fp:
        assert len(fp.read().split('\n')) - 1 == len(pages[0][2])
