"""Host side of fine-tuning a loaded model: the codec that grows (`codec.resize_codec`), the output layer that
grows with it (`pred.resize_output`, `synth.output_row`), and the command's `-c/--codec`, `--resize`, `--freeze-backbone` handling
as far as it needs no device."""
import hashlib
import json
import math

import numpy as np
import pytest
import torch

from conformer_ocr_amd import synth
from conformer_ocr_amd.codec import PytorchCodec, resize_codec
from conformer_ocr_amd.pred import PytorchRecognitionModel, resize_output, save_safetensors

FAIL_MESSAGE = "the model's codec does not cover the training alphabet: missing 'dx'"


def _abc():
    return PytorchCodec('abc')           # a, b, c -> 1, 2, 3; the model has 11 classes: rows 4..10 belong to no grapheme


def test_union_keeps_every_old_row_and_appends_the_missing_characters():
    new, row_map = resize_codec(_abc(), ['abd', 'xa'], 'union', 11)
    assert new.c2l == {'a': [1], 'b': [2], 'c': [3], 'd': [11], 'x': [12]}
    assert row_map.dtype == np.int32 and row_map.tolist() == list(range(11)) + [-1, -1]
    assert new.encode('xad') == [12, 1, 11]
    # without the layer's size the codec's own top label bounds the old rows
    new, row_map = resize_codec(_abc(), ['abd', 'xa'], 'union')
    assert new.c2l['d'] == [4] and new.c2l['x'] == [5] and row_map.tolist() == [0, 1, 2, 3, -1, -1]
    # nothing missing: the codec is unchanged, the map the identity
    new, row_map = resize_codec(_abc(), ['abc'], 'union', 11)
    assert new.c2l == _abc().c2l and row_map.tolist() == list(range(11))


def test_new_becomes_exactly_the_training_alphabet():
    new, row_map = resize_codec(_abc(), ['abd', 'xa'], 'new', 11)
    assert new.c2l == {'a': [1], 'b': [2], 'd': [3], 'x': [4]}
    assert row_map.dtype == np.int32 and row_map.tolist() == [0, 1, 2, -1, -1]
    # kept graphemes are renumbered in the order of their OLD labels, whatever the order of the texts
    old = PytorchCodec({'q': [7], 'a': [2], 'm': [5]})
    new, row_map = resize_codec(old, ['zmq'], 'new', 9)
    assert new.c2l == {'m': [1], 'q': [2], 'z': [3]} and row_map.tolist() == [0, 5, 7, -1]


def test_fail_is_todays_behaviour():
    with pytest.raises(ValueError) as e:
        resize_codec(_abc(), ['abd', 'xa'], 'fail', 11)
    assert str(e.value) == FAIL_MESSAGE
    from conformer_ocr_amd.dataset import check_codec
    with pytest.raises(ValueError) as e:
        check_codec(_abc(), ['abd', 'xa'])
    assert str(e.value) == FAIL_MESSAGE
    same, row_map = resize_codec(_abc(), ['abc', 'ca'], 'fail', 11)
    assert same.c2l == _abc().c2l and row_map.tolist() == list(range(11))
    with pytest.raises(ValueError):
        resize_codec(_abc(), ['abc'], 'intersect', 11)
    with pytest.raises(ValueError):
        resize_codec(_abc(), ['abc'], 'union', 3)            # label 3 does not fit a 3-row layer


def test_multi_label_codecs_grow_under_union_and_are_refused_under_new():
    old = PytorchCodec({'a': [1], 'ch': [2, 3], 'c': [4]})
    new, row_map = resize_codec(old, ['chad', 'hc'], 'union', 6)
    # the greedy longest match takes 'ch' as one grapheme: the lone 'h' of the second text and 'd' are what is missing
    assert new.c2l == {'a': [1], 'ch': [2, 3], 'c': [4], 'd': [6], 'h': [7]}
    assert row_map.tolist() == [0, 1, 2, 3, 4, 5, -1, -1]
    assert new.encode('chadh') == [2, 3, 1, 6, 7]
    with pytest.raises(ValueError, match='1:1'):
        resize_codec(old, ['chad'], 'new', 6)
    # a 1:1 codec with a two-character grapheme is fine under 'new': the grapheme is a token, its letters are not missing
    lig = PytorchCodec({'a': [1], 'ch': [2], 'b': [3]})
    new, row_map = resize_codec(lig, ['chaz'], 'new', 4)
    assert new.c2l == {'a': [1], 'ch': [2], 'z': [3]} and row_map.tolist() == [0, 1, 2, -1]


def _output_row(seed, c, fan_in):
    """`synth.output_row` restated: PCG64 seeded with the first 8 bytes (little-endian) of sha256('seed:resize:c'), weight then bias
    from U(-1/sqrt(fan_in), 1/sqrt(fan_in))."""
    g = np.random.Generator(np.random.PCG64(int.from_bytes(hashlib.sha256(f'{seed}:resize:{c}'.encode()).digest()[:8], 'little')))
    a = 1 / math.sqrt(fan_in)
    w = g.uniform(-a, a, fan_in).astype(np.float32)
    return w, np.float32(g.uniform(-a, a))


def _tiny(codec):
    hp = synth.hparams('tiny')
    net = PytorchRecognitionModel(**hp.as_dict(), input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1,
                                  codec=codec)
    state = synth.make_state_dict(hp, seed=7)
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return net.eval(), hp


def test_resize_output_carries_rows_and_draws_the_new_ones(tmp_path):
    net, hp = _tiny(_abc())
    w0, b0 = net.nn['decoder'].weight.detach().clone(), net.nn['decoder'].bias.detach().clone()
    enc0 = {k: v.clone() for k, v in net.nn['encoder'].state_dict().items()}
    new, row_map = resize_codec(net.codec, ['abd', 'xa'], 'union', hp.num_classes)
    resize_output(net, new, row_map, seed=5)
    dec = net.nn['decoder']
    D = hp.encoder_dim
    assert isinstance(dec, torch.nn.Linear) and tuple(dec.weight.shape) == (13, D) and tuple(dec.bias.shape) == (13,)
    assert not dec.weight.requires_grad and not dec.bias.requires_grad
    assert torch.equal(dec.weight[:11], w0) and torch.equal(dec.bias[:11], b0)
    for j, c in ((11, 'd'), (12, 'x')):
        w, b = _output_row(5, c, D)
        assert np.array_equal(dec.weight[j].numpy(), w) and dec.bias[j].item() == b
        sw, sb = synth.output_row(5, c, D)
        assert np.array_equal(sw, w) and sb == b and sw.dtype == np.float32
        assert float(np.abs(w).max()) <= 1 / math.sqrt(D) and abs(float(b)) <= 1 / math.sqrt(D)
    assert net.hparams_record.num_classes == 13 and net.hparams_record.encoder_dim == D
    assert net.codec is new
    assert all(torch.equal(v, enc0[k]) for k, v in net.nn['encoder'].state_dict().items())
    # the archive round trip keeps the new size and codec
    path = str(tmp_path / 'resized.safetensors')
    save_safetensors(net, path)
    back = PytorchRecognitionModel.load_safetensors(path)
    assert back.hparams_record.num_classes == 13 and back.codec.c2l == new.c2l
    assert torch.equal(back.nn['decoder'].weight, dec.weight) and torch.equal(back.nn['decoder'].bias, dec.bias)


def test_a_characters_row_does_not_depend_on_what_else_was_added():
    one, hp = _tiny(_abc())
    five, _ = _tiny(_abc())
    resize_output(one, *resize_codec(one.codec, ['ax'], 'union', hp.num_classes), seed=0)
    resize_output(five, *resize_codec(five.codec, ['axyzdw'], 'union', hp.num_classes), seed=0)
    assert one.hparams_record.num_classes == 12 and five.hparams_record.num_classes == 16
    jx = five.codec.c2l['x'][0]
    assert one.codec.c2l['x'] == [11] and jx == 13                 # d, w, x, y, z in sorted order from 11
    assert torch.equal(one.nn['decoder'].weight[11], five.nn['decoder'].weight[jx])
    assert torch.equal(one.nn['decoder'].bias[11], five.nn['decoder'].bias[jx])
    other, _ = _tiny(_abc())
    resize_output(other, *resize_codec(other.codec, ['ax'], 'union', hp.num_classes), seed=1)
    assert not torch.equal(one.nn['decoder'].weight[11], other.nn['decoder'].weight[11])


def test_resize_output_new_mode_and_bad_maps():
    net, hp = _tiny(_abc())
    w0, b0 = net.nn['decoder'].weight.detach().clone(), net.nn['decoder'].bias.detach().clone()
    new, row_map = resize_codec(net.codec, ['cxa'], 'new', hp.num_classes)
    resize_output(net, new, row_map)
    assert new.c2l == {'a': [1], 'c': [2], 'x': [3]} and net.hparams_record.num_classes == 4
    assert torch.equal(net.nn['decoder'].weight[:3], w0[[0, 1, 3]]) and torch.equal(net.nn['decoder'].bias[:3], b0[[0, 1, 3]])
    with pytest.raises(ValueError):
        resize_output(net, new, [1, 0, 2, 3])                      # the blank must keep row 0
    with pytest.raises(ValueError):
        resize_output(net, new, [0, 1, 2, 9])                      # row 9 of a 4-row layer


def _gt(tmp_path, texts):
    """Line-image ground truth (`-f path`): only the .gt.txt files are read before the codec is settled."""
    files = []
    for i, t in enumerate(texts):
        (tmp_path / f'l{i}.gt.txt').write_text(t, encoding='utf-8')
        files.append(str(tmp_path / f'l{i}.png'))
    return files


def test_codec_file_and_usage_errors_of_the_command(tmp_path, capsys):
    from conformer_ocr_amd import train
    files = _gt(tmp_path, ['abd', 'xa', 'ab'])
    good = tmp_path / 'codec.json'
    good.write_text(json.dumps({'a': [1], 'b': [2], 'ch': [3, 4]}), encoding='utf-8')
    codec = train.load_codec_file(str(good))
    assert codec.c2l == {'a': [1], 'b': [2], 'ch': [3, 4]} and codec.max_label == 4
    bad = tmp_path / 'bad.json'
    bad.write_text(json.dumps(['a', 'b']), encoding='utf-8')
    with pytest.raises(ValueError):
        train.load_codec_file(str(bad))
    # a codec file that cannot encode the training alphabet: ValueError naming the characters, before any device work
    with pytest.raises(ValueError, match="missing 'dx'"):
        train.main(['-f', 'path', '-c', str(good), '--device', 'cpu', '-e', files[2]] + files)
    # usage errors
    for argv in (['-c', str(good), '-i', 'model.safetensors'] + files,             # a loaded model brings its codec
                 ['--resize', 'union'] + files,                                     # resizing needs a loaded model
                 ['--resize', 'grow', '-i', 'model.safetensors'] + files,
                 ['--freeze-backbone', '-3'] + files):
        with pytest.raises(SystemExit) as e:
            train.main(['-f', 'path'] + argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def test_dataset_signature_carries_the_resize():
    import inspect
    from conformer_ocr_amd.dataset import GroundTruthDataset
    from conformer_ocr_amd.train import Trainer
    p = inspect.signature(GroundTruthDataset.__init__).parameters
    assert p['resize'].default == 'fail' and p['codec_num_classes'].default is None
    assert inspect.signature(Trainer.__init__).parameters['freeze_backbone'].default == 0
