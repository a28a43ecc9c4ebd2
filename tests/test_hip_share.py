"""cocr_share_weights: packed copies of one model that read one set of weights (include/cocr.h)."""
import numpy as np
import pytest
import torch

from conformer_ocr_amd import synth
from conformer_ocr_amd.engine import HipRecognizer

pytestmark = pytest.mark.gpu


def _engines(dtype='bf16'):
    hp = synth.hparams('cfg2', num_encoder_layers=2)
    state = synth.make_state_dict(hp, seed=41, decoder_gain=4.0)
    dev = torch.device('cuda', 0)
    owner = HipRecognizer(hp, dev, dtype)
    owner.load_state(state)
    owner.finalize()
    private = HipRecognizer(hp, dev, dtype)
    private.load_state(state)
    private.finalize()
    sharer = HipRecognizer(hp, dev, dtype)
    sharer.share_weights(owner)
    return hp, state, owner, private, sharer


def test_a_model_that_shares_weights_computes_what_its_owner_computes():
    hp, state, owner, private, sharer = _engines()
    img, lens = synth.make_lines(5, hp.height, 700, seed=3, widths=[700, 650, 300, 40, 512])
    x = torch.from_numpy(img[:, 0]).cuda()
    for eng in (owner, private, sharer):
        eng.set_graph(True)
    outs = []
    for rep in range(3):                                 # plain run, captured run, replay
        outs.append([eng.forward(x, lens)[0].cpu().numpy() for eng in (owner, private, sharer)])
    torch.cuda.synchronize()
    for a, b, c in outs:
        assert np.array_equal(a, b) and np.array_equal(a, c)
    # two sharers on two streams at once
    other = HipRecognizer(hp, owner.device, 'bf16')
    other.share_weights(owner)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        l1, _ = sharer.forward(x, lens)
    with torch.cuda.stream(s2):
        l2, _ = other.forward(x, lens)
    torch.cuda.synchronize()
    assert np.array_equal(l1.cpu().numpy(), outs[0][0]) and np.array_equal(l2.cpu().numpy(), outs[0][0])


def test_a_line_longer_than_the_tables_seen_first_by_the_sharer():
    """The positional tables grow for a long line (embedding.py:35-41) -- here inside the model that shares them; the owner, with launch
    sequences captured on the old tables, must follow."""
    hp, state, owner, private, sharer = _engines()
    for eng in (owner, private, sharer):
        eng.set_graph(True)
    img, lens = synth.make_lines(2, hp.height, 600, seed=5)
    x = torch.from_numpy(img[:, 0]).cuda()
    before = [owner.forward(x, lens)[0].cpu().numpy() for _ in range(3)][-1]          # owner: captured on the first tables
    limg, llens = synth.make_lines(1, hp.height, 4 * 5200, seed=6)                     # 5200 frames > the 4999 the first tables cover
    lx = torch.from_numpy(limg[:, 0]).cuda()
    long_shared = sharer.forward(lx, llens)[0].cpu().numpy()
    long_private = private.forward(lx, llens)[0].cpu().numpy()
    assert np.array_equal(long_shared, long_private)
    after = owner.forward(x, lens)[0].cpu().numpy()
    assert np.array_equal(after, before)
    assert np.array_equal(owner.forward(lx, llens)[0].cpu().numpy(), long_private)


def test_weights_change_through_the_owner_only():
    hp, state, owner, private, sharer = _engines('fp32')
    with pytest.raises(RuntimeError, match='owner'):
        sharer.weight_blob()
    with pytest.raises((RuntimeError, ValueError)):
        sharer.share_weights(sharer)
    with pytest.raises((RuntimeError, ValueError)):
        owner.share_weights(sharer)                      # the owner of a sharer cannot share (sharer is not an owner: it shares itself)
    img, lens = synth.make_lines(2, hp.height, 300, seed=9)
    x = torch.from_numpy(img[:, 0]).cuda()
    a = sharer.forward(x, lens)[0].cpu().numpy()
    state2 = {k: (v * 1.01 if k == 'decoder.weight' else v) for k, v in state.items()}
    owner.load_state(state2)
    owner.finalize()                                     # the owner's buffers move
    private.load_state(state2)
    private.finalize()
    b = sharer.forward(x, lens)[0].cpu().numpy()
    assert not np.array_equal(a, b) and np.array_equal(b, private.forward(x, lens)[0].cpu().numpy())
    sharer.load_state(state)
    sharer.finalize()                                    # weights of its own again
    assert np.array_equal(sharer.forward(x, lens)[0].cpu().numpy(), a)
    del owner                                            # (the sharer no longer depends on it)
    assert np.array_equal(sharer.forward(x, lens)[0].cpu().numpy(), a)


def test_owner_finalized_again_in_another_compute_dtype():
    """The header allows weight changes through the owner (set_tensor + finalize): also a finalize in the OTHER compute dtype.  The
    sharer then follows -- layout, plan, workspace and captured launches re-derived at its next forward -- instead of running its bf16
    kernels over an fp32 blob.  And a sharer hands out no blob copy (its view of the owner's buffer may be gone): the owner does."""
    hp, state, owner, private, sharer = _engines('bf16')
    img, lens = synth.make_lines(3, hp.height, 500, seed=12, widths=[500, 420, 77])
    x = torch.from_numpy(img[:, 0]).cuda()
    sharer.set_graph(True)
    bf = [sharer.forward(x, lens)[0].cpu().numpy() for _ in range(3)][-1]
    assert np.array_equal(bf, private.forward(x, lens)[0].cpu().numpy())
    with pytest.raises(RuntimeError, match='owner'):
        sharer.export_blob()
    owner.compute_dtype = 'fp32'
    owner.finalize()
    p32 = HipRecognizer(hp, owner.device, 'fp32')
    p32.load_state(state)
    p32.finalize()
    want = p32.forward(x, lens)[0].cpu().numpy()
    for _ in range(3):                                   # plain, captured, replayed: all on the new blob
        got = sharer.forward(x, lens)[0].cpu().numpy()
        assert np.array_equal(got, want)
    assert np.abs(got - bf).max() > 1e-4                 # (it is the fp32 result, not the old one)
    owner.compute_dtype = 'bf16'
    owner.finalize()
    assert np.array_equal(sharer.forward(x, lens)[0].cpu().numpy(), bf)


# ---- every entry point of a sharing model reads the owner's CURRENT weights (csrc/weights.hip.h), not only its next forward ----------
# one encoder layer, 2 lines of 300 px (75 frames): seconds per case
_SMALL = [('bf16', {}), ('fp32', {}), ('bf16', dict(encoder_dim=144, num_attention_heads=4))]      # the last: a zero-padded model (tr_pad path)


def _small(dtype, **override):
    hp = synth.hparams('cfg2', num_encoder_layers=1, **override)
    state = synth.make_state_dict(hp, seed=41, decoder_gain=4.0)
    img, lens = synth.make_lines(2, hp.height, 300, seed=9)
    return hp, state, torch.from_numpy(img[:, 0]).cuda(), lens


def _engine(hp, dtype, state=None, owner=None):
    eng = HipRecognizer(hp, torch.device('cuda', 0), dtype)
    if owner is not None:
        eng.share_weights(owner)
    else:
        eng.load_state(state)
        eng.finalize()
    return eng


def _grad(hp, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((2, 75, hp.num_classes), generator=g, dtype=torch.float32).cuda()


@pytest.mark.parametrize('dtype,override', _SMALL, ids=['bf16', 'fp32', 'bf16-padded144'])
def test_decoder_backward_of_a_sharer_reads_the_owners_current_weights(dtype, override):
    hp, state, x, lens = _small(dtype, **override)
    owner, private = _engine(hp, dtype, state), _engine(hp, dtype, state)
    sharer = _engine(hp, dtype, owner=owner)
    for eng in (owner, sharer, private):
        eng.forward(x, lens)
    state2 = {k: (v * 1.01 if k == 'decoder.weight' else v) for k, v in state.items()}      # the encoder output `xn` of all three stays valid
    owner.load_state(state2)
    owner.finalize()                                     # the owner's buffers move
    private.load_state(state2)
    private.finalize()
    g = _grad(hp)
    got = sharer.decoder_backward(g, with_input_grad=True)          # no forward in between
    want = private.decoder_backward(g, with_input_grad=True)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert float(want[2].abs().max()) > 0


def test_a_sharer_follows_a_compute_dtype_change_before_its_next_forward():
    hp, state, x, lens = _small('bf16')
    owner = _engine(hp, 'bf16', state)
    sharer = _engine(hp, 'bf16', owner=owner)
    sharer.forward(x, lens)
    owner.compute_dtype = 'fp32'
    owner.finalize()
    fresh = _engine(hp, 'fp32', owner=owner)
    assert sharer.chain_rows(2, 300) == fresh.chain_rows(2, 300)
    with pytest.raises(RuntimeError, match='no forward of shape'):          # its encoder output went with the bf16 workspace
        sharer.decoder_backward(_grad(hp), with_input_grad=True)
    p32 = _engine(hp, 'fp32', state)
    want = p32.forward(x, lens)[0].cpu().numpy()
    assert np.array_equal(sharer.forward(x, lens)[0].cpu().numpy(), want)
    got = sharer.decoder_backward(_grad(hp), with_input_grad=True)
    ref = p32.decoder_backward(_grad(hp), with_input_grad=True)
    for a, b in zip(got, ref):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_owner_destroyed_before_its_sharer(dtype):
    """cocr.h asks for the owner to outlive its sharers; a sharer left behind is not finalized, and says so at every entry point."""
    hp, state, x, lens = _small(dtype)
    owner = _engine(hp, dtype, state)
    sharer = _engine(hp, dtype, owner=owner)
    want = owner.forward(x, lens)[0].cpu().numpy()
    sharer.forward(x, lens)
    torch.cuda.synchronize()
    sharer._weights_owner = None
    del owner
    with pytest.raises(RuntimeError, match='not finalized'):
        sharer.forward(x, lens)
    with pytest.raises(RuntimeError):
        sharer.decoder_backward(_grad(hp), with_input_grad=True)
    with pytest.raises(RuntimeError):
        sharer.chain_rows(2, 300)
    sharer.load_state(state)
    sharer.finalize()                                    # weights of its own
    assert np.array_equal(sharer.forward(x, lens)[0].cpu().numpy(), want)
