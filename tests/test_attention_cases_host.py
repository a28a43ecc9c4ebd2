"""CPU: what the cases of tests/attention_cases.py are meant to do, asserted on the kernels' decision rule restated on the float64 scores
(`simulate`: per 16-query walk, key steps of 32 -- the 32-key form -- and of 64 -- the merged and the resident forms), and the float64
reference itself against the oracle's attention.  A pattern changed so that it no longer reaches the rescale branch fails here, not
silently on the GPU."""
import numpy as np
import pytest
import torch

from conformer_ocr_amd import synth
from tests import attention_cases as ac

GEOS = list(ac.GEOMETRY)


def _walks(T):
    return -(-T // 16)


def _steps(T, tile):
    return -(-T // tile)


@pytest.mark.parametrize('geometry', GEOS)
def test_rising_staircase_fires_at_every_step_and_underflows_on_the_longest_lines(geometry):
    for T in ac.LENGTHS:
        c = ac.make('rising', geometry, T)
        for tile in (32, 64):
            ev, rise = ac.simulate(c, tile)
            assert (ev == _steps(T, tile) - 1).all(), (T, tile)
            assert T <= tile or 11.0 <= rise <= 16.5 * tile / 32, (T, tile, rise)
        S, _ = ac.scores(c, 'bf16')
        climb = S.max(-1) - S[..., :32].max(-1)
        print(f'{geometry} T={T}: cumulative rise {climb.min():.1f} .. {climb.max():.1f}')
        if T >= 600:
            assert climb.min() > 126.0       # the first steps' contributions underflow after the rescales (2^-126: the smallest normal float32)


@pytest.mark.parametrize('geometry', GEOS)
def test_falling_staircase_never_fires_and_later_numerators_underflow(geometry):
    for T in ac.LENGTHS:
        c = ac.make('falling', geometry, T)
        for tile in (32, 64):
            assert ac.simulate(c, tile)[0].sum() == 0
        S, _ = ac.scores(c, 'bf16')
        if T >= 600:
            assert (S.min(-1) - S.max(-1)).max() < -150.0


@pytest.mark.parametrize('geometry', GEOS)
def test_threshold_rise_of_7p5_does_not_fire_and_8p5_does(geometry):
    for T in ac.LENGTHS:
        c = ac.make('threshold', geometry, T)
        S, _ = ac.scores(c, 'bf16')
        for tile in (32, 64):
            ev, rise = ac.simulate(c, tile)
            has_step = T > (64 if T > 64 else 32) and (tile == 32 or T > 64)
            for n in range(c.N):
                for h in range(c.heads):
                    want = 1 if has_step and (n + h) % 2 == 1 else 0
                    assert (ev[n, h] == want).all(), (T, tile, n, h)
        if T > 64:
            d = S[:, :, 0, -1] - S[:, :, 0, 0]                        # the rise itself, as the kernels' operands give it
            for n in range(c.N):
                for h in range(c.heads):
                    assert (7.3 < d[n, h] < 7.7) if (n + h) % 2 == 0 else (8.3 < d[n, h] < 8.7), d[n, h]
            assert 2.0 ** 7.3 < np.exp2(S - S[..., :1]).max() < 2.0 ** 8.7      # a numerator of an unmoved reference: up to 2^7.5 as a bf16 operand


@pytest.mark.parametrize('geometry', GEOS)
def test_one_dominating_key_gives_its_v_row(geometry):
    seen = set()
    for T in ac.LENGTHS:
        c = ac.make('dominant', geometry, T)
        for mode in ('bf16', 'fp32'):
            ref = ac.reference(c, mode)
            for n in range(c.N):
                for h in range(c.heads):
                    p = ac.dominant_key(T, n, h)
                    seen.add('first' if p == 0 else 'last' if p == T - 1 else p)
                    assert np.abs(ref[n, :, h] - c.v[n, h, p]).max() < 1e-12
    assert seen >= {'first', 'last', 63, 64}


@pytest.mark.parametrize('geometry', GEOS)
def test_mixed_wave_one_query_of_a_walk_jumps_while_fifteen_drop(geometry):
    for T in ac.LENGTHS:
        c = ac.make('mixed', geometry, T)
        S, _ = ac.scores(c, 'bf16')
        for tile in (32, 64):
            ev, rise = ac.simulate(c, tile)
            if T <= 64:
                assert ev.sum() == 0
                continue
            assert 38.0 < rise < 41.0
            for w in range(_walks(T)):
                rows = S[:, :, 16 * w:16 * w + 16]
                jump = rows[..., 64:96].max(-1) - rows[..., :64].max(-1)          # (N, h, queries of the walk)
                up = (jump > 38.0).sum(-1)
                assert ((up == 1) | ((up == 0) & (16 * w + 16 > T))).all()         # one jumper per walk (a partial last walk may have lost its own)
                assert ((jump > 38.0) | (jump < -38.0)).all()
                assert (ev[:, :, w] == up).all(), (T, tile, w)


@pytest.mark.parametrize('geometry', GEOS)
def test_single_jump_of_300_and_where_it_falls(geometry):
    for T in ac.LENGTHS:
        c = ac.make('jump300', geometry, T)
        ev32, rise32 = ac.simulate(c, 32)
        ev64, rise64 = ac.simulate(c, 64)
        for n in range(c.N):
            J = ac.jump_key(T, n)
            assert (ev32[n] == (1 if J >= 32 else 0)).all() and (ev64[n] == (1 if J >= 64 else 0)).all(), (T, n, J)
        if T > 64:
            assert 295.0 < rise64 < 305.0 and 295.0 < rise32 < 305.0 and np.exp2(np.float32(-rise64)) == 0.0      # alpha underflows to exactly 0
    # the multi-pass lengths: the jump in the second pass (321, 600, 705) and in the third (705)
    passes = {T: {ac.jump_key(T, n) // ac.PASS_KEYS[T] for n in range(ac.n_lines(T))} for T in ac.PASS_KEYS}
    assert 1 in passes[321] and 1 in passes[600] and {1, 2} <= passes[705], passes


@pytest.mark.parametrize('geometry', GEOS)
def test_equal_scores_give_the_mean_of_the_valid_rows(geometry):
    for T in ac.LENGTHS:
        c = ac.make('equal', geometry, T)
        assert ac.simulate(c, 32)[0].sum() == 0 and ac.simulate(c, 64)[0].sum() == 0
        for mode in ('bf16', 'fp32'):
            ref = ac.reference(c, mode)
            mean = c.v.astype(np.float64).mean(2)                                  # (N, h, dh)
            assert np.abs(ref - mean[:, None]).max() < 1e-13


@pytest.mark.parametrize('geometry', GEOS)
def test_random_keys_under_the_positional_table_fire_in_half_the_walks(geometry):
    for T in ac.LENGTHS:
        if T <= 64:
            continue
        c = ac.make('table', geometry, T)
        for mode in ('bf16', 'fp32'):
            for tile in (32, 64):
                ev, rise = ac.simulate(c, tile, mode)
                print(f'{geometry} T={T} {mode} tile {tile}: {int(ev.sum())} events in {ev.size} walks, largest rise {rise:.1f}')
                if T > 2 * tile:
                    assert ev.sum() >= 0.5 * ev.size, (T, mode, tile)


def test_generators_are_pinned():
    """The recipes, so that a change of them shows here and not as a changed case."""
    assert [ac.n_lines(T) for T in ac.LENGTHS] == [1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2]
    assert [ac.jump_key(321, n) for n in range(3)] == [256, 64, 256] and ac.jump_key(600, 0) == 384 and [ac.jump_key(705, n) for n in range(2)] == [576, 320]
    assert ac.jump_key(1, 0) == 0 and ac.jump_key(17, 1) == 8 and [ac.jump_key(129, n) for n in range(3)] == [64, 32, 96]
    c = ac.make('rising', 'dh64', 129)
    assert c.q.shape == (3, 4, 129, 64) and not c.q.any() and np.array_equal(ac.bf16(c.k), c.k) and np.array_equal(ac.bf16(c.v), c.v)
    assert c.k[0, 1, 128, 0] == ac.bf16(np.float32(13.0 * 4 - 0.25 * ((128 * 7 + 1) % 5)))
    x = np.array([1.0, 1.00390625, 1.01171875, 1.005, -3.0e38, 2.0 ** -130, 300.0], dtype=np.float32)       # ties go to even, both ways
    assert ac.bf16(x)[:4].tolist() == [1.0, 1.0, 1.015625, 1.0078125]
    assert np.array_equal(ac.bf16(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())


@pytest.mark.parametrize('cfg,heads', [('cfg2', 4), ('cfg1', 4)])
def test_reference_agrees_with_the_oracle_attention_in_float64(cfg, heads):
    """`reference` shares no code with oracle/conformer_ref.py's `mhsa`; on the q, k, v that a random model's projection produces (synth's
    own u, v and positional projection) the two float64 evaluations agree to what the float32 sinusoids -- each side's own, a float32 step
    (6e-8) apart here and there -- leave on rows whose scores span 75 log2 units: measured 2e-6, nine orders below a wrong index."""
    from oracle.conformer_ref import Oracle
    hp = synth.hparams(cfg, num_encoder_layers=1, num_attention_heads=heads, num_classes=8, height=32, subsampling_conv_channels=32)
    state = synth.make_state_dict(hp, seed=17)
    for key in state:                                                             # a gain at which the rows are peaked: a wrong index would show
        if key.endswith(('query_proj.linear.weight', 'u_bias', 'v_bias')):
            state[key] = state[key] * np.float32(6.0)
    o = Oracle(hp, state, torch.float64)
    for B, T in ((2, 77), (1, 130)):
        y = torch.from_numpy(np.random.default_rng(T).standard_normal((B, T, hp.encoder_dim)))
        taps = {}
        with torch.no_grad():
            o.mhsa(y, 0, taps)
        q, k, v = (taps[f'l0.{nm}'].numpy().transpose(0, 2, 1, 3) for nm in 'qkv')
        c = ac.Case(q, k, v, state, 0)
        ref = ac.reference(c, 'fp32').reshape(B, T, -1)
        S, _ = ac.scores(c, 'fp32')
        spread = float((S.max(-1) - S.min(-1)).max())
        dev = float(np.abs(ref - taps['l0.ctx'].numpy()).max())
        print(f'{cfg} T={T}: score spread {spread:.1f} log2 units, reference vs oracle {dev:.3g}')
        assert spread > 8.0 and dev < 1e-5


def test_gain_16_model_takes_the_rescale_branch_in_most_walks():
    """The model-level case of tests/test_hip_bf16_path.py (cfg2, two blocks, query path x 16): simulated on the fp32 oracle's own q, k, v,
    both rules fire in at least half of the 72 walks (2 lines x 4 heads x 9) of each block."""
    from oracle.conformer_ref import Oracle
    hp, state = ac.gain16_model()
    image, lens = synth.make_lines(2, hp.height, 520, seed=77, widths=[520, 483])
    taps = {}
    with torch.no_grad():
        lg, _ = Oracle(hp, state).forward(torch.from_numpy(image), torch.from_numpy(lens), taps)
    assert torch.isfinite(lg).all()
    for l in range(hp.num_encoder_layers):
        q, k, v = (taps[f'l{l}.{nm}'].numpy().transpose(0, 2, 1, 3) for nm in 'qkv')
        c = ac.Case(q, k, v, state, l)
        S, _ = ac.scores(c, 'fp32')
        for tile in (64, 32):
            ev, rise = ac.simulate(c, tile, 'fp32')
            print(f'block {l}, {tile}-key rule: {int(ev.sum())} events, {int((ev > 0).sum())} of {ev.size} walks fire, largest rise {rise:.1f}; scores {S.min():.0f} .. {S.max():.0f}')
            assert ev.size == 72 and ev.sum() >= 36
