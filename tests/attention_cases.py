"""The inputs on which the three relative-position attention kernels (csrc/attention.hip.h) are compared with a float64 softmax
(tests/test_hip_attention.py), built so that the online softmax's lazy rescale -- the running reference `m_run` rises when a query
of a 16-query walk exceeds it by more than 8 log2 units, and the accumulators and the denominator are multiplied by
2^(old - new) -- is taken, not taken, taken by one query of a walk only, and taken in every key pass of the LDS-resident kernel.
tests/test_attention_cases_host.py asserts, without a GPU, what each pattern is meant to do to the kernels' decision rule
(`simulate`) and that `reference` agrees with the oracle's attention.

Scores come from a few coordinates whose values are exact in bfloat16, so q, k and v mean the same to the bf16 and the fp32
engine.  Block 0 of a geometry's model (`weights`) has u = CU e_0 in every head, v = 0 and a zero positional projection:
    score(i, j) = ((q_i + u) . k_j) / sqrt(dh),   in log2 units ~ k_j[0] + a_i k_j[dh - 1]   with q_i = a_i CU e_(dh-1),
CU = sqrt(dh) / log2(e).  Block 1 has random u, v and the positional projection 4 I: its table is 4 x the sinusoids themselves --
every relative position a row of its own, which is what the kernels' shift geometry needs, and a table the host restates exactly
(a product with 4 I has one non-zero term per element: no accumulation order, so the same bf16 roundings on both sides).

All lines of one call have the same number of frames T: the attention core takes one T per launch (no key mask), so the
1 - 3 lines of a case differ in where their pattern is placed, not in length."""
import functools
import math

import numpy as np

LOG2E = math.log2(math.e)
LAZY = 8.0                       # attention.hip.h: the reference moves when a query exceeds it by more than this (log2 units)
LENGTHS = (1, 16, 17, 63, 64, 65, 96, 128, 129, 300, 320, 321, 600, 705)      # 321 = 2 x 192 keys, 600 = 2 x 320, 705 = 3 x 256 (key passes)
PASS_KEYS = {321: 192, 600: 320, 705: 256}     # keys per pass of the resident kernel's multi-pass form (forward.hip: launch_attention)
PATTERNS = ('rising', 'falling', 'threshold', 'dominant', 'mixed', 'jump300', 'equal', 'table')
# head geometries of the kernel forms: (encoder_dim, heads) -> d_head 64 (merged 64-key bf16 form, resident forms, fp32 32-key form), 32
# (merged), 128 (bf16 32-key form), 36 in a 64 slot (dh != dhp, partial store)
GEOMETRY = {'dh64': ('cfg2', 256, 4), 'dh32': ('cfg2', 256, 8), 'dh128': ('cfg4', 512, 4), 'dh36': ('cfg1', 144, 4)}
TABLE_GAIN = 4.0                 # block 1: q, k ~ N(0, 1) x this; positional projection = this x I


def bf16(x):
    """Round to nearest even to bfloat16, as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)).view(np.float32)


def n_lines(T):
    return 1 + LENGTHS.index(T) % 3


def cu(dh):
    """The u coordinate of block 0: (0 + CU) / sqrt(dh) * log2(e) ~ 1, i.e. k_j[0] is key j's score in log2 units."""
    return np.float32(math.sqrt(dh) / LOG2E)


def hparams(geometry):
    from conformer_ocr_amd import synth
    cfg, D, heads = GEOMETRY[geometry]
    return synth.hparams(cfg, num_encoder_layers=2, num_attention_heads=heads)


@functools.lru_cache(maxsize=None)
def weights(geometry):
    """The state dict of a geometry's two-block model: synth's draws with the attention weights of both blocks replaced (module docstring)."""
    from conformer_ocr_amd import synth
    hp = hparams(geometry)
    state = synth.make_state_dict(hp, seed=5)
    D, h = hp.encoder_dim, hp.num_attention_heads
    dh = D // h
    a = 'encoder.layers.%d.sequential.1.module.attention.'
    u0 = np.zeros((h, dh), dtype=np.float32)
    u0[:, 0] = cu(dh)
    state[a % 0 + 'u_bias'] = u0
    state[a % 0 + 'v_bias'] = np.zeros((h, dh), dtype=np.float32)
    state[a % 0 + 'pos_proj.linear.weight'] = np.zeros((D, D), dtype=np.float32)
    g = np.random.default_rng(700 + dh)
    state[a % 1 + 'u_bias'] = (g.standard_normal((h, dh)) * TABLE_GAIN).astype(np.float32)
    state[a % 1 + 'v_bias'] = (g.standard_normal((h, dh)) * TABLE_GAIN).astype(np.float32)
    state[a % 1 + 'pos_proj.linear.weight'] = (np.eye(D) * TABLE_GAIN).astype(np.float32)
    return state


def gain16_model(gain=16.0):
    """The model-level case (tests/test_hip_bf16_path.py): cfg2, two blocks, the 'text' draw of seed 31 with the query path -- query_proj's
    weight and bias, u_bias, v_bias -- of every block x 16: scores of +-120 log2 units, finite logits, the rescale branch on most walks."""
    from conformer_ocr_amd import synth
    hp = synth.hparams('cfg2', num_encoder_layers=2)
    state = synth.make_state_dict(hp, seed=31, decoder_gain=1.0, style='text')
    for key in state:
        if key.endswith(('attention.query_proj.linear.weight', 'attention.query_proj.linear.bias', 'attention.u_bias', 'attention.v_bias')):
            state[key] = (state[key] * np.float32(gain)).astype(np.float32)
    return hp, state


def sinusoids(D, T):
    """Rows p = T - 1 ... -(T - 1) of the sinusoid table as the library computes them (cocr_api.hip: compute_pos_tables -- float32 angle
    from a float32 frequency), the transcendental functions themselves correctly rounded from float64."""
    i = np.arange(0, D, 2)
    div = np.exp((i.astype(np.float32) * np.float32(-(math.log(10000.0) / D))).astype(np.float64)).astype(np.float32)
    ang = (np.arange(T - 1, -T, -1, dtype=np.float32)[:, None] * div[None, :]).astype(np.float64)
    pe = np.zeros((2 * T - 1, D), dtype=np.float32)
    pe[:, 0::2] = np.sin(ang).astype(np.float32)
    pe[:, 1::2] = np.cos(ang).astype(np.float32)
    return pe


class Case:
    """q, k, v: (N, heads, T, dh), in the designed cases float32 with bf16-exact values; `state`, `layer`: the state dict and the block whose
    attention weights (u_bias, v_bias, pos_proj) apply.  `key`: (pattern, geometry, T) of a case of `make`, whose scores and reference are
    computed once per process."""
    def __init__(self, q, k, v, state, layer, key=None):
        self.q, self.k, self.v, self.state, self.layer, self.key = q, k, v, state, layer, key
        self.N, self.heads, self.T, self.dh = q.shape

    def attention_weights(self):
        a = 'encoder.layers.%d.sequential.1.module.attention.' % self.layer
        return tuple(np.asarray(self.state[a + nm]) for nm in ('u_bias', 'v_bias', 'pos_proj.linear.weight'))


def jump_key(T, n):
    """First key of the 300 jump on line n.  The multi-pass lengths: 64 keys into a key pass of the resident kernel -- line 0 in the last
    pass (321, 600: the second; 705: the third), line 1 in the one before, line 2 in the last again.  Other lengths: key 32, 64 or 96 by
    line (the ones the line has), the middle key on lines of at most 32 frames."""
    if T in PASS_KEYS:
        npass = -(-T // PASS_KEYS[T])
        return ((npass - 1 - n) % npass) * PASS_KEYS[T] + 64
    at = [j for j in (64, 32, 96) if j < T]
    return at[n % len(at)] if at else T // 2


def dominant_key(T, n, h):
    """Key 0, key T - 1 (beside the masked keys of the tail tile) and the two sides of the 64-key seam, by (line, head)."""
    at = [p for p in (0, T - 1, 63, 64) if p < T]
    return at[(n + h) % len(at)]


@functools.lru_cache(maxsize=64)
def make(pattern, geometry, T):
    _, D, h = GEOMETRY[geometry]
    dh = D // h
    N = n_lines(T)
    g = np.random.default_rng(1000 * PATTERNS.index(pattern) + 7 * T + dh)
    v = bf16(g.standard_normal((N, h, T, dh)))
    q = np.zeros((N, h, T, dh), dtype=np.float32)
    k = np.zeros((N, h, T, dh), dtype=np.float32)
    j = np.arange(T)
    step = j // 32
    if pattern == 'table':
        q = bf16(g.standard_normal((N, h, T, dh)) * TABLE_GAIN)
        k = bf16(g.standard_normal((N, h, T, dh)) * TABLE_GAIN)
        return Case(q, k, v, weights(geometry), 1, (pattern, geometry, T))
    for n in range(N):
        for hh in range(h):
            wiggle = -0.25 * ((j * 7 + n + hh) % 5)                  # keys of one step are not all equal
            if pattern == 'rising':                                   # the step maximum rises by 12 .. 15 (by head) every 32 keys
                b = (12.0 + hh % 4) * step + wiggle
            elif pattern == 'falling':                                # the first step dominates; later numerators underflow
                b = -(12.0 + hh % 4) * step + wiggle
            elif pattern == 'threshold':                              # one rise at key 64 (key 32 on lines of at most 64 frames): 7.5 must not fire, 8.5 must
                b = np.where(j >= (64 if T > 64 else 32), 7.5 if (n + hh) % 2 == 0 else 8.5, 0.0)
            elif pattern == 'dominant':
                b = wiggle.copy()
                b[dominant_key(T, n, hh)] = 60.0
            elif pattern == 'mixed':                                  # third 32-key step: one query of every walk + 40, the other fifteen - 40
                b = wiggle
                k[n, hh, :, dh - 1] = np.where(step == 2, 40.0, 0.0)
                i = np.arange(T)
                q[n, hh, :, dh - 1] = np.where(i % 16 == (5 + 3 * (i // 16) + n + hh) % 16, 1.0, -1.0) * cu(dh)
            elif pattern == 'jump300':
                b = np.where(j >= jump_key(T, n), 300.0, 0.0) + wiggle
            elif pattern == 'equal':
                b = np.zeros(T)
            else:
                raise ValueError(pattern)
            k[n, hh, :, 0] = b
    return Case(bf16(q), bf16(k), v, weights(geometry), 0, (pattern, geometry, T))


def _scores_of(c, mode):
    u, vb, wpos = c.attention_weights()
    dh, h, T = c.dh, c.heads, c.T
    q32, k64 = c.q, c.k.astype(np.float64)
    if mode == 'bf16':
        # the kernels' query operands: float32 (q + u) x (1/sqrt(dh) x log2(e)), that product of two float32 constants, rounded to bf16
        sc = np.float32(1.0) / np.sqrt(np.float32(dh)) * np.float32(1.44269504088896340736)
        qu = bf16((q32.astype(np.float32) + u[None, :, None, :]) * sc).astype(np.float64)
        qv = bf16((q32.astype(np.float32) + vb[None, :, None, :]) * sc).astype(np.float64)
    elif mode == 'fp32':
        qu = (q32.astype(np.float64) + u[None, :, None, :]) * (LOG2E / math.sqrt(dh))
        qv = (q32.astype(np.float64) + vb[None, :, None, :]) * (LOG2E / math.sqrt(dh))
    else:
        raise ValueError(mode)
    S = qu @ k64.transpose(0, 1, 3, 2)                                # (N, h, T, T), log2 units
    A = np.abs(qu) @ np.abs(k64).transpose(0, 1, 3, 2)                # sum of the products' magnitudes (the fp32 bound)
    if wpos.any():
        pe = sinusoids(dh * h, T)                                      # rows p = T - 1 ... -(T - 1)
        P = (pe.astype(np.float64) @ wpos.astype(np.float64).T)        # one non-zero term per element: exact in float32 as well
        P = (bf16(P) if mode == 'bf16' else P.astype(np.float32)).astype(np.float64).reshape(2 * T - 1, h, dh)
        i, j = np.arange(T)[:, None], np.arange(T)[None, :]
        rel = (T - 1) - (i - j)                                        # row of relative position i - j
        R = qv @ P.transpose(1, 2, 0)[None]                            # (N, h, T, 2T - 1)
        RA = np.abs(qv) @ np.abs(P).transpose(1, 2, 0)[None]
        S = S + np.take_along_axis(R, np.broadcast_to(rel, S.shape), 3)
        A = A + np.take_along_axis(RA, np.broadcast_to(rel, S.shape), 3)
    S.setflags(write=False)
    A.setflags(write=False)
    return S, A


@functools.lru_cache(maxsize=2)
def _scores(key, mode):
    return _scores_of(make(*key), mode)


def scores(case, mode):
    """(score, sum of |products|) of every (line, head, query, key) in log2 units: ((q_i + u) . k_j + (q_i + v) . P[cen - (i - j)]) / sqrt(dh) x log2(e)."""
    return _scores(case.key, mode) if case.key else _scores_of(case, mode)


def _reference_of(c, mode):
    S, _ = scores(c, mode)
    p = np.exp2(S - S.max(-1, keepdims=True))
    ctx = (p @ c.v.astype(np.float64)) / p.sum(-1, keepdims=True)     # (N, h, T, dh)
    ctx = np.ascontiguousarray(ctx.transpose(0, 2, 1, 3))
    ctx.setflags(write=False)
    return ctx


@functools.lru_cache(maxsize=64)
def _reference(key, mode):
    return _reference_of(make(*key), mode)


def reference(case, mode):
    """ctx (N, T, heads, dh) float64: softmax over all j < T of the documented scores, times v.  mode 'bf16': the two query operands and the
    positional table rounded where the kernels round them, nothing else; mode 'fp32': nothing rounded."""
    return _reference(case.key, mode) if case.key else _reference_of(case, mode)


def simulate(case, tile, mode='bf16'):
    """The kernels' decision rule on the float64 scores, per (line, head, 16-query walk) with key steps of `tile` (32 or 64): the first
    step sets every query's reference to its step maximum; a later step fires when any query's step maximum exceeds its reference by
    more than LAZY, and every query's reference then rises to max(old, step maximum).  Returns (events (N, heads, walks), largest rise)."""
    S, _ = scores(case, mode)
    N, h, T, _ = S.shape
    walks = -(-T // 16)
    events = np.zeros((N, h, walks), dtype=np.int64)
    rise = 0.0
    for w in range(walks):
        rows = S[:, :, 16 * w:16 * w + 16, :]
        m = rows[..., :tile].max(-1)                                   # (N, h, <= 16)
        for j0 in range(tile, T, tile):
            sm = rows[..., j0:j0 + tile].max(-1)
            fire = (sm > m + LAZY).any(-1)                             # (N, h)
            new = np.where(fire[..., None], np.maximum(m, sm), m)
            rise = max(rise, float((new - m).max()))
            events[:, :, w] += fire
            m = new
    return events, rise


def bound_bf16(case, ref):
    """|ctx - ref| allowed in bf16 mode: every softmax numerator carries at most half a bf16 step (2^-9 relative) and so does the stored
    output: 2^-8 (|ref| + Vmax), Vmax the largest |v| of the (line, head); allowed twice: 2^-7 (|ref| + Vmax)."""
    vmax = np.abs(case.v).max((2, 3))[:, None, :, None]               # (N, 1, h, 1)
    return 2.0 ** -7 * (np.abs(ref) + vmax)


def bound_fp32(case):
    """|ctx - ref| allowed in fp32 mode, from the case's score magnitudes.  A score is a sum of dhp <= 128 float32 products of operands
    that carry two float32 roundings each ((q + u) x scale), accumulated in float32 from -m_run (|m_run| <= max |score| of the row):
        e_score(i) <= (dhp + 6) 2^-24 max_j (sum_d |product| + 2 max_j' |score(i, j')|)        log2 units,
    the numerator 2^(score - m_run) is off by e_score ln 2 plus the hardware exponential's 2^-22, relatively; a relative error r of the
    numerators moves the quotient by at most 2 r Vmax; numerator and denominator sums of T float32 terms, at most T / 32 rescales of both
    and the reciprocal add (2 T + 16) 2^-24 Vmax:
        bound(i) = Vmax (2 (ln 2 e_score(i) + 2^-22) + (2 T + 16) 2^-24)."""
    S, A = scores(case, 'fp32')
    e = (128 + 6) * 2.0 ** -24 * (A + 2.0 * np.abs(S).max(-1, keepdims=True)).max(-1)       # (N, h, T)
    vmax = np.abs(case.v).max((2, 3))[:, :, None]
    b = vmax * (2.0 * (math.log(2.0) * e + 2.0 ** -22) + (2 * case.T + 16) * 2.0 ** -24)
    return np.ascontiguousarray(b.transpose(0, 2, 1))[..., None]     # (N, T, h, 1)


def device_layout(a, dhp, Tp):
    """(N, heads, T, dh) -> the library's (N, heads, Tp, dhp), zero beyond T and beyond dh."""
    N, h, T, dh = a.shape
    out = np.zeros((N, h, Tp, dhp), dtype=np.float32)
    out[:, :, :T, :dh] = a
    return out
