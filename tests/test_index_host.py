"""Host: the search index's definition (index.pack_host / expand_host), its file and its model-less search.

Nothing here has a tolerance except where a step that is no power of two makes the one float32 multiply round; with step = 1/8 every
code times step is exact and the four properties of section 7l hold to the bit:
  (a) expand(pack(x)) <= r everywhere, and r - expanded < step for kept classes below the clamp;
  (b) the greedy records of the expanded table are those of the original logits;
  (c) spot candidates: e~_t <= e_t, and with keep = C and no code at the clamp e~_t > e_t - step (t + 1);
  (d) e~_t == 0 exactly where e_t == 0, with the same carried start."""
import json
import math

import numpy as np
import pytest

from conformer_ocr_amd import index as I
from conformer_ocr_amd import search as S
from conformer_ocr_amd.codec import ascii_codec
from oracle.ctc_ref import greedy_decoder

STEP = 0.125


def _plant(x, lab, pos, width, top):
    """tests/test_hip_search.py's plant on a (T, C) line: `width` frames of each label, then one blank frame, at the value `top`."""
    for k, l in enumerate(lab):
        at = pos + (width + 1) * k
        x[at:at + width, l] = top
        x[at + width, 0] = top


def _case(kind, C, T, seed):
    """(logits (T, C) float32, planted queries): grid logits are multiples of 1/8 in [-8, 8] with planted frames at 9, real ones
    standard normal with planted frames at 9."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-64, 65, (T, C)) / 8.0 if kind == 'grid' else rng.standard_normal((T, C))).astype(np.float32)
    queries = [[int(v) for v in rng.integers(1, C, L)] for L in (2, 3, 1)]
    at = int(rng.integers(0, 3))
    for lab in queries[:2]:
        _plant(x, lab, at, 2, 9.0)
        at += 3 * len(lab) + int(rng.integers(0, 3))
    assert at <= T
    return x, queries


CASES = [(kind, C, T, 10 * C + T) for kind in ('grid', 'real') for C, T in ((4, 33), (9, 40), (64, 37))]


def _r(x):
    return x - x.max(axis=1, keepdims=True)


@pytest.mark.parametrize('kind,C,T,seed', CASES)
@pytest.mark.parametrize('keep', [1, 3, 'C'])
def test_a_expanded_table_bounds_the_ratios_from_below(kind, C, T, seed, keep):
    x, _ = _case(kind, C, T, seed)
    K = min(C, 32) if keep == 'C' else keep
    cls, cod = I.pack_host(x.T, K, STEP)
    assert cls.dtype == np.uint16 and cod.dtype == np.uint8 and cls.shape == cod.shape == (T, K)
    table = I.expand_host(cls, cod, C, STEP).T
    r = _r(x)
    assert (table <= r).all() and (table.max(axis=1) == 0).all()
    kept = np.zeros((T, C), dtype=bool)
    kept[np.arange(T)[:, None], cls] = True
    assert (table[~kept] == np.float32(-255 * STEP)).all()
    free = kept & (r > np.float32(-255 * STEP))
    assert free.any() and (r[free] - table[free] < STEP).all()
    assert ((table == 0) == (kept & (r == 0))).all()                  # code 0 exactly where the ratio is 0
    if kind == 'grid':
        assert (table[free] == r[free]).all()                         # multiples of the step are stored exactly


def test_a_with_a_step_that_is_no_power_of_two():
    """code * step and d * inv_step round once each: r~ <= r up to those two roundings (2^-23 relative each, of magnitudes <= 25.5)."""
    x, _ = _case('real', 9, 40, 5)
    cls, cod = I.pack_host(x.T, 9, 0.1)
    table, r = I.expand_host(cls, cod, 9, 0.1).T, _r(x)
    assert (cod < 255).all()
    assert (table <= r + 2 * 25.5 * 2.0 ** -23).all() and (r - table < 0.1 + 2 * 25.5 * 2.0 ** -23).all()
    assert ((table == 0) == (r == 0)).all()


@pytest.mark.parametrize('kind,C,T,seed', CASES)
@pytest.mark.parametrize('keep', [1, 2])
def test_b_greedy_records_survive(kind, C, T, seed, keep):
    x, _ = _case(kind, C, T, seed)
    if kind == 'grid':
        x[5] = x[5].max()                                             # a frame where every class ties: np.argmax takes class 0
        x[6, 1:3] = 9.0
    cls, cod = I.pack_host(x.T, keep, STEP)
    assert (cls[:, 0] == np.argmax(x, axis=1)).all()
    want = [rec[:3] for rec in greedy_decoder(x.T)]
    assert [rec[:3] for rec in greedy_decoder(I.expand_host(cls, cod, C, STEP))] == want and len(want) >= 3


# zero-score candidates of the planted queries under spot_candidates on the ORIGINAL logits alone: what each seeded case gives
# (_zero_count), so that the comparison of property (d) cannot pass on nothing
ZERO = {('grid', 4): 21, ('grid', 9): 10, ('grid', 64): 4, ('real', 4): 17, ('real', 9): 8, ('real', 64): 6}


def _zero_count(x, queries):
    return sum(int((S.spot_candidates(x.T, q)[0] == 0).sum()) for q in queries)


@pytest.mark.parametrize('kind,C,T,seed', CASES)
def test_c_candidates_are_bounded_on_both_sides(kind, C, T, seed):
    x, queries = _case(kind, C, T, seed)
    K = min(C, 32)
    cls, cod = I.pack_host(x.T, K, STEP)
    if K == C:
        assert (cod < 255).all()
    table = I.expand_host(cls, cod, C, STEP)
    for q in queries:
        e, _ = S.spot_candidates(x.T, q)
        e2, _ = S.spot_candidates(table, q)
        assert ((e2 > -np.inf) == (e > -np.inf)).all() and (e2 <= e).all()
        if K == C:
            live = e > -np.inf
            assert live.any() and (e2[live] > e[live] - STEP * (np.arange(T)[live] + 1)).all()
    # pruned: still a lower bound
    table = I.expand_host(*I.pack_host(x.T, 2, STEP), C, STEP)
    for q in queries:
        assert (S.spot_candidates(table, q)[0] <= S.spot_candidates(x.T, q)[0]).all()


@pytest.mark.parametrize('kind,C,T,seed', CASES)
@pytest.mark.parametrize('keep', [1, 3])
def test_d_zero_score_candidates_are_preserved_exactly(kind, C, T, seed, keep):
    x, queries = _case(kind, C, T, seed)
    n_zero = _zero_count(x, queries)
    print(f'{kind} C {C} T {T}: {n_zero} zero-score candidates')
    assert n_zero == ZERO[kind, C]
    table = I.expand_host(*I.pack_host(x.T, keep, STEP), C, STEP)
    for q in queries:
        e, st = S.spot_candidates(x.T, q)
        e2, st2 = S.spot_candidates(table, q)
        assert ((e2 == 0) == (e == 0)).all() and (st2[e == 0] == st[e == 0]).all()
        # hence the leading score-0 hits of the selection are the same spans
        a, b = S.spot_host(x.T, q, 8), S.spot_host(table, q, 8)
        lead = [h for h in a if h[2] == 0.0]
        assert b[:len(lead)] == lead and all(h[2] < 0.0 for h in b[len(lead):])


def test_hand_cases():
    x = np.array([[1.0, 3.0, 3.0, -2.0],                               # a two-way tie at the maximum
                  [0.0, -0.125 - 2.0 ** -20, -0.25, -np.inf],            # just above one step; exactly two steps; -inf
                  [0.0, -31.75, -31.875, -40.0]], dtype=np.float32)      # 254, the clamp reached exactly, the clamp
    cls, cod = I.pack_host(x.T, 4, STEP)
    assert cls.tolist() == [[1, 2, 0, 3], [0, 1, 2, 3], [0, 1, 2, 3]]
    assert cod.tolist() == [[0, 0, 16, 40], [0, 2, 2, 255], [0, 254, 255, 255]]
    table = I.expand_host(cls, cod, 4, STEP).T
    assert table.tolist() == [[-2.0, 0.0, 0.0, -5.0], [0.0, -0.25, -0.25, -31.875], [0.0, -31.75, -31.875, -31.875]]
    cls, cod = I.pack_host(x.T, 2, STEP)
    assert cls.tolist() == [[1, 2], [0, 1], [0, 1]] and cod.tolist() == [[0, 0], [0, 2], [0, 254]]
    assert I.expand_host(cls, cod, 4, STEP).T[0].tolist() == [-31.875, 0.0, 0.0, -31.875]
    # an entry whose class is beyond the table is ignored; the later of two entries of one class wins
    assert I.expand_host(np.array([[1, 7, 1]], dtype=np.uint16), np.array([[0, 3, 2]], dtype=np.uint8), 3, STEP).T.tolist() == [[-31.875, -0.25, -31.875]]
    # no frames
    cls, cod = I.pack_host(np.zeros((4, 0), dtype=np.float32), 2, STEP)
    assert cls.shape == cod.shape == (0, 2) and I.expand_host(cls, cod, 4, STEP).shape == (4, 0)
    assert I.inv_step(0.125) == 8.0 and I.inv_step(0.1) == np.float32(1.0 / float(np.float32(0.1)))


def test_value_errors():
    x = np.zeros((5, 3), dtype=np.float32)
    for keep in (0, 6, -1, 2.5):
        with pytest.raises(ValueError):
            I.pack_host(x, keep, STEP)
    with pytest.raises(ValueError):
        I.pack_host(np.zeros((40, 3), dtype=np.float32), 33, STEP)
    for step in (0.0, -1.0, np.inf, np.nan, 1e-46, 1e39):
        with pytest.raises(ValueError):
            I.pack_host(x, 2, step)
        with pytest.raises(ValueError):
            I.expand_host(np.zeros((3, 2), dtype=np.uint16), np.zeros((3, 2), dtype=np.uint8), 5, step)
    with pytest.raises(ValueError):
        I.pack_host(np.zeros((65536, 1), dtype=np.float32), 1, STEP)
    with pytest.raises(ValueError):
        I.pack_host(np.zeros(5, dtype=np.float32), 1, STEP)
    with pytest.raises(ValueError):
        I.expand_host(np.zeros((3, 2), dtype=np.uint16), np.zeros((3, 3), dtype=np.uint8), 5, STEP)
    with pytest.raises(ValueError):
        I.expand_host(np.zeros((3, 4), dtype=np.uint16), np.zeros((3, 4), dtype=np.uint8), 3, STEP)      # keep > C
    with pytest.raises(ValueError):
        I.expand_host(np.zeros((3, 2), dtype=np.uint16), np.zeros((3, 2), dtype=np.uint8), 65536, STEP)


# ---- the file and the model-less search ---------------------------------------------------------------------------------------------
C_FILE = 12


def _corpus(tmp_path, keep=3):
    """Five lines on two pages (one without frames), grid logits with planted queries; returns (path, logits per line, query strings)."""
    codec = ascii_codec(C_FILE)
    rng = np.random.default_rng(77)
    words = [[3, 4, 5], [7, 7], [2, 9, 1, 6]]
    logits, lines = [], []
    for i, T in enumerate([40, 26, 0, 33, 40]):
        x = (rng.integers(-64, 65, (T, C_FILE)) / 8.0).astype(np.float32)
        if T:
            at = i % 3
            for w in (words[i % 3], words[(i + 1) % 3]):
                _plant(x, w, at, 2, 9.0)
                at += 3 * len(w) + 1
        logits.append(x)
        y = 100.0 * i
        lines.append({'page': 0 if i < 2 else 1, 'id': f'l{i}', 'seq_len': 4 * T + 32,
                      'baseline': [[10.0, y + 30.0], [410.5, y + 34.0]], 'boundary': [[10, y], [411, y + 4], [411, y + 44], [10, y + 40]]})
    packed = [I.pack_host(x.T, keep, STEP) for x in logits]
    header = {'keep': keep, 'step': STEP, 'ncls': C_FILE, 'codec': codec.c2l, 'height': 96, 'pad': 16, 'subsampling_factor': 4,
              'model': {'hyper_params': {'num_classes': C_FILE}, 'codec': codec.c2l, 'compute_dtype': 'bf16'}, 'pages': ['a.xml', 'b.xml'], 'lines': lines}
    path = tmp_path / 'corpus.cidx'
    I.write_index(path, header, np.concatenate([c for c, _ in packed]), np.concatenate([c for _, c in packed]),
                  np.concatenate([[0], np.cumsum([x.shape[0] for x in logits])]))
    return path, logits, [''.join(codec.l2c[(l,)] for l in w) for w in words]


def test_file_round_trip_and_rejections(tmp_path):
    path, logits, _ = _corpus(tmp_path)
    assert not (tmp_path / 'corpus.cidx.tmp').exists()
    idx = I.load_index(path)
    assert len(idx) == 5 and (idx.keep, idx.step, idx.ncls) == (3, STEP, C_FILE) and idx.header['format'] == I.FORMAT
    assert [idx.frames(i) for i in range(5)] == [40, 26, 0, 33, 40]
    for i, x in enumerate(logits):
        cls, cod = I.pack_host(x.T, 3, STEP)
        assert (idx.line(i)[0] == cls).all() and (idx.line(i)[1] == cod).all()
    assert I.read_header(path) == idx.header and idx.header['lines'][3]['baseline'] == [[10.0, 330.0], [410.5, 334.0]]
    info = I.index_info(path)
    assert (info['lines'], info['frames'], info['pages'], info['keep']) == (5, 139, 2, 3)
    assert info['packed_bytes'] == 139 * 3 * 3 + 6 * 8 and info['dense_bytes_per_line'] == 139 * C_FILE * 4 / 5
    data = path.read_bytes()
    # a cut file
    (tmp_path / 'cut.cidx').write_bytes(data[:-7])
    with pytest.raises(ValueError, match='cut.cidx'):
        I.load_index(tmp_path / 'cut.cidx')
    (tmp_path / 'stub.cidx').write_bytes(data[:5])
    with pytest.raises(ValueError, match='stub.cidx'):
        I.load_index(tmp_path / 'stub.cidx')
    # another version
    import safetensors.numpy
    tensors = safetensors.numpy.load(data)
    (tmp_path / 'v2.cidx').write_bytes(safetensors.numpy.save(tensors, metadata={I.META_KEY: json.dumps(dict(idx.header, format=2))}))
    with pytest.raises(ValueError, match='v2.cidx.*format 2'):
        I.load_index(tmp_path / 'v2.cidx')
    # tensors that disagree with the header
    for name, bad in (('keep', dict(tensors, codes=tensors['codes'][:, :2])), ('rows', dict(tensors, classes=tensors['classes'][:-1], codes=tensors['codes'][:-1])),
                      ('offs', dict(tensors, line_offsets=tensors['line_offsets'][:-1])), ('gone', {k: v for k, v in tensors.items() if k != 'codes'}),
                      ('type', dict(tensors, classes=tensors['classes'].astype(np.int32)))):
        (tmp_path / f'{name}.cidx').write_bytes(safetensors.numpy.save({k: np.ascontiguousarray(v) for k, v in bad.items()},
                                                                       metadata={I.META_KEY: json.dumps(idx.header)}))
        with pytest.raises(ValueError, match=f'{name}.cidx'):
            I.load_index(tmp_path / f'{name}.cidx')
    (tmp_path / 'other.cidx').write_bytes(safetensors.numpy.save(tensors, metadata={'x': 'y'}))
    with pytest.raises(ValueError, match='other.cidx'):
        I.load_index(tmp_path / 'other.cidx')
    with pytest.raises(ValueError):
        I.write_index(tmp_path / 'w.cidx', dict(idx.header, keep=2), idx.classes, idx.codes, idx.line_offsets)
    assert not (tmp_path / 'w.cidx').exists()


def test_greedy_text_is_the_greedy_decoder_on_the_original_logits(tmp_path):
    path, logits, _ = _corpus(tmp_path, keep=1)
    idx = I.load_index(path)
    codec = idx.codec()
    some = 0
    for i, x in enumerate(logits):
        want = greedy_decoder(x.T)
        assert I.greedy_records(idx, i) == [rec[:3] for rec in want]
        assert I.greedy_text(idx, i) == ''.join(c[0] for c in codec.decode(want))
        some += len(want)
    assert some >= 20 and I.greedy_text(idx, 2) == ''


def test_search_index_on_the_host(tmp_path, capsys):
    from conformer_ocr_amd.page import cut_quads, line_geometry
    path, logits, queries = _corpus(tmp_path)
    idx = I.load_index(path)
    codec = idx.codec()
    found = I.search_index(path, queries, hits=4, device='cpu')
    assert found == I.search_index(idx, queries, hits=4, batch_size=1, device='cpu')
    assert all(set(h) == {'page', 'line', 'query', 'start', 'end', 'score', 'conf', 'quad'} for h in found)
    order = [(h['page'], int(h['line'][1:]), queries.index(h['query'])) for h in found]
    assert order == sorted(order) and {h['page'] for h in found} == {0, 1} and not any(h['line'] == 'l2' for h in found)
    zero = 0
    for i, x in enumerate(logits):
        if not x.shape[0]:
            continue
        ln = idx.header['lines'][i]
        geom = line_geometry(ln['id'], ln['baseline'], ln['boundary'])
        table = I.expand_host(*idx.line(i), C_FILE, STEP)
        for q in queries:
            lab = codec.encode(q)
            mine = [h for h in found if h['line'] == ln['id'] and h['query'] == q]
            want = S.spot_host(table, lab, 4)
            assert [(h['start'], h['end'], h['score']) for h in mine] == want
            for h in mine:
                assert h['conf'] == math.exp(h['score'] / len(lab))          # (search_pages' expression)
                assert h['quad'] == cut_quads(geom, [(0, h['start'], h['end'], h['conf'])], ln['seq_len'], x.shape[0], 16)[0][1]
            # property (d) through the whole path: the leading zero-score hits are those of the original logits
            lead = [h for h in S.spot_host(x.T, lab, 4) if h[2] == 0.0]
            assert want[:len(lead)] == lead
            zero += len(lead)
    assert zero >= 8
    kept = I.search_index(idx, queries, hits=4, min_conf=0.5, device='cpu')
    assert kept == [h for h in found if h['conf'] >= 0.5] and 0 < len(kept) < len(found)
    # a query of more than 255 labels takes the same path
    assert I.search_index(idx, [queries[0], queries[1] * 130], hits=1, device='cpu') == [h for h in I.search_index(idx, queries[:1], device='cpu')]
    for bad in (['☃'], [], ['']):
        with pytest.raises(ValueError):
            I.search_index(idx, bad, device='cpu')
    for kw in (dict(hits=0), dict(hits=9), dict(min_conf=0.0), dict(min_conf=1.5), dict(batch_size=0)):
        with pytest.raises(ValueError):
            I.search_index(idx, queries, device='cpu', **kw)

    # the command: search and info
    (tmp_path / 'queries.txt').write_text(queries[1] + '\n☃\n', encoding='utf-8')
    capsys.readouterr()
    out = tmp_path / 'hits.json'
    assert I.main(['search', '--index', str(path), '-q', queries[0], '-Q', str(tmp_path / 'queries.txt'), '--hits', '4', '-d', 'cpu', str(out)]) == 0
    err = capsys.readouterr().err
    assert 'skipped' in err and 'a.xml: ' in err and 'b.xml: ' in err and 'of 2 queries' in err
    back = json.loads(out.read_text(encoding='utf-8'))
    want = I.search_index(idx, queries[:2], hits=4, device='cpu')
    assert len(back) == len(want) > 0
    for b, w in zip(back, want):
        assert b == dict(w, page=idx.header['pages'][w['page']], quad=[list(p) for p in w['quad']])
    assert I.main(['search', '--index', str(path), '-q', '☃', '-d', 'cpu', str(out)]) == 1
    assert 'codec can encode' in capsys.readouterr().err
    assert I.main(['search', '--index', str(tmp_path / 'queries.txt'), '-q', 'a', '-d', 'cpu', str(out)]) == 1
    assert I.main(['search', '-q', 'a', str(out)]) == 1 and I.main(['build', '-o', str(out)]) == 1 and I.main([]) == 1
    capsys.readouterr()
    assert I.main(['info', '--index', str(path)]) == 0
    assert json.loads(capsys.readouterr().out) == json.loads(json.dumps(I.index_info(path)))
    with pytest.raises(SystemExit):
        I.main(['build', '--help'])
    assert ' '.join(capsys.readouterr().out.split()).count('not tuned') >= 2          # keep and step are placeholders, and the help says so
