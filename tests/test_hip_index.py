"""GPU: the search index (cocr_posterior_pack / cocr_posterior_unpack, index.build_index / search_index) against
the host definition `index.pack_host` / `index.expand_host` and `search.spot_host`.

Everything is exact: both kernels do one correctly rounded float32 operation per value (a subtraction and a multiply in the pack, a
multiply in the unpack) and integer work otherwise, so classes, codes and expanded tables are compared bit for bit; the spotter then
runs on tables whose entries are multiples of the step (1/8), where its float32 sums are exact (tests/test_hip_search.py)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from conformer_ocr_amd import _lib
from conformer_ocr_amd import index as I
from conformer_ocr_amd import search as S
from conformer_ocr_amd.codec import ascii_codec
from conformer_ocr_amd.page import Line, recognize_pages
from conformer_ocr_amd.pred import PytorchRecognitionModel, save_safetensors
from tests import page_synth

pytestmark = pytest.mark.gpu
DROPS = dict(input_dropout_p=0.1, feed_forward_dropout_p=0.1, attention_dropout_p=0.1, conv_dropout_p=0.1)
STEP = 0.125


def _engine():
    from conformer_ocr_amd.ctc_decoder import _scratch_engine
    return _scratch_engine(torch.device('cuda', 0))


def _pack(logits, out_lens, keep, step=STEP):
    cls, cod = _engine().posterior_pack(torch.from_numpy(logits).cuda(), out_lens, keep, step)
    return cls.cpu().numpy(), cod.cpu().numpy()


def _unpack(classes, codes, ncls, step=STEP):
    return _engine().posterior_unpack(torch.from_numpy(classes).cuda(), torch.from_numpy(codes).cuda(), ncls, step).cpu().numpy()


def _pack_want(logits, out_lens, keep, step=STEP):
    N, T, _ = logits.shape
    classes, codes = np.zeros((N, T, keep), dtype=np.uint16), np.full((N, T, keep), 255, dtype=np.uint8)      # past out_len: (0, 255)
    for n in range(N):
        classes[n, :out_lens[n]], codes[n, :out_lens[n]] = I.pack_host(logits[n, :out_lens[n]].T, keep, step)
    return classes, codes


def _expand_want(classes, codes, ncls, step=STEP):
    return np.stack([I.expand_host(classes[n], codes[n], ncls, step).T for n in range(classes.shape[0])])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. pack and unpack against the definition, bit for bit ---------------------------------------------------------------------------
SHAPES = [
    (3, 37, 5, (1, 3, 5), [37, 0, 30]),              # keep = C; a line without frames
    (2, 64, 64, (8,), [64, 1]),                      # exactly one class per lane
    (2, 50, 65, (8, 32), [50, 49]),                  # the second register and its tail
    (2, 50, 130, (8, 32), [13, 50]),
    (1, 20, 300, (8,), [20]),                        # class ids above 255 (5 registers of 8)
    (4, 300, 128, (8,), [300, 0, 251, 64]),          # the production row
    (1, 6, 512, (8, 32), [6]),                       # the widest row held in registers
    (1, 5, 513, (8, 32), [4]),                       # the first row staged in LDS
    (1, 3, 16384, (8,), [3]),                        # the widest row staged in LDS
    (1, 3, 16385, (8,), [3]),                        # the first row left in global memory
]


def _logits(kind, N, T, ncls, seed):
    rng = np.random.default_rng(seed)
    if kind == 'ties':
        return rng.integers(-2, 3, (N, T, ncls)).astype(np.float32)
    return rng.standard_normal((N, T, ncls)).astype(np.float32)


@pytest.mark.parametrize('kind', ['ties', 'real'])
@pytest.mark.parametrize('N,T,ncls,keeps,out_lens', SHAPES)
def test_pack_and_unpack_are_the_definition(N, T, ncls, keeps, out_lens, kind):
    logits = _logits(kind, N, T, ncls, 1000 + ncls + T)
    for keep in keeps:
        classes, codes = _pack(logits, out_lens, keep)
        want_cls, want_cod = _pack_want(logits, out_lens, keep)
        assert classes.dtype == np.uint16 and codes.dtype == np.uint8 and classes.shape == codes.shape == (N, T, keep)
        assert (classes == want_cls).all() and (codes == want_cod).all()
        for n in range(N):
            assert (classes[n, out_lens[n]:] == 0).all() and (codes[n, out_lens[n]:] == 255).all()
        if kind == 'ties' and keep >= 2 and ncls >= 16:
            assert (codes[0, :out_lens[0], 1] == 0).any()                       # ties at the maximum do occur
        table = _unpack(classes, codes, ncls)
        assert table.shape == (N, T, ncls) and (_bits(table) == _bits(_expand_want(classes, codes, ncls))).all()
        assert (table[0, :out_lens[0]].max(axis=1) == 0).all() and (table[N - 1, out_lens[N - 1]:] == -255 * STEP).all()


def test_minus_infinity_a_step_that_is_no_power_of_two_and_reproducibility():
    logits = _logits('real', 2, 40, 70, 5)
    logits[:, :, 3] = -np.inf                                                   # a -inf column beside finite maxima
    logits[0, 7, 10:] = -np.inf
    logits *= 4.0                                                               # differences up to the clamp at step 0.1
    for step in (STEP, 0.1):
        for keep in (8, 32):
            classes, codes = _pack(logits, [40, 33], keep, step)
            want_cls, want_cod = _pack_want(logits, [40, 33], keep, step)
            assert (classes == want_cls).all() and (codes == want_cod).all()
            table = _unpack(classes, codes, 70, step)
            assert (_bits(table) == _bits(_expand_want(classes, codes, 70, step))).all()
            again = _pack(logits, [40, 33], keep, step)
            assert (again[0] == classes).all() and (again[1] == codes).all() and (_bits(_unpack(classes, codes, 70, step)) == _bits(table)).all()
        assert (codes == 255).any() and (codes[0, 7, 10:] == 255).all() and ((codes > 0) & (codes < 255)).any()
    full = _pack(logits[:, :, :32].copy(), [40, 33], 32)
    assert (full[0][0, 0] == 3).sum() == 1 and full[1][0, 0][full[0][0, 0] == 3] == 255      # -inf is kept last, at the clamp


def test_unpack_ignores_a_class_beyond_the_table():
    """An entry whose class is >= ncls, planted in the packed input: nothing outside its row changes, and within it only what the
    definition says (the entry is ignored)."""
    ncls, keep = 37, 4
    logits = _logits('real', 2, 9, ncls, 3)
    classes, codes = _pack_want(logits, [9, 9], keep)
    clean = _unpack(classes, codes, ncls)
    planted = classes.copy()
    planted[0, 4, 2], planted[1, 8, 0], planted[1, 0, 3] = ncls, 65535, ncls + 64 * 5
    eng = _engine()
    guard = torch.full((2 * 9 * ncls + 2 * ncls,), 7.0, device='cuda')          # the table sits between two guard rows
    out = guard[ncls:-ncls].view(2, 9, ncls)
    d_cls, d_cod = torch.from_numpy(planted).cuda(), torch.from_numpy(codes).cuda()
    _lib.check(eng.lib.cocr_posterior_unpack(eng._h, C.c_void_p(d_cls.data_ptr()), C.c_void_p(d_cod.data_ptr()), 2, 9, keep, ncls, C.c_float(STEP),
                                             C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (guard[:ncls] == 7.0).all() and (guard[-ncls:] == 7.0).all()
    assert (_bits(got) == _bits(_expand_want(planted, codes, ncls))).all()
    same = np.ones((2, 9), dtype=bool)
    same[0, 4] = same[1, 8] = same[1, 0] = False
    assert (_bits(got[same]) == _bits(clean[same])).all()
    assert got[0, 4, classes[0, 4, 2]] == -255 * STEP and (got[1, 8] == -255 * STEP).sum() == ncls - keep + 1


# ---- 2. unpack + cocr_ctc_spot is spot_host on the expanded table ------------------------------------------------------------------
def _plant(x, lab, pos, width):
    """tests/test_hip_search.py's plant: `lab` from frame `pos` of the (T, C) line x, `width` frames of each label, then one blank frame."""
    for k, l in enumerate(lab):
        at = pos + (width + 1) * k
        x[at:at + width + 1] = np.minimum(x[at:at + width + 1], 8.0)
        x[at:at + width, l] = 9.0
        x[at + width, 0] = 9.0


def _grid_case(N, T, ncls, lens_q, seed, out_lens, width=2):
    """tests/test_hip_search.py's grid construction: logits that are multiples of 1/8 in [-8, 8], planted frames at 9."""
    rng = np.random.default_rng(seed)
    logits = (rng.integers(-64, 65, (N, T, ncls)) / 8.0).astype(np.float32)
    queries = [[int(v) for v in rng.integers(1, ncls, L)] for L in lens_q]
    if len(queries) > 1 and len(queries[1]) > 1:
        queries[1][1] = queries[1][0]
    if len(queries) > 2 and len(queries[0]) > 1:
        queries[2] = (queries[0][1:] + queries[2])[:max(len(queries[2]), 2)]
    for n in range(N):
        at = int(rng.integers(0, 3))
        for qi, lab in enumerate(queries[:-1]):
            for _ in range(2 if qi == 0 else 1):
                span = (width + 1) * len(lab)
                if at + span <= out_lens[n] and (qi + n) % 3 != 2:
                    _plant(logits[n], lab, at, width)
                    at += span + (0 if qi == 0 else int(rng.integers(0, 4)))
    return logits, queries


@pytest.mark.parametrize('N,T,ncls,lens_q,K,out_lens,keeps', [
    (3, 37, 5, [2, 3, 2, 1, 4], 3, [37, 0, 30], (2, 5)),
    (4, 300, 64, [7, 12, 8, 40, 1, 3, 25, 5, 9], 4, [300, 0, 251, 64], (8, 32)),
])
def test_unpack_then_spot_is_the_definition_on_the_expanded_table(N, T, ncls, lens_q, K, out_lens, keeps):
    logits, queries = _grid_case(N, T, ncls, lens_q, 100 + T, out_lens)
    eng = _engine()
    direct = eng.ctc_spot(torch.from_numpy(logits).cuda(), out_lens, queries, K)
    for keep in keeps:
        classes, codes = eng.posterior_pack(torch.from_numpy(logits).cuda(), out_lens, keep, STEP)
        got = eng.ctc_spot(eng.posterior_unpack(classes, codes, ncls, STEP), out_lens, queries, K)
        zero = 0
        for n in range(N):
            table = I.expand_host(*I.pack_host(logits[n, :out_lens[n]].T, keep, STEP), ncls, STEP)
            for qi, q in enumerate(queries):
                want = S.spot_host(table, q, K)
                assert got[n][qi] == want, (keep, n, qi)                         # counts, starts, ends and scores
                lead = [h for h in direct[n][qi] if h[2] == 0.0]
                assert want[:len(lead)] == lead                                 # property (d)
                zero += len(lead)
        assert zero >= 2
        if keep == ncls:
            assert got == direct          # nothing pruned, every code exact on the grid: the search of the original logits


# ---- 3. errors, with the engine usable afterwards; the greedy shortcut ----------------------------------------------------------------
def test_error_codes_and_the_engine_afterwards():
    eng = _engine()
    logits = torch.zeros((2, 4, 6), device='cuda')
    cls, cod = torch.zeros((2, 4, 3), dtype=torch.uint16, device='cuda'), torch.zeros((2, 4, 3), dtype=torch.uint8, device='cuda')
    out = torch.zeros((2, 4, 6), device='cuda')
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = C.POINTER(C.c_int32)

    def pack(N=2, T=4, ncls=6, lens=(4, 4), keep=3, inv=8.0, logits_p=logits.data_ptr()):
        lens = np.asarray(lens, dtype=np.int32)
        return eng.lib.cocr_posterior_pack(eng._h, C.c_void_p(logits_p), N, T, ncls, lens.ctypes.data_as(i32), keep, C.c_float(inv), C.c_void_p(cls.data_ptr()),
                                           C.c_void_p(cod.data_ptr()), stream)

    def unpack(N=2, T=4, keep=3, ncls=6, step=STEP, out_p=out.data_ptr()):
        return eng.lib.cocr_posterior_unpack(eng._h, C.c_void_p(cls.data_ptr()), C.c_void_p(cod.data_ptr()), N, T, keep, ncls, C.c_float(step), C.c_void_p(out_p),
                                             stream)
    assert pack(lens=(4, 5)) == _lib.EINVAL and pack(lens=(-1, 4)) == _lib.EINVAL
    assert pack(keep=0) == _lib.EINVAL and pack(keep=7) == _lib.EINVAL and pack(keep=33, ncls=40) == _lib.EINVAL
    for inv in (0.0, -8.0, float('inf'), float('nan')):
        assert pack(inv=inv) == _lib.EINVAL
    assert pack(logits_p=None) == _lib.EINVAL and pack(N=0, lens=()) == _lib.EINVAL
    assert pack(ncls=65536) == _lib.EUNSUPPORTED and pack(N=65536, lens=[4] * 65536) == _lib.EUNSUPPORTED
    assert pack(keep=0) == _lib.EINVAL and b'keep' in eng.lib.cocr_last_error()
    assert unpack(keep=0) == _lib.EINVAL and unpack(keep=7) == _lib.EINVAL and unpack(out_p=None) == _lib.EINVAL and unpack(T=0) == _lib.EINVAL
    for step in (0.0, -1.0, float('inf'), float('nan')):
        assert unpack(step=step) == _lib.EINVAL
    assert unpack(ncls=65536) == _lib.EUNSUPPORTED
    # the Python layer: ValueError / NotImplementedError
    with pytest.raises(ValueError):
        eng.posterior_pack(logits, [4, 5], 3, STEP)
    with pytest.raises(ValueError):
        eng.posterior_pack(logits, [4, 4], 7, STEP)
    with pytest.raises(ValueError):
        eng.posterior_pack(logits, [4, 4], 3, 0.0)
    with pytest.raises(ValueError):
        eng.posterior_pack(logits, [4], 3, STEP)
    with pytest.raises(ValueError):
        eng.posterior_unpack(cls, cod[:, :, :2], 6, STEP)
    # still usable: all classes tie, the lowest three are kept at code 0
    got_cls, got_cod = eng.posterior_pack(logits, [4, 2], 3, STEP)
    assert got_cls.cpu().numpy()[0].tolist() == [[0, 1, 2]] * 4 and got_cod.cpu().numpy()[1].tolist() == [[0, 0, 0]] * 2 + [[255] * 3] * 2
    assert eng.posterior_unpack(got_cls, got_cod, 6, STEP).cpu().numpy()[0, 0].tolist() == [0.0, 0.0, 0.0, -31.875, -31.875, -31.875]


def _net(tc, dtype):
    net = PytorchRecognitionModel(**tc.hp.as_dict(), **DROPS, codec=ascii_codec(tc.hp.num_classes), compute_dtype=dtype)
    net.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    return net.to('cuda:0').eval()


def test_greedy_shortcut_is_not_disturbed_and_the_model_call(text_case):
    """`posterior_pack` between a forward and its `ctc_greedy`: the decoder epilogue's per-frame argmax still belongs to the logits."""
    tc = text_case('cfg2_text')
    net = _net(tc, 'bf16')
    image, lens, idx = tc.batch(0)
    line = torch.from_numpy(image[:8]).cuda().squeeze(1)
    eng = net.engine(torch.device('cuda', 0))
    logits, out_lens = eng.forward(line, lens[:8])
    assert eng._argmax_is_fresh(logits)
    classes, codes = eng.posterior_pack(logits, out_lens, 8, STEP)
    assert eng._argmax_is_fresh(logits)
    after = eng.ctc_greedy(logits, out_lens)
    assert eng.ctc_greedy(logits.clone(), out_lens) == after               # from the values, without the shortcut
    want_cls, want_cod = _pack_want(logits.cpu().numpy(), [int(l) for l in out_lens], 8)
    assert (classes.cpu().numpy() == want_cls).all() and (codes.cpu().numpy() == want_cod).all()
    # entry 0 reads as the greedy decoder does
    for n, recs in enumerate(after):
        lab = want_cls[n, :int(out_lens[n]), 0]
        runs = [int(l) for k, l in enumerate(lab) if l != 0 and (k == 0 or lab[k - 1] != l)]
        assert runs == [r[0] for r in recs]
    # the model-level call: per line, cut to the output length
    per_line = net.pack_posteriors(torch.from_numpy(image[:8]).cuda(), torch.from_numpy(lens[:8]))
    assert len(per_line) == 8
    for n, (c, d) in enumerate(per_line):
        assert c.shape == d.shape == (int(out_lens[n]), 8) and (c == want_cls[n, :int(out_lens[n])]).all() and (d == want_cod[n, :int(out_lens[n])]).all()


# ---- 4. pages: build once, search without the model -----------------------------------------------------------------------------------
KINDS = [('line', 0.0), ('line', 7.0), ('arc', 2600.0, 1), ('line', -7.0), ('line', 15.0), ('line', 0.0), ('line', -15.0),
         ('arc', 2500.0, -1), ('line', 0.0), ('line', 3.0)]
PICK = [3, 4, 14, 7, 11, 12, 16, 22, 23, 6]          # tests/test_hip_page.py PICK
FIXTURE_FORM = dict(pad=0, edge=1200)
M = 6                                                # a query is labels k .. k + 5 of the line's greedy reading


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_pages_are_indexed_once_and_searched_without_the_model(text_case, tmp_path, capsys, dtype):
    from PIL import Image
    tc = text_case('cfg2_text')
    lines = [np.rint(tc.lines[i] * 255.0).astype(np.uint8) for i in PICK]
    page, placed = page_synth.text_page(lines, KINDS)
    page_lines = [Line(f'line{k}', P, B) for k, (_, P, B) in enumerate(placed)]
    net = _net(tc, dtype)
    pages = [(page, page_lines[:6]), (page, page_lines[6:])]               # two "pages": the lines of one image split in two
    read = [r for per_page in recognize_pages(net, pages, batch_size=4, **FIXTURE_FORM) for r in per_page]
    path = tmp_path / 'corpus.cidx'
    built = I.build_index(net, pages, path, batch_size=4, names=['first', 'second'], **FIXTURE_FORM)
    idx = I.load_index(path)
    assert (built.classes == idx.classes).all() and (built.codes == idx.codes).all() and built.header == idx.header
    assert len(idx) == 10 and (idx.keep, idx.step, idx.ncls) == (8, STEP, tc.hp.num_classes) and idx.header['pages'] == ['first', 'second']
    assert [ln['page'] for ln in idx.header['lines']] == [0] * 6 + [1] * 4 and [ln['id'] for ln in idx.header['lines']] == [l.id for l in page_lines]
    assert idx.header['model']['hyper_params']['num_classes'] == tc.hp.num_classes and idx.header['pad'] == 0
    # page and line order, whatever the batches were
    other = I.build_index(net, pages, tmp_path / 'other.cidx', batch_size=3, names=['first', 'second'], **FIXTURE_FORM)
    assert other.header['lines'] == idx.header['lines'] and (other.line_offsets == idx.line_offsets).all()
    # the 1-best reading, from entry 0
    assert [I.greedy_text(idx, j) for j in range(10)] == [r['text'] for r in read]
    queries = []
    for j, r in enumerate(read):
        assert len(r['text']) > M
        k = (3 * j + 1) % (len(r['text']) - M + 1)
        q = r['text'][k:k + M]
        if q in queries:
            q = r['text'][:M]
        assert q not in queries
        queries.append(q)
    codec = idx.codec()
    found = I.search_index(path, queries, hits=8)
    assert found == I.search_index(idx, queries, hits=8, batch_size=1) == I.search_index(idx, queries, hits=8, batch_size=3)
    direct = S.search_pages(net, pages, queries, hits=8, batch_size=4, **FIXTURE_FORM)
    span = lambda h: (h['page'], h['line'], h['query'], h['start'], h['end'], h['score'], h['conf'], h['quad'])
    for j, q in enumerate(queries):
        mine = [h for h in found if h['line'] == f'line{j}' and h['query'] == q]
        theirs = [h for h in direct if h['line'] == f'line{j}' and h['query'] == q]
        assert mine and mine[0]['score'] == 0.0 and mine[0]['conf'] == 1.0, (j, q, mine[:1])
        lead = [span(h) for h in theirs if h['score'] == 0.0]
        assert lead and [span(h) for h in mine[:len(lead)]] == lead                  # property (d): the same frames and the same quad
        assert all(h['score'] < 0.0 for h in mine[len(lead):])
    # every hit is the definition on the stored entries
    order = [(h['page'], int(h['line'][4:]), queries.index(h['query'])) for h in found]
    assert order == sorted(order)
    for j in range(10):
        table = I.expand_host(*idx.line(j), idx.ncls, idx.step)
        for q in queries:
            want = S.spot_host(table, codec.encode(q), 8)
            assert [(h['start'], h['end'], h['score']) for h in found if h['line'] == f'line{j}' and h['query'] == q] == want
    assert found == I.search_index(idx, queries, hits=8, device='cpu')
    kept = I.search_index(idx, queries, hits=8, min_conf=0.5)
    assert kept == [h for h in found if h['conf'] >= 0.5] and 0 < len(kept) < len(found)
    with pytest.raises(ValueError):
        I.search_index(idx, ['☃'])
    if dtype != 'bf16':
        return

    # the commands on the same page (the loaded model computes in bf16)
    Image.fromarray(page).save(tmp_path / 'scan.png')
    pts = lambda a: ' '.join(f'{x:.3f},{y:.3f}' for x, y in a)
    body = ''.join(f'<TextLine id="{l.id}"><Coords points="{pts(l.boundary)}"/><Baseline points="{pts(l.baseline)}"/></TextLine>\n' for l in page_lines)
    (tmp_path / 'scan.xml').write_text('<?xml version="1.0" encoding="UTF-8"?>\n<PcGts xmlns="http://schema.primaresearch.org/PAGE/gts/pagecontent/2019-07-15">'
                                       f'<Page imageFilename="scan.png"><TextRegion id="r">{body}</TextRegion></Page></PcGts>\n', encoding='utf-8')
    src = PytorchRecognitionModel(**tc.hp.as_dict(), **DROPS, codec=ascii_codec(tc.hp.num_classes))
    src.nn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in tc.state.items()})
    save_safetensors(src, tmp_path / 'model.tar')
    xml, cidx, out = str(tmp_path / 'scan.xml'), str(tmp_path / 'cmd.cidx'), tmp_path / 'hits.json'
    capsys.readouterr()
    assert I.main(['build', '-m', str(tmp_path / 'model.tar'), '-f', 'page', '-i', xml, '-o', cidx, '--pad', '0', '--edge', '1200', '--batch-size', '4']) == 0
    assert f'{cidx}: 10 lines of 1 pages' in capsys.readouterr().err
    from conformer_ocr_amd.page import read_page_xml
    want = I.build_index(net, [(page, read_page_xml(tmp_path / 'scan.xml').lines)], tmp_path / 'want.cidx', batch_size=4, names=[xml], **FIXTURE_FORM)
    cmd = I.load_index(cidx)
    assert cmd.header == want.header and (cmd.classes == want.classes).all() and (cmd.codes == want.codes).all() and (cmd.line_offsets == want.line_offsets).all()
    (tmp_path / 'queries.txt').write_text(queries[1] + '\n☃\n', encoding='utf-8')
    assert I.main(['search', '--index', cidx, '-q', queries[0], '-Q', str(tmp_path / 'queries.txt'), '--hits', '2', str(out)]) == 0
    err = capsys.readouterr().err
    assert 'skipped' in err and f'{xml}: ' in err and 'of 2 queries' in err
    from conformer_ocr_amd.dataset import normalize_text
    asked = [normalize_text(q, None, True) for q in queries[:2]]
    hits = I.search_index(want, asked, hits=2)
    back = json.loads(out.read_text(encoding='utf-8'))
    assert len(back) == len(hits) > 0
    for b, w in zip(back, hits):
        assert b == dict(w, page=xml, quad=[list(p) for p in w['quad']])
    assert I.main(['info', '--index', cidx]) == 0
    info = json.loads(capsys.readouterr().out)
    assert info == json.loads(json.dumps(I.index_info(cidx))) and info['lines'] == 10 and info['frames'] == int(cmd.line_offsets[-1])
    assert info['packed_bytes_per_line'] < info['dense_bytes_per_line']
