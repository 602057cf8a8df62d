"""query_db at database scale: dctfp_l1_knn (fused L1 + k nearest) against row_select(l1_matrix(...)), and QuerySearch (device
ranking and device text) against the lines of query_db.search(), byte for byte."""

import os
from types import SimpleNamespace

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu
FIX = os.path.join(gu.GOLD, 'ref_fixtures')


def _expected(q, b, k, col0=0):
    from dctdomain_amd.similarity import l1_matrix, row_select
    v, i = row_select(l1_matrix(q, b), k)
    return v, i + col0


def _check(q, b, k, col0=0, msg=''):
    from dctdomain_amd.similarity import l1_knn
    v, i = l1_knn(q, b, k, col0)
    ev, ei = _expected(q, b, k, col0)
    np.testing.assert_array_equal(v, ev, err_msg=msg)
    np.testing.assert_array_equal(i, ei, err_msg=msg)


def test_l1_knn_random_shapes_and_k():
    rng = np.random.default_rng(1)
    for nq, nb, d in ((1, 1, 480), (5, 127, 480), (127, 128, 16), (129, 129, 17), (5, 4000, 500), (129, 3000, 480)):
        q = rng.integers(-128, 128, size=(nq, d)).astype(np.int8)
        b = rng.integers(-128, 128, size=(nb, d)).astype(np.int8)
        for k in (1, 2, 63, 64, 65, 100, 300, 1024, nb + 5):
            _check(q, b, k, msg=f'{nq} x {nb} x {d}, k = {k}')


def test_l1_knn_ties_and_duplicates():
    rng = np.random.default_rng(2)
    b = rng.integers(-1, 2, size=(700, 480)).astype(np.int8)
    b[300:400] = b[:100]                                              # duplicated rows: equal distances, ties to the lower row
    q = np.concatenate([b[:3], rng.integers(-1, 2, size=(130, 480)).astype(np.int8)])
    for k in (1, 65, 300, 1024):
        _check(q, b, k, msg=f'ties, k = {k}')
    _check(q, np.repeat(b[:1], 500, axis=0), 100, msg='all columns equal')


def test_l1_knn_adversarial_column_order():
    """Distances falling along the columns: every column enters every row's list."""
    nb, d = 3000, 480
    base = np.zeros((nb, d), np.int8)
    lev = (np.arange(nb)[::-1] * 127 * d // nb)
    for c in range(d):
        base[:, c] = np.clip(lev // d + (c < lev % d), 0, 127)
    q = np.zeros((7, d), np.int8)
    for k in (1, 64, 1024):
        _check(q, base, k, msg=f'adversarial, k = {k}')


def test_l1_knn_large_database_and_query_counts():
    rng = np.random.default_rng(3)
    b = rng.integers(-128, 128, size=(100003, 480)).astype(np.int8)
    q = rng.integers(-128, 128, size=(5, 480)).astype(np.int8)
    for k in (1, 100, 1024):
        _check(q, b, k, msg=f'100003 columns, k = {k}')
    q = rng.integers(-128, 128, size=(4097, 480)).astype(np.int8)
    _check(q, b[:5000], 100, msg='4097 rows')


def test_l1_knn_strides_col0_empty_and_fallback():
    import torch
    from dctdomain_amd.similarity import l1_knn
    rng = np.random.default_rng(4)
    wide_q = torch.from_numpy(rng.integers(-128, 128, size=(40, 528)).astype(np.int8)).cuda()
    wide_b = torch.from_numpy(rng.integers(-128, 128, size=(900, 528)).astype(np.int8)).cuda()
    for d in (16, 17, 480, 500):                                     # ld = 528 > d
        _check(wide_q[:, :d], wide_b[:, :d], 70, msg=f'strided d = {d}')
        _check(wide_q[:, :d], wide_b[:, :d], 70, col0=123456, msg=f'col0, d = {d}')
    v, i = l1_knn(np.zeros((0, 480), np.int8), wide_b[:, :480], 10)
    assert v.shape == (0, 10) and i.shape == (0, 10)
    v, i = l1_knn(wide_q[:, :480], np.zeros((0, 480), np.int8), 10)
    assert v.shape == (40, 0)
    _check(wide_q[:, :480], wide_b[:, :480], 1025, msg='k = 1025: l1_matrix + row_select')
    _check(wide_q[:5, :480], torch.cat([wide_b[:, :480]] * 2), 1025, msg='k = 1025 over 1800 rows')


def test_l1_knn_kernel_limit_is_reported():
    import torch
    from dctdomain_amd import _lib
    q = torch.zeros((2, 480), dtype=torch.int8, device='cuda')
    b = torch.zeros((2000, 480), dtype=torch.int8, device='cuda')
    v = torch.empty((2, 1025), dtype=torch.int32, device='cuda')
    ctx = _lib.get_context(0)
    rc = ctx._lib.dctfp_l1_knn(ctx.handle, q.data_ptr(), 2, 480, b.data_ptr(), 2000, 480, 480, 1025, 0, v.data_ptr(), v.data_ptr(), None)
    assert rc == _lib.DCTFP_ERR_LIMIT


# ---- QuerySearch against search()

def _table(pids, doms, fps):
    from dctdomain_amd.query_db import Table
    return Table(list(pids), list(doms), np.ascontiguousarray(fps, dtype=np.int8))


def _old_bytes(qt, dt, khits):
    from dctdomain_amd import query_db
    qrows = [(i, p, d) for i, (p, d) in enumerate(zip(_strs(qt.pid, qt.pid_off), _strs(qt.dom, qt.dom_off)))]
    drows = [(i, p, d) for i, (p, d) in enumerate(zip(_strs(dt.pid, dt.pid_off), _strs(dt.dom, dt.dom_off)))]
    return ''.join(line + '\n' for line in query_db.search(qrows, qt.fps, drows, dt.fps, khits)).encode('utf8')


def _strs(txt, off):
    return [txt[off[i]:off[i + 1]].decode('utf8') for i in range(len(off) - 1)]


def _new_bytes(qt, dt, khits, **kw):
    from dctdomain_amd.query_db import QuerySearch
    out = []
    init = {x: kw.pop(x) for x in ('block_rows', 'device_budget', 'knn') if x in kw}
    QuerySearch(dt, **init).search(qt, khits, out.append, **kw)
    return b''.join(out)


def _random_tables(rng, n_prot_q, n_prot_d, levels=3, scale=1, pid_fn=None):
    def one(n_prot, tag):
        pids, doms, rows = [], [], []
        for p in range(n_prot):
            f = int(rng.integers(1, 6))
            pid = pid_fn(tag, p) if pid_fn else f'{tag}{p}'
            for j in range(f):
                pids.append(pid)
                doms.append(f'{j + 1}-{j + 40},{j + 60}-{j + 90}' if j % 2 else f'1-{j + 50}')
                rows.append(rng.integers(0, levels, size=480) * scale)
        order = rng.permutation(len(pids))                          # a protein's rows need not be adjacent in the table
        return [pids[i] for i in order], [doms[i] for i in order], np.clip(np.array(rows)[order], -128, 127)
    return _table(*one(n_prot_q, 'q')), _table(*one(n_prot_d, 'd'))


def test_query_search_random_ragged_with_ties():
    rng = np.random.default_rng(10)
    qt, dt = _random_tables(rng, 30, 200)
    for khits in (1, 50, 100, 300, 5000):
        exp = _old_bytes(qt, dt, khits)
        for knn in ('auto', 'fused', 'matrix'):
            assert _new_bytes(qt, dt, khits, knn=knn) == exp, (khits, knn)


def test_query_search_negative_scores_and_odd_pids():
    rng = np.random.default_rng(11)
    qt, dt = _random_tables(rng, 12, 60, levels=2, scale=127)       # L1 far above 17000: negative scores
    assert _new_bytes(qt, dt, 50) == _old_bytes(qt, dt, 50)
    odd = lambda tag, p: (f'{tag}-ß-λ-{p}' if p % 3 == 0 else (tag * 300 + str(p) if p % 3 == 1 else f'{tag}{p}'))
    qt, dt = _random_tables(rng, 12, 60, pid_fn=odd)
    assert _new_bytes(qt, dt, 30) == _old_bytes(qt, dt, 30)


def test_query_search_host_route_batches_and_blocks():
    rng = np.random.default_rng(12)
    qt, dt = _random_tables(rng, 20, 150)
    exp = _old_bytes(qt, dt, 40)
    assert _new_bytes(qt, dt, 40, rank_cap=50) == exp               # proteins of f * k > 50 ranked on the host
    assert _new_bytes(qt, dt, 40, batch_rows=3, text_bytes=300) == exp
    assert _new_bytes(qt, dt, 40, block_rows=37, batch_rows=7, text_bytes=1000) == exp
    for knn in ('fused', 'matrix'):                                   # blocks streamed from the host: a device budget of 0
        assert _new_bytes(qt, dt, 40, block_rows=50, device_budget=0, knn=knn, text_bytes=700) == exp


def _example_db(tmp_path):
    from dctdomain_amd.database import Database
    z = np.load(os.path.join(FIX, 'example-dct.npz'))
    db = Database(str(tmp_path / 'ex'), os.path.join(FIX, 'example.fasta'))
    fps = []
    for i, pid in enumerate(z['sid']):
        s, e = z['idx'][i], z['idx'][i + 1]
        doms = [str(d) for d in z['dom'][s:e]]
        fps.append(SimpleNamespace(pid=str(pid), domains=doms, quants={d: z['dct'][s + k] for k, d in enumerate(doms)}))
    db.add_fprints(fps)
    db.rename_vid()
    db.close()
    return str(tmp_path / 'ex.db')


def test_query_search_example_fixture_and_main(tmp_path):
    from dctdomain_amd import query_db
    from dctdomain_amd.database import Database
    path = _example_db(tmp_path)
    db = Database(path)
    t = query_db.load_table(db)
    db.close()
    for khits in (1, 50, 100, 300):
        assert _new_bytes(t, t, khits) == _old_bytes(t, t, khits), khits
    out = str(tmp_path / 'search.txt')
    query_db.main(['--query', path, '--db', path, '--out', out, '--khits', '50'])
    with open(out, 'rb') as fh:
        got = fh.read()
    with open(os.path.join(FIX, 'example-search.txt'), 'rb') as fh:
        assert got == fh.read()
    assert got == _old_bytes(t, t, 50)


def test_search_db_non_utf8_stream_goes_through_logging(tmp_path):
    """A log stream that is not UTF-8 gets the lines through logging.info, one by one: same text in that encoding."""
    import logging
    from dctdomain_amd import query_db
    from dctdomain_amd.database import Database
    path = _example_db(tmp_path)
    db = Database(path)
    t = query_db.load_table(db)
    db.close()
    out = str(tmp_path / 'search-utf16.txt')
    logging.basicConfig(level=logging.INFO, handlers=[logging.FileHandler(out, mode='w', encoding='utf-16')], format='%(message)s',
                        force=True)
    try:
        assert query_db._utf8_binary(logging.getLogger().handlers[0].stream) is None
        query_db.search_db(SimpleNamespace(khits=30), path, path)
        logging.getLogger().handlers[0].flush()
        with open(out, encoding='utf-16') as fh:
            got = fh.read()
    finally:
        logging.basicConfig(level=logging.WARNING, force=True)
    assert got.encode('utf8') == _old_bytes(t, t, 30)
