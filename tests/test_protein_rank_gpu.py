"""dct-sim --db --rank domain: dctfp_protein_min (similarity.protein_min) against numpy and against l1_matrix + block_min, and
the command's output against a CPU oracle of the reference's db_search loop with DCTdomain as the key."""

import gzip
import json
import os

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu
GOLD = os.path.join(gu.GOLD, 'protein_search')
BIG = 0x7fffffff


def _l1(a, b):
    """int64 (na, nb) row L1 matrix, in chunks of rows of a."""
    out = np.empty((len(a), len(b)), dtype=np.int64)
    b16 = b.astype(np.int16)
    for i0 in range(0, len(a), 8):
        out[i0:i0 + 8] = np.abs(a[i0:i0 + 8, None, :].astype(np.int16) - b16[None]).sum(-1, dtype=np.int64)
    return out


def _np_protein_min(a, ia, b, ib):
    """Row L1 matrix -> minimum per (protein of a, protein of b) block; 0x7fffffff for a protein without rows."""
    ia, ib = np.asarray(ia, np.int64), np.asarray(ib, np.int64)
    out = np.full((len(ia) - 1, len(ib) - 1), BIG, dtype=np.int64)
    ne_a, ne_b = np.flatnonzero(np.diff(ia) > 0), np.flatnonzero(np.diff(ib) > 0)
    if len(ne_a) == 0 or len(ne_b) == 0:
        return out
    dist = _l1(a[ia[0]:ia[-1]], b[ib[0]:ib[-1]])
    rows = np.minimum.reduceat(dist, ia[ne_a] - ia[0], axis=0)
    out[np.ix_(ne_a, ne_b)] = np.minimum.reduceat(rows, ib[ne_b] - ib[0], axis=1)
    return out


def _idx(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _check(a, ia, b, ib, **kw):
    import torch
    from dctdomain_amd.similarity import block_min, l1_matrix, protein_min
    got = protein_min(a, ia, b, ib, **kw)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (len(ia) - 1, len(ib) - 1)
    got = got.cpu().numpy()
    exp = _np_protein_min(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a), ia,
                          np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b), ib)
    np.testing.assert_array_equal(got.astype(np.int64), exp)
    if (np.diff(ia) > 0).any() and (np.diff(ib) > 0).any():
        ref = block_min(l1_matrix(a, b), ia, ib)[0]
        assert got.tobytes() == ref.tobytes()
    return got


@pytest.mark.parametrize('d', [480, 475, 33, 512])
def test_protein_min_ragged_against_numpy(d):
    rng = np.random.default_rng(d)
    counts_a = np.array([1, 5, 0, 4, 300, 1, 0, 5, 4, 129, 1, 1, 2, 0])          # a 300-row protein spans three sub-tiles
    counts_b = np.concatenate([rng.integers(0, 6, size=150), [0, 131, 1], np.ones(200, int), rng.integers(4, 6, size=60), [0]])
    ia, ib = _idx(counts_a), _idx(counts_b)
    a = rng.integers(-128, 128, size=(ia[-1], d)).astype(np.int8)
    b = rng.integers(-128, 128, size=(ib[-1], d)).astype(np.int8)
    a[ia[4] + 17] = 127                                                          # full-range values: the largest distances
    b[ib[151] + 3] = -128
    b[ib[10]:ib[10] + 1] = a[ia[4] + 250]                                       # exact matches deep inside large proteins
    b[ib[151] + 130] = a[ia[9] + 128]
    _check(a, ia, b, ib)
    _check(b, ib, a, ia)                                                         # the other way round


def test_protein_min_single_protein_and_many_segments():
    rng = np.random.default_rng(5)
    counts_b = rng.integers(0, 7, size=2500)                                    # several 1024-protein packing segments
    counts_b[rng.random(2500) < 0.1] = 0
    ib = _idx(counts_b)
    b = rng.integers(-60, 61, size=(ib[-1], 480)).astype(np.int8)
    for counts_a in ([3], [1], [260], [0, 2]):
        ia = _idx(counts_a)
        a = rng.integers(-60, 61, size=(ia[-1], 480)).astype(np.int8)
        _check(a, ia, b, ib)
    one = _idx([1])
    _check(b[:1], one, b[:1], one)                                              # one row on each side


def test_protein_min_empty_sides():
    rng = np.random.default_rng(6)
    a = rng.integers(-128, 128, size=(7, 480)).astype(np.int8)
    got = _check(a, _idx([3, 0, 4]), np.zeros((0, 480), np.int8), _idx([0, 0]))
    assert (got == BIG).all()
    got = _check(a, _idx([0, 0, 0]), a, _idx([3, 4]))
    assert (got == BIG).all()


def test_protein_min_strided_rows_and_output():
    import torch
    rng = np.random.default_rng(7)
    ia, ib = _idx([2, 5, 1, 0, 140, 4]), _idx(rng.integers(0, 6, size=70))
    wide_a = torch.from_numpy(rng.integers(-128, 128, size=(ia[-1], 528)).astype(np.int8)).cuda()
    wide_b = torch.from_numpy(rng.integers(-128, 128, size=(ib[-1], 496)).astype(np.int8)).cuda()
    a, b = wide_a[:, :480], wide_b[:, :480]                                     # lda = 528, ldb = 496
    assert a.stride(0) == 528 and b.stride(0) == 496
    canvas = torch.full((len(ia) - 1, 90), -5, dtype=torch.int32, device='cuda')
    out = canvas[:, 7:7 + len(ib) - 1]                                          # ldo = 90, not a multiple of anything
    got = _check(a, ia, b, ib, out=out)
    c = canvas.cpu().numpy()
    assert (c[:, :7] == -5).all() and (c[:, 7 + len(ib) - 1:] == -5).all()       # nothing written outside the tile
    np.testing.assert_array_equal(out.cpu().numpy(), got)


def test_protein_min_wider_than_the_kernel_falls_back():
    from dctdomain_amd import _lib
    from dctdomain_amd.similarity import to_device_int8
    rng = np.random.default_rng(8)
    ia, ib = _idx([1, 4, 0, 3]), _idx([2, 0, 5])
    a = rng.integers(-128, 128, size=(ia[-1], 600)).astype(np.int8)
    b = rng.integers(-128, 128, size=(ib[-1], 600)).astype(np.int8)
    _check(a, ia, b, ib)
    import ctypes
    import torch
    ta, tb = to_device_int8(a), to_device_int8(b)
    da, db = torch.as_tensor(ia, device='cuda'), torch.as_tensor(ib, device='cuda')
    out = torch.full((3, 2), -1, dtype=torch.int32, device='cuda')
    ctx = _lib.get_context(0)
    rc = ctx._lib.dctfp_protein_min(ctx.handle, ta.data_ptr(), 600, da.data_ptr(), 3, tb.data_ptr(), 600, db.data_ptr(), 2, 600,
                                    out.data_ptr(), 2, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.DCTFP_ERR_LIMIT and (out.cpu().numpy() == -1).all()      # a limit: nothing written


# ---- the command against a CPU oracle

def _oracle(qf, dbf, top, threshold):
    """The reference's db_search loop (src/dct-sim.py:136-156) with the domain score as the key: every (query, database)
    minimum, a stable sort by DCTdomain descending, the first `top` lines, then more while DCTdomain >= threshold."""
    from dctdomain_amd import dct_sim
    q, d = np.load(qf), np.load(dbf)
    qi, di = np.asarray(q['idx'], np.int64), np.asarray(d['idx'], np.int64)
    mn = _np_protein_min(q['dct'], qi, d['dct'], di)
    ql, qe = dct_sim._last_rows(q['dct'], qi)
    dl, de = dct_sim._last_rows(d['dct'], di)
    lines = [dct_sim.HEADER]
    for i, query in enumerate(q['sid']):
        last = _l1(ql[i:i + 1], dl)[0]
        last[de.astype(bool)] = BIG
        if qe[i]:
            last[:] = BIG
        scores = [dct_sim._scores(m, l) for m, l in zip(mn[i], last)]
        order = sorted(range(len(scores)), key=lambda j: scores[j][0], reverse=True)
        for rank, j in enumerate(order):
            if rank >= top and scores[j][0] < threshold:
                break
            lines.append(f'{query} {d["sid"][j]} {scores[j][0]} {scores[j][1]}')
    return '\n'.join(lines) + '\n'


def _run(tmp_path, argv):
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    dct_sim.main(argv + ['--output', out])
    return open(out).read()


def _refuse(*a, **k):
    raise AssertionError('the all-against-all block matrix must not be built')


GOLDEN_CASES = [(5, 0.25), (5, 0.0), (5, 1.5), (1000, 0.25), (3, 0.5)]


@pytest.mark.parametrize('top,threshold', GOLDEN_CASES)
def test_rank_domain_on_the_committed_goldens(tmp_path, monkeypatch, top, threshold):
    from dctdomain_amd import dct_sim
    qf, dbf = os.path.join(GOLD, 'query-dct.npz'), os.path.join(GOLD, 'db-dct.npz')
    monkeypatch.setattr(dct_sim.Blocks, '__init__', _refuse)
    got = _run(tmp_path, ['--dct', qf, '--db', dbf, '--top', str(top), '--threshold', str(threshold), '--rank', 'domain'])
    assert got == _oracle(qf, dbf, top, threshold)


def test_rank_global_given_explicitly_prints_what_no_flag_prints(tmp_path):
    with gzip.open(os.path.join(GOLD, 'expected.json.gz'), 'rt') as fh:
        runs = [r for r in json.load(fh)['runs'] if r['mode'] == 'db']
    qf, dbf = os.path.join(GOLD, 'query-dct.npz'), os.path.join(GOLD, 'db-dct.npz')
    for run in runs:
        argv = ['--dct', qf, '--db', dbf, '--top', str(run['top']), '--threshold', str(run['threshold'])]
        plain = _run(tmp_path, argv)
        assert plain == run['expected']
        assert _run(tmp_path, argv + ['--rank', 'global']) == plain


def _planted_files(tmp_path, seed):
    """Random ragged files (empty proteins, four families) with planted cases: query q0 is one zero row; database proteins
    at L1 exactly 17 000 / 17 001 / 12 750 (the 0.25 bound) from it, twins (ties), and far rows around the planted ones."""
    rng = np.random.default_rng(seed)
    centers = rng.integers(-40, 41, size=(4, 480))

    def ragged(n, lo):
        counts = rng.integers(lo, 6, size=n)
        counts[rng.random(n) < 0.12] = 0
        idx = _idx(counts)
        fam = rng.integers(0, 4, size=int(idx[-1]))
        dct = np.clip(centers[fam] + rng.integers(-30, 31, size=(int(idx[-1]), 480)), -128, 127).astype(np.int8)
        return counts, dct

    qc, qd = ragged(30, 0)
    qc, qd = np.concatenate([[1], qc]), np.concatenate([np.zeros((1, 480), np.int8), qd])
    dc, dd = ragged(90, 0)
    rows = []
    for l1 in (17000, 17001, 12750, 12750, 12749):
        row = np.full(480, l1 // 480, np.int64)
        row[:l1 % 480] += 1
        assert row.sum() == l1
        rows.append(np.stack([np.full(480, -128), row, np.full(480, -128)]).astype(np.int8))
    twin = dd[_idx(dc)[7]:_idx(dc)[8]]
    extra = rows + [twin, twin]
    dc = np.concatenate([dc, [len(e) for e in extra]])
    dd = np.concatenate([dd] + extra)
    qf, dbf = str(tmp_path / f'q{seed}-dct.npz'), str(tmp_path / f'db{seed}-dct.npz')
    np.savez(qf, sid=np.array([f'q{i}' for i in range(len(qc))]), idx=_idx(qc), dom=np.array(['1-9']), dct=qd)
    np.savez(dbf, sid=np.array([f'd{i}' for i in range(len(dc))]), idx=_idx(dc), dom=np.array(['1-9']), dct=dd)
    return qf, dbf


@pytest.mark.parametrize('seed', [1, 2])
def test_rank_domain_on_random_files_and_tiny_tiles(tmp_path, monkeypatch, seed):
    from dctdomain_amd import dct_sim
    qf, dbf = _planted_files(tmp_path, seed)
    cases = [(5, 0.25), (1, 0.0), (3, 1.5), (0, 0.25), (0, 0.5), (1000, 0.25), (2, 0.6)]
    expected = {c: _oracle(qf, dbf, *c) for c in cases}
    q0 = [ln.split()[2] for ln in expected[(0, 0.25)].split('\n') if ln.startswith('q0 ')]
    assert q0.count('0.25') == 2 and '0.0' not in q0                          # the bound is inclusive, both twins kept
    monkeypatch.setattr(dct_sim.Blocks, '__init__', _refuse)
    for small in (False, True):
        if small:      # several database groups (merged per query) and several query tiles and chunks
            monkeypatch.setattr(dct_sim.ProteinSearch, 'COL_ROWS', 9)
            monkeypatch.setattr(dct_sim.ProteinSearch, 'TILE_INTS', 40)
        for top, thr in cases:
            got = _run(tmp_path, ['--dct', qf, '--db', dbf, '--top', str(top), '--threshold', str(thr), '--rank', 'domain'])
            assert got == expected[(top, thr)], (small, top, thr)


# ---- scale

def test_rank_domain_finds_shared_domains_among_200k_proteins(tmp_path, monkeypatch):
    """200 000 database proteins x 300 queries.  Planted: database proteins that share one domain fingerprint (within a small
    distance) with a query but whose whole-protein fingerprints are unrelated -- DCTglobal below 0.25, DCTdomain above.  The
    domain ranking reports every one of them; the global ranking does not reach them."""
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(31)
    n_db, n_q = 200_000, 300
    counts = rng.integers(1, 5, size=n_db)
    counts[rng.random(n_db) < 0.01] = 0
    idx = _idx(counts)
    dct = rng.integers(-48, 49, size=(int(idx[-1]), 480), dtype=np.int8)      # unrelated pairs: L1 ~ 15 000 (sim ~ 0.1)
    qcounts = rng.integers(2, 5, size=n_q)
    qidx = _idx(qcounts)
    qdct = rng.integers(-48, 49, size=(int(qidx[-1]), 480), dtype=np.int8)
    planted_q = rng.choice(n_q, size=40, replace=False)
    multi = np.flatnonzero(counts >= 2)
    planted = {}
    for k, q in enumerate(planted_q):
        targets = rng.choice(multi, size=3 + k % 3, replace=False)
        for t in targets:
            dom = qdct[qidx[q] + rng.integers(0, qcounts[q] - 1)].astype(np.int16)  # a domain row, not the whole protein
            dct[idx[t]] = np.clip(dom + rng.integers(-9, 10, size=480), -128, 127)
        planted[q] = targets
    qf, dbf = str(tmp_path / 'q-dct.npz'), str(tmp_path / 'db-dct.npz')
    np.savez(qf, sid=np.array([f'q{i}' for i in range(n_q)]), idx=qidx, dom=np.array(['1-9']), dct=qdct)
    np.savez(dbf, sid=np.array([f'd{i}' for i in range(n_db)]), idx=idx, dom=np.array(['1-9']), dct=dct)
    monkeypatch.setattr(dct_sim.Blocks, '__init__', _refuse)
    text = _run(tmp_path, ['--dct', qf, '--db', dbf, '--top', '5', '--threshold', '0.25', '--rank', 'domain'])
    glob = _run(tmp_path, ['--dct', qf, '--db', dbf, '--top', '5', '--threshold', '0.25'])

    def by_query(t):
        out = {}
        for ln in t.split('\n')[1:-1]:
            q, d, dom, g = ln.split()
            out.setdefault(q, []).append((d, dom, g))
        return out

    dom_hits, glob_hits = by_query(text), by_query(glob)
    assert len(dom_hits) == n_q
    found_only_by_domain = 0
    for q, targets in planted.items():
        hits = {d: (float(dom), float(g)) for d, dom, g in dom_hits[f'q{q}']}
        for t in targets:
            assert f'd{t}' in hits, (q, t)
            dom, g = hits[f'd{t}']
            assert dom >= 0.25 and g < 0.25
            found_only_by_domain += f'd{t}' not in {d for d, _, _ in glob_hits[f'q{q}']}
    assert found_only_by_domain >= 100
    # sampled queries line for line against the oracle (the whole database, numpy)
    db_last, db_empty = dct_sim._last_rows(dct, idx)
    for q in list(planted_q[:2]) + list(rng.choice(n_q, size=2, replace=False)):
        qrows = qdct[qidx[q]:qidx[q + 1]]
        mn = np.full(n_db, BIG, dtype=np.int64)
        for c0 in range(0, n_db, 25_000):
            c1 = min(n_db, c0 + 25_000)
            mn[c0:c1] = _np_protein_min(qrows, [0, len(qrows)], dct, idx[c0:c1 + 1])[0]
        last = _l1(qrows[-1:], db_last)[0]
        last[db_empty.astype(bool)] = BIG
        dom = dct_sim._sim(mn)
        order = np.argsort(-dom, kind='stable')
        m = max(5, int(np.count_nonzero(dom >= 0.25)))
        exp = []
        for t in order[:m]:
            a, g = dct_sim._scores(mn[t], last[t])
            exp.append((f'd{t}', str(a), str(g)))
        assert dom_hits[f'q{q}'] == exp, q
