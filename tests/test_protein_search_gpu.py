"""Protein-level search without the all-against-all block matrix (dct_sim.ProteinSearch, dctfp_pair_min,
dctfp_select_count / dctfp_select_fill): the reference's own output on committed synthetic goldens, the block-matrix path
(dct_sim.Blocks) on random ragged files, the kernels against numpy, and a database Blocks could not hold."""

import gzip
import json
import os

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu
GOLD = os.path.join(gu.GOLD, 'protein_search')


def _run(tmp_path, argv):
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    dct_sim.main(argv + ['--output', out])
    return open(out).read()


def _goldens():
    with gzip.open(os.path.join(GOLD, 'expected.json.gz'), 'rt') as fh:
        return json.load(fh)


@pytest.mark.parametrize('run', _goldens()['runs'], ids=lambda r: f"{r['mode']}-top{r.get('top')}-thr{r.get('threshold')}")
def test_reference_goldens_byte_for_byte(tmp_path, run):
    if run['mode'] == 'db':
        got = _run(tmp_path, ['--dct', os.path.join(GOLD, 'query-dct.npz'), '--db', os.path.join(GOLD, 'db-dct.npz'),
                              '--top', str(run['top']), '--threshold', str(run['threshold'])])
    else:
        pairf, found = str(tmp_path / 'db.pair'), str(tmp_path / 'found.txt')
        with open(pairf, 'w') as fh:
            fh.write(_goldens()['pairs'])
        got = _run(tmp_path, ['--dct', os.path.join(GOLD, 'db-dct.npz'), '--pair', pairf, '--pairfound', found])
        assert open(found).read() == run['pairfound']
    assert got == run['expected']


# ---- the block-matrix path as it printed before ProteinSearch (the yardstick for ragged files with empty proteins)

def _blocks_db_search(qf, dbf, top, threshold):
    from dctdomain_amd import dct_sim
    blk = dct_sim.Blocks(qf, dbf)
    glob = dct_sim._sim(blk.last)
    lines = [dct_sim.HEADER]
    for i, query in enumerate(blk.rows):
        order = np.argsort(-glob[i], kind='stable')
        for rank, q in enumerate(order):
            if rank >= top and glob[i, q] < threshold:
                break
            maxs, s = blk.scores(i, q)
            lines.append(f'{query} {blk.cols[q]} {maxs} {s}')
    return '\n'.join(lines) + '\n'


def _blocks_pair_sim(npz, pairfile):
    from dctdomain_amd import dct_sim
    blk = dct_sim.Blocks(npz)
    where = {name: i for i, name in enumerate(blk.rows)}
    lines = [dct_sim.HEADER]
    for text in open(pairfile):
        if text.startswith('#'):
            continue
        a, b = text.split()[:2]
        if a in where and b in where:
            maxs, s = blk.scores(where[a], where[b])
            lines.append(f'{a} {b} {maxs} {s}')
    return '\n'.join(lines) + '\n'


def _ragged_npz(path, rng, n, prefix, spread):
    counts = rng.integers(0, 6, size=n)
    counts[rng.random(n) < 0.15] = 0                                # proteins without a fingerprint
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    centers = rng.integers(-40, 41, size=(4, 480))
    fam = rng.integers(0, 4, size=int(idx[-1]))
    dct = np.clip(centers[fam] + rng.integers(-spread, spread + 1, size=(int(idx[-1]), 480)), -128, 127).astype(np.int8)
    names = np.array([f'{prefix}{i}' for i in range(n)])
    if n > 6:
        names[5] = names[2]                                         # a repeated id
    np.savez(path, sid=names, idx=idx, dom=np.array(['1-9'] * int(idx[-1])), dct=dct)
    return names


@pytest.mark.parametrize('seed', [1, 2])
def test_db_search_and_pair_sim_match_the_block_path(tmp_path, monkeypatch, seed):
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(seed)
    qf, dbf = str(tmp_path / 'q-dct.npz'), str(tmp_path / 'db-dct.npz')
    _ragged_npz(qf, rng, 37, 'q', 30)
    names = _ragged_npz(dbf, rng, 83, 'd', 30)
    pairf = str(tmp_path / 'p.pair')
    with open(pairf, 'w') as fh:
        fh.write('# comment\n')
        for _ in range(200):
            i, j = rng.integers(0, len(names), size=2)
            fh.write(f'{names[i]} {names[j]}\n')
        fh.write('missing d1\n')
    cases = [(5, 0.25), (1, 0.0), (3, 1.5), (200, 0.25), (2, 0.6), (0, 0.5)]
    expected = {c: _blocks_db_search(qf, dbf, *c) for c in cases}
    exp_pairs = _blocks_pair_sim(dbf, pairf)
    monkeypatch.setattr(dct_sim.Blocks, '__init__', _refuse)
    for small in (False, True):
        if small:      # several database groups (merged per query), several query tiles, several pair chunks
            monkeypatch.setattr(dct_sim.ProteinSearch, 'COL_ROWS', 9)
            monkeypatch.setattr(dct_sim.ProteinSearch, 'TILE_INTS', 40)
        for top, thr in cases:
            got = _run(tmp_path, ['--dct', qf, '--db', dbf, '--top', str(top), '--threshold', str(thr)])
            assert got == expected[(top, thr)], (small, top, thr)
        assert _run(tmp_path, ['--dct', dbf, '--pair', pairf]) == exp_pairs


def _refuse(*a, **k):
    raise AssertionError('the all-against-all block matrix must not be built')


# ---- kernels

def test_pair_min_against_numpy():
    from dctdomain_amd.similarity import pair_min
    rng = np.random.default_rng(4)
    for d in (480, 475, 33, 600):
        counts_a = np.array([1, 60, 0, 3, 2, 1, 5, 0, 12])
        counts_b = np.array([4, 1, 0, 60, 7, 2])
        ia = np.concatenate([[0], np.cumsum(counts_a)])
        ib = np.concatenate([[0], np.cumsum(counts_b)])
        a = rng.integers(-128, 128, size=(ia[-1], d)).astype(np.int8)
        b = rng.integers(-128, 128, size=(ib[-1], d)).astype(np.int8)
        b[ib[4]:ib[4] + 2] = a[ia[1] + 7]                             # an exact match inside a block
        pairs = np.array([(i, j) for i in range(len(counts_a)) for j in range(len(counts_b))] + [(1, 3)] * 5 + [(0, 0)])
        dist = np.abs(a.astype(np.int64)[:, None, :] - b.astype(np.int64)[None, :, :]).sum(-1)
        mn, last = pair_min(a, ia, b, ib, pairs)
        for k, (i, j) in enumerate(pairs):
            blk = dist[ia[i]:ia[i + 1], ib[j]:ib[j + 1]]
            exp = (blk.min(), blk[-1, -1]) if blk.size else (0x7fffffff, 0x7fffffff)
            assert (mn[k], last[k]) == exp, (d, i, j)
        # a protein against itself (the same matrix on both sides): min 0
        mn, last = pair_min(a, ia, a, ia, [(1, 1), (6, 6), (2, 2)])
        assert mn.tolist() == [0, 0, 0x7fffffff] and last.tolist() == [0, 0, 0x7fffffff]
    with pytest.raises(IndexError):
        pair_min(a, ia, b, ib, [(0, len(counts_b))])


def _expected_selection(dist, top, bound, row_empty, col_empty):
    key = np.minimum(dist.astype(np.int64), 17000)
    key[row_empty.astype(bool)] = 17000
    key[:, col_empty.astype(bool)] = 17000
    out = []
    for r in range(len(key)):
        order = np.argsort(key[r], kind='stable')
        m = min(key.shape[1], max(top, int(np.count_nonzero(key[r] <= bound))))
        out.append((key[r][order[:m]], order[:m]))
    return out


def test_threshold_select_against_stable_argsort():
    import torch
    from dctdomain_amd.similarity import threshold_select
    rng = np.random.default_rng(9)
    for n_cols in (1, 7, 1000, 3000, 70000):
        n_rows = 12
        dist = rng.integers(5000, 40000, size=(n_rows, n_cols)).astype(np.int32)
        dist[0] = rng.integers(0, 3, size=n_cols) * 6000              # ties everywhere: c == n_cols at bound 17000
        dist[1] = 12750                                              # every entry exactly at the bound
        dist[2] = 99999                                              # c == 0: the first `top` columns
        dist[3, ::7] = rng.integers(0, 13000, size=len(dist[3, ::7]))  # c > top for small top
        dist[4, :3] = 100                                            # c < top
        dist[5, -1] = 16999
        dist[5, max(0, n_cols - 2)] = 17000
        row_empty = np.zeros(n_rows, np.uint8)
        row_empty[6] = 1
        col_empty = (rng.random(n_cols) < 0.1).astype(np.uint8)
        dev = torch.from_numpy(dist).cuda()
        for top in (1, 5, 2000):
            for bound in (-1, 12750, 17000, 0):
                off, key, col = threshold_select(dev, top, bound, row_empty, col_empty)
                exp = _expected_selection(dist, top, bound, row_empty, col_empty)
                for r in range(n_rows):
                    s = slice(off[r], off[r + 1])
                    np.testing.assert_array_equal(col[s], exp[r][1], err_msg=f'{n_cols} {top} {bound} row {r}')
                    np.testing.assert_array_equal(key[s], exp[r][0])
    # a strided tile (a column slice of a wider matrix) and no flags
    wide = torch.from_numpy(rng.integers(0, 20000, size=(5, 900)).astype(np.int32)).cuda()
    off, key, col = threshold_select(wide[:, 100:700], 4, 12750)
    exp = _expected_selection(wide[:, 100:700].cpu().numpy(), 4, 12750, np.zeros(5, np.uint8), np.zeros(600, np.uint8))
    for r in range(5):
        np.testing.assert_array_equal(col[off[r]:off[r + 1]], exp[r][1])


# ---- scale

def test_db_search_at_300k_database_proteins(tmp_path, monkeypatch):
    """300 000 database proteins x 3 000 queries: the block matrix would be 2 x 3.6 GB of host int32 and 1.7e10 L1 values;
    the search ranks 9e8 whole-protein pairs and prints a few per query.  Hits of sampled queries against brute force."""
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(21)
    n_db, n_q = 300_000, 3_000
    counts = rng.integers(1, 5, size=n_db)
    counts[rng.random(n_db) < 0.01] = 0
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    dct = rng.integers(-48, 49, size=(int(idx[-1]), 480), dtype=np.int8)    # unrelated pairs: L1 ~ 15 000, below 17 000
    qcounts = rng.integers(1, 4, size=n_q)
    qidx = np.concatenate([[0], np.cumsum(qcounts)]).astype(np.int64)
    qdct = rng.integers(-48, 49, size=(int(qidx[-1]), 480), dtype=np.int8)
    planted = rng.choice(n_q, size=60, replace=False)                       # near-duplicates: 6-9 threshold hits each
    for k, q in enumerate(planted):
        for t in rng.choice(np.flatnonzero(counts > 0), size=6 + k % 4, replace=False):
            dct[idx[t + 1] - 1] = np.clip(qdct[qidx[q + 1] - 1].astype(np.int16) + rng.integers(-9, 10, size=480), -128, 127)
    qf, dbf = str(tmp_path / 'q-dct.npz'), str(tmp_path / 'db-dct.npz')
    np.savez(qf, sid=np.array([f'q{i}' for i in range(n_q)]), idx=qidx, dom=np.array(['1-9']), dct=qdct)
    np.savez(dbf, sid=np.array([f'd{i}' for i in range(n_db)]), idx=idx, dom=np.array(['1-9']), dct=dct)
    monkeypatch.setattr(dct_sim.Blocks, '__init__', _refuse)
    text = _run(tmp_path, ['--dct', qf, '--db', dbf, '--top', '5', '--threshold', '0.25'])
    lines = text.split('\n')[1:-1]
    by_query = {}
    for ln in lines:
        q, d, dom, glob = ln.split()
        by_query.setdefault(q, []).append((d, dom, glob))
    assert len(by_query) == n_q
    db_last, db_empty = dct_sim._last_rows(dct, idx)
    for q in list(planted[:5]) + list(rng.choice(n_q, size=5, replace=False)):
        ql = qdct[qidx[q + 1] - 1].astype(np.int16)
        l1 = np.abs(db_last.astype(np.int16) - ql).sum(1, dtype=np.int64)
        key = np.where(db_empty.astype(bool), 17000, np.minimum(l1, 17000))
        order = np.argsort(key, kind='stable')
        m = max(5, int(np.count_nonzero(key <= 12750)))
        exp = []
        for t in order[:m]:
            blk = np.abs(qdct[qidx[q]:qidx[q + 1]].astype(np.int16)[:, None, :] - dct[idx[t]:idx[t + 1]].astype(np.int16)[None]).sum(-1)
            mn, last = (int(blk.min()), int(blk[-1, -1])) if blk.size else (0x7fffffff, 0x7fffffff)
            maxs, s = dct_sim._scores(mn, last)
            exp.append((f'd{t}', str(maxs), str(s)))
        assert by_query[f'q{q}'] == exp, q
    assert sum(len(v) > 5 for v in by_query.values()) >= 30                 # the planted queries report threshold hits
