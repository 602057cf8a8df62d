"""dct-sim --db --zscore on the GPU (similarity.rect_moments = dctfp_rect_moments; ProteinSearch.search(zscore=True); ReciprocalBest;
the text) against the rule of zscore_rule.py (pinned on hand-computed cases in test_zscore_host.py).  Everything is compared exactly:
the moments are integers, and z follows from them with the rule's own arithmetic."""

import os

import numpy as np
import pytest

import rbh_rule as rrule
import zscore_rule as zr

pytestmark = pytest.mark.gpu
LIMIT = 255 * 480 + 1
# the edges of a step of 1024 columns and of a band of 64 rows: 65 x 1025 = a second band of one row and a second step of one column,
# 129 x 3 = three bands, 130 x 2051 = three bands, the third of two rows, and three steps, the third of three columns
SHAPES = [(1, 1), (1, 1025), (63, 3), (64, 1024), (65, 1025), (129, 3), (130, 2051)]
G6PD = os.path.join(rrule.gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')
EXAMPLE = os.path.join(rrule.gu.GOLD, 'ref_fixtures', 'example-dct.npz')
GOLD_Q, GOLD_DB = (os.path.join(rrule.GOLD, name + '-dct.npz') for name in ('query', 'db'))


# ---- 1. rect_moments against numpy on raw tiles

def _tile(rng, n_rows, n_cols, limit=LIMIT):
    """Values 0 .. 5 (many repeats), about a tenth replaced by limit - 1 (counts), limit, 0x7fffffff and -1 (do not), and -- in a tile
    of three rows or more -- one row that is limit - 1 throughout: its sum of squares passes 2^32 with one entry, a column's over a
    band too."""
    t = rng.integers(0, 6, size=(n_rows, n_cols)).astype(np.int64)
    u = rng.random((n_rows, n_cols))
    for k, v in enumerate((limit - 1, limit, 0x7fffffff, -1)):
        t[(u >= 0.025 * k) & (u < 0.025 * (k + 1))] = v
    if n_rows >= 3:
        t[n_rows // 2] = limit - 1
    return t.astype(np.int32)


def _view(t):
    """The tile as the view big[:, 1:1 + n_cols] of a wider device tensor: ld != n_cols, rows off 16-byte boundaries; what lies
    beside it is 1, which would change every sum if it were read."""
    import torch
    big = torch.ones((t.shape[0], t.shape[1] + 6), dtype=torch.int32, device='cuda')
    view = big[:, 1:1 + t.shape[1]]
    view.copy_(torch.as_tensor(t, device='cuda'))
    assert view.data_ptr() - big.data_ptr() == 4 and (t.shape[0] == 1 or view.stride(0) == t.shape[1] + 6)
    return view


def _words(state):
    """(row, col) as uint64, None for a side the state lacks -- through moments(), which hands out int64."""
    out = state.moments()
    assert all(m is None or (m.dtype == np.int64 and m.shape[0] == 3) for m in out)
    return tuple(None if m is None else m.view(np.uint64) for m in out)


@pytest.mark.parametrize('n_rows,n_cols', SHAPES)
def test_rect_moments_against_numpy(n_rows, n_cols):
    from dctdomain_amd.similarity import MomentState, rect_moments
    rng = np.random.default_rng(100 * n_rows + n_cols)
    t = _tile(rng, n_rows, n_cols)
    view = _view(t)
    for k, (row0, col0) in enumerate([(0, 0), (5, 0), (0, 7), (3, 1030)]):
        n_a, n_b = row0 + n_rows + k, col0 + n_cols + 2 * k
        for flags in ((None, None), (rng.random(n_rows) < 0.2, rng.random(n_cols) < 0.2)):
            want = zr.tile_moments(t, row0, col0, n_a, n_b, LIMIT, *flags)
            if flags[0] is None and n_rows >= 3:
                # what the case exercises: the full row counts everywhere, a tenth of the rest does not; S2 beyond 32 bits
                assert want[0][0, row0 + n_rows // 2] == n_cols and int(want[0][2].max()) >= n_cols * (LIMIT - 1) ** 2 > 1 << 32
                assert want[0][0].sum() < n_rows * n_cols and int(want[1][2].max()) > 1 << 32
            for rows, cols in ((True, True), (True, False), (False, True)):
                state = MomentState(n_a, n_b, rows=rows, cols=cols)
                rect_moments(view, row0, col0, state, *flags, limit=LIMIT)
                got = _words(state)
                # every word equals numpy's; the words outside the tile are numpy's zeros
                assert (got[0] is None) == (not rows) and (got[1] is None) == (not cols)
                for side in range(2):
                    assert got[side] is None or np.array_equal(got[side], want[side]), (row0, col0, flags[0] is not None, rows, cols, side)


def test_one_value_everywhere_and_sums_beyond_32_bits():
    """300 x 2100 of limit - 1: every 32-bit partial sum is at its largest for this limit, every row's S1 passes 2^27 and a column's
    S2 over a band of 64 rows passes 2^39; then the largest limit the kernel takes, where the partial sums just fit 32 bits."""
    import torch
    from dctdomain_amd.similarity import MomentState, rect_moments
    for limit in (LIMIT, 1 << 24):
        t = np.full((300, 2100), limit - 1, dtype=np.int32)
        state = MomentState(300, 2100)
        rect_moments(torch.as_tensor(t, device='cuda'), 0, 0, state, limit=limit)
        want = zr.tile_moments(t, 0, 0, 300, 2100, limit)
        got = _words(state)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert int(got[0][2, 0]) == 2100 * (limit - 1) ** 2 and int(got[1][1, 0]) == 300 * (limit - 1)
    assert 64 * 4 * ((1 << 24) - 1) > 0xf0000000                         # (a wave's sum of a row at that limit: just below 2^32)


# ---- 2. accumulation

def test_sub_tiles_in_any_order_equal_one_call():
    from dctdomain_amd.similarity import MomentState, rect_moments
    n_rows, n_cols = SHAPES[-1]
    rng = np.random.default_rng(7)
    t = _tile(rng, n_rows, n_cols)
    view = _view(t)
    row_empty, col_empty = rng.random(n_rows) < 0.1, rng.random(n_cols) < 0.1
    whole = MomentState(n_rows + 1, n_cols + 1)
    rect_moments(view, 1, 1, whole, row_empty, col_empty, limit=LIMIT)
    parts = [(r0, r1, c0, c1) for r0, r1 in ((0, 67), (67, n_rows)) for c0, c1 in ((0, 1000), (1000, 1029), (1029, n_cols))]
    cut = MomentState(n_rows + 1, n_cols + 1)
    for k in rng.permutation(len(parts)).tolist():
        r0, r1, c0, c1 = parts[k]
        rect_moments(view[r0:r1, c0:c1], 1 + r0, 1 + c0, cut, row_empty[r0:r1], col_empty[c0:c1], limit=LIMIT)
    want = zr.tile_moments(t, 1, 1, n_rows + 1, n_cols + 1, LIMIT, row_empty, col_empty)
    assert all(np.array_equal(a, b) for a, b in zip(_words(cut), _words(whole)))
    assert all(np.array_equal(a, b) for a, b in zip(_words(whole), want))
    # a second call over the same tile adds the same again
    rect_moments(view, 1, 1, whole, row_empty, col_empty, limit=LIMIT)
    assert all(np.array_equal(a, 2 * b) for a, b in zip(_words(whole), want))


# ---- 3. refusals

def test_rect_moments_refuses_what_it_cannot_hold():
    import torch
    from dctdomain_amd import _lib, similarity
    from dctdomain_amd.similarity import MomentState, rect_moments
    tile = torch.full((4, 8), 3, dtype=torch.int32, device='cuda')
    state = MomentState(4, 8)
    for bad in (tile.long(), tile[0], tile.t(), tile.cpu()):
        with pytest.raises(ValueError):
            rect_moments(bad, 0, 0, state)
    for row0, col0 in ((-1, 0), (0, -1)):
        with pytest.raises(ValueError):
            rect_moments(tile, row0, col0, state)
    for row0, col0 in ((1, 0), (0, 1)):
        with pytest.raises(IndexError):
            rect_moments(tile, row0, col0, state)
    with pytest.raises(ValueError):
        rect_moments(tile, 0, 0, MomentState(4, 8, rows=False, cols=False))
    broken = MomentState(4, 8)
    broken.row = broken.row.to(torch.int32)
    with pytest.raises(ValueError):
        rect_moments(tile, 0, 0, broken)
    broken = MomentState(4, 8)
    broken.col = broken.col[:, :7]
    with pytest.raises(ValueError):
        rect_moments(tile, 0, 0, broken)
    # a side the state does not have is not compared with the tile: rows only, far to the right
    rows_only = MomentState(4, 0, cols=False)
    assert rows_only.col is None and rows_only.moments()[1] is None
    rect_moments(tile, 0, 1000, rows_only)
    assert rows_only.row.cpu().tolist() == [[8] * 4, [24] * 4, [72] * 4]
    with pytest.raises(IndexError):
        rect_moments(tile, 1, 1000, rows_only)
    cols_only = MomentState(0, 8, rows=False)
    rect_moments(tile, 1000, 0, cols_only)
    assert cols_only.col.cpu().tolist() == [[4] * 8, [12] * 8, [36] * 8]
    # the export's own conditions
    dev, name = tile.device, 'dctfp_rect_moments'
    lead = (tile.data_ptr(), 4, 8, 8, 0, 0, None, None, LIMIT, LIMIT)
    arrays = (state.row.data_ptr(), 4, state.col.data_ptr(), 8)

    def refused(*args):
        with pytest.raises(_lib.DctfpError) as err:
            similarity._launch(dev, name, *args)
        assert err.value.code == _lib.DCTFP_ERR_INVALID and err.value.msg.startswith(name + ': ')
        return err.value.msg

    assert 'both NULL' in refused(*lead, None, 4, None, 8)
    assert 'NULL' in refused(None, *lead[1:], *arrays)
    assert 'shape' in refused(*lead[:3], 7, *lead[4:], *arrays)                                       # ld < n_cols
    assert 'shape' in refused(*lead[:1], -1, *lead[2:], *arrays)
    assert 'shape' in refused(*lead[:4], -1, *lead[5:], *arrays)
    assert 'shape' in refused(*lead[:8], -1, -1, *arrays)                                             # cap < 0
    assert 'aligned' in refused(lead[0] + 2, *lead[1:], *arrays)
    assert 'aligned' in refused(*lead, arrays[0] + 4, 4, arrays[2], 8)
    assert 'aligned' in refused(*lead, arrays[0], 4, arrays[2] + 4, 8)
    assert 'outside' in refused(*lead, arrays[0], 3, arrays[2], 8)
    assert 'outside' in refused(*lead, arrays[0], 4, arrays[2], 7)
    assert 'outside' in refused(*lead[:4], 1, 0, *lead[6:], *arrays)
    assert 'n_a and n_b' in refused(*lead, arrays[0], -1, arrays[2], 8)
    assert 'n_a and n_b' in refused(*lead, arrays[0], 4, arrays[2], 1 << 31)
    assert 'cap above 16777216' in refused(*lead[:8], (1 << 24) + 1, (1 << 24) + 1, *arrays)
    with pytest.raises(_lib.DctfpError, match='cap above 16777216'):
        rect_moments(tile, 0, 0, state, limit=(1 << 24) + 1)
    # n (limit - 1)^2 must fit 64 bits.  A row that meets 2^20 columns: (limit - 1)^2 < 2^44, so 2^22 is the largest limit
    far = (1 << 20) - 8
    with pytest.raises(_lib.DctfpError, match='does not fit the 64 bits') as err:
        rect_moments(tile, 0, far, rows_only, limit=(1 << 22) + 1)
    assert err.value.code == _lib.DCTFP_ERR_INVALID and err.value.msg.startswith(name + ': ')
    top = torch.full((4, 8), (1 << 22) - 1, dtype=torch.int32, device='cuda')
    most = MomentState(4, 0, cols=False)
    rect_moments(top, 0, far, most, limit=1 << 22)
    assert most.row.cpu().tolist() == [[8] * 4, [8 * ((1 << 22) - 1)] * 4, [8 * ((1 << 22) - 1) ** 2] * 4]
    # ... and the columns' side the same with the rows it meets: n_a of the state counts, not the tile alone
    tall = MomentState(1 << 20, 8)
    with pytest.raises(_lib.DctfpError, match='does not fit the 64 bits'):
        rect_moments(tile, 0, 0, tall, limit=(1 << 22) + 1)
    rect_moments(top, 0, 0, tall, limit=1 << 22)
    assert tall.col.cpu().tolist() == [[4] * 8, [4 * ((1 << 22) - 1)] * 8, [4 * ((1 << 22) - 1) ** 2] * 8]
    # an empty tile: nothing launched, nothing written -- as by every refusal above
    for empty in (tile[:0], tile[:, :0]):
        rect_moments(empty, 0, 0, state)
    similarity._launch(dev, name, tile.data_ptr(), 0, 8, 8, 0, 0, None, None, LIMIT, LIMIT, *arrays)
    assert not state.row.any().item() and not state.col.any().item()


# ---- 4. ProteinSearch.search(zscore=True) against the rule

def _load(path):
    with np.load(path) as data:
        return [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']


def _ragged(seed, n, width=480, families=9, bare=4, dups=3, tag='p'):
    """(sid, idx, fps): ``n`` proteins of 1 .. 4 fingerprints around family centres, ``bare`` of them without any and ``dups``
    exact copies of others."""
    rng = np.random.default_rng(seed)
    centre = np.random.default_rng(99).integers(-60, 61, size=(families, width))      # (the same families in every file)
    prots = [np.clip(centre[int(rng.integers(0, families))] + rng.integers(-25, 26, size=(int(rng.integers(1, 5)), width)), -127, 127).astype(np.int8)
             for _ in range(n)]
    for k in rng.choice(n, size=bare, replace=False).tolist():
        prots[k] = np.zeros((0, width), dtype=np.int8)
    full = [k for k in range(n) if len(prots[k])]
    for k in rng.choice(full, size=dups, replace=False).tolist():
        prots[k] = prots[full[0] if k != full[0] else full[1]].copy()
    idx = np.concatenate([[0], np.cumsum([len(p) for p in prots])]).astype(np.int64)
    return [f'{tag}{k:03d}' for k in range(n)], idx, np.concatenate(prots)


_FILES = {}


def _pair(name):
    """(query file, database file, {score: protein L1 matrix}) of a named case, computed once and left unchanged."""
    if name not in _FILES:
        if name == 'golden':
            q, db = _load(GOLD_Q), _load(GOLD_DB)
        elif name == 'g6pd':
            q = db = _load(G6PD)
        elif name == 'ragged':
            q, db = _ragged(5, 41, tag='q'), _ragged(6, 67, tag='d')
        elif name == 'one':                                             # a database of one protein: n < 2 for every query
            q, db = _ragged(5, 41, tag='q'), _ragged(8, 1, bare=0, dups=0, tag='d')
        dist = rrule.row_l1(q[2], db[2])
        _FILES[name] = (q, db, {s: rrule.protein_l1(q[2], q[1], db[2], db[1], s, dist) for s in ('domain', 'global')})
    return _FILES[name]


@pytest.fixture
def small_tiles(monkeypatch):
    """Several database groups, query chunks and tiles even for these small files."""
    from dctdomain_amd import dct_sim
    monkeypatch.setattr(dct_sim.ProteinSearch, 'COL_ROWS', 40)
    monkeypatch.setattr(dct_sim.ProteinSearch, 'TILE_INTS', 300)
    monkeypatch.setattr(dct_sim.ProteinSearch, 'MAX_TILE_ROWS', 9)
    return dct_sim


def _same_z(got, want):
    """A float64 array against the rule's list: NaN exactly where the rule has None, the same float elsewhere."""
    assert got.dtype == np.float64 and len(got) == len(want)
    assert [None if v != v else v for v in got.tolist()] == want


@pytest.mark.parametrize('rank', ['global', 'domain'])
@pytest.mark.parametrize('name', ['golden', 'ragged', 'one'])
def test_search_with_zscore_against_the_rule(small_tiles, name, rank):
    (_, qidx, qfps), (_, db_idx, db_fps), l1 = _pair(name)
    job = small_tiles.ProteinSearch(db_fps, db_idx)
    assert len(job.groups) > 1 or name == 'one'
    undefined = printed = 0
    for top, threshold, domains in ((5, 0.25, False), (3, 0.6, True), (0, 0.5, False)):
        plain = job.search(qfps, qidx, top, threshold, rank=rank, domains=domains)
        got = job.search(qfps, qidx, top, threshold, rank=rank, domains=domains, zscore=True)
        want = zr.search_z(l1[rank], [hit[0] for hit in plain])
        assert len(got) == len(plain) == len(qidx) - 1
        for q, (with_z, without) in enumerate(zip(got, plain)):
            assert len(with_z) == len(without) + 1 == (6 if domains else 4)
            assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(with_z, without))   # every other array: identical
            _same_z(with_z[-1], want[q])
            # the hit's L1 under the ranking score is the rule's
            pairs = [(b, d) for b, d in zip(without[0].tolist(), without[1 if rank == 'domain' else 2].tolist()) if l1[rank][q, b] != zr.NONE]
            assert all(l1[rank][q, b] == d for b, d in pairs)
            undefined += sum(v is None for v in want[q])
            printed += len(want[q])
    total = sum(len(w) for w in zr.search_z(l1[rank], [hit[0] for hit in job.search(qfps, qidx, 5, 0.25, rank=rank)]))
    if name == 'golden':
        assert undefined == 0 and total > 100                            # (no protein without fingerprints, 197 to compare with)
    elif name == 'ragged':
        assert 0 < undefined                                             # (queries without fingerprints, and hits on such proteins)
    else:
        assert undefined == printed >= 41 * 2                            # (the one protein, for top 5 and top 3: nothing to compare it with)
    # the keyword left out: today's tuples
    assert all(len(hit) == 3 for hit in job.search(qfps, qidx, 5, 0.25, rank=rank))


def test_search_of_an_empty_side_with_zscore(small_tiles):
    (_, qidx, qfps), (_, db_idx, db_fps), _ = _pair('ragged')
    none = small_tiles.ProteinSearch(db_fps[:0], db_idx[:1]).search(qfps, qidx, 5, 0.25, zscore=True)
    assert len(none) == 41 and all(len(hit) == 4 and hit[-1].dtype == np.float64 and len(hit[-1]) == 0 for hit in none)
    assert small_tiles.ProteinSearch(db_fps, db_idx).search(qfps[:0], qidx[:1], 5, 0.25, zscore=True) == []


def test_the_background_of_every_query_is_the_whole_database(small_tiles):
    """The moments themselves, both ranks: rows of the protein L1 matrix, proteins without fingerprints left out on either side."""
    (_, qidx, qfps), (_, db_idx, db_fps), l1 = _pair('ragged')
    job = small_tiles.ProteinSearch(db_fps, db_idx)
    for rank in ('global', 'domain'):
        state = small_tiles.MomentState(len(qidx) - 1, 0, cols=False)
        for t0, p0, tile, flags in job.tiles(qfps, qidx, rank):
            small_tiles.rect_moments(tile, t0, p0, state, *flags, limit=job.moment_limit())
        assert small_tiles._moment_ints(state.moments()[0]) == zr.backgrounds(l1[rank])[0]
    assert job.moment_limit() == LIMIT and sum(n == 0 for n, _, _ in zr.backgrounds(l1['global'])[0]) == 4


# ---- 5. the text

def _write_npz(path, side):
    sid, idx, fps = side
    np.savez(path, sid=np.asarray(sid), idx=idx, dct=fps)
    return str(path)


def _lines(path):
    with open(path) as fh:
        return fh.read().splitlines()


@pytest.mark.parametrize('rank', ['global', 'domain'])
@pytest.mark.parametrize('name', ['golden', 'g6pd', 'ragged'])
def test_db_search_lines_are_the_flagless_lines_plus_one_field(tmp_path, small_tiles, name, rank):
    q, db, l1 = _pair(name)
    pq, pdb = _write_npz(tmp_path / 'q-dct.npz', q), _write_npz(tmp_path / 'db-dct.npz', db)
    out = str(tmp_path / 'out.txt')
    where_q, where_db = ({s: k for k, s in enumerate(side[0])} for side in (q, db))
    rows = zr.backgrounds(l1[rank])[0]
    for domains in (False, True):
        small_tiles.db_search(pq, pdb, 5, 0.25, out, rank=rank, domains=domains)
        plain = _lines(out)
        small_tiles.db_search(pq, pdb, 5, 0.25, out, rank=rank, domains=domains, zscore=True)
        with_z = _lines(out)
        assert plain[0] == rrule.HEADER + (' dom1 dom2' if domains else '') and with_z[0] == plain[0] + f' z-{rank}'
        assert len(with_z) == len(plain) > 20
        fields, exact = [], []
        for a, b in zip(with_z[1:], plain[1:]):
            head, z = a.rsplit(' ', 1)
            assert head == b
            i, j = where_q[b.split()[0]], where_db[b.split()[1]]
            exact.append(zr.zscore(*rows[i], l1[rank][i, j]))
            assert z == zr.text(exact[-1])
            fields.append(z)
        assert ('-' in fields) == (name == 'ragged') and any(z not in ('-', '0.00') for z in fields)
        # --min-z: a filter on those lines, nothing else
        values = sorted(float(z) for z in fields if z != '-')
        for min_z in (values[len(values) // 2], -100.0, 100.0):
            small_tiles.db_search(pq, pdb, 5, 0.25, out, rank=rank, domains=domains, min_z=min_z)
            kept = [a for a, z in zip(with_z[1:], exact) if z is not None and z >= min_z]
            assert _lines(out) == [with_z[0]] + kept
            assert (min_z != 100.0 or not kept) and (min_z != -100.0 or len(kept) == len(fields) - fields.count('-'))


@pytest.mark.parametrize('score', ['domain', 'global'])
@pytest.mark.parametrize('name', ['golden', 'ragged'])
def test_rbh_lines_are_the_flagless_lines_plus_two_fields(tmp_path, monkeypatch, name, score):
    from dctdomain_amd import dct_sim
    monkeypatch.setattr(dct_sim.ReciprocalBest, 'COL_ROWS', 40)
    monkeypatch.setattr(dct_sim.ReciprocalBest, 'TILE_INTS', 300)
    q, db, l1 = _pair(name)
    pq, pdb = _write_npz(tmp_path / 'q-dct.npz', q), _write_npz(tmp_path / 'db-dct.npz', db)
    out = str(tmp_path / 'out.txt')
    where_q, where_db = ({s: k for k, s in enumerate(side[0])} for side in (q, db))
    rows, cols = zr.backgrounds(l1[score])
    for domains in (False, True):
        dct_sim.rbh_sim(pq, pdb, out, score=score, domains=domains)
        plain = _lines(out)
        dct_sim.rbh_sim(pq, pdb, out, score=score, domains=domains, zscore=True)
        with_z = _lines(out)
        assert with_z[0] == plain[0] + ' z-query z-db' and len(with_z) == len(plain) > 3
        both = []
        for a, b in zip(with_z[1:], plain[1:]):
            head, z_a, z_b = a.rsplit(' ', 2)
            i, j = where_q[b.split()[0]], where_db[b.split()[1]]
            assert head == b and z_a == zr.text(zr.zscore(*rows[i], l1[score][i, j])) and z_b == zr.text(zr.zscore(*cols[j], l1[score][i, j]))
            both.append((zr.zscore(*rows[i], l1[score][i, j]), zr.zscore(*cols[j], l1[score][i, j])))
        assert any(z_a != z_b for z_a, z_b in both)                      # (the column side is another background)
        min_z = sorted(min(pair) for pair in both)[len(both) // 2]
        dct_sim.rbh_sim(pq, pdb, out, score=score, domains=domains, min_z=min_z)
        assert _lines(out) == [with_z[0]] + [a for a, pair in zip(with_z[1:], both) if min(pair) >= min_z]
    # pairs() is what it was
    job, ref = dct_sim.ReciprocalBest(*q, *db, score=score).with_zscore(), dct_sim.ReciprocalBest(*q, *db, score=score)
    assert all(np.array_equal(a, b) for a, b in zip(job.pairs(), ref.pairs()))
    with pytest.raises(ValueError):
        ref.zscores([0], [0], [0])
    with pytest.raises(ValueError):
        ref.with_zscore()                                                # (its pass has been made)


def test_main_prints_the_z_columns_and_nothing_else_changes(tmp_path):
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')

    def run(*argv):
        dct_sim.main(['--dct', GOLD_Q, '--db', GOLD_DB, '--output', out] + list(argv))
        return _lines(out)

    plain = run()
    assert plain[1:] == rrule.reference_lines()                          # (the reference's own lines, as before)
    with_z = run('--zscore')
    assert with_z[0] == rrule.HEADER + ' z-global' and [a.rsplit(' ', 1)[0] for a in with_z[1:]] == plain[1:]
    z = [float(a.rsplit(' ', 1)[1]) for a in with_z[1:]]
    min_z = sorted(z)[len(z) // 2] + 0.005                               # (between two printed values: the text decides as the exact z does)
    assert run('--min-z', repr(min_z)) == [with_z[0]] + [a for a, v in zip(with_z[1:], z) if v >= min_z] and 0 < sum(v >= min_z for v in z) < len(z)
    dom = run('--rank', 'domain', '--domains', '--zscore')
    assert dom[0] == rrule.HEADER + ' dom1 dom2 z-domain' and all(len(a.split()) == 7 for a in dom[1:])
    assert [a.rsplit(' ', 1)[0] for a in dom[1:]] == run('--rank', 'domain', '--domains')[1:]
    rbh = run('--rbh', 'global', '--zscore')
    assert rbh[0] == rrule.HEADER + ' z-query z-db' and [a.rsplit(' ', 2)[0] for a in rbh[1:]] == rrule.reference_rbh_lines()[1]
    # the example of the reference against itself: every protein's first hit is itself, the closest of its background
    own = dct_sim.main(['--dct', EXAMPLE, '--db', EXAMPLE, '--output', out, '--top', '1', '--threshold', '2', '--zscore'])
    lines = _lines(out)[1:]
    assert own is None and len(lines) == 8 and all(a.split()[0] == a.split()[1] and float(a.split()[4]) > 0 for a in lines)
