"""``ProteinSearch.tiles``, the one walk over the rectangle A x database under ``search`` (both ranks) and ``ReciprocalBest.best`` (both
scores), against rbh_rule.protein_l1 (brute-force numpy): at tiny class constants the tiles cover the rectangle once and hold the
oracle's blocks; a database without any fingerprint still gives ``search`` its tiles and ``ReciprocalBest`` none; and the last rows
of A go to the device once for a global-rank search."""

import numpy as np
import pytest

import rbh_rule as rrule

pytestmark = pytest.mark.gpu
N_A, N_B = 37, 53
ROUTES = ('global', 'domain')

_CASES = {}


def _case(width):
    """((idx, fps) of A, the same of B, {route: the oracle's (37, 53) L1}) of a width, computed once."""
    if width not in _CASES:
        rng = np.random.default_rng(5)
        ia, ib = (np.concatenate([[0], np.cumsum(rng.integers(0, 5, n))]).astype(np.int64) for n in (N_A, N_B))
        a, b = (rng.integers(-128, 128, (int(i[-1]), width), dtype=np.int8) for i in (ia, ib))
        assert (int(ia[-1]), int(ib[-1])) == (68, 94) and ((np.diff(ia) == 0).sum(), (np.diff(ib) == 0).sum()) == (10, 13)
        dist = rrule.row_l1(a, b)
        _CASES[width] = ((ia, a), (ib, b), {r: rrule.protein_l1(a, ia, b, ib, r, dist) for r in ROUTES})
    return _CASES[width]


def _bare_b(width=480):
    """A database of five proteins without any fingerprint."""
    return np.zeros(6, dtype=np.int64), np.zeros((0, width), dtype=np.int8)


@pytest.fixture
def tiny(monkeypatch):
    from dctdomain_amd import dct_sim
    monkeypatch.setattr(dct_sim.ProteinSearch, 'COL_ROWS', 16)
    monkeypatch.setattr(dct_sim.ProteinSearch, 'TILE_INTS', 60)
    return dct_sim


def _walk(job, a, ia, route, n_b, **kw):
    """([(t0, t1, p0, p1, tile, row flags, column flags)] on the host, how often each protein pair was covered)."""
    out, count = [], np.zeros((len(ia) - 1, n_b), dtype=np.int64)
    for t0, p0, tile, (row_empty, col_empty) in job.tiles(a, ia, route, **kw):
        assert tile.device.type == 'cuda' and str(tile.dtype) == 'torch.int32' and tile.dim() == 2
        t1, p1 = t0 + tile.shape[0], p0 + tile.shape[1]
        count[t0:t1, p0:p1] += 1
        out.append((t0, t1, p0, p1, tile.cpu().numpy(), np.asarray(row_empty), np.asarray(col_empty)))
    return out, count


@pytest.mark.parametrize('width', [480, 100])
@pytest.mark.parametrize('route', ROUTES)
def test_the_tiles_cover_the_rectangle_once_and_hold_the_oracle(tiny, route, width):
    (ia, a), (ib, b), want = _case(width)
    job = tiny.ProteinSearch(b, ib)
    tiles, count = _walk(job, a, ia, route, N_B)
    assert count.shape == (N_A, N_B) and (count == 1).all()
    # the geometry the constants are there for: several database groups (the last of one protein), several chunks of A, several
    # tiles per chunk (domain) or group (global)
    chunks = list(tiny._protein_groups(ia, 16))
    assert len(job.groups) > 1 and job.groups[-1] == (N_B - 1, N_B) and len(chunks) > 1
    assert sorted({(p0, p1) for _, _, p0, p1, *_ in tiles}) == job.groups
    if route == 'domain':
        per_chunk = [sum(1 for t0, _, p0, *_ in tiles if c0 <= t0 < c1 and p0 == 0) for c0, c1 in chunks]
        assert max(per_chunk) > 1 and all(any(c0 <= t0 and t1 <= c1 for c0, c1 in chunks) for t0, t1, *_ in tiles)
    else:
        per_group = [sum(1 for _, _, p0, *_ in tiles if p0 == g0) for g0, _ in job.groups]
        assert max(per_group) > 1
    empty_a, empty_b = np.diff(ia) == 0, np.diff(ib) == 0
    for t0, t1, p0, p1, tile, row_empty, col_empty in tiles:
        assert np.array_equal(row_empty.astype(bool), empty_a[t0:t1]) and np.array_equal(col_empty.astype(bool), empty_b[p0:p1])
        block = want[route][t0:t1, p0:p1]
        if route == 'domain':
            assert np.array_equal(tile, block)                  # (0x7fffffff included)
        else:
            full = ~empty_a[t0:t1, None] & ~empty_b[None, p0:p1]
            assert np.array_equal(tile[full], block[full])
    assert (want['domain'][empty_a] == 0x7fffffff).all() and (want['domain'][:, empty_b] == 0x7fffffff).all()


def test_a_database_without_fingerprints(tiny):
    (ia, a), _, _ = _case(480)
    ib, b = _bare_b()
    job = tiny.ProteinSearch(b, ib)
    for route in ROUTES:                                        # search's setting: tiles that cover the rectangle
        tiles, count = _walk(job, a, ia, route, 5)
        assert (count == 1).all() and all(col_empty.all() for *_, col_empty in tiles)
        assert route == 'global' or all((tile == 0x7fffffff).all() for _, _, _, _, tile, _, _ in tiles)
    assert _walk(job, a, ia, 'domain', 5, bare=False)[0] == []  # ReciprocalBest's: nothing
    for rank in ROUTES:
        hits = tiny.ProteinSearch(b, ib).search(a, ia, top=2, threshold=0.25, rank=rank)
        assert len(hits) == N_A and all(cols.tolist() == [0, 1] for cols, _, _ in hits)      # (the first top, whatever they score)
    sid_a, sid_b = [f'a{k}' for k in range(N_A)], [f'b{k}' for k in range(5)]
    for score in ROUTES:
        assert all(len(v) == 0 for v in tiny.ReciprocalBest(sid_a, ia, a, sid_b, ib, b, score=score).pairs())


def test_a_global_search_uploads_the_last_rows_of_the_queries_once(monkeypatch):
    from dctdomain_amd import dct_sim
    (ia, a), (ib, b), want = _case(480)
    monkeypatch.setattr(dct_sim.ProteinSearch, 'COL_ROWS', 40)  # (above 37: the last rows of A stay on the device)
    monkeypatch.setattr(dct_sim.ProteinSearch, 'TILE_INTS', 60)
    last_a, _ = dct_sim._last_rows(a, ia)
    uploads, first_args = [], []
    real_up, real_l1 = dct_sim.to_device_int8, dct_sim.l1_matrix

    def up(x):
        if isinstance(x, np.ndarray) and x.shape == last_a.shape and np.array_equal(x, last_a):
            uploads.append(x)
        return real_up(x)

    def l1(x, y, *args, **kw):
        first_args.append(x)
        return real_l1(x, y, *args, **kw)

    monkeypatch.setattr(dct_sim, 'to_device_int8', up)
    monkeypatch.setattr(dct_sim, 'l1_matrix', l1)
    job = dct_sim.ProteinSearch(b, ib)
    assert len(job.groups) > 1 and all(p1 - p0 != N_A for p0, p1 in job.groups)      # (no group's last rows look like A's)
    hits = job.search(a, ia, top=1, threshold=2.0, rank='global')
    assert len(first_args) > 2 * len(job.groups)               # (several tiles per group)
    assert len(uploads) == 1 and all(not isinstance(x, np.ndarray) and x.device.type == 'cuda' for x in first_args)
    keys = np.minimum(want['global'], 17000)
    keys[np.diff(ia) == 0] = 17000
    keys[:, np.diff(ib) == 0] = 17000
    assert [int(cols[0]) for cols, _, _ in hits] == keys.argmin(axis=1).tolist()      # (ties to the lower index, as argmin)
