"""python -m dctdomain_amd.cluster_quality on the GPU (similarity.silhouette_rows = dctfp_silhouette_rows; Silhouette; the command)
against the rule of silhouette_rule.py (pinned on scikit-learn in test_silhouette_host.py).  Integer sums and neighbours are compared
for equality, the text byte for byte."""

import os

import numpy as np
import pytest

import golden_util as gu
import make_golden_silhouette as golden
import silhouette_rule as rule

pytestmark = pytest.mark.gpu
CAP = 17000
UNTOUCHED = -7                  # what the result arrays hold before a call: only the entries of the tile's rows may change


def _run(tile, row0, col0, cid, size, first, row_empty=None, col_empty=None, cap=CAP, pass_clusters=4096, ld_extra=0):
    """{global row: (Sa, Sb, |B|, first of B)} of one call on a host tile; ``ld_extra``: the tile as a column view of a wider tensor."""
    import torch
    from dctdomain_amd.similarity import silhouette_rows
    n_rows, n_cols = tile.shape
    n = len(cid)
    store = torch.full((n_rows, n_cols + ld_extra), 1, dtype=torch.int32, device='cuda')       # (1 would count if it were read)
    view = store[:, :n_cols]
    view.copy_(torch.as_tensor(np.ascontiguousarray(tile), device='cuda'))
    out = [torch.full((n,), UNTOUCHED, dtype=dtype, device='cuda') for dtype in (torch.int64, torch.int64, torch.int32, torch.int32)]
    silhouette_rows(view, row0, col0, *(torch.as_tensor(np.asarray(a, dtype=np.int32), device='cuda') for a in (cid, size, first)), *out,
                    row_empty, col_empty, cap=cap, pass_clusters=pass_clusters)
    torch.cuda.synchronize()
    back = [t.cpu().numpy() for t in out]
    other = np.ones(n, dtype=bool)
    other[row0:row0 + n_rows] = False
    assert all((a[other] == UNTOUCHED).all() for a in back)
    return {i: tuple(int(a[i]) for a in back) for i in range(row0, row0 + n_rows)}


def _values(rng, n_rows, n_cols, cap=CAP):
    """L1 values of every kind: 0, 1, cap - 1, cap, above it, 0x7fffffff, negative ones and a few ordinary ones (ties are common)."""
    t = rng.integers(0, 6, size=(n_rows, n_cols)) * 1000
    kind = rng.random((n_rows, n_cols))
    for lo, v in ((0.0, 0), (0.1, 1), (0.15, cap - 1), (0.2, cap), (0.25, cap + 1), (0.3, 0x7fffffff), (0.35, -5), (0.4, -0x80000000)):
        t[(kind >= lo) & (kind < lo + 0.05)] = v
    return t.astype(np.int32)


def _labels(rng, n, clusters, lone=0.2):
    """cid / size / first of n proteins in about ``clusters`` clusters, a share of singletons between them."""
    labels = [int(1000 + i) if rng.random() < lone else int(rng.integers(0, clusters)) for i in range(n)]
    return rule.kernel_arrays(labels)


@pytest.mark.parametrize('n_cols', [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_the_export_on_hand_made_tiles(n_cols):
    rng = np.random.default_rng(n_cols)
    col0, n_rows = 3, min(n_cols, 6)
    n = col0 + n_cols + 4
    cid, size, first = _labels(rng, n, clusters=7)
    for row0 in sorted({col0, col0 + n_cols - n_rows, 0}):           # the diagonal at the start, at the end of the columns, partly outside
        tile = _values(rng, n_rows, n_cols)
        for r in range(n_rows):                                     # the diagonal holds 0, a large value, protein_min's fill: never counted
            if 0 <= row0 + r - col0 < n_cols:
                tile[r, row0 + r - col0] = (0, 16000, 0x7fffffff)[r % 3]
        for flags in ((None, None), (rng.random(n_rows) < 0.3, rng.random(n_cols) < 0.3)):
            want = rule.tile_sums(rule.tile_keys(tile, *flags), row0, col0, cid, size, first)
            for ld_extra in (0, 37):
                assert _run(tile, row0, col0, cid, size, first, *flags, ld_extra=ld_extra) == want, (row0, flags[0] is not None, ld_extra)
    # the diagonal really is inside and really would have counted
    tile = np.full((1, n_cols), 5, dtype=np.int32)
    one = np.zeros(n, dtype=np.int32)
    got = _run(tile, col0, col0, one, [n], [0])
    assert got == {col0: (5 * (n_cols - 1), 0, 0, -1)}
    # another cap: the key is min(L1, cap)
    tile = _values(rng, 2, n_cols)
    assert _run(tile, 0, col0, cid, size, first, cap=999) == rule.tile_sums(rule.tile_keys(tile, cap=999), 0, col0, cid, size, first)


N = 300
LAYOUTS = {
    'one_cluster': lambda: ['a'] * N,
    'all_singletons': lambda: list(range(N)),
    'two_clusters': lambda: ['a' if i % 7 < 3 else 'b' for i in range(N)],
    'giant_and_singletons': lambda: ['g' if i % 3 else i for i in range(N)],
    'interleaved_100x3': lambda: [i % 100 for i in range(N)],
    'contiguous_100x3': lambda: [i // 3 for i in range(N)],
}


@pytest.fixture(scope='module')
def square():
    """300 x 300 values, symmetric, few distinct ones, 5 % of the proteins flagged empty."""
    rng = np.random.default_rng(300)
    t = _values(rng, N, N).astype(np.int64)
    t = np.triu(t, 1)
    t = (t + t.T).astype(np.int32)
    np.fill_diagonal(t, 0x7fffffff)
    empty = rng.random(N) < 0.05
    return t, empty, rule.tile_keys(t, empty, empty)


@pytest.mark.parametrize('layout', sorted(LAYOUTS))
def test_label_layouts(square, layout):
    tile, empty, key = square
    labels = LAYOUTS[layout]()
    arrays = rule.kernel_arrays(labels)
    want = rule.tile_sums(key, 0, 0, *arrays)
    assert _run(tile, 0, 0, *arrays, empty, empty) == want
    if layout == 'one_cluster':
        assert all(v[1:] == (0, 0, -1) for v in want.values())
    if layout == 'all_singletons':
        assert all(v[0] == 0 and v[2] == 1 and v[3] >= 0 for v in want.values()) and len(arrays[1]) == 0
    if layout.endswith('100x3'):
        # a pass length that leaves the last cluster id to a pass of its own
        assert _run(tile, 0, 0, *arrays, empty, empty, pass_clusters=33) == want


def _thirteen():
    """39 proteins in 13 clusters of 3 (protein i in cluster i % 13) and 3 singletons; row r is close to cluster TARGET[r] alone."""
    labels = [i % 13 for i in range(39)] + [100, 101, 102]
    n = len(labels)
    target = {0: 1, 1: 6, 2: 12, 3: 0, 39: 7}                      # row -> the cluster that must come out as its neighbour
    tile = np.full((n, n), 9000, dtype=np.int32)
    for r, c in target.items():
        tile[r, [j for j in range(39) if j % 13 == c]] = 10 + r
    return labels, tile, target


@pytest.mark.parametrize('pass_clusters', [1, 4, 5, 13, 4096])
def test_the_result_does_not_depend_on_the_pass_length(pass_clusters):
    labels, tile, target = _thirteen()
    arrays = rule.kernel_arrays(labels)
    want = rule.tile_sums(rule.tile_keys(tile), 0, 0, *arrays)
    got = _run(tile, 0, 0, *arrays, pass_clusters=pass_clusters)
    assert got == want
    # the neighbour found in the first, a middle and the last pass (and, for a singleton's row, among all clusters)
    for r, c in target.items():
        assert got[r][1:] == (3 * (10 + r), 3, c), (r, c)


@pytest.mark.parametrize('pass_clusters', [1, 2, 4096])
def test_ties_go_to_the_first_member_that_comes_first(pass_clusters):
    # row 0 of cluster {0, 1}: 6 / 2, 9 / 3 and a singleton at 3 / 1 -- equal fractions, different (S, size)
    row = np.zeros((1, 8), dtype=np.int32)
    row[0] = [0, 5, 2, 4, 3, 3, 3, 3]
    for labels, want in ((['a', 'a', 'b', 'b', 'c', 'c', 'c', 'd'], (5, 6, 2, 2)), (['a', 'a', 'c', 'c', 'b', 'b', 'b', 'd'], (5, 6, 2, 2))):
        assert _run(row, 0, 0, *rule.kernel_arrays(labels), pass_clusters=pass_clusters)[0] == want
    row[0] = [0, 5, 3, 3, 3, 2, 4, 3]                               # 9 / 3 first in the file, then 6 / 2
    assert _run(row, 0, 0, *rule.kernel_arrays(['a', 'a', 'b', 'b', 'b', 'c', 'c', 'd']), pass_clusters=pass_clusters)[0] == (5, 9, 3, 2)
    row[0] = [0, 3, 5, 2, 4, 3, 3, 3]                               # the singleton first in the file: it is the neighbour
    assert _run(row, 0, 0, *rule.kernel_arrays(['a', 'd', 'a', 'b', 'b', 'c', 'c', 'c']), pass_clusters=pass_clusters)[0] == (5, 3, 1, 1)
    row[0] = [0, 5, 4, 3, 3, 3, 3, 3]                               # singletons that tie among themselves and with 9 / 3: the lowest index wins
    assert _run(row, 0, 0, *rule.kernel_arrays(['a', 'a', 'x', 'y', 'c', 'c', 'c', 'd']), pass_clusters=pass_clusters)[0] == (5, 3, 1, 3)
    assert _run(row, 0, 0, *rule.kernel_arrays(['a', 'a', 'x', 'y', 'p', 'q', 'r', 's']), pass_clusters=pass_clusters)[0] == (5, 3, 1, 3)


def test_sums_beyond_32_bits():
    n = 300_000
    row = np.full((1, n), 20000, dtype=np.int32)                    # (above the cap: key 17000)
    # one cluster: Sa = 299 999 x 17000 = 5.1e9 > 2^32
    got = _run(row, 0, 0, np.zeros(n, dtype=np.int32), [n], [0])[0]
    assert got == (299_999 * 17000, 0, 0, -1) and got[0] > 1 << 32
    # the same columns as the neighbour cluster, against a pair at 33 999 / 2 -- which is nearer by half a unit
    cid = np.full(n, 2, dtype=np.int32)
    cid[:3], cid[3:5] = 0, 1
    row[0, 3:5] = [17000, 16999]
    arrays = (cid, [3, 2, n - 5], [0, 3, 5])
    assert _run(row, 0, 0, *arrays)[0] == (2 * 17000, 33_999, 2, 3)
    # at 34 000 / 2 the two tie: the pair, first in the file, wins; with the pair behind it the giant does, with its sum above 2^32
    row[0, 3:5] = 17000
    assert _run(row, 0, 0, *arrays)[0] == (2 * 17000, 34_000, 2, 3)
    cid[3:], cid[n - 2:] = 1, 2
    got = _run(row, 0, 0, cid, [3, n - 5, 2], [0, 3, n - 2])[0]
    assert got == (2 * 17000, (n - 5) * 17000, n - 5, 3) and got[1] > 1 << 32
    # ... and a pair one unit nearer beats it from behind
    row[0, n - 1] = 16999
    assert _run(row, 0, 0, cid, [3, n - 5, 2], [0, 3, n - 2])[0] == (2 * 17000, 33_999, 2, n - 2)


def _random_file(rng, n=200, width=480):
    """200 proteins of 0 to 6 fingerprints, some with none; near-duplicates inside 12 planted groups so that keys lie below the cap."""
    counts = rng.integers(0, 7, size=n)
    counts[rng.random(n) < 0.05] = 0
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    centres = rng.integers(-20, 21, size=(12, width))
    group = rng.integers(0, 12, size=n)
    rows = [np.clip(centres[group[p]] + rng.integers(-12, 13, size=(counts[p], width)), -128, 127) for p in range(n)]
    dct = np.concatenate(rows).astype(np.int8) if idx[-1] else np.zeros((0, width), dtype=np.int8)
    sid = np.array([f'q{p:03d}' for p in range(n)])
    labels = [f'lone{p}' if rng.random() < 0.1 else f'c{(group[p] + (rng.random() < 0.2)) % 12}' for p in range(n)]
    return sid, idx, dct, labels


def _files():
    for name in ('G6PD-dct.npz', 'example-dct.npz'):
        with np.load(os.path.join(gu.GOLD, 'ref_fixtures', name)) as data:
            sid, idx, dct = data['sid'], np.asarray(data['idx'], dtype=np.int64), data['dct']
        labels = golden.g6pd()[3] if name.startswith('G6PD') else [k % 3 for k in range(len(sid))]
        yield name, sid, idx, dct, labels, max(2, len(sid) // 3)
    yield ('random',) + _random_file(np.random.default_rng(7)) + (60,)


@pytest.mark.parametrize('case', list(_files()), ids=lambda c: c[0])
def test_silhouette_end_to_end(case):
    from dctdomain_amd.cluster_quality import Silhouette
    _name, sid, idx, dct, labels, rows = case
    n, total = len(sid), int(idx[-1])

    class Striped(Silhouette):      # three stripes of rows and three groups of columns at least
        TILE_INTS = rows * n
        COL_ROWS = max(1, total // 4)
    from dctdomain_amd.dct_sim import _protein_groups
    keys = rule.key_matrices(dct, idx)
    for score in ('domain', 'global'):
        want = rule.sums(keys[score], labels)
        whole, striped = Silhouette(sid, idx, dct, labels, score=score), Striped(sid, idx, dct, labels, score=score)
        assert len(whole._stripes()) == 1 and len(striped._stripes()) >= 3 and len(list(_protein_groups(idx, Striped.COL_ROWS))) >= 3
        for job in (whole, striped):
            got = job.sums()
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), score
            for per in ('protein', 'cluster'):
                out = []
                job.write(out.append, per=per)
                assert b''.join(out) == rule.text(sid, labels, want, per)
        assert np.array_equal(whole.values(), rule.values(want, labels), equal_nan=True)


def test_the_command_on_g6pd_is_the_golden_byte_for_byte(tmp_path, capsys):
    import cluster_rule
    from dctdomain_amd import cluster_quality
    sid, idx, dct, _labels_ = golden.g6pd()
    label, _ = cluster_rule.labels(dct, idx, min_global=0.6)
    clusters = tmp_path / 'clusters.txt'
    clusters.write_bytes(cluster_rule.HEADER + cluster_rule.text(sid, label))
    npz = os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')
    for score in ('global', 'domain'):
        out = tmp_path / f'{score}.txt'
        cluster_quality.main(['--dct', npz, '--clusters', str(clusters), '--score', score, '--out', str(out)])
        with open(os.path.join(golden.OUT, f'G6PD_{score}.txt'), 'rb') as fh:
            assert out.read_bytes() == fh.read()
    cluster_quality.main(['--dct', npz, '--clusters', str(clusters), '--per', 'cluster'])
    printed = capsys.readouterr().out
    assert '#cluster size mean_silhouette min_silhouette negative\nA0A2K6GTL0 13 0.0133 -0.2879 8\n' in printed
    assert printed.endswith('# proteins=27 clusters=4 singletons=1 mean_silhouette=0.2500 negative=8\n')


def test_refusals():
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.similarity import silhouette_rows
    n = 10
    tile = torch.zeros((4, n), dtype=torch.int32, device='cuda')

    def args(**kw):
        a = {'cid': torch.zeros(n, dtype=torch.int32, device='cuda'), 'size': torch.full((1,), n, dtype=torch.int32, device='cuda'),
             'first': torch.zeros(1, dtype=torch.int32, device='cuda'), 'own_sum': torch.zeros(n, dtype=torch.int64, device='cuda'),
             'near_sum': torch.zeros(n, dtype=torch.int64, device='cuda'), 'near_size': torch.zeros(n, dtype=torch.int32, device='cuda'),
             'near_first': torch.zeros(n, dtype=torch.int32, device='cuda')}
        a.update(kw)
        return list(a.values())
    silhouette_rows(tile, 0, 0, *args())                            # (the call the refusals depart from)
    for name in ('cid', 'size', 'first', 'near_size', 'near_first'):
        with pytest.raises(ValueError):
            silhouette_rows(tile, 0, 0, *args(**{name: torch.zeros(n if name not in ('size', 'first') else 1, dtype=torch.int64, device='cuda')}))
    for name in ('own_sum', 'near_sum'):
        with pytest.raises(ValueError):
            silhouette_rows(tile, 0, 0, *args(**{name: torch.zeros(n, dtype=torch.int32, device='cuda')}))
        with pytest.raises(ValueError):
            silhouette_rows(tile, 0, 0, *args(**{name: torch.zeros(n - 1, dtype=torch.int64, device='cuda')}))       # short
        with pytest.raises(ValueError):
            silhouette_rows(tile, 0, 0, *args(**{name: torch.zeros(n, dtype=torch.int64)}))                          # on the host
    with pytest.raises(ValueError):
        silhouette_rows(tile, 0, 0, *args(cid=torch.zeros(n, dtype=torch.int32)))
    with pytest.raises(ValueError):
        silhouette_rows(tile, 0, 0, *args(first=torch.zeros(2, dtype=torch.int32, device='cuda')))
    with pytest.raises(ValueError):
        silhouette_rows(tile, 0, 0, *args(near_first=torch.zeros(2 * n, dtype=torch.int32, device='cuda')[::2]))     # not contiguous
    with pytest.raises(ValueError):
        silhouette_rows(tile.to(torch.int64), 0, 0, *args())
    with pytest.raises(ValueError):
        silhouette_rows(tile, 0, 0, *args(), row_empty=np.zeros(3, dtype=np.uint8))
    for bad in ([0] * 9 + [1], [0] * 9 + [-2]):                     # a cluster id outside n_clusters
        with pytest.raises(IndexError):
            silhouette_rows(tile, 0, 0, *args(cid=torch.tensor(bad, dtype=torch.int32, device='cuda')))
    with pytest.raises(IndexError):
        silhouette_rows(tile, n - 3, 0, *args())                    # rows outside n_nodes
    with pytest.raises(IndexError):
        silhouette_rows(tile, 0, 1, *args())                        # columns outside n_nodes
    with pytest.raises(ValueError):
        silhouette_rows(tile, -1, 0, *args())
    for pass_clusters, code in ((0, _lib.DCTFP_ERR_INVALID), (4097, _lib.DCTFP_ERR_LIMIT)):
        with pytest.raises(_lib.DctfpError) as err:
            silhouette_rows(tile, 0, 0, *args(), pass_clusters=pass_clusters)
        assert err.value.code == code and 'dctfp_silhouette_rows' in err.value.msg
    with pytest.raises(_lib.DctfpError) as err:
        silhouette_rows(tile, 0, 0, *args(), cap=(1 << 22) + 1)
    assert err.value.code == _lib.DCTFP_ERR_LIMIT
    torch.cuda.synchronize()
