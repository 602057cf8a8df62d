"""dct-sim --cluster --level domain (dct_sim.DomainClusters; dctfp_rows_link) against the numpy oracle of domain_cluster_rule.py
(pinned on the CPU in test_domain_cluster_host.py): the kernel on prefixes of a reference fixture, the three fixtures end to end,
a synthetic file with planted families whose same-protein exclusion crosses a block edge, independence from stripes and groups,
the three widths of the dispatch, a skip array, the state of the forest afterwards, the projection to the protein clusters and
the error codes."""

import os

import numpy as np
import pytest

import cluster_rule as crule
import domain_cluster_rule as drule
import golden_util as gu

pytestmark = pytest.mark.gpu
FIXTURES = {'G6PD': os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz'), 'example': os.path.join(gu.GOLD, 'ref_fixtures', 'example-dct.npz'),
            'all': os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')}
EXAMPLE_DOM = os.path.join(gu.GOLD, 'ref_fixtures', 'example.dom')
BOUND = 8500                                                  # sim_bound(0.5)


def _load(path):
    with np.load(path) as data:
        return [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']


def _forest(n):
    import torch
    return torch.arange(n, dtype=torch.int32, device='cuda')


def _link(fps, owner, bound, skip=None, n_nodes=None, a0=0, parent=None, cap=17000):
    """One rows_link call of all rows against themselves; returns the forest."""
    import torch
    from dctdomain_amd.similarity import rows_link
    n = len(fps) if n_nodes is None else n_nodes
    parent = _forest(n) if parent is None else parent
    dev = torch.as_tensor(np.ascontiguousarray(fps), device='cuda')
    rows_link(dev, a0, dev, a0, torch.as_tensor(np.asarray(owner, dtype=np.int32), device='cuda'), parent, bound, skip, cap=cap)
    return parent


def _np_labels(fps, owner, bound, skip=None, cap=17000):
    """The components of rows_link's edges, in numpy."""
    l1 = drule.row_l1(fps)
    owner = np.asarray(owner)
    n = len(fps)
    keep = np.ones(n, dtype=bool) if skip is None else ~np.asarray(skip, dtype=bool)
    ok = (np.minimum(l1, cap) <= bound) & (owner[:, None] != owner[None, :]) & keep[:, None] & keep[None, :] & np.triu(np.ones((n, n), dtype=bool), 1)
    return crule.components(n, *np.nonzero(ok)), int(ok.sum())


def _check_forest(parent, want):
    """Labels equal the oracle's; parent[x] <= x; cluster_labels twice gives the same; further link_pairs on the forest work."""
    import torch
    from dctdomain_amd.similarity import cluster_labels, link_pairs
    n = parent.numel()
    assert np.array_equal(cluster_labels(parent).cpu().numpy(), want)
    p = parent.cpu().numpy()
    assert (p <= np.arange(n)).all() and (p >= 0).all()
    assert np.array_equal(crule.components(n, np.arange(n), p), want)      # (parent is a forest of the same components)
    assert np.array_equal(cluster_labels(parent).cpu().numpy(), want)
    roots = np.unique(want)
    if len(roots) > 1:
        a, b = int(roots[-1]), int(roots[0])
        link_pairs(torch.tensor([a], dtype=torch.int32, device='cuda'), torch.tensor([b], dtype=torch.int32, device='cuda'), parent)
        more = want.copy()
        more[want == a] = b
        assert np.array_equal(cluster_labels(parent).cpu().numpy(), more)
        assert (parent.cpu().numpy() <= np.arange(n)).all()


# ---- 1. the kernel against the rule on prefixes of a fixture

@pytest.fixture(scope='module')
def files():
    return {name: _load(path) for name, path in FIXTURES.items()}


@pytest.mark.parametrize('rows', [1, 2, 127, 128, 129, 257, 323])
def test_rows_link_against_the_rule(files, rows):
    _, idx, dct = files['all']
    assert int(idx[-1]) == 323
    idx = np.concatenate([idx[idx < rows], [rows]])            # the proteins of the first `rows` rows, the last one cut short
    want = drule.labels(dct[:rows], idx, 0.5)
    assert rows < 100 or 1 < len(np.unique(want)) < rows
    parent = _link(dct[:rows], drule.owners(idx), BOUND)
    _check_forest(parent, want)


# ---- 2. the three fixtures end to end

def _run(path, out, cut, *more) -> bytes:
    from dctdomain_amd import dct_sim
    dct_sim.main(['--dct', path, '--output', out, '--cluster', '--level', 'domain', '--min-domain', str(cut)] + list(more))
    with open(out, 'rb') as fh:
        return fh.read()


def _synthetic_dom(path, sid, idx):
    """A .dom file that names all but the last row of every protein of several rows (that one prints ``whole``)."""
    with open(path, 'w', encoding='utf8') as fh:
        for name, k in zip(sid, np.diff(idx).tolist()):
            names = [f'{30 * j + 1}-{30 * j + 30}' for j in range(max(1, k - 1))]
            fh.write(f'{name} {len(names)} {";".join(names)}\n')
    return path


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_fixtures_end_to_end(files, tmp_path, name):
    from dctdomain_amd import dct_sim
    sid, idx, dct = files[name]
    out = str(tmp_path / 'out.txt')
    by_index = dct_sim.fingerprint_labels(sid, idx)
    dom = EXAMPLE_DOM if name == 'example' else _synthetic_dom(str(tmp_path / 'x.dom'), sid, idx)
    by_dom = dct_sim.fingerprint_labels(sid, idx, dct_sim.read_dom_file(dom))
    assert 'whole' in by_dom and by_dom != by_index
    for cut in (0.5, 0.8):
        want = drule.labels(dct, idx, cut)
        kept = drule.labels(dct, idx, cut, whole=False)
        assert _run(FIXTURES[name], out, cut) == drule.HEADER + drule.text(sid, idx, want, by_index)
        assert _run(FIXTURES[name], out, cut, '--no-whole') == drule.HEADER + drule.text(sid, idx, kept, by_index)
        assert _run(FIXTURES[name], out, cut, '--dom', dom) == drule.HEADER + drule.text(sid, idx, want, by_dom)
        assert _run(FIXTURES[name], out, cut, '--dom', dom, '--no-whole') == drule.HEADER + drule.text(sid, idx, kept, by_dom)
    if name == 'G6PD':
        text = _run(FIXTURES[name], out, 0.5)
        lines = text.split(b'\n')[1:-1]
        assert len(lines) == 221 and len({(ln.split()[0], ln.split()[2]) for ln in lines}) == 67


def test_stdout_keeps_its_closing_lines(files, capfd):
    from dctdomain_amd import dct_sim
    sid, idx, dct = files['example']
    want = drule.text(sid, idx, drule.labels(dct, idx, 0.5), dct_sim.fingerprint_labels(sid, idx)).decode('utf8').split('\n')[:-1]
    dct_sim.main(['--dct', FIXTURES['example'], '--cluster', '--level', 'domain', '--min-domain', '0.5'])
    got = capfd.readouterr().out.split('\n')
    assert got[0] == '#representative member dom1 dom2' and got[1].startswith('dct loaded for 8 sequences')
    assert got[2:2 + len(want)] == want and got[2 + len(want)].startswith('total time used ')


# ---- 3. planted families, the same-protein exclusion across a block edge, the bound exactly

def _planted(d=480, seed=3):
    """About 600 rows: proteins of 0, 1, 2 and 7 rows and one of 150 (rows 10 .. 159: it crosses the 128-row block edge).  Half of the
    rows are a family's base row within +-3 per coordinate (L1 <= 1 440 of each other), the others random in [-60, 60] (L1 near
    19 000 of everything); the rows of the long protein are of ONE family each half -- the first 75 of a family no other protein
    has, so that only the owner rule keeps them apart, the others of a family shared with other proteins; two rows of one protein
    are identical; and single rows sit at exactly BOUND and BOUND + 1 of a lonely row of another protein."""
    rng = np.random.default_rng(seed)
    counts = [0, 1, 2, 7, 150]
    while sum(counts) < 600:
        counts.append(int(rng.choice([0, 1, 2, 7])))
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(idx[-1])
    fam = rng.integers(-60, 61, size=(13, d))
    member = rng.integers(0, 12, size=total)
    member[rng.random(total) < 0.5] = -1
    member[10:85], member[85:160] = 12, 0
    twin = int(idx[3]) + 2                                      # inside the protein of 7 rows
    member[twin:twin + 2] = -1
    dct = np.where(member[:, None] >= 0, fam[np.maximum(member, 0)] + rng.integers(-3, 4, size=(total, d)), rng.integers(-60, 61, size=(total, d)))
    lonely = np.flatnonzero(member < 0)
    lonely = lonely[lonely >= 200]
    u1, y, u2, z = lonely[0], lonely[20], lonely[40], lonely[60]
    step = np.zeros(d, dtype=np.int64)
    step[:170] = 50                                             # 170 x 50 = 8 500
    dct[y] = dct[u1] + step
    step[170] = 1
    dct[z] = dct[u2] + step
    dct[twin + 1] = dct[twin]
    sid = [f'p{k}' if k % 5 else f'é{k}' for k in range(len(counts))]
    return sid, idx, dct.astype(np.int8), (u1, y, u2, z, twin)


@pytest.fixture(scope='module')
def planted():
    sid, idx, dct, marks = _planted()
    return sid, idx, dct, marks, drule.labels(dct, idx, 0.5), drule.labels(dct, idx, 0.5, whole=False)


def test_planted_families(planted):
    from dctdomain_amd import dct_sim
    sid, idx, dct, (u1, y, u2, z, twin), want, kept = planted
    own = drule.owners(idx)
    l1 = drule.row_l1(dct)
    assert {0, 1, 2, 7, 150} == set(np.diff(idx).tolist()) and 600 <= int(idx[-1]) < 620
    assert (l1[u1, y], l1[u2, z]) == (BOUND, BOUND + 1) and own[u1] != own[y] and own[u2] != own[z]
    assert want[y] == want[u1] and want[z] != want[u2]                     # the bound exactly: at it joined, one above it not
    assert l1[twin, twin + 1] == 0 and own[twin] == own[twin + 1] and want[twin] != want[twin + 1]
    long_rows = np.arange(10, 160)
    assert (own[long_rows] == own[10]).all() and max(l1[10:85, 10:85].max(), l1[85:160, 85:160].max()) <= BOUND
    assert len(np.unique(want[10:85])) == 75                               # rows of one protein, all within the bound, stay apart
    assert len(np.unique(want[85:160])) == 1 and (want == want[85]).sum() > 75        # ... unless rows of other proteins join them
    assert 100 < len(np.unique(want)) < 500
    got = dct_sim.DomainClusters(sid, idx, dct, 0.5).labels()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(dct_sim.DomainClusters(sid, idx, dct, 0.5, whole=False).labels(), kept)
    assert (kept < 0).sum() == (np.diff(idx) > 1).sum() and not np.array_equal(kept[kept >= 0], want[kept >= 0])


@pytest.mark.parametrize('stripe,group', [(100, 130), (300, 130), (130, 100), (1, 600), (1 << 20, 1 << 22)])
def test_labels_do_not_depend_on_stripes_or_groups(planted, monkeypatch, stripe, group):
    """a0 / b0 offsets that are no multiples of the block, groups that start inside a stripe, blocks left of the diagonal (a
    stripe of more than 128 rows), a file that does not stay on the device."""
    from dctdomain_amd import dct_sim, similarity
    sid, idx, dct, _, want, kept = planted
    monkeypatch.setattr(dct_sim.DomainClusters, 'STRIPE_ROWS', stripe)
    monkeypatch.setattr(dct_sim.DomainClusters, 'COL_ROWS', group)
    calls = []
    real = similarity.rows_link
    monkeypatch.setattr(dct_sim, 'rows_link', lambda a, a0, b, b0, *rest, **kw: (calls.append((a0, a.shape[0], b0, b.shape[0])), real(a, a0, b, b0, *rest, **kw))[1])
    if stripe == 1:
        idx, dct, want, kept = idx[:20], dct[:idx[19]], drule.labels(dct[:idx[19]], idx[:20], 0.5), None   # (a launch per row: a short file)
        sid = sid[:19]
    assert np.array_equal(dct_sim.DomainClusters(sid, idx, dct, 0.5).labels(), want)
    total = int(idx[-1])
    assert all(a0 <= b0 and a0 + na <= total and b0 + nb <= total and na <= stripe and nb <= group for a0, na, b0, nb in calls)
    assert len(calls) == sum(len(range(s0, total, group)) for s0 in range(0, total, stripe))
    if kept is not None:
        assert np.array_equal(dct_sim.DomainClusters(sid, idx, dct, 0.5, whole=False).labels(), kept)


# ---- 4. the three widths of the dispatch, the skip array, the cap

@pytest.mark.parametrize('d', [480, 36, 37, 1, 16, 500])
def test_widths_and_a_skip_array_given_directly(d):
    """d = 480: rows on 16-byte boundaries; 36: on 4-byte ones; 37: on none; every int8 value, -128 included."""
    rng = np.random.default_rng(d)
    n = 300
    fps = rng.integers(-128, 128, size=(n, d)).astype(np.int8)
    fps[rng.integers(0, n, size=60)] = fps[rng.integers(0, n, size=60)]            # exact copies
    near = rng.integers(0, n, size=(60, 2))
    fps[near[:, 0]] = np.clip(fps[near[:, 1]].astype(np.int64) + rng.integers(-1, 2, size=(60, d)), -128, 127)
    owner = np.sort(rng.integers(0, 80, size=n))
    l1 = drule.row_l1(fps)
    bound = int(np.quantile(l1[np.triu_indices(n, 1)], 0.004))
    skip = rng.random(n) < 0.2
    seen = []
    for flags in (None, skip):
        want, edges = _np_labels(fps, owner, bound, flags, cap=1 << 30)
        seen.append(edges)
        _check_forest(_link(fps, owner, bound, flags, cap=1 << 30), want)
    assert 400 > seen[0] > seen[1] > 20
    # the cap: min(L1, cap) <= bound with bound = cap joins every pair of different owners
    assert np.array_equal(_np_labels(fps, owner, 40, None, cap=40)[0], _np_labels(fps, owner, 1 << 30)[0])
    import torch
    from dctdomain_amd.similarity import cluster_labels, rows_link
    dev, parent = torch.as_tensor(fps, device='cuda'), _forest(n)
    rows_link(dev, 0, dev, 0, torch.as_tensor(owner.astype(np.int32), device='cuda'), parent, 40, cap=40)
    assert np.array_equal(cluster_labels(parent).cpu().numpy(), _np_labels(fps, owner, 40, None, cap=40)[0])


@pytest.mark.parametrize('ld', [496, 492, 489])
def test_rows_wider_than_the_fingerprints(ld):
    """Row strides above the width, straight through the C ABI: the bytes behind a fingerprint are not its own (here: as far apart
    as bytes get between a row and its near copy), and the 16-byte arm ends on a narrow round (487 = 30 x 16 + 7)."""
    import ctypes as C
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.similarity import cluster_labels
    rng = np.random.default_rng(ld)
    n, d = 200, 487
    wide = rng.integers(-128, 128, size=(n, ld)).astype(np.int8)
    wide[100:, :d] = np.clip(wide[:100, :d].astype(np.int64) + rng.integers(-1, 2, size=(100, d)), -128, 127)
    wide[:100, d:], wide[100:, d:] = -128, 127
    owner = np.arange(n) // 2
    dev, own, parent = torch.as_tensor(wide, device='cuda'), torch.as_tensor(owner.astype(np.int32), device='cuda'), _forest(n)
    ctx = _lib.get_context(0)
    _lib.check(ctx._lib.dctfp_rows_link(ctx.handle, dev.data_ptr(), n, ld, 0, dev.data_ptr(), n, ld, 0, d, own.data_ptr(), None, 17000, d, parent.data_ptr(),
                                        n, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    want, edges = _np_labels(wide[:, :d], owner, d)
    assert edges == 100 and _np_labels(wide, owner, d)[1] == 0              # (the padding read as data would join nothing)
    assert np.array_equal(cluster_labels(parent).cpu().numpy(), want)


def test_one_non_empty_protein_stays_apart_at_the_full_bound():
    from dctdomain_amd import dct_sim
    fps = np.zeros((5, 480), dtype=np.int8)
    got = dct_sim.DomainClusters(['a', 'b', 'c'], [0, 0, 5, 5], fps, 0.0).labels()
    assert got.tolist() == [0, 1, 2, 3, 4]
    got = dct_sim.DomainClusters(['a', 'b', 'c'], [0, 2, 2, 5], fps, 0.0).labels()
    assert got.tolist() == [0, 0, 0, 0, 0]                                  # (two proteins: every row of one joins every row of the other)


def test_links_go_on_in_a_forest_that_other_calls_share():
    """Nodes beyond the rows (n_nodes > a0 + na), an offset a0, and rows_link after link_pairs on one forest."""
    import torch
    from dctdomain_amd.similarity import link_pairs
    rng = np.random.default_rng(8)
    fps = rng.integers(-60, 61, size=(150, 480)).astype(np.int8)
    fps[100:] = np.clip(fps[:50].astype(np.int64) + rng.integers(-2, 3, size=(50, 480)), -127, 127)      # row 100 + k is a copy of row k
    owner = np.arange(7, 157) // 3
    n, a0 = 200, 7
    full_owner = np.concatenate([np.full(a0, -1), owner, np.full(n - a0 - 150, -1)])
    parent = _forest(n)
    link_pairs(torch.tensor([0, 199], dtype=torch.int32, device='cuda'), torch.tensor([a0, a0 + 100], dtype=torch.int32, device='cuda'), parent)
    _link(fps, full_owner, BOUND, n_nodes=n, a0=a0, parent=parent)
    want = np.arange(n, dtype=np.int32)
    want[a0 + 100:a0 + 150] = np.arange(a0, a0 + 50)
    want[[a0, a0 + 100, 199]] = 0
    _check_forest(parent, want)


# ---- 5. the projection to the protein clusters, on the device

@pytest.mark.parametrize('name', sorted(FIXTURES) + ['planted'])
def test_row_components_project_to_the_protein_clusters(files, planted, name):
    from dctdomain_amd import dct_sim
    sid, idx, dct = files[name] if name != 'planted' else planted[:3]
    for cut in (0.3, 0.5, 0.8):
        rows = dct_sim.DomainClusters(sid, idx, dct, cut).labels()
        assert np.array_equal(drule.project(rows, idx), dct_sim.Clusters(sid, idx, dct, min_domain=cut).labels())


# ---- 6. the error codes

def test_error_codes_surface_as_exceptions_without_a_launch():
    import ctypes as C
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.similarity import cluster_labels, rows_link
    fps = torch.zeros((6, 480), dtype=torch.int8, device='cuda')            # (all equal: any launch would join the owners)
    owner = torch.arange(10, dtype=torch.int32, device='cuda')
    parent = _forest(10)
    for kw in (dict(a0=5), dict(b0=5), dict(a0=-1), dict(bound=-1), dict(cap=-1)):
        args = dict(a0=0, b0=0, bound=100, cap=17000)
        args.update(kw)
        with pytest.raises(_lib.DctfpError) as e:
            rows_link(fps, args['a0'], fps, args['b0'], owner, parent, args['bound'], cap=args['cap'])
        assert e.value.code == _lib.DCTFP_ERR_INVALID and 'dctfp_rows_link' in e.value.msg
    with pytest.raises(ValueError):
        rows_link(fps, 0, fps[:, :479], 0, owner, parent, 100)              # widths differ
    with pytest.raises(ValueError):
        rows_link(fps, 0, fps, 0, owner[:9], parent, 100)
    with pytest.raises(ValueError):
        rows_link(fps, 0, fps, 0, owner, parent.long(), 100)
    with pytest.raises(ValueError):
        rows_link(fps, 0, fps, 0, owner, parent, 100, skip=np.zeros(9, dtype=np.uint8))
    ctx = _lib.get_context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda na=6, lda=480, d=480, n_nodes=10, a=fps.data_ptr(), own=owner.data_ptr(): ctx._lib.dctfp_rows_link(   # noqa: E731
        ctx.handle, a, na, lda, 0, fps.data_ptr(), 6, 480, 0, d, own, None, 17000, 100, parent.data_ptr(), n_nodes, stream)
    assert call(lda=479) == call(d=0) == call(na=-1) == call(n_nodes=5) == call(a=None) == call(own=None) == _lib.DCTFP_ERR_INVALID
    assert call(n_nodes=2 ** 31) == _lib.DCTFP_ERR_LIMIT
    assert call(na=0) == 0
    assert cluster_labels(parent).cpu().tolist() == list(range(10))         # nothing was linked by any of these
    assert call() == 0 and not cluster_labels(parent).cpu().numpy()[:6].any()
