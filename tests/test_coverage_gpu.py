"""dct-sim --min-coverage on the GPU (similarity.protein_cover = dctfp_protein_cover; FilteredPairs, Clusters and Representatives with
a coverage; the command line) against the numpy rule of coverage_rule.py (worked by hand in test_coverage_host.py)."""

import os

import numpy as np
import pytest

import all_sim_filter_rule as rule
import coverage_rule as cr
import golden_util as gu

pytestmark = pytest.mark.gpu
G6PD = os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz')
NO_L1 = cr.NO_L1


# ---- 1. protein_cover against numpy on raw inputs

def _primes(n):
    out, k = [], 2
    while len(out) < n:
        if all(k % p for p in out if p * p <= k):
            out.append(k)
        k += 1
    return np.array(out, dtype=np.int64)


def _at_distance(x, dist):
    """A row at exactly L1 ``dist`` of the row ``x`` (values within +-60: nothing clips)."""
    d = len(x)
    y = x.astype(np.int64) + dist // d
    y[:dist % d] += 1
    return y.astype(np.int8)


def _side(rng, counts, d, pool, first_prime):
    """(rows, idx, weights): rows = a base fingerprint of the pool + noise of 0 .. 4 units (an amplitude per row, so that the L1
    of two rows of one base lies on either side of 2.1 d); weights = distinct primes, the last row of a protein of several
    rows weighing the sum of the others -- what coverage_weights hands the kernel."""
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(idx[-1])
    amp = rng.integers(0, 5, size=(total, 1))
    rows = (pool[rng.integers(0, len(pool), size=total)] + rng.integers(-4, 5, size=(total, d)) * amp // 4).astype(np.int8)
    w = _primes(first_prime + total)[first_prime:].copy()
    for lo, hi in zip(idx[:-1], idx[1:]):
        if hi - lo > 1:
            w[hi - 1] = w[lo:hi - 1].sum()
    return rows, idx, w


def _small(rng, n):
    return rng.integers(1, 7, size=n).tolist()


def _shapes():
    rng = np.random.default_rng(5)
    return [
        ('1x1', [1], [1], 480),
        ('97x97', [1] * 97, [1] * 97, 480),                                   # crosses the 96-protein block
        ('rows127', [64, 63], [2, 0, 3, 1, 0], 480),                          # a protein without rows in the middle and at the end
        ('rows128', [64, 64], _small(rng, 30), 480),
        ('rows129', [64, 65], _small(rng, 30), 480),
        ('rows127-129b', _small(rng, 25), [60, 67, 5, 59, 69, 64, 65], 480),
        ('130x40small', [130], _small(rng, 40), 480),
        ('40smallx130', _small(rng, 40), [130], 480),
        ('130+x200+', [2, 130, 3], [200, 1], 480),
        ('130x200', [130], [200], 480),
        ('d20', _small(rng, 50) + [0], [0] + _small(rng, 45), 20),            # rows padded by the wrapper
        ('d20-130x200', [130, 4], [3, 200], 20),
    ]


def _case(name, counts_a, counts_b, d):
    """The inputs of one shape, with exact L1 == bound and L1 == bound + 1 planted between rows that are near nothing else."""
    rng = np.random.default_rng([len(counts_a), len(counts_b), d, sum(counts_a)])
    pool = rng.integers(-50, 51, size=(12, d))
    bound = int(2.1 * d)
    a, ia, wa = _side(rng, counts_a, d, pool, 0)
    b, ib, wb = _side(rng, counts_b, d, pool, len(a))
    if len(a) > 3 and len(b) > 3:
        special = rng.integers(-50, 51, size=(2, d)).astype(np.int8)          # (two rows far from the pool and from each other)
        ra, rb = rng.choice(len(a), 2, replace=False), rng.choice(len(b), 2, replace=False)
        a[ra[0]], b[rb[0]] = special[0], _at_distance(special[0], bound)
        a[ra[1]], b[rb[1]] = special[1], _at_distance(special[1], bound + 1)
    return a, ia, wa, b, ib, wb, bound


def _needs(idx, w, c):
    return cr.need(cr.protein_weights(idx, w), c)


@pytest.fixture(scope='module')
def raw_cases():
    """Per shape: the inputs and the numpy tiles for c = 0.01, 0.5, 1.0 on both sides and 0.5 on the a side only."""
    cases = {}
    for name, counts_a, counts_b, d in _shapes():
        a, ia, wa, b, ib, wb, bound = _case(name, counts_a, counts_b, d)
        dist = cr.row_l1(a, b)
        want = {}
        for c, one_side in ((0.01, False), (0.5, False), (1.0, False), (0.5, True)):
            na, nb = _needs(ia, wa, c), (np.zeros(len(ib) - 1, dtype=np.int64) if one_side else _needs(ib, wb, c))
            want[(c, one_side)] = (na, nb, cr.cover_tile(a, ia, wa, na, b, ib, wb, nb, bound, dist=dist))
        cases[name] = (a, ia, wa, b, ib, wb, bound, want)
    return cases


def test_the_inputs_hold_every_class_of_pair(raw_cases):
    seen = {k: 0 for k in ('whole', 'domains', 'drop_a', 'drop_b', 'drop_both', 'above', 'at_bound', 'past_bound')}
    for a, ia, wa, b, ib, wb, bound, want in raw_cases.values():
        for (c, one_side), (na, nb, t) in want.items():
            if one_side:
                continue
            within = t['min'] <= bound
            kept = t['out'] != NO_L1
            assert not (kept & ~within).any()                   # (a minimum above the bound: no row is matched)
            seen['whole'] += int((kept & t['whole']).sum())
            seen['domains'] += int((kept & ~t['whole']).sum())
            seen['drop_a'] += int((within & ~t['ok_a'] & t['ok_b']).sum())
            seen['drop_b'] += int((within & t['ok_a'] & ~t['ok_b']).sum())
            seen['drop_both'] += int((within & ~t['ok_a'] & ~t['ok_b']).sum())
            seen['above'] += int(((t['min'] > bound) & (t['min'] != NO_L1)).sum())
        near = t['dist'].min(axis=1) if t['dist'].size else np.zeros(0)
        seen['at_bound'] += int((near == bound).sum())
        seen['past_bound'] += int((near == bound + 1).sum())
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize('name', [s[0] for s in _shapes()])
def test_protein_cover_against_numpy(raw_cases, name):
    import torch
    from dctdomain_amd.similarity import protein_cover, protein_min
    a, ia, wa, b, ib, wb, bound, want = raw_cases[name]
    dev = torch.device('cuda', torch.cuda.current_device())
    ta, tb = torch.as_tensor(a, device=dev), torch.as_tensor(b, device=dev)
    npa, npb = len(ia) - 1, len(ib) - 1
    for (c, one_side), (na, nb, t) in want.items():
        got = protein_cover(ta, ia, wa, na, tb, ib, wb, nb, bound)
        assert got.dtype == torch.int32 and tuple(got.shape) == (npa, npb)
        assert np.array_equal(got.cpu().numpy().astype(np.int64), t['out']), (name, c, one_side)
    # into a column range of a wider tensor: nothing else is written
    wide = torch.full((npa, npb + 7), -3, dtype=torch.int32, device=dev)
    na, nb, t = want[(0.5, False)]
    protein_cover(ta, ia, wa, na, tb, ib, wb, nb, bound, out=wide[:, 3:3 + npb])
    host = wide.cpu().numpy().astype(np.int64)
    assert np.array_equal(host[:, 3:3 + npb], t['out']) and (host[:, :3] == -3).all() and (host[:, 3 + npb:] == -3).all()
    # no requirement on either side: protein_min, byte for byte
    zero_a, zero_b = np.zeros(npa, dtype=np.int64), np.zeros(npb, dtype=np.int64)
    plain = protein_min(ta, ia, tb, ib)
    assert torch.equal(protein_cover(ta, ia, wa, zero_a, tb, ib, wb, zero_b, bound), plain)
    assert np.array_equal(plain.cpu().numpy().astype(np.int64), t['min'])
    # a bound that matches every row keeps every pair that has rows; one below 0 keeps none that asks for anything
    assert torch.equal(protein_cover(ta, ia, wa, na, tb, ib, wb, nb, 17000), plain)
    none = protein_cover(ta, ia, wa, na, tb, ib, wb, nb, -1).cpu().numpy()
    assert np.array_equal(none != NO_L1, (t['min'] != NO_L1) & (na[:, None] == 0) & (nb[None, :] == 0))


def test_protein_cover_refuses_wide_rows_and_wrong_vectors():
    import torch
    from dctdomain_amd.similarity import protein_cover
    dev = torch.device('cuda', torch.cuda.current_device())
    rows = torch.zeros((2, 528), dtype=torch.int8, device=dev)
    with pytest.raises(ValueError, match='512'):
        protein_cover(rows, [0, 2], [1, 1], [1], rows, [0, 2], [1, 1], [1], 100)
    rows = rows[:, :480].contiguous()
    with pytest.raises(ValueError, match='w_a'):
        protein_cover(rows, [0, 2], [1], [1], rows, [0, 2], [1, 1], [1], 100)
    with pytest.raises(ValueError, match='need_b'):
        protein_cover(rows, [0, 2], [1, 1], [1], rows, [0, 2], [1, 1], [1, 1], 100)
    empty = protein_cover(rows, [0, 0, 2], [1, 1], [0, 1], rows[:0], [0, 0], [], [0], 100)
    assert empty.cpu().numpy().tolist() == [[NO_L1], [NO_L1]]


# ---- 2. the three consumers on a planted file

D = 160
CUT = 0.98              # bound 340: two rows of one family lie on either side of it
GLOBAL = 0.9


@pytest.fixture(scope='module')
def planted():
    """About 300 proteins: 1 - 6 domains each from 20 families (a row = the family's base + noise of 0 .. 4 units), a protein of
    several domains followed by its whole-protein row (the mean of its domains' bases + noise: one architecture, one whole row),
    some proteins without rows; residue names with a discontinuous one here and there."""
    rng = np.random.default_rng(11)
    fam = rng.integers(-50, 51, size=(20, D))
    archs = [rng.integers(0, 20, size=int(k)) for k in rng.integers(1, 7, size=40)]
    rows, names, counts = [], [], []

    def noisy(base):
        amp = int(rng.integers(0, 5))
        return np.clip(base + rng.integers(-4, 5, size=D) * amp // 4, -127, 127)

    for p in range(300):
        if rng.random() < 0.04:
            counts.append(0)
            continue
        arch = archs[int(rng.integers(0, len(archs)))]
        if rng.random() < 0.3:                                 # a part of the architecture: shares domains, not the whole row
            arch = arch[:max(1, int(rng.integers(1, len(arch) + 1)))]
        start = 1
        for f in arch:
            length = int(rng.integers(30, 200))
            rows.append(noisy(fam[f]))
            if length > 60 and rng.random() < 0.2:
                names.append(f'{start}-{start + 19},{start + 40}-{start + length - 1}')
            else:
                names.append(f'{start}-{start + length - 1}')
            start += length
        if len(arch) > 1:
            rows.append(noisy(np.round(fam[arch].mean(axis=0)).astype(np.int64)))
            names.append(f'1-{start - 1}')
        counts.append(len(arch) + (len(arch) > 1))
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    dct = np.array(rows, dtype=np.int8)
    sid = np.array([f'p{k}' for k in range(len(counts))])
    return sid, idx, dct, names, cr.row_l1(dct, dct)


_COMBOS = [(c, unit, g) for c in (0.5, 1.0) for unit in ('residues', 'domains') for g in (None, GLOBAL)]


@pytest.fixture(scope='module')
def planted_rule(planted):
    sid, idx, dct, names, dist = planted
    out = {}
    for c, unit, g in _COMBOS:
        w = cr.weights(idx, names, unit)
        out[(c, unit, g)] = (w,) + cr.edges(dct, idx, w, CUT, c, g, dist=dist)
    return out


def test_the_planted_file_separates_the_cut_offs(planted, planted_rule):
    sid, idx, dct, names, dist = planted
    n = len(sid)
    i, j = np.triu_indices(n, 1)
    kept = {k: int(v[5].sum()) for k, v in planted_rule.items()}
    _, _, mn, last, _ = planted_rule[(0.5, 'domains', None)][1:]
    plain = int(rule.kept(mn, last, CUT, None).sum())
    assert (np.diff(idx) == 0).any() and (np.diff(idx) > 1).any() and (np.diff(idx) == 1).any()
    assert plain > kept[(0.5, 'domains', None)] > kept[(1.0, 'domains', None)] > 0, (plain, kept)
    assert kept[(0.5, 'domains', None)] > kept[(0.5, 'domains', GLOBAL)] > 0 and kept[(0.5, 'residues', None)] > kept[(0.5, 'residues', GLOBAL)]
    assert kept[(0.5, 'residues', None)] != kept[(0.5, 'domains', None)]


def _jobs(dct_sim, small: bool):
    kinds = (dct_sim.FilteredPairs, dct_sim.Clusters, dct_sim.Representatives)
    if not small:
        return kinds
    return tuple(type('Small' + k.__name__, (k,), {'TILE_INTS': 20000, 'COL_ROWS': 400, 'TEXT_BYTES': 1 << 14}) for k in kinds)


@pytest.mark.parametrize('small', [False, True], ids=['one-stripe', 'stripes-and-groups'])
@pytest.mark.parametrize('c,unit,g', _COMBOS)
def test_pairs_clusters_and_representatives_follow_the_rule(planted, planted_rule, c, unit, g, small):
    from dctdomain_amd import dct_sim
    sid, idx, dct, names, _ = planted
    n = len(sid)
    w, i, j, mn, last, keep = planted_rule[(c, unit, g)]
    assert np.array_equal(dct_sim.coverage_weights(sid, idx, names, unit), w)
    pairs, clusters, reps = _jobs(dct_sim, small)
    job = pairs(sid, idx, dct, min_domain=CUT, min_global=g, min_coverage=c, weights=w)
    if small:
        assert len(list(job.stripes())) > 2 and int(idx[-1]) > 2 * job.COL_ROWS
    gi, gj, gmn, glast = job.pairs()
    assert np.array_equal(gi, i[keep]) and np.array_equal(gj, j[keep])
    assert np.array_equal(gmn, mn[keep]) and np.array_equal(glast, last[keep])
    got = clusters(sid, idx, dct, min_domain=CUT, min_global=g).with_coverage(c, w).labels()
    assert np.array_equal(got, cr.components(n, i, j, keep))
    got = reps(sid, idx, dct, min_domain=CUT, min_global=g).with_coverage(c, w).labels()
    assert np.array_equal(got, cr.greedy(n, i, j, keep))


# ---- 3. the command line on the reference fixture

def _main(tmp_path, *argv) -> bytes:
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    dct_sim.main(['--dct', G6PD, '--output', out] + list(argv))
    with open(out, 'rb') as fh:
        return fh.read()


@pytest.fixture(scope='module')
def g6pd_rule():
    with np.load(G6PD) as data:
        sid, idx, dct, dom = data['sid'], data['idx'], data['dct'], data['dom']
    out = {'sid': sid, 'idx': idx, 'dct': dct}
    for unit in ('residues', 'domains'):
        out[unit] = cr.edges(dct, idx, cr.weights(idx, dom, unit), 0.5, 0.8)
    return out


@pytest.mark.parametrize('more', [[], ['--domains'], ['--cov-unit', 'domains']], ids=['plain', 'domains', 'unit-domains'])
def test_cli_prints_the_lines_of_the_cut_off_that_the_rule_keeps(tmp_path, g6pd_rule, more):
    i, j, mn, last, keep = g6pd_rule['domains' if '--cov-unit' in more else 'residues']
    within = rule.kept(mn, last, 0.5, None)
    base = [x for x in more if x == '--domains']
    lines = _main(tmp_path, '--min-domain', '0.5', *base).split(b'\n')[:-1]
    assert len(lines) == 1 + int(within.sum()) == 352
    want = rule.filtered_text(lines, keep[within])
    assert _main(tmp_path, '--min-domain', '0.5', '--min-coverage', '0.8', *more) == want
    assert want.count(b'\n') == 1 + 109


def test_cli_clusters_and_representatives(tmp_path, g6pd_rule):
    import cluster_rule
    sid, idx = [str(s) for s in g6pd_rule['sid']], g6pd_rule['idx']
    i, j, mn, last, keep = g6pd_rule['residues']
    single = cr.components(len(sid), i, j, keep)
    assert len(set(single.tolist())) == 4
    assert _main(tmp_path, '--cluster', '--min-domain', '0.5', '--min-coverage', '0.8') == cluster_rule.HEADER + cluster_rule.text(sid, single)
    greedy = cr.greedy(len(sid), i, j, keep)
    reps_out = str(tmp_path / 'reps-dct.npz')
    text = _main(tmp_path, '--cluster', '--linkage', 'greedy', '--min-domain', '0.5', '--min-coverage', '0.8', '--reps-out', reps_out)
    assert text == cluster_rule.HEADER + cluster_rule.text(sid, greedy)
    chosen = np.flatnonzero(greedy == np.arange(len(sid)))
    with np.load(reps_out) as data:
        assert [str(s) for s in data['sid']] == [sid[k] for k in chosen]
        assert np.array_equal(data['dct'], np.concatenate([g6pd_rule['dct'][idx[k]:idx[k + 1]] for k in chosen]))
        assert np.array_equal(np.diff(data['idx']), np.diff(idx)[chosen]) and len(data['dom']) == len(data['dct'])
    # --dom gives the residues beside --cluster (here: the names the npz carries, written out as a .dom file)
    with np.load(G6PD) as data:
        dom = data['dom']
    path = str(tmp_path / 'g6pd.dom')
    with open(path, 'w', encoding='utf8') as fh:
        for k, name in enumerate(sid):
            fh.write(f'{name} {idx[k + 1] - idx[k]} {";".join(dom[idx[k]:idx[k + 1]])}\n')
    assert _main(tmp_path, '--cluster', '--min-domain', '0.5', '--min-coverage', '0.8', '--dom', path) == cluster_rule.HEADER + cluster_rule.text(sid, single)
