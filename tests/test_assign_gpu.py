"""dct-sim --assign (dct_sim.Assignment; dctfp_rows_assign) against numpy and the plain-Python oracle of assign_rule.py (worked by
hand on the CPU in test_assign_host.py): the kernel on planted rows at every alignment, empty sides and limits, random ragged
files end to end, independence from the split into groups and stripes, the split and chain properties through the command line,
and planted families.  Every assertion is exact integer or byte equality."""

import ctypes as C
import os

import numpy as np
import pytest

import all_sim_filter_rule as rule
import assign_rule as arule
import golden_util as gu
import greedy_rule as grule
from test_assign_host import split_oracle

pytestmark = pytest.mark.gpu
NPZ = os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')
NONE = 0x7fffffff
CAP = 17000


# ---- 1. the kernel against numpy

def _l1_at(row, target):
    """A copy of an int8 row moved to L1 exactly ``target`` from it (coordinate by coordinate, towards the farther end)."""
    out = row.astype(np.int64).copy()
    left = int(target)
    for k in range(len(out)):
        up, down = 127 - out[k], out[k] + 128
        step = min(left, max(up, down))
        out[k] += step if up >= down else -step
        left -= step
    assert left == 0
    return out.astype(np.int8)


def _rows(na, nb, d, bound, rng):
    """Uniform int8 rows (L1 between two of them ~ 85 d: above the cap at d = 480 / 475), near copies (+-10), identical rows, and
    where d allows it (255 d > bound) a pair at L1 exactly ``bound`` and one at ``bound + 1``.  Returns (a, b, planted)."""
    a = rng.integers(-128, 128, size=(na, d)).astype(np.int8)
    b = rng.integers(-128, 128, size=(nb, d)).astype(np.int8)
    for c in rng.choice(nb, size=max(1, nb // 3), replace=False):               # near copies: survivors at 8500 and 17000
        b[c] = np.clip(a[rng.integers(0, na)].astype(np.int64) + rng.integers(-10, 11, size=d), -128, 127)
    planted = {}
    b[nb - 1] = a[na - 1]                                                       # identical: the last row of each set
    planted['same'] = (na - 1, nb - 1)
    if nb >= 3 and 127 * d >= bound + 1:
        r = int(rng.integers(0, na))
        b[0], b[1] = _l1_at(a[r], bound), _l1_at(a[r], bound + 1)
        planted['at'], planted['above'] = (r, 0), (r, 1)
    return a, b, planted


def _view(t, d, arm):
    """The rows of ``t`` as a device view at 16-byte alignment, at 4-byte alignment, or at a 1-byte offset with odd ld."""
    import torch
    n = t.shape[0]
    ld, off = {16: ((d + 15) // 16 * 16, 0), 4: ((d + 3) // 4 * 4 + (4 if ((d + 3) // 4 * 4 + 4) % 16 else 8), 4), 1: (d + 1 + d % 2, 1)}[arm]
    buf = torch.zeros(256 + off + n * ld, dtype=torch.int8, device='cuda')
    view = torch.as_strided(buf, (n, d), (ld, 1), off)
    view.copy_(torch.as_tensor(t, device='cuda'))
    bits = view.data_ptr() | ld
    assert {16: bits % 16 == 0, 4: bits % 4 == 0 and bits % 16 != 0, 1: bits % 2 == 1 and ld % 2 == 1}[arm] and ld >= d
    return view


def _want(dist, bound, value, slot, start):
    """assign = the minimum, over the row pairs within the bound, of the value -- slots outside it and negative values ignored."""
    want = start.copy()
    r, c = np.nonzero(np.minimum(dist, CAP) <= bound)
    ok = (slot[c] >= 0) & (slot[c] < len(want)) & (value[r] >= 0)
    np.minimum.at(want, slot[c][ok], value[r][ok])
    return want


@pytest.mark.parametrize('bound', [0, 8500, 17000])
@pytest.mark.parametrize('d', [480, 475, 7])
@pytest.mark.parametrize('na,nb', [(1, 1), (127, 129), (128, 128), (129, 257), (300, 1)])
def test_kernel_against_numpy(na, nb, d, bound):
    import torch
    from dctdomain_amd.similarity import rows_assign
    rng = np.random.default_rng(100000 * na + 100 * nb + d + bound)
    a, b, planted = _rows(na, nb, d, bound, rng)
    dist = np.abs(a.astype(np.int64)[:, None, :] - b.astype(np.int64)[None, :, :]).sum(axis=2)
    assert dist[planted['same']] == 0
    if 'at' in planted:
        assert dist[planted['at']] == bound and dist[planted['above']] == bound + 1
    else:
        assert nb < 3 or 127 * d < bound + 1                  # (d = 7: no L1 reaches 8500; every pair survives there)
    if d >= 475 and na * nb >= 4:
        assert dist.max() > CAP                               # the cap matters at bound = 17000: such a pair survives there
        assert na * nb < 4 or (np.minimum(dist, CAP) > bound).any() or bound == CAP
    # maps: several rows share a slot, values not monotone in the row, one slot out of range, one negative value
    n_assign = nb // 3 + 4
    slot = (np.arange(nb) // 3 + 1).astype(np.int32)
    value = rng.permutation(na).astype(np.int32) + 5
    start = np.where(rng.random(n_assign) < 0.3, rng.integers(0, 8, size=n_assign), NONE).astype(np.int32)      # some lower values already there
    if nb > 1:
        slot[nb - 1] = n_assign + 7                           # (the identical pair's column: out of range, ignored)
    if nb > 4:
        slot[2] = -1
    if na > 1:
        value[na - 1] = -3                                    # (the identical pair's row: negative, ignored)
    want = _want(dist, bound, value.astype(np.int64), slot.astype(np.int64), start)
    # NULL maps: value = a0 + r, slot = b0 + c; assign shorter than b0 + nb when there is more than one column
    a0, b0 = 1000, 3
    n_plain = b0 + nb - (1 if nb > 1 else 0)
    start_plain = np.where(rng.random(n_plain) < 0.3, a0 + rng.integers(0, max(1, na // 2), size=n_plain), NONE).astype(np.int32)
    want_plain = _want(dist, bound, a0 + np.arange(na), b0 + np.arange(nb), start_plain)
    dev = lambda x: torch.as_tensor(x, device='cuda')         # noqa: E731
    for arm in (16, 4, 1):
        va, vb = _view(a, d, arm), _view(b, d, arm)
        assign = dev(start)
        rows_assign(va, vb, assign, bound, dev(value), dev(slot))
        assert np.array_equal(assign.cpu().numpy(), want), arm
        rows_assign(va, vb, assign, bound, dev(value), dev(slot))                # (a second launch changes nothing)
        assert np.array_equal(assign.cpu().numpy(), want), arm
        assign = dev(start_plain)
        rows_assign(va, vb, assign, bound, a0=a0, b0=b0)
        assert np.array_equal(assign.cpu().numpy(), want_plain), arm
    assert (want[start != NONE] <= start[start != NONE]).all()                   # (what was lower stayed)
    # the result does not depend on how the rows are split into calls
    if na > 100 and nb > 100:
        assign = dev(start)
        for r0, r1 in ((0, 50), (50, na)):
            for c0, c1 in ((0, nb - 70), (nb - 70, nb)):
                rows_assign(va[r0:r1], vb[c0:c1], assign, bound, dev(value[r0:r1]), dev(slot[c0:c1]))
        assert np.array_equal(assign.cpu().numpy(), want)


def test_empty_sides_limits_and_bad_arguments():
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.similarity import rows_assign
    fps = torch.zeros((6, 480), dtype=torch.int8, device='cuda')
    assign = torch.full((10,), NONE, dtype=torch.int32, device='cuda')
    ctx = _lib.get_context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda na=6, nb=6, lda=480, d=480, bound=0, cap=CAP, n_assign=10, a=fps.data_ptr(), out=assign.data_ptr(), a0=0: \
        ctx._lib.dctfp_rows_assign(ctx.handle, a, na, lda, None, a0, fps.data_ptr(), nb, 480, None, 0, d, cap, bound, out, n_assign, stream)   # noqa: E731
    # empty: succeeds and changes nothing
    assert call(na=0) == 0 and call(nb=0) == 0 and call(n_assign=0) == 0
    # the row limit of the 2-D grid: refused before any launch (nothing is read from the six rows there are)
    assert call(na=65535 * 128 + 1) == _lib.DCTFP_ERR_LIMIT and b'8M rows' in ctx._lib.dctfp_last_error()
    assert call(n_assign=2 ** 31) == _lib.DCTFP_ERR_LIMIT
    for bad in (dict(na=-1), dict(nb=-1), dict(lda=479), dict(d=0), dict(bound=-1), dict(cap=-1), dict(n_assign=-1), dict(a=None), dict(out=None),
                dict(a0=-1)):
        assert call(**bad) == _lib.DCTFP_ERR_INVALID, bad
    torch.cuda.synchronize()
    assert (assign.cpu().numpy() == NONE).all()               # nothing was touched by any of these
    rows_assign(fps[:0], fps, assign, 0)
    rows_assign(fps, fps[:0], assign, 0)
    assert (assign.cpu().numpy() == NONE).all()
    with pytest.raises(ValueError):
        rows_assign(fps, fps[:, :479], assign, 0)             # widths differ
    with pytest.raises(ValueError):
        rows_assign(fps, fps, assign.long(), 0)
    with pytest.raises(ValueError):
        rows_assign(fps, fps, assign, 0, value_a=assign[:5])  # one value per row
    with pytest.raises(_lib.DctfpError) as e:
        rows_assign(fps, fps, assign, -1)
    assert e.value.code == _lib.DCTFP_ERR_INVALID and 'dctfp_rows_assign' in e.value.msg
    rows_assign(fps, fps, assign, 0)                          # six identical rows: slot c gets row 0
    assert assign.cpu().tolist() == [0] * 6 + [NONE] * 4


# ---- 2. end to end against assign_rule, on random ragged files

_ALPHABET = list('abcdefghijklmnopqrstuvwxyz0123456789_|.-') + ['é', 'ß', 'α', '蛋', '😀']


def _ragged(seed, n, tag):
    """Proteins of 0-6 fingerprints (15 % empty) from four families at L1 ~ 6 500 (0.62) within a family, plus planted near
    copies (+-2) of single fingerprints at random places of other proteins (test_greedy_gpu's generator, more rows)."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 7, size=n)
    counts[rng.random(n) < 0.15] = 0
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(idx[-1])
    fam = np.random.default_rng(99).integers(-60, 61, size=(4, 480))             # (the same families in every file)
    dct = np.clip(fam[rng.integers(0, 4, size=total)] + rng.integers(-20, 21, size=(total, 480)), -127, 127).astype(np.int8)
    for _ in range(n // 4 if total else 0):
        a, b = rng.integers(0, total, size=2)
        dct[b] = np.clip(dct[a].astype(np.int64) + rng.integers(-2, 3, size=480), -127, 127)
    names = [tag + ''.join(rng.choice(_ALPHABET, size=int(m))) + f'{k}' for k, m in enumerate(rng.choice([1, 5, 17, 40, 333], size=n))]
    return names, idx, dct


SHAPES = [(40, 60), (1, 150), (150, 1), (0, 30), (30, 0)]
# per shape, cut-offs at which between 10 % and 90 % of the new proteins are covered by a representative of R (asserted
# below from the oracle's labels) -- where that can be: with no representative nothing is covered, and one new protein is
# covered or not
E2E_CUTS = {'domain': {'min_domain': 0.62}, 'global': {'min_global': 0.62}, 'both': {'min_domain': 0.63, 'min_global': 0.6}}
ONE_REP_CUTS = {'domain': {'min_domain': 0.62}, 'global': {'min_global': 0.6}, 'both': {'min_domain': 0.61, 'min_global': 0.6}}   # (m = 1)
SEEDS = {('r', 1): 1025, ('n', 1): 2002}                      # (a lone protein that has fingerprints)
_files = {}


def _cuts(m, cut):
    return (ONE_REP_CUTS if m == 1 else E2E_CUTS)[cut]


def _case(m, n):
    """(R, N, pair_values) of a shape, made once."""
    if (m, n) not in _files:
        rep, new = _ragged(SEEDS.get(('r', m), 1000 + m), m, 'r'), _ragged(SEEDS.get(('n', n), 2000 + n), n, 'n')
        _files[m, n] = rep, new, arule.pair_values(rep[2], rep[1], new[2], new[1])
    return _files[m, n]


def _oracle(m, n, kw):
    rep, new, values = _case(m, n)
    i, j = arule.edges(rep[2], rep[1], new[2], new[1], values=values, **kw)
    return arule.assign(m, n, i, j), i, j


@pytest.mark.parametrize('cut', list(E2E_CUTS))
@pytest.mark.parametrize('m,n', SHAPES)
def test_end_to_end_against_the_rule(tmp_path, m, n, cut):
    from dctdomain_amd import dct_sim
    kw = _cuts(m, cut)
    rep, new, _ = _case(m, n)
    want, i, j = _oracle(m, n, kw)
    arule.check(m, n, i, j, want)
    covered = int((want < m).sum())
    print(f'm={m} n={n} {cut}: {covered} of {n} new proteins covered, {len(np.unique(want))} clusters')
    if m >= 1 and n >= 10:
        assert 0.1 * n <= covered <= 0.9 * n
    for idx in (rep[1], new[1]):
        assert len(idx) < 31 or (np.diff(idx) == 0).any()     # (proteins without fingerprints on either side)
    job = dct_sim.Assignment(*rep, *new, **kw)
    got = job.labels()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(job.labels(), want)                 # (twice: the same)
    paths = [str(tmp_path / name) for name in ('r-dct.npz', 'n-dct.npz', 'out.txt')]
    for path, (sid, idx, dct) in zip(paths, (rep, new)):
        np.savez(path, sid=np.array(sid, dtype=str), idx=idx, dct=dct.reshape(-1, 480))
    argv = ['--dct', paths[1], '--assign', paths[0], '--output', paths[2]] + [x for k, v in kw.items() for x in ('--' + k.replace('_', '-'), str(v))]
    dct_sim.main(argv)
    assert open(paths[2], 'rb').read() == arule.HEADER + arule.text(rep[0], new[0], want)


# ---- 3. independence from the split

@pytest.mark.parametrize('cut', list(E2E_CUTS))
def test_labels_do_not_depend_on_groups_stripes_or_tiles(monkeypatch, cut):
    from dctdomain_amd import dct_sim
    kw = E2E_CUTS[cut]
    rep, new, _ = _case(40, 60)
    want, _, _ = _oracle(40, 60, kw)
    whole = dct_sim.Assignment(*rep, *new, **kw)
    assert np.array_equal(whole.labels(), want) and whole.calls == 1
    seen = set()
    for col_rows, stripe_rows, tile_ints in [(10, 15, 150), (1, 16, 60), (7, 3, 1), (11, 17, 300)]:
        for name, v in (('COL_ROWS', col_rows), ('STRIPE_ROWS', stripe_rows), ('TILE_INTS', tile_ints)):
            monkeypatch.setattr(dct_sim.Assignment, name, v)
        job = dct_sim.Assignment(*rep, *new, **kw)
        assert np.array_equal(job.labels(), want), (col_rows, stripe_rows, tile_ints)
        seen.add(job.calls)
        assert job.calls >= 9                                 # at least 3 groups x 3 stripes (34 / 51 last rows on the DCTglobal route)
    assert len(seen) > 1


# ---- 4. the split and chain properties, through the command line

def _cli(*argv, **kw):
    from dctdomain_amd import dct_sim
    dct_sim.main(list(argv) + [x for k, v in kw.items() for x in ('--' + k.replace('_', '-'), str(v))])


def _npz(path):
    with np.load(path) as data:
        return [str(s) for s in data['sid']], np.asarray(data['idx']), data['dct'], (data['dom'].tolist() if 'dom' in data.files else None)


@pytest.mark.parametrize('kw', [{'min_domain': 0.5}, {'min_global': 0.5}, {'min_domain': 0.25, 'min_global': 0.1}, {'min_domain': 0.62, 'min_global': 0.6}],
                         ids=['domain', 'global', 'both', 'both-ragged-range'])
@pytest.mark.parametrize('which', ['golden', 'ragged'])
def test_split_and_chain_properties_through_the_command_line(tmp_path, which, kw):
    """greedy --reps-out R0 on the first k proteins, then --assign R0 --reps-out R1 on the rest: the rest get the labels of one
    greedy run over the whole file (greedy_rule alone), and R1 holds exactly that run's representatives."""
    if which == 'golden':
        with np.load(NPZ) as data:
            sid, idx, dct = [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']
    else:
        sid, idx, dct = _ragged(31, 120, 'f')
    n = len(sid)
    k = n // 3
    dom = np.array([f'{r}-{r + 7}' for r in range(int(idx[-1]))])
    first, rest, full, r0, r1, rall, out = (str(tmp_path / name) for name in ('first-dct.npz', 'rest-dct.npz', 'full-dct.npz', 'r0-dct.npz',
                                                                                 'r1-dct.npz', 'rall-dct.npz', 'out.txt'))
    np.savez(first, sid=np.array(sid[:k]), idx=idx[:k + 1], dom=dom[:idx[k]], dct=dct[:idx[k]])
    np.savez(rest, sid=np.array(sid[k:]), idx=idx[k:] - idx[k], dom=dom[idx[k]:], dct=dct[idx[k]:])
    np.savez(full, sid=np.array(sid), idx=idx, dom=dom, dct=dct)
    reps, want, _ = split_oracle(rule.triangle_l1(dct, idx), n, k, kw)
    _cli('--dct', first, '--cluster', '--linkage', 'greedy', '--reps-out', r0, '--output', out, **kw)
    assert _npz(r0)[0] == [sid[p] for p in reps]
    _cli('--dct', rest, '--assign', r0, '--reps-out', r1, '--output', out, **kw)
    assert open(out, 'rb').read() == arule.HEADER + arule.text([sid[p] for p in reps], sid[k:], want)
    _cli('--dct', full, '--cluster', '--linkage', 'greedy', '--reps-out', rall, '--output', out, **kw)
    got, whole = _npz(r1), _npz(rall)
    assert got[0] == whole[0] and np.array_equal(got[1], whole[1]) and np.array_equal(got[2], whole[2]) and got[3] == whole[3] and got[3]
    labels = grule.labels(dct, idx, **kw)[0]
    all_reps = np.flatnonzero(labels == np.arange(n))
    assert got[0] == [sid[p] for p in all_reps] and 1 < len(all_reps) < n
    assert np.array_equal(got[2], np.concatenate([dct[idx[p]:idx[p + 1]] for p in all_reps]))


# ---- 5. planted families

def test_planted_families_get_their_seed_and_strangers_stay_alone(tmp_path):
    """20 families of 30 proteins of 1-4 fingerprints: uniform int8 in [-48, 48] (L1 ~ 15 500 between unrelated rows, far above
    --min-domain 0.5's bound of 8 500), members = their seed's rows within +-2 each (L1 <= 960 to the seed).  The seeds are R; N
    holds the 580 other members and 5 unrelated proteins, shuffled."""
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(77)
    seeds = [rng.integers(-48, 49, size=(int(rng.integers(1, 5)), 480)).astype(np.int8) for _ in range(20)]
    members = [(f, np.clip(seeds[f].astype(np.int64) + rng.integers(-2, 3, size=seeds[f].shape), -127, 127).astype(np.int8))
               for f in range(20) for _ in range(29)]
    strangers = [(20 + s, rng.integers(-48, 49, size=(int(rng.integers(1, 5)), 480)).astype(np.int8)) for s in range(5)]
    new = members + strangers
    new = [new[t] for t in rng.permutation(len(new))]
    pack = lambda rows: (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), np.concatenate(rows))   # noqa: E731
    rep_idx, rep_dct = pack(seeds)
    idx, dct = pack([rows for _, rows in new])
    rep_sid, sid = [f'seed{f}' for f in range(20)], [f'p{t}of{f}' for t, (f, _) in enumerate(new)]
    # the condition on the input, from the oracle's L1 values on a sample of pairs
    vals = rule.pair_l1(np.concatenate([rep_dct, dct]), np.concatenate([rep_idx, rep_idx[-1] + idx[1:]]), np.repeat(np.arange(20), 5),
                        20 + np.arange(100))
    fam = np.array([f for f, _ in new[:100]])
    own = np.repeat(np.arange(20), 5) == fam
    assert own.any() and vals[0][own].max() <= 960 and vals[0][~own].min() > 8500 + 3000
    want = np.array([f if f < 20 else 20 + t for t, (f, _) in enumerate(new)], dtype=np.int32)
    assert np.array_equal(dct_sim.Assignment(rep_sid, rep_idx, rep_dct, sid, idx, dct, min_domain=0.5).labels(), want)
    paths = [str(tmp_path / name) for name in ('r-dct.npz', 'n-dct.npz', 'out.txt', 'all-dct.npz')]
    np.savez(paths[0], sid=np.array(rep_sid), idx=rep_idx, dct=rep_dct)
    np.savez(paths[1], sid=np.array(sid), idx=idx, dct=dct)
    _cli('--dct', paths[1], '--assign', paths[0], '--output', paths[2], '--reps-out', paths[3], min_domain=0.5)
    assert open(paths[2], 'rb').read() == arule.HEADER + arule.text(rep_sid, sid, want)
    got = _npz(paths[3])
    lone = [t for t, (f, _) in enumerate(new) if f >= 20]
    assert len(got[0]) == 25 and got[0] == rep_sid + [sid[t] for t in lone] and got[3] is None
    assert np.array_equal(got[2], np.concatenate([rep_dct] + [new[t][1] for t in lone]))
