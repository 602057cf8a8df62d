"""dct-sim all-against-all with score cut-offs (dct_sim.FilteredPairs; dctfp_tri_filter_count / dctfp_tri_filter_fill /
dctfp_pair_lines): the reference's own output with lines removed by the numpy rule of all_sim_filter_rule.py (pinned on the CPU
in test_all_sim_filter_host.py), the unfiltered path on random ragged files, exactness at the bound, the two routes, the kernels
on their own, and a file whose unfiltered output (20 GB) no test could write."""

import os

import numpy as np
import pytest

import all_sim_filter_rule as rule
import golden_util as gu

pytestmark = pytest.mark.gpu
GOLD = os.path.join(gu.GOLD, 'all_sim')
NPZ = os.path.join(GOLD, 'all-dct.npz')
CUTS = (0.1, 0.25, 0.5, 0.9, 1.0)


def _run(path, out, min_domain=None, min_global=None) -> bytes:
    from dctdomain_amd import dct_sim
    argv = ['--dct', path, '--output', out]
    for name, v in (('--min-domain', min_domain), ('--min-global', min_global)):
        if v is not None:
            argv += [name, str(v)]
    dct_sim.main(argv)
    with open(out, 'rb') as fh:
        return fh.read()


def _load(path):
    with np.load(path) as data:
        return [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']


@pytest.fixture(scope='module')
def golden():
    _, idx, dct = _load(NPZ)
    lines = rule.read_lines(os.path.join(GOLD, 'expected.txt.gz'))
    _, _, mn, last = rule.triangle_l1(dct, idx)
    return lines, mn, last


# ---- the reference golden

@pytest.mark.parametrize('min_domain,min_global',
                         [(x, None) for x in CUTS] + [(None, y) for y in CUTS] + [(0.25, 0.1), (0.1, 0.25), (0.9, 0.5), (0.5, 0.9)])
def test_reference_golden_with_lines_removed(tmp_path, golden, min_domain, min_global):
    lines, mn, last = golden
    want = rule.filtered_text(lines, rule.kept(mn, last, min_domain, min_global))
    assert _run(NPZ, str(tmp_path / 'out.txt'), min_domain, min_global) == want


@pytest.mark.parametrize('cut', ['0', '-1', 'nan'])
@pytest.mark.parametrize('which', ['domain', 'global', 'both'])
def test_a_cut_off_nothing_fails_gives_the_unfiltered_golden(tmp_path, golden, cut, which):
    lines = golden[0]
    got = _run(NPZ, str(tmp_path / 'out.txt'), cut if which != 'global' else None, cut if which != 'domain' else None)
    assert got == b''.join(x + b'\n' for x in lines)


@pytest.mark.parametrize('which', ['domain', 'global', 'both'])
def test_a_cut_off_above_one_gives_the_header_only(tmp_path, which):
    from dctdomain_amd import dct_sim
    got = _run(NPZ, str(tmp_path / 'out.txt'), 1.0001 if which != 'global' else None, 1.0001 if which != 'domain' else None)
    assert got == (dct_sim.HEADER + '\n').encode()


def test_stdout_keeps_its_closing_lines(capfd, golden):
    from dctdomain_amd import dct_sim
    lines, mn, last = golden
    dct_sim.main(['--dct', NPZ, '--min-domain', '0.9'])
    got = capfd.readouterr().out.split('\n')
    want = rule.filtered_text(lines, rule.kept(mn, last, 0.9)).decode('utf8').split('\n')[:-1]
    assert got[0] == want[0] == dct_sim.HEADER
    assert got[1].startswith('dct loaded for 139 sequences, time used: ')
    assert got[2:len(want) + 1] == want[1:]
    assert got[len(want) + 1].startswith('total time used ') and got[len(want) + 2].startswith('distance calculation used ')
    assert got[len(want) + 3:] == ['']


def test_all_sim_and_pairs_take_the_keywords(tmp_path, golden):
    from dctdomain_amd import dct_sim
    lines, mn, last = golden
    keep = rule.kept(mn, last, 0.5, 0.25)
    out = str(tmp_path / 'out.txt')
    dct_sim.all_sim(NPZ, out, min_domain=0.5, min_global=0.25)
    assert open(out, 'rb').read() == rule.filtered_text(lines, keep)
    sid, idx, dct = _load(NPZ)
    i, j = np.triu_indices(139, 1)
    for kw in ({'min_domain': 0.5, 'min_global': 0.25}, {'min_domain': 0.5}):
        keep = rule.kept(mn, last, **kw)
        got = dct_sim.FilteredPairs(sid, idx, dct, **kw).pairs()
        assert all(g.dtype == np.int64 for g in got)
        for g, w in zip(got, (i[keep], j[keep], mn[keep], last[keep])):
            assert np.array_equal(g, w)


# ---- against the unfiltered path on random ragged files (test_all_sim_stream_gpu.py's recipe)

_ALPHABET = list('abcdefghijklmnopqrstuvwxyz0123456789_|.-') + ['é', 'ß', 'α', '蛋', '😀']


def _ragged_file(path, seed, n):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 4, size=n)
    counts[rng.random(n) < 0.15] = 0                         # proteins without fingerprints
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    fam = rng.integers(-60, 61, size=(4, 480))
    dct = np.clip(fam[rng.integers(0, 4, size=int(idx[-1]))] + rng.integers(-20, 21, size=(int(idx[-1]), 480)), -127, 127).astype(np.int8)
    if idx[-1] > 3:
        dct[1] = dct[0]                                      # ties
    lens = rng.choice([1, 2, 5, 17, 40, 333], size=n, p=[.1, .1, .3, .3, .15, .05])
    names = [''.join(rng.choice(_ALPHABET, size=int(m))) for m in lens]
    np.savez(path, sid=np.array(names), idx=idx, dom=np.array(['1-9'] * len(dct)), dct=dct)


# (pairs of one family lie near L1 6 500 = 0.62, of two families above 17 000 = 0: the cut-offs fall inside, between and outside)
_RAGGED_CUTS = [(0.5, None), (None, 0.6), (0.62, 0.3), (0.3, 0.62), (0.0, None), (None, 1.0), (1e-9, None), (None, 1e-9), (1.0, 0.0)]


@pytest.mark.parametrize('seed,n,small', [(1, 60, False), (2, 45, True), (3, 2, False), (4, 1, False), (5, 33, True), (6, 2, True),
                                          (7, 70, True)])
def test_same_bytes_as_the_unfiltered_path_with_lines_dropped(tmp_path, monkeypatch, seed, n, small):
    from dctdomain_amd import dct_sim
    path = str(tmp_path / 'r-dct.npz')
    _ragged_file(path, seed, n)
    lines = _run(path, str(tmp_path / 'all.txt')).split(b'\n')[:-1]          # (AllPairs, untouched)
    _, idx, dct = _load(path)
    _, _, mn, last = rule.triangle_l1(dct, idx)
    assert len(lines) == 1 + n * (n - 1) // 2
    if small:                                                # single-row stripes, many column groups, split stripes
        monkeypatch.setattr(dct_sim.FilteredPairs, 'TEXT_BYTES', 1 + seed * 40)
        monkeypatch.setattr(dct_sim.FilteredPairs, 'COL_ROWS', 3)
        monkeypatch.setattr(dct_sim.FilteredPairs, 'TILE_INTS', 5 if seed != 7 else 300)
    for min_domain, min_global in _RAGGED_CUTS:
        want = rule.filtered_text(lines, rule.kept(mn, last, min_domain, min_global))
        assert _run(path, str(tmp_path / 'out.txt'), min_domain, min_global) == want, (min_domain, min_global)


def test_small_limits_take_every_split(tmp_path, monkeypatch):
    """The limits of the test above do what they are there for: several stripes, several column groups, ranges of rows."""
    from dctdomain_amd import dct_sim
    path = str(tmp_path / 'r-dct.npz')
    _ragged_file(path, 7, 70)
    sid, idx, dct = _load(path)
    monkeypatch.setattr(dct_sim.FilteredPairs, 'TEXT_BYTES', 281)
    monkeypatch.setattr(dct_sim.FilteredPairs, 'COL_ROWS', 3)
    monkeypatch.setattr(dct_sim.FilteredPairs, 'TILE_INTS', 300)
    calls = {'protein_min': 0, 'fill': 0}
    real_pm, real_fill = dct_sim.protein_min, dct_sim.tri_filter_fill
    monkeypatch.setattr(dct_sim, 'protein_min', lambda *a, **k: (calls.__setitem__('protein_min', calls['protein_min'] + 1), real_pm(*a, **k))[1])
    monkeypatch.setattr(dct_sim, 'tri_filter_fill', lambda *a, **k: (calls.__setitem__('fill', calls['fill'] + 1), real_fill(*a, **k))[1])
    f = dct_sim.FilteredPairs(sid, idx, dct, min_domain=0.0)  # (every pair survives: every row has lines)
    stripes = list(f.stripes())
    assert len(stripes) > 5 and any(b - a > 1 for a, b in stripes)
    first_rows = [int(c[0][0]) for c in f.chunks()]
    assert calls['protein_min'] > 2 * len(stripes)            # (column groups)
    assert calls['fill'] == len(first_rows) > len(stripes)    # (ranges of rows within a stripe)
    assert first_rows == list(range(69))                      # (281 bytes hold no two rows: one range per row)


# ---- exactness at the bound

def _row_with_l1(v):
    row = np.zeros(480, dtype=np.int8)
    q, r = divmod(int(v), 127)
    row[:q] = 127
    row[q] = r
    return row


@pytest.mark.parametrize('cut', [0.5, 0.25, 1e-9, 1.0, 0.0])
def test_kept_and_dropped_exactly_at_the_bound(cut):
    from dctdomain_amd import dct_sim
    bound = dct_sim.sim_bound(cut)
    values = sorted({max(bound, 0), bound + 1, 16999, 17000, 17001, 40000})
    # protein 0: one zero fingerprint.  A_v: one fingerprint at L1 v from it (min = last = v).  B_v: one at v, then one at 40 000
    # (min = v, last = 40 000).  C_v: one at 40 000 ... no: min <= last always, so DCTglobal's own bound is probed with A_v.
    rows, counts = [np.zeros(480, dtype=np.int8)], [1]
    for v in values:
        rows += [_row_with_l1(v)]
        counts += [1]
    for v in values:
        rows += [_row_with_l1(v), _row_with_l1(40000)]
        counts += [2]
    dct = np.stack(rows)
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    sid = [f'p{k}' for k in range(len(counts))]
    i, j, mn, last = rule.triangle_l1(dct, idx)
    first = i == 0
    assert list(mn[first]) == values + values and list(last[first]) == values + [40000] * len(values)
    for kw in ({'min_domain': cut}, {'min_global': cut}, {'min_domain': cut, 'min_global': cut}):
        gi, gj, gmn, glast = dct_sim.FilteredPairs(sid, idx, dct, **kw).pairs()
        # as sim_bound says, on the integers ...
        keep = np.ones(len(i), dtype=bool)
        if 'min_domain' in kw:
            keep &= np.minimum(mn, 17000) <= bound
        if 'min_global' in kw:
            keep &= np.minimum(last, 17000) <= bound
        assert np.array_equal(gi, i[keep]) and np.array_equal(gj, j[keep]), kw
        assert np.array_equal(gmn, mn[keep]) and np.array_equal(glast, last[keep])
        # ... which is the reference's comparison on the floats
        assert np.array_equal(keep, rule.kept(mn, last, **kw))
        # and, spelled out for the pairs with protein 0: v is kept exactly when min(v, 17000) <= bound
        got0 = set(gj[gi == 0].tolist())
        for k, v in enumerate(values):
            a, b = 1 + k, 1 + len(values) + k
            ok = min(v, 17000) <= bound
            assert (a in got0) == ok, (kw, v)
            assert (b in got0) == (ok if 'min_global' not in kw else 17000 <= bound), (kw, v)


# ---- the two routes

def _counting(monkeypatch):
    from dctdomain_amd import dct_sim
    calls = {'protein_min': 0, 'l1_matrix': 0}
    real_pm, real_l1 = dct_sim.protein_min, dct_sim.l1_matrix

    def pm(*a, **k):
        calls['protein_min'] += 1
        return real_pm(*a, **k)

    def l1(*a, **k):
        calls['l1_matrix'] += 1
        return real_l1(*a, **k)
    monkeypatch.setattr(dct_sim, 'protein_min', pm)
    monkeypatch.setattr(dct_sim, 'l1_matrix', l1)
    return calls


@pytest.mark.parametrize('cut', [0.25, 0.5, 0.9])
def test_the_two_routes_agree(tmp_path, monkeypatch, cut):
    def refuse(*a, **k):
        raise AssertionError('a cut-off must not take the unfiltered path')
    from dctdomain_amd import dct_sim
    monkeypatch.setattr(dct_sim.AllPairs, 'write', refuse)
    calls = _counting(monkeypatch)
    out = str(tmp_path / 'out.txt')
    both = _run(NPZ, out, cut, cut)                           # DCTdomain is never below DCTglobal: the second cut-off removes nothing
    assert calls['protein_min'] == 0 and calls['l1_matrix'] > 0
    calls.update(protein_min=0, l1_matrix=0)
    assert _run(NPZ, out, None, cut) == both
    assert calls['protein_min'] == 0 and calls['l1_matrix'] > 0
    calls.update(protein_min=0, l1_matrix=0)
    alone = _run(NPZ, out, cut, None)
    assert calls['protein_min'] > 0 and calls['l1_matrix'] == 0
    calls.update(protein_min=0, l1_matrix=0)
    assert _run(NPZ, out, cut, -1) == alone                   # a cut-off nothing fails does not change the route
    assert calls['protein_min'] > 0 and calls['l1_matrix'] == 0
    assert len(alone) > len(both) > len(dct_sim.HEADER) + 1


# ---- the kernels on their own

_np_filter, _random_tile = rule.tile_filter, rule.random_tile


@pytest.mark.parametrize('n_rows,n_cols', [(7, 3000), (1, 5000), (40, 1), (3, 1023), (5, 1025), (9, 2048), (4, 0), (0, 10), (300, 37)])
@pytest.mark.parametrize('bound', [-1, 0, 8500, 17000])
def test_filter_kernels_against_numpy(n_rows, n_cols, bound):
    import torch
    from dctdomain_amd.similarity import tri_filter
    rng = np.random.default_rng(1000 * n_rows + n_cols + bound)
    # the diagonal inside the tile, the tile right of it (every entry has j > i) and left of it (none has)
    places = [(10, 5), (n_rows + 3, 0) if n_cols else (0, 0), (0, n_rows + 20), (3, 3 + n_rows + n_cols), (0, 1), (2 ** 31 - 1 - n_cols - 7, 5)]
    for k, (col0, row0) in enumerate(places):
        t = _random_tile(rng, n_rows, n_cols, bound)
        if n_rows > 4 and n_cols:
            t[2] = 17001                                      # a row with no survivor (below 17000) between rows with many
            t[1], t[3] = 0, 0
        pad, shift = int(rng.integers(0, 9)), int(rng.integers(0, 4))
        big = torch.full((max(n_rows, 1), n_cols + pad + shift + 1), -1, dtype=torch.int32, device='cuda')   # strided rows, any alignment
        view = big[:n_rows, shift:shift + n_cols]
        view.copy_(torch.as_tensor(t, device='cuda'))
        flags = [(None, None), (rng.random(n_rows) < 0.3, None), (None, rng.random(n_cols) < 0.3),
                 (rng.random(n_rows) < 0.2, rng.random(n_cols) < 0.2)][k % 4]
        count, i, j = tri_filter(view, row0, col0, bound, *flags)
        wc, wi, wj = _np_filter(t, row0, col0, bound, *flags)
        assert np.array_equal(count, wc), (k, col0, row0)
        assert np.array_equal(i, wi) and np.array_equal(j, wj), (k, col0, row0)
        if n_rows > 4 and n_cols and bound < 17000 and flags[0] is None and col0 + n_cols > row0 + 4:
            assert count[2] == 0
        if bound == 17000:                                    # everything right of the diagonal
            assert count.sum() == np.count_nonzero(col0 + np.arange(n_cols)[None, :] > row0 + np.arange(n_rows)[:, None])


def test_filter_fill_stays_within_its_buffer_and_rejects_bad_arguments():
    import ctypes as C
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.similarity import tri_filter_count
    t = torch.zeros((6, 100), dtype=torch.int32, device='cuda')
    count = tri_filter_count(t, 0, 0, 17000)
    assert count.cpu().tolist() == [99, 98, 97, 96, 95, 94]
    offsets = torch.zeros(7, dtype=torch.int64, device='cuda')
    torch.cumsum(count, 0, out=offsets[1:])
    out = torch.full((2, 700), -7, dtype=torch.int32, device='cuda')
    ctx = _lib.get_context(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda out_len, bound=17000, ld=100: ctx._lib.dctfp_tri_filter_fill(   # noqa: E731
        ctx.handle, t.data_ptr(), 6, 100, ld, 0, 0, None, None, 17000, bound, offsets.data_ptr(), out_len, out[0].data_ptr(), out[1].data_ptr(), stream)
    assert call(250) == 0                                     # (a buffer shorter than the survivors: the rest is not written)
    got = out.cpu().numpy()
    assert (got[:, 250:] == -7).all() and (got[:, :250] >= 0).all()
    assert list(got[1, :99]) == list(range(1, 100)) and list(got[0, 99:197]) == [1] * 98
    assert call(579, bound=17001) == _lib.DCTFP_ERR_INVALID and call(579, bound=-2) == _lib.DCTFP_ERR_INVALID
    assert call(579, ld=99) == _lib.DCTFP_ERR_INVALID
    rc = ctx._lib.dctfp_tri_filter_count(ctx.handle, t.data_ptr(), 6, 100, 100, 2 ** 31 - 3, 0, None, None, 17000, 0, count.data_ptr(), stream)
    assert rc == _lib.DCTFP_ERR_LIMIT


def test_line_kernel_against_python_formatting():
    import torch
    from dctdomain_amd import dct_sim
    from dctdomain_amd.similarity import LineIds, pair_line_offsets, pair_lines
    rng = np.random.default_rng(11)
    names = ['x', 'é', 'M' * 301, 'L' * 5000, '蛋' * 1500] + [''.join(rng.choice(_ALPHABET, size=int(m))) for m in rng.integers(1, 60, size=400)]
    ids = LineIds(names)
    # L1 values on both sides of every .3f rounding boundary: 1 - v / 17000 crosses k + 0.5 thousandths between v = 17 k + 8 and + 9
    edge = np.array([17 * k + d for k in range(0, 1000, 7) for d in (8, 9)] + [0, 1, 16991, 16992, 16999, 17000, 17001, 17002, 40000, 0x7fffffff])
    n = 3000
    pi, pj = rng.integers(0, len(names), size=n), rng.integers(0, len(names), size=n)
    pi[:5], pj[:5] = [0, 3, 4, 3, 2], [3, 0, 3, 3, 1]
    mn, last = rng.choice(edge, size=n), rng.choice(edge, size=n)
    mn[:len(edge)] = edge
    last[len(edge):2 * len(edge)] = edge
    want = []
    for a, b, m, l in zip(pi, pj, mn, last):
        sa, sb = dct_sim._scores(m, l)
        want.append(f'{names[a]} {names[b]} {sa:.3f} {sb:.3f}\n'.encode('utf8'))
    dev = lambda a: torch.as_tensor(np.asarray(a).astype(np.int32), device='cuda')   # noqa: E731
    tp = [dev(x) for x in (pi, pj, mn, last)]
    off = pair_line_offsets(tp[0], tp[1], ids)
    assert off.cpu().tolist() == [0] + list(np.cumsum([len(w) for w in want]))
    total = int(off[-1])
    table = torch.as_tensor(dct_sim.score_table(), device='cuda')
    for lead in (0, 3, 13):                                   # (the text's first byte on any alignment)
        buf = torch.full((lead + total + 9,), 0xAB, dtype=torch.uint8, device='cuda')
        pair_lines(*tp, ids, table, off, buf[lead:lead + total])
        got = buf.cpu().numpy().tobytes()
        assert got[lead:lead + total] == b''.join(want)
        assert set(got[:lead]) <= {0xAB} and set(got[lead + total:]) == {0xAB}
    # a buffer that ends early: the lines that do not fit are left out, nothing is written beyond it
    cut = int(off[n // 2]) + 5
    buf = torch.full((total,), 0xAB, dtype=torch.uint8, device='cuda')
    pair_lines(*tp, ids, table, off, buf[:cut])
    got = buf.cpu().numpy().tobytes()
    assert got[:cut - 5] == b''.join(want[:n // 2]) and set(got[cut - 5:]) == {0xAB}


# ---- scale: 30 000 proteins, 4.5 x 10^8 pairs, 20 GB of unfiltered text

def test_thirty_thousand_proteins_print_the_planted_pairs_only(tmp_path, monkeypatch):
    """Random proteins (1-8 uniform int8 rows in [-48, 48]) lie at L1 ~ 15 500 +- 500 from each other (per entry E|x - y| = 32.3,
    standard deviation 22.9 -> 480 entries: 15 500 +- 500; the minimum over at most 64 row pairs lowers that by some 2.5
    standard deviations), 14 standard deviations above --min-domain 0.5's bound of 8 500: a condition on the inputs.  The printed
    set is compared with the planted set exactly and every printed line is recomputed."""
    from scipy.spatial.distance import cdist
    from dctdomain_amd import dct_sim
    from tools.all_sim_bench import synth

    def refuse(*a, **k):
        raise AssertionError('the unfiltered path would write 20 GB')
    monkeypatch.setattr(dct_sim.AllPairs, 'write', refuse)
    n, n_planted = 30000, 300
    path = str(tmp_path / 's-dct.npz')
    synth(path, n, 7)
    sid, idx, dct = _load(path)
    rng = np.random.default_rng(23)
    chosen = rng.choice(n, size=2 * n_planted, replace=False)
    src, dst = chosen[:n_planted], chosen[n_planted:]
    per = [dct[idx[p]:idx[p + 1]] for p in range(n)]
    for s, d in zip(src, dst):                                # a copy of one protein's rows with +-2 noise under another id
        per[d] = np.clip(per[s].astype(np.int64) + rng.integers(-2, 3, size=per[s].shape), -127, 127).astype(np.int8)
    idx = np.concatenate([[0], np.cumsum([len(r) for r in per])]).astype(np.int64)
    dct = np.concatenate(per)
    del per
    np.savez(path, sid=np.array(sid), idx=idx, dom=np.array(['1-9'] * len(dct)), dct=dct)
    got = _run(path, str(tmp_path / 'out.txt'), 0.5).decode('utf8').split('\n')
    assert got[0] == dct_sim.HEADER and got[-1] == ''
    where = {name: k for k, name in enumerate(sid)}
    printed = [(where[a], where[b], line) for a, b, line in ((*x.split(' ')[:2], x) for x in got[1:-1])]
    # the numpy rule among the planted proteins and their partners: all 600 x 600 pairs
    members = np.sort(chosen)
    rows = np.concatenate([np.arange(idx[p], idx[p + 1]) for p in members])
    sub_idx = np.concatenate([[0], np.cumsum(idx[members + 1] - idx[members])])
    d = cdist(dct[rows].astype(np.float64), dct[rows].astype(np.float64), 'cityblock').astype(np.int64)
    mn = np.minimum.reduceat(np.minimum.reduceat(d, sub_idx[:-1], axis=0), sub_idx[:-1], axis=1)
    a, b = np.triu_indices(len(members), 1)
    keep = rule.kept(mn[a, b], mn[a, b], min_domain=0.5)
    want = sorted(zip(members[a[keep]].tolist(), members[b[keep]].tolist()))
    planted = {(min(s, t), max(s, t)) for s, t in zip(src.tolist(), dst.tolist())}
    assert planted <= set(want) and len(want) < 2 * n_planted
    assert [(i, j) for i, j, _ in printed] == want            # the planted set exactly, in output order
    # every printed line, recomputed from the two proteins
    pi, pj = np.array([p[0] for p in printed]), np.array([p[1] for p in printed])
    pm, pl = rule.pair_l1(dct, idx, pi, pj)
    for (i, j, line), m, l in zip(printed, pm, pl):
        sa, sb = dct_sim._scores(m, l)
        assert line == f'{sid[i]} {sid[j]} {sa:.3f} {sb:.3f}'
        assert sa >= 0.5
    # the oracle's own guard: 2 000 random pairs outside the planted set are rightly absent
    ri, rj = rng.integers(0, n, size=2000), rng.integers(0, n, size=2000)
    ok = (ri != rj) & np.array([(min(x, y), max(x, y)) not in set(want) for x, y in zip(ri.tolist(), rj.tolist())])
    rm, rl = rule.pair_l1(dct, idx, ri[ok], rj[ok])
    assert ok.sum() > 1900 and not rule.kept(rm, rl, min_domain=0.5).any()
    assert rm.min() > 8500 + 3000                             # (the condition on the inputs, seen: nowhere near the bound)
