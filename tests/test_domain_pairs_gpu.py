"""dct-sim --domains: dctfp_pair_argmin and dctfp_pair_domain_lines against the numpy rule of domain_pair_rule.py (pinned on the CPU
against the reference's loop in test_domain_pairs_host.py), and every mode of dct_sim.main against text built from that rule --
with the first four fields of every line equal to the same run's without the flag."""

import os
import re

import numpy as np
import pytest

import domain_pair_rule as rule
import golden_util as gu

pytestmark = pytest.mark.gpu
FIX = os.path.join(gu.GOLD, 'ref_fixtures')
ALL_NPZ = os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')
SEARCH = os.path.join(gu.GOLD, 'protein_search')


def _load(path):
    with np.load(path) as data:
        return [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']


# ---- dctfp_pair_argmin

def test_pair_argmin_on_the_all_sim_golden():
    from dctdomain_amd.similarity import pair_argmin, pair_min
    _, idx, dct = _load(ALL_NPZ)
    i, j, mn, last, arg_i, arg_j = rule.triangle_args(dct, idx)
    tied, whole = rule.pair_facts(dct, idx, dct, idx, i, j)
    # the fixture holds all three cases: no domain pair, a tied minimum, whole x whole
    assert (len(i), int((arg_i < 0).sum()), int(tied.sum()), int(whole.sum())) == (9591, 1110, 271, 2460)
    pairs = np.stack([i, j], axis=1)
    got = pair_argmin(dct, idx, dct, idx, pairs)
    assert all(g.dtype == np.int64 and g.shape == (9591,) for g in got)
    for g, w, name in zip(got, (mn, last, arg_i, arg_j), ('min', 'last', 'arg_a', 'arg_b')):
        assert np.array_equal(g, w), name
    ref = pair_min(dct, idx, dct, idx, pairs)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    # the transposed pairs: the tie order follows the first protein
    got_t = pair_argmin(dct, idx, dct, idx, pairs[:, ::-1])
    want_t = rule.pair_args(dct, idx, dct, idx, j, i)
    for g, w in zip(got_t, want_t):
        assert np.array_equal(g, w)


def _ragged_sets(seed, d, n_a=40, n_b=33):
    """Two fingerprint sets of width d around shared families (near pairs and far ones), proteins of 0 .. 9 rows, exact duplicates
    planted at several positions of both sides: ties within a protein and across the unroll of four b rows."""
    rng = np.random.default_rng(seed)
    scale = 60 if d <= 512 else 20                              # (wide rows: keep some pairs below 17000)
    fam = rng.integers(-scale, scale + 1, size=(4, d))
    out = []
    for n in (n_a, n_b):
        counts = rng.integers(1, 10, size=n)
        counts[rng.random(n) < 0.15] = 0
        idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        rows = int(idx[-1])
        dct = np.clip(fam[rng.integers(0, 4, size=rows)] + rng.integers(-8, 9, size=(rows, d)), -128, 127).astype(np.int8)
        out.append((idx, dct))
    (ia, a), (ib, b) = out
    for _ in range(60):                                         # one fingerprint at two places of b (and sometimes of a)
        src = a[rng.integers(0, len(a))]
        b[rng.integers(0, len(b), size=int(rng.integers(2, 6)))] = src
        if rng.random() < 0.5:
            a[rng.integers(0, len(a), size=2)] = src
    return ia, a, ib, b


@pytest.mark.parametrize('d', [1, 7, 480, 512, 516, 1000])
def test_pair_argmin_ragged_against_the_rule(d):
    import torch
    from dctdomain_amd.similarity import pair_argmin, pair_argmin_device, pair_min, pair_min_device
    ia, a, ib, b = _ragged_sets(100 + d, d)
    npa, npb = len(ia) - 1, len(ib) - 1
    i, j = (x.ravel() for x in np.meshgrid(np.arange(npa), np.arange(npb), indexing='ij'))
    want = rule.pair_args(a, ia, b, ib, i, j)
    tied, _ = rule.pair_facts(a, ia, b, ib, i, j)
    assert int((tied & (want[2] >= 0)).sum()) >= 20 and int((want[2] < 0).sum()) >= 20 and int((want[2] > 0).sum()) >= 20
    pairs = np.stack([i, j], axis=1)
    got = pair_argmin(a, ia, b, ib, pairs)
    for g, w, name in zip(got, want, ('min', 'last', 'arg_a', 'arg_b')):
        assert np.array_equal(g, w), (d, name)
    ref = pair_min(a, ia, b, ib, pairs)
    assert len(ref) == 2 and all(r.dtype == np.int64 for r in ref + got)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    # rows at any stride and base (the kernel's byte path), and pair indices out of range: -1 in all four outputs
    dev = torch.device('cuda')
    views = []
    for m, lead, pad in ((a, 1, 3), (b, 2, 1)):
        ld = d + pad
        flat = torch.zeros(lead + len(m) * ld + 8, dtype=torch.int8, device=dev)
        view = flat[lead:lead + len(m) * ld].view(len(m), ld)[:, :d]
        view.copy_(torch.as_tensor(m, device=dev))
        assert view.data_ptr() & 3 and view.stride(0) == ld
        views.append(view)
    bad = np.array([(-1, 0), (0, -1), (npa, 0), (0, npb), (2 ** 31 - 1, 2 ** 31 - 1)])
    tp = torch.as_tensor(np.concatenate([pairs, bad]).astype(np.int32), device=dev)
    out = pair_argmin_device(views[0], torch.as_tensor(ia, device=dev), views[1], torch.as_tensor(ib, device=dev), tp)
    assert all(t.dtype == torch.int32 and t.is_cuda for t in out)
    out = [t.cpu().numpy().astype(np.int64) for t in out]
    for g, w, name in zip(out, want, ('min', 'last', 'arg_a', 'arg_b')):
        assert np.array_equal(g[:len(i)], w), (d, 'strided', name)
        assert (g[len(i):] == -1).all(), (d, 'out of range', name)
    # ... and the form without the position: the same two, by the other instantiation of the kernel
    both = pair_min_device(views[0], torch.as_tensor(ia, device=dev), views[1], torch.as_tensor(ib, device=dev), tp)
    assert len(both) == 2 and all(t.dtype == torch.int32 and t.is_cuda for t in both)
    for g, w, name in zip((t.cpu().numpy().astype(np.int64) for t in both), ref, ('min', 'last')):
        assert np.array_equal(g[:len(i)], w), (d, 'strided, no position', name)
        assert (g[len(i):] == -1).all(), (d, 'out of range, no position', name)


def test_pair_argmin_tie_order_does_not_depend_on_the_unroll():
    """One a row against b proteins of 1 .. 9 rows where the same smallest L1 sits at every pair of positions: always the first."""
    from dctdomain_amd.similarity import pair_argmin
    rng = np.random.default_rng(3)
    for d in (480, 600):                                        # (both paths of the kernel)
        base = rng.integers(-50, 51, size=d).astype(np.int8)
        far = np.clip(base.astype(np.int64) + 40, -128, 127).astype(np.int8)
        protos, want = [], []
        for k in range(1, 10):
            for x in range(k):
                for y in range(x, k):
                    rows = np.stack([far] * k)
                    rows[x] = rows[y] = base
                    protos.append(rows)
                    want.append(x)
        ib = np.concatenate([[0], np.cumsum([len(p) for p in protos])])
        other = np.clip(base.astype(np.int64) - 40, -128, 127).astype(np.int8)
        a = np.stack([other, base, base])                        # protein 0 of a: the match is its row 1, not 0 or 2
        mn, last, arg_a, arg_b = pair_argmin(a, [0, 3], np.concatenate(protos), ib, [(0, q) for q in range(len(protos))])
        assert (mn == 0).all() and (arg_a == 1).all() and arg_b.tolist() == want


def test_pair_argmin_arguments():
    import torch
    from dctdomain_amd.similarity import pair_argmin, pair_argmin_device
    a = np.zeros((3, 480), dtype=np.int8)
    none = np.zeros((0, 480), dtype=np.int8)
    for x, ix, y, iy in ((a, [0, 3], none, [0, 0]), (none, [0, 0], a, [0, 1, 3])):
        got = pair_argmin(x, ix, y, iy, [(0, 0), (0, 0)])
        assert [g.tolist() for g in got] == [[0x7fffffff] * 2, [0x7fffffff] * 2, [-1, -1], [-1, -1]]
    assert [g.tolist() for g in pair_argmin(a, [0, 3], a, [0, 1, 3], [(0, 1)])] == [[0], [0], [0], [0]]
    assert [g.shape for g in pair_argmin(a, [0, 3], a, [0, 3], np.zeros((0, 2)))] == [(0,)] * 4
    with pytest.raises(IndexError):
        pair_argmin(a, [0, 3], a, [0, 3], [(0, 1)])
    with pytest.raises(ValueError):
        pair_argmin(a, [0, 4], a, [0, 3], [(0, 0)])
    with pytest.raises(ValueError):
        pair_argmin(a, [0, 3], np.zeros((3, 479), dtype=np.int8), [0, 3], [(0, 0)])
    t = torch.zeros((3, 480), dtype=torch.int8, device='cuda')
    idx = torch.as_tensor(np.array([0, 3]), device='cuda')
    with pytest.raises(ValueError):
        pair_argmin_device(t, idx, t, idx, torch.zeros((1, 2), dtype=torch.int64, device='cuda'))
    with pytest.raises(ValueError):
        pair_argmin_device(t, idx.to(torch.int32), t, idx, torch.zeros((1, 2), dtype=torch.int32, device='cuda'))


def test_best_domain_pair():
    from dctdomain_amd import dct_sim
    _, idx, dct = _load(os.path.join(FIX, 'example-dct.npz'))
    sets = [dct[idx[p]:idx[p + 1]] for p in range(len(idx) - 1)]
    for a in sets[:4]:
        for b in sets[4:]:
            mn, last, arg_a, arg_b = rule.best_pair(a, b)
            got = dct_sim.best_domain_pair(a, b)
            assert got[:2] == dct_sim.domain_sim(a, b)
            assert got[2:] == ((arg_a, arg_b) if arg_a >= 0 else (None, None))
    far = np.full((2, 480), 127, dtype=np.int8)
    assert dct_sim.best_domain_pair(far, -far) == (0, 0, None, None)


# ---- dctfp_pair_domain_lines

def test_domain_line_kernel_against_python_formatting():
    import torch
    from dctdomain_amd import dct_sim
    from dctdomain_amd.similarity import LineIds, pair_domain_line_offsets, pair_domain_lines
    rng = np.random.default_rng(12)
    names = ['x', 'é', 'M' * 301, '蛋' * 700, 'sp|P1|α'] + [f'p{k}' for k in range(50)]
    labels = ['1', '35-169', '1-20,50-80', 'whole', 'δομή-1', 'L' * 400] + [str(k) for k in range(1, 40)] + ['-']
    ids, tab = LineIds(names), LineIds(labels)
    n = 2000
    pi, pj = rng.integers(0, len(names), size=n), rng.integers(0, len(names), size=n)
    la, lb = rng.integers(0, len(labels), size=n), rng.integers(0, len(labels), size=n)
    pi[:4], pj[:4], la[:4], lb[:4] = [0, 3, 1, 2], [3, 0, 4, 2], [len(labels) - 1, 5, 4, 2], [len(labels) - 1, 4, 5, 3]   # (the sentinel first)
    mn = rng.choice([0, 1, 8, 9, 8499, 8500, 16999, 17000, 17001, 40000, 0x7fffffff], size=n)
    last = rng.choice([0, 25, 26, 12750, 17000, 0x7fffffff], size=n)
    want = []
    for a, b, m, l, x, y in zip(pi, pj, mn, last, la, lb):
        sa, sb = dct_sim._scores(m, l)
        want.append(f'{names[a]} {names[b]} {sa:.3f} {sb:.3f} {labels[x]} {labels[y]}\n'.encode('utf8'))
    dev = lambda v: torch.as_tensor(np.asarray(v).astype(np.int32), device='cuda')   # noqa: E731
    tp = [dev(v) for v in (pi, pj, mn, last, la, lb)]
    off = pair_domain_line_offsets(tp[0], tp[1], tp[4], tp[5], ids, tab)
    assert off.cpu().tolist() == [0] + list(np.cumsum([len(w) for w in want]))
    total = int(off[-1])
    table = torch.as_tensor(dct_sim.score_table(), device='cuda')
    for lead in (0, 3, 13):                                     # (the text's first byte on any alignment)
        buf = torch.full((lead + total + 9,), 0xAB, dtype=torch.uint8, device='cuda')
        pair_domain_lines(*tp, ids, tab, table, off, buf[lead:lead + total])
        got = buf.cpu().numpy().tobytes()
        assert got[lead:lead + total] == b''.join(want)
        assert set(got[:lead]) <= {0xAB} and set(got[lead + total:]) == {0xAB}
    # skipped lines: a label or a protein outside its table leaves the line's bytes alone, the others are written
    skip = {5: (4, len(labels)), 77: (5, -1), 300: (0, len(names)), 301: (1, -3)}
    tq = [t.clone() for t in tp]
    for k, (which, value) in skip.items():
        tq[which][k] = value
    buf = torch.full((total,), 0xAB, dtype=torch.uint8, device='cuda')
    pair_domain_lines(*tq, ids, tab, table, off, buf)
    got = buf.cpu().numpy().tobytes()
    starts = off.cpu().tolist()
    for k in range(n):
        piece = got[starts[k]:starts[k + 1]]
        assert piece == (b'\xab' * len(want[k]) if k in skip else want[k]), k
    # a buffer that ends early: the lines that do not fit are left out, nothing is written beyond it
    cut = starts[n // 2] + 5
    buf = torch.full((total,), 0xAB, dtype=torch.uint8, device='cuda')
    pair_domain_lines(*tp, ids, tab, table, off, buf[:cut])
    got = buf.cpu().numpy().tobytes()
    assert got[:cut - 5] == b''.join(want[:n // 2]) and set(got[cut - 5:]) == {0xAB}
    with pytest.raises(ValueError):
        pair_domain_lines(*tp[:5], tp[5].long(), ids, tab, table, off, buf)
    with pytest.raises(ValueError):
        pair_domain_lines(*tp, ids, tab, table, off[:10].contiguous(), buf)


def test_line_kernel_with_and_without_labels_writes_the_same_first_four_fields():
    """The two instantiations of the line kernel against each other and against Python, at the edges of the score table."""
    import torch
    from dctdomain_amd import dct_sim
    from dctdomain_amd.similarity import LineIds, pair_domain_line_offsets, pair_domain_lines, pair_line_offsets, pair_lines
    names = ['', 'a', 'B' * 17, 'pé-1']                         # (empty, one byte, more than the sixteen lanes, a two-byte character)
    labels = ['1', '', '12-40;55-90', '-']
    edge = [0, 1, 16999, 17000, 17001, 0x7fffffff]
    pi, pj = [0, 1, 2, 3, 2, 0], [1, 2, 3, 0, 2, 0]
    mn, last = edge, edge[::-1]
    la, lb = [0, 1, 2, 3, 1, 2], [3, 2, 1, 0, 1, 2]
    score = dct_sim.score_table()
    plain = [f'{names[a]} {names[b]} '.encode('utf8') + bytes(score[0, min(m, 17001)]) + b' ' + bytes(score[1, min(l, 17001)])
             for a, b, m, l in zip(pi, pj, mn, last)]
    assert plain[0] == b' a 1.000 0.000' and plain[2].endswith(b' 0.000 0.000') and plain[4] == b'B' * 17 + b' ' + b'B' * 17 + b' 0.000 1.000'
    named = [t + f' {labels[x]} {labels[y]}'.encode('utf8') for t, x, y in zip(plain, la, lb)]
    want = {False: b''.join(t + b'\n' for t in plain), True: b''.join(t + b'\n' for t in named)}
    ids, tab = LineIds(names), LineIds(labels)
    tp = [torch.as_tensor(np.asarray(v, dtype=np.int32), device='cuda') for v in (pi, pj, mn, last, la, lb)]
    table = torch.as_tensor(score, device='cuda')
    got = {}
    for named_lines in (False, True):
        if named_lines:
            off = pair_domain_line_offsets(tp[0], tp[1], tp[4], tp[5], ids, tab)
        else:
            off = pair_line_offsets(tp[0], tp[1], ids)
        total = int(off[-1])
        assert total == len(want[named_lines])
        for short in (0, 1):                                    # (1: `out` ends one byte before the last line does)
            buf = torch.full((5 + total + 3,), 0xAB, dtype=torch.uint8, device='cuda')
            out = buf[5:5 + total - short]
            assert out.data_ptr() & 1
            if named_lines:
                pair_domain_lines(*tp, ids, tab, table, off, out)
            else:
                pair_lines(*tp[:4], ids, table, off, out)
            text = buf.cpu().numpy().tobytes()
            assert text[:5] == b'\xab' * 5 and text[5 + total:] == b'\xab' * 3
            if short:                                           # the last line is left out whole: its bytes keep their fill
                start = int(off[-2])
                assert text[5:5 + start] == want[named_lines][:start] and text[5 + start:] == b'\xab' * (total - start + 3)
            else:
                assert text[5:5 + total] == want[named_lines]
                got[named_lines] = text[5:5 + total]
    cut = [line.rsplit(b' ', 2)[0] for line in got[True].split(b'\n')[:-1]]
    assert b''.join(c + b'\n' for c in cut) == got[False]


# ---- end to end

def _main(tmp_path, argv) -> list:
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    dct_sim.main(argv + ['--output', out])
    with open(out, encoding='utf8') as fh:
        text = fh.read()
    assert text.endswith('\n')
    return text.split('\n')[:-1]


def _write_dom(path, sid, idx, seed, whole_last=True):
    """A .dom file for an npz: per protein with k fingerprints, k - 1 names (the last row is the whole protein) or, for some
    proteins, k names; one of them discontinuous.  Proteins without fingerprints get no line.  Returns {pid: [names]}."""
    rng = np.random.default_rng(seed)
    doms = {}
    for p, k in enumerate(np.diff(idx).tolist()):
        if k == 0:
            continue
        m = k - 1 if whole_last and k > 1 and rng.random() < 0.8 else k
        names = [f'{20 * r + 1}-{20 * r + 20}' for r in range(m)]
        if m > 1 and rng.random() < 0.3:
            names[1] = names[1] + f',{900 + p}-{950 + p}'
        doms[sid[p]] = names
    with open(path, 'w', encoding='utf8') as fh:
        for pid, names in doms.items():
            fh.write(f'{pid} {len(names)} {";".join(names)}\n')
    return doms


def _expect(flagless, sid_a, idx_a, dct_a, names_a, sid_b, idx_b, dct_b, names_b):
    """The flagless lines with the rule's two fields appended; the proteins of a line found by id (unique in the fixtures)."""
    from dctdomain_amd import dct_sim
    assert flagless[0] == dct_sim.HEADER
    wa, wb = {s: k for k, s in enumerate(sid_a)}, {s: k for k, s in enumerate(sid_b)}
    out = [dct_sim.DOMAIN_HEADER]
    for line in flagless[1:]:
        first, second = line.split(' ')[:2]
        i, j = wa[first], wb[second]
        _, _, x, y = rule.best_pair(dct_a[idx_a[i]:idx_a[i + 1]], dct_b[idx_b[j]:idx_b[j + 1]])
        out.append(f'{line} {rule.label(names_a, idx_a[i], x)} {rule.label(names_b, idx_b[j], y)}')
    return out


def _four_fields(lines):
    return [lines[0].rsplit(' ', 2)[0]] + [' '.join(x.split(' ')[:4]) for x in lines[1:]]


def test_pair_mode_on_the_reference_example(tmp_path):
    npz, pair, dom = (os.path.join(FIX, n) for n in ('example-dct.npz', 'example.pair', 'example.dom'))
    sid, idx, dct = _load(npz)
    flagless = _main(tmp_path, ['--dct', npz, '--pair', pair])
    assert len(flagless) == 5
    for extra, names in ((['--domains'], rule.labels(idx)), (['--dom', dom], rule.labels(idx, rule.read_dom(dom), sid)),
                         (['--domains', '--dom', dom], rule.labels(idx, rule.read_dom(dom), sid))):
        got = _main(tmp_path, ['--dct', npz, '--pair', pair] + extra)
        assert got == _expect(flagless, sid, idx, dct, names, sid, idx, dct, names), extra
        assert _four_fields(got) == flagless
    # the mode function called as a library opens its own report with the wider header
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'lib.txt')
    dct_sim.pair_sim(npz, pair, None, out, dom=dom)
    with open(out, encoding='utf8') as fh:
        assert fh.read().split('\n')[:-1] == got
    # the pairfound copy is written as without the flag
    found = str(tmp_path / 'found.txt')
    _main(tmp_path, ['--dct', npz, '--pair', pair, '--pairfound', found, '--domains'])
    assert open(found).read() == open(pair).read()


@pytest.mark.parametrize('rank', [None, 'global', 'domain'])
@pytest.mark.parametrize('small', [False, True])
def test_db_mode_on_the_protein_search_golden(tmp_path, monkeypatch, rank, small):
    from dctdomain_amd import dct_sim
    qf, dbf = os.path.join(SEARCH, 'query-dct.npz'), os.path.join(SEARCH, 'db-dct.npz')
    q, d = _load(qf), _load(dbf)
    qdom, ddom = str(tmp_path / 'q.dom'), str(tmp_path / 'db.dom')
    qnames = rule.labels(q[1], _write_dom(qdom, q[0], q[1], 1), q[0])
    dnames = rule.labels(d[1], _write_dom(ddom, d[0], d[1], 2), d[0])
    base = ['--dct', qf, '--db', dbf, '--top', '7', '--threshold', '0.3'] + (['--rank', rank] if rank else [])
    flagless = _main(tmp_path, base)
    assert len(flagless) > 1 + 7 * 27
    if small:                                                   # several database groups and query chunks: nothing stays resident
        monkeypatch.setattr(dct_sim.ProteinSearch, 'COL_ROWS', 11)
        monkeypatch.setattr(dct_sim.ProteinSearch, 'TILE_INTS', 50)
        assert _main(tmp_path, base) == flagless
    for extra, na, nb in ((['--domains'], rule.labels(q[1]), rule.labels(d[1])), (['--db-dom', ddom], rule.labels(q[1]), dnames),
                          (['--dom', qdom], qnames, rule.labels(d[1])), (['--dom', qdom, '--db-dom', ddom], qnames, dnames)):
        got = _main(tmp_path, base + extra)
        assert got == _expect(flagless, *q, na, *d, nb), extra
        assert _four_fields(got) == flagless
    assert sum('whole' in x for x in got[1:]) > 0
    # every database protein printed for every query: the pairs without a domain pair are among the lines
    base[base.index('--top') + 1] = '197'
    flagless = _main(tmp_path, base)
    got = _main(tmp_path, base + ['--db-dom', ddom])
    assert len(got) == 1 + 28 * 197 and got == _expect(flagless, *q, rule.labels(q[1]), *d, dnames)
    assert sum(x.endswith(' - -') for x in got[1:]) > 100


_CUTS = [(0.5, None), (None, 0.25), (0.25, 0.1), (0.9, 0.5), (None, None), (0.0, None), (1.0001, None)]


def _cut_args(min_domain, min_global):
    return ([] if min_domain is None else ['--min-domain', str(min_domain)]) + ([] if min_global is None else ['--min-global', str(min_global)])


@pytest.mark.parametrize('small', [False, True])
def test_all_against_all_on_the_all_sim_golden(tmp_path, monkeypatch, small):
    from dctdomain_amd import dct_sim
    sid, idx, dct = _load(ALL_NPZ)
    dom = str(tmp_path / 'all.dom')
    named = rule.labels(idx, _write_dom(dom, sid, idx, 3), sid)
    flagless = {c: _main(tmp_path, ['--dct', ALL_NPZ] + _cut_args(*c)) for c in _CUTS}
    assert len(flagless[(None, None)]) == 1 + 9591 and flagless[(0.0, None)] == flagless[(None, None)] and len(flagless[(1.0001, None)]) == 1
    assert 1 < len(flagless[(0.9, 0.5)]) < len(flagless[(0.5, None)]) < 9591
    if small:                                                   # single-row stripes, column groups, split ranges, the file not resident
        monkeypatch.setattr(dct_sim.FilteredPairs, 'TEXT_BYTES', 2000)
        monkeypatch.setattr(dct_sim.FilteredPairs, 'COL_ROWS', 7)
        monkeypatch.setattr(dct_sim.FilteredPairs, 'TILE_INTS', 300)
        f = dct_sim.FilteredPairs(sid, idx, dct, min_domain=0.5, labels=named)
        assert f.resident_rows() is None and len(list(f.stripes())) > 20

    def refuse(*a, **k):
        raise AssertionError('--domains composes its lines through FilteredPairs')
    monkeypatch.setattr(dct_sim.AllPairs, 'write', refuse)
    for c in _CUTS:
        for extra, names in ((['--domains'], rule.labels(idx)), (['--dom', dom], named)):
            got = _main(tmp_path, ['--dct', ALL_NPZ] + _cut_args(*c) + extra)
            assert got == _expect(flagless[c], sid, idx, dct, names, sid, idx, dct, names), (c, extra)
            assert _four_fields(got) == flagless[c]
    got = _main(tmp_path, ['--dct', ALL_NPZ, '--dom', dom])
    assert sum(x.endswith(' - -') for x in got[1:]) == 1110 and sum(x.endswith(' whole whole') for x in got[1:]) > 100


def test_filtered_pairs_yield_the_arguments(monkeypatch):
    from dctdomain_amd import dct_sim
    sid, idx, dct = _load(ALL_NPZ)
    i, j, mn, last, arg_i, arg_j = rule.triangle_args(dct, idx)
    for small in (False, True):
        if small:
            monkeypatch.setattr(dct_sim.FilteredPairs, 'COL_ROWS', 7)
            monkeypatch.setattr(dct_sim.FilteredPairs, 'TILE_INTS', 300)
        for kw in ({'min_domain': 0.5}, {'min_global': 0.25}, {'min_domain': 0.5, 'min_global': 0.1}, {}):
            keep = np.ones(len(i), dtype=bool)
            if 'min_domain' in kw:
                keep &= np.minimum(mn, 17000) <= dct_sim.sim_bound(kw['min_domain'])
            if 'min_global' in kw:
                keep &= np.minimum(last, 17000) <= dct_sim.sim_bound(kw['min_global'])
            got = dct_sim.FilteredPairs(sid, idx, dct, labels=rule.labels(idx), **kw).pairs()
            assert len(got) == 6
            for g, w in zip(got, (i, j, mn, last, arg_i, arg_j)):
                assert np.array_equal(g, w[keep]), (small, kw)
            assert len(dct_sim.FilteredPairs(sid, idx, dct, **kw).pairs()) == 4


def test_ragged_file_with_empty_proteins_and_other_ids(tmp_path, monkeypatch):
    """Proteins without fingerprints (no .dom line, '-' in every pair), non-ASCII ids, a .dom with k names for some proteins."""
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(9)
    n = 40
    counts = rng.integers(0, 5, size=n)
    counts[rng.random(n) < 0.2] = 0
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    fam = rng.integers(-60, 61, size=(3, 480))
    dct = np.clip(fam[rng.integers(0, 3, size=int(idx[-1]))] + rng.integers(-20, 21, size=(int(idx[-1]), 480)), -127, 127).astype(np.int8)
    dct[3] = dct[0]
    sid = [f'{"蛋é|"[k % 3]}id{k}' for k in range(n)]
    path, dom = str(tmp_path / 'r-dct.npz'), str(tmp_path / 'r.dom')
    np.savez(path, sid=np.array(sid), idx=idx, dom=np.array(['1-9'] * len(dct)), dct=dct)
    named = rule.labels(idx, _write_dom(dom, sid, idx, 4), sid)
    for small in (False, True):
        if small:
            monkeypatch.setattr(dct_sim.FilteredPairs, 'TEXT_BYTES', 300)
            monkeypatch.setattr(dct_sim.FilteredPairs, 'COL_ROWS', 3)
            monkeypatch.setattr(dct_sim.FilteredPairs, 'TILE_INTS', 50)
        for cut in ([], ['--min-domain', '0.5'], ['--min-global', '0.3']):
            flagless = _main(tmp_path, ['--dct', path] + cut)
            got = _main(tmp_path, ['--dct', path, '--dom', dom] + cut)
            assert got == _expect(flagless, sid, idx, dct, named, sid, idx, dct, named), (small, cut)
    assert len(flagless) > 1
    # a protein with fingerprints that the .dom file does not name
    with open(dom, encoding='utf8') as fh:
        lines = fh.readlines()
    with open(dom, 'w', encoding='utf8') as fh:
        fh.writelines(lines[1:])
    with pytest.raises(ValueError, match=re.escape(lines[0].split(' ')[0])):
        _main(tmp_path, ['--dct', path, '--dom', dom])
