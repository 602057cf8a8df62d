"""dct-sim --domain-map on the GPU: dctfp_pair_row_best and the two passes of dctfp_pair_map_lines against the double loop of
domain_map_rule.py (pinned on the CPU in test_domain_map_host.py), and every mode of dct_sim.main that prints pair lines against
text built from that rule -- with the fields before the map equal to the same run's with --domains."""

import os

import numpy as np
import pytest

import domain_map_rule as rule
import golden_util as gu

pytestmark = pytest.mark.gpu
FIX = os.path.join(gu.GOLD, 'ref_fixtures')
G6PD, EXAMPLE = os.path.join(FIX, 'G6PD-dct.npz'), os.path.join(FIX, 'example-dct.npz')
COUNTS = (0, 1, 2, 3, 4, 5, 9)                                  # rows per protein: the edges of the unroll of four


def _load(path):
    with np.load(path) as data:
        return [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']


def _files(seed, d):
    """Two different files of width d, one protein of each row count of COUNTS in either, rows drawn from a pool of five
    fingerprints (so most minima are tied, on both sides) with a few rows nudged by one unit (so some are not)."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(-128, 128, size=(5, d)).astype(np.int8)
    out = []
    for order in (COUNTS, COUNTS[::-1]):
        idx = np.concatenate([[0], np.cumsum(order)]).astype(np.int64)
        dct = pool[rng.integers(0, 5, size=int(idx[-1]))].copy()
        for r in rng.choice(len(dct), size=6, replace=False):
            dct[r, rng.integers(0, d)] ^= 1
        out.append((idx, dct))
    return out[0] + out[1]


def _all_pairs(ia, ib):
    return [(i, j) for i in range(len(ia) - 1) for j in range(len(ib) - 1)]


def _tied(a, ia, b, ib, pairs):
    """How many rows, over both sides of all pairs, reach their smallest L1 at more than one row of the other protein."""
    n = 0
    for i, j in pairs:
        p, q = a[ia[i]:ia[i + 1]].astype(np.int64), b[ib[j]:ib[j + 1]].astype(np.int64)
        if len(p) and len(q):
            d = np.abs(p[:, None] - q[None]).sum(2)
            n += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum() + ((d == d.min(0, keepdims=True)).sum(0) > 1).sum())
    return n


# ---- dctfp_pair_row_best

@pytest.mark.parametrize('d', [1, 3, 4, 5, 255, 256, 257, 480, 512, 516, 1000])
def test_pair_row_best_against_the_rule(d):
    import torch
    from dctdomain_amd.similarity import pair_row_best, pair_row_best_device
    ia, a, ib, b = _files(200 + d, d)
    pairs = _all_pairs(ia, ib)
    want = rule.flat(a, ia, b, ib, pairs)
    assert len(pairs) == 49 and want[0][-1] == 2 * 7 * 24 and _tied(a, ia, b, ib, pairs) >= 40
    got = pair_row_best(a, ia, b, ib, pairs)
    for g, w, name in zip(got, want, ('row_off', 'l1', 'arg')):
        assert g.dtype == np.int64 and np.array_equal(g, w), (d, name)
    # rows at a stride above d, base and stride unaligned: the kernel's byte path
    dev = torch.device('cuda')
    views = []
    for m, lead, pad in ((a, 1, 3), (b, 2, 1)):
        ld = d + pad
        flat = torch.zeros(lead + len(m) * ld + 8, dtype=torch.int8, device=dev)
        view = flat[lead:lead + len(m) * ld].view(len(m), ld)[:, :d]
        view.copy_(torch.as_tensor(m, device=dev))
        assert view.data_ptr() & 3 and view.stride(0) == ld > d
        views.append(view)
    tp = torch.as_tensor(np.asarray(pairs, dtype=np.int32), device=dev)
    out = pair_row_best_device(views[0], torch.as_tensor(ia, device=dev), views[1], torch.as_tensor(ib, device=dev), tp)
    assert [t.dtype for t in out] == [torch.int64, torch.int32, torch.int32] and all(t.is_cuda for t in out)
    for g, w, name in zip(out, want, ('row_off', 'l1', 'arg')):
        assert np.array_equal(g.cpu().numpy().astype(np.int64), w), (d, 'strided', name)


def test_pair_row_best_returns_the_raw_l1():
    """Rows of +127 against -128: 255 per byte, 122 400 at d = 480, far above the 17000 at which the scores stop."""
    from dctdomain_amd.similarity import pair_row_best
    hi, lo = np.full((3, 480), 127, dtype=np.int8), np.full((2, 480), -128, dtype=np.int8)
    off, l1, arg = pair_row_best(hi, [0, 3], lo, [0, 2], [(0, 0)])
    assert off.tolist() == [0, 5] and l1.tolist() == [122400] * 5 and arg.tolist() == [0] * 5
    assert rule.row_best(hi, lo) == ([122400] * 3, [0] * 3, [122400] * 2, [0] * 2)


@pytest.mark.parametrize('n', [0, 1, 5])
def test_pair_row_best_any_number_of_pairs(n):
    from dctdomain_amd.similarity import pair_row_best
    ia, a, ib, b = _files(7, 480)
    pairs = [(6, 0), (2, 3), (0, 6), (5, 5), (3, 1)][:n]           # (9 x 9 rows, an empty protein on either side among them)
    got = pair_row_best(a, ia, b, ib, pairs)
    for g, w in zip(got, rule.flat(a, ia, b, ib, pairs)):
        assert np.array_equal(g, w)
    assert len(got[0]) == n + 1


def test_pair_row_best_skips_what_it_cannot_place():
    """A pair index out of range, a row_off range of the wrong width and one that ends beyond out_len write nothing: the rows of
    those pairs, and everything around the output, keep their fill."""
    import torch
    from dctdomain_amd import similarity
    ia, a, ib, b = _files(8, 480)
    dev = torch.device('cuda')
    pairs = [(6, 0), (7, 0), (2, 3), (0, -1), (5, 5), (3, 1), (4, 4)]
    bad = {1, 3}                                                # (out of range: no rows are theirs)
    width = [0 if k in bad else int(ia[i + 1] - ia[i] + ib[j + 1] - ib[j]) for k, (i, j) in enumerate(pairs)]
    width[4] += 1                                               # (pair 4: one entry too many)
    off = np.concatenate([[0], np.cumsum(width)]).astype(np.int64)
    out_len = int(off[-1]) - 1                                  # (pair 6: its range ends one beyond the output)
    fill, room = 0x55555555, int(off[-1]) + 16
    l1 = torch.full((room,), fill, dtype=torch.int32, device=dev)
    arg = torch.full((room,), fill, dtype=torch.int32, device=dev)
    ta, tb = similarity.to_device_int8(a), similarity.to_device_int8(b)
    tp, tia, tib, toff = (torch.as_tensor(v, device=dev) for v in (np.asarray(pairs, dtype=np.int32), ia, ib, off))
    similarity._launch(ta.device, 'dctfp_pair_row_best', tp.data_ptr(), len(pairs), ta.data_ptr(), 480, tia.data_ptr(), len(ia) - 1, tb.data_ptr(), 480,
                       tib.data_ptr(), len(ib) - 1, 480, toff.data_ptr(), out_len, l1.data_ptr(), arg.data_ptr())
    torch.cuda.synchronize()
    l1, arg = l1.cpu().numpy().astype(np.int64), arg.cpu().numpy().astype(np.int64)
    written = 0
    for k, (i, j) in enumerate(pairs):
        got = l1[off[k]:off[k + 1]].tolist(), arg[off[k]:off[k + 1]].tolist()
        if k in bad or k in (4, 6):
            assert got == ([fill] * width[k], [fill] * width[k]), k
        else:
            l1_p, arg_p, l1_q, arg_q = rule.row_best(a[ia[i]:ia[i + 1]], b[ib[j]:ib[j + 1]])
            assert got == (l1_p + l1_q, arg_p + arg_q), k
            written += width[k]
    assert written == 18 + 5 + 8 and (l1[off[-1]:] == fill).all() and (arg[off[-1]:] == fill).all()


def test_pair_row_best_names_the_pair_of_pair_argmin_on_g6pd():
    """All 351 pairs of the fixture: the first-side entry with the smallest L1, ties to the first row, is dctfp_pair_argmin's."""
    from dctdomain_amd.similarity import pair_argmin, pair_row_best
    _, idx, dct = _load(G6PD)
    n = len(idx) - 1
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    off, l1, arg = pair_row_best(dct, idx, dct, idx, pairs)
    for g, w in zip((off, l1, arg), rule.flat(dct, idx, dct, idx, pairs)):
        assert np.array_equal(g, w)
    mn, _, arg_a, arg_b = pair_argmin(dct, idx, dct, idx, pairs)
    assert len(pairs) == 351 and (mn < 17000).all()
    for p, (i, _) in enumerate(pairs):
        side = l1[off[p]:off[p] + idx[i + 1] - idx[i]]
        r = int(np.argmin(side))                                # (the first minimum)
        assert (r, int(arg[off[p] + r]), int(side[r])) == (arg_a[p], arg_b[p], mn[p]), p


def test_domain_map_of_two_fingerprint_sets():
    from dctdomain_amd import dct_sim
    sid, idx, dct = _load(G6PD)
    i, j = sid.index('A0A2K6GTL0'), sid.index('A0A341BUD1')
    p, q = dct[idx[i]:idx[i + 1]], dct[idx[j]:idx[j + 1]]
    for x in (0.5, 0.25, 1e-9, 1):
        assert dct_sim.domain_map(p, q, x) == rule.sides(p, q, rule.bound(x))
    assert dct_sim.domain_map(p, q) == rule.sides(p, q, 12750)
    first, _ = dct_sim.domain_map(p, q, 0.5)
    assert min(first, key=lambda e: e[2])[:2] == dct_sim.best_domain_pair(p, q)[2:] == (1, 1)


# ---- dctfp_pair_map_lines

def _line_case():
    """Proteins of 0, 1 and 9 rows, ids of 1 and of 300 bytes and one that is not ASCII, labels of 1 to 40 bytes; per line hand-made
    row results, so that a side holds 0, 1 or 9 entries whatever the fingerprints would say."""
    rng = np.random.default_rng(21)
    names = ['x', 'N' * 300, 'sp|P1|α蛋', 'q', 'none']
    idx = np.array([0, 1, 10, 19, 20, 20], dtype=np.int64)
    labels = [('%d-%d,' % (7 * r + 1, 7 * r + 5) * 8)[:1 + (r * 41) % 40] for r in range(20)]
    labels[0], labels[9], labels[10] = '1', 'δ' * 20, 'L' * 40
    assert {len(s.encode()) for s in labels} >= {1, 40} and max(len(s.encode()) for s in labels) == 40
    bound = 8500
    lines = []                                                  # (i, j, mn, last, la, lb, l1 of the k + m rows, arg of them)

    def add(i, j, l1, arg):
        lines.append((i, j, int(rng.choice([0, 8500, 16999, 17000, 0x7fffffff])), int(rng.choice([0, 25, 17001])),
                      int(rng.integers(0, 21)), int(rng.integers(0, 21)), l1, arg))

    k = lambda p: int(idx[p + 1] - idx[p])                      # noqa: E731
    for i, j in ((1, 2), (2, 1)):                               # nine entries on both sides; then none; then one on either
        add(i, j, [0] * 18, list(range(9)) + list(range(8, -1, -1)))
        add(i, j, [8501] * 18, [0] * 18)
        add(i, j, [17000] * 4 + [8500] + [0x7fffffff] * 13, [3] * 18)
        add(i, j, [9000] * 17 + [1], [8] * 18)
    add(0, 3, [0, 8500], [0, 0])                                # one row each
    add(0, 4, [0x7fffffff], [-1])                               # a protein without rows: "-/-"
    add(4, 4, [], [])
    add(4, 2, [0x7fffffff] * 9, [-1] * 9)
    for _ in range(150):
        i, j = (int(v) for v in rng.integers(0, 5, size=2))
        rows = k(i) + k(j)
        if k(i) == 0 or k(j) == 0:
            add(i, j, [0x7fffffff] * rows, [-1] * rows)
        else:
            add(i, j, rng.choice([0, 1, 4250, 8500, 8501, 12750, 16999, 17000, 122400], size=rows).tolist(),
                rng.integers(0, k(j), size=k(i)).tolist() + rng.integers(0, k(i), size=k(j)).tolist())
    return names, idx, labels, bound, lines


def test_map_line_kernel_against_the_host_composer():
    import torch
    from dctdomain_amd import dct_sim
    from dctdomain_amd.similarity import LineIds, pair_map_line_lengths, pair_map_lines
    names, idx, labels, bound, lines = _line_case()
    score = dct_sim.score_table()
    five = lambda v: bytes(score[0, v]).decode()                # noqa: E731
    table_labels = labels + ['-']
    want, sides = [], []
    for i, j, mn, last, la, lb, l1, arg in lines:
        ki = int(idx[i + 1] - idx[i])
        first, second = dct_sim.map_entries(l1[:ki], arg[:ki], bound), dct_sim.map_entries(l1[ki:], arg[ki:], bound)
        field = dct_sim.map_field(first, second, labels[idx[i]:idx[i + 1]], labels[idx[j]:idx[j + 1]], five)
        head = f'{names[i]} {names[j]} '.encode('utf8') + bytes(score[0, min(mn, 17001)]) + b' ' + bytes(score[1, min(last, 17001)])
        want.append(head + f' {table_labels[la]} {table_labels[lb]} {field}\n'.encode('utf8'))
        sides.append((len(first), len(second)))
    assert {(9, 9), (0, 0), (1, 0), (0, 1), (1, 1)} <= set(sides) and sum(w.endswith(b' -/-\n') for w in want) >= 10
    assert want[0].count(b';') == 16 and want[0].endswith(b':1.000\n')
    dev = torch.device('cuda')
    ids, tab = LineIds(names), LineIds(table_labels)
    cols = [torch.as_tensor(np.array([ln[c] for ln in lines], dtype=np.int32), device=dev) for c in range(6)]
    row_off = np.concatenate([[0], np.cumsum([len(ln[6]) for ln in lines])]).astype(np.int64)
    l1 = torch.as_tensor(np.array([v for ln in lines for v in ln[6]], dtype=np.int32), device=dev)
    arg = torch.as_tensor(np.array([v for ln in lines for v in ln[7]], dtype=np.int32), device=dev)
    common = (*cols, ids, tab, torch.as_tensor(score, device=dev), torch.as_tensor(idx, device=dev), torch.as_tensor(row_off, device=dev), l1, arg,
              bound)
    # the count pass: every line's length, which sum to the fill's bytes
    count = pair_map_line_lengths(*common)
    assert count.dtype == torch.int64 and count.cpu().tolist() == [len(w) for w in want]
    off = torch.zeros(len(lines) + 1, dtype=torch.int64, device=dev)
    torch.cumsum(count, 0, out=off[1:])
    total = int(off[-1])
    assert total == sum(len(w) for w in want)
    for lead in (0, 3):                                         # (the text's first byte on any alignment)
        buf = torch.full((lead + total + 9,), 0xAB, dtype=torch.uint8, device=dev)
        pair_map_lines(*common, off, buf[lead:lead + total])
        got = buf.cpu().numpy().tobytes()
        assert got[lead:lead + total] == b''.join(want)
        assert set(got[:lead]) <= {0xAB} and set(got[lead + total:]) == {0xAB}
    # an output one byte short of the last line: that line is not written, the rest are intact
    buf = torch.full((total + 4,), 0xAB, dtype=torch.uint8, device=dev)
    pair_map_lines(*common, off, buf[:total - 1])
    got = buf.cpu().numpy().tobytes()
    start = total - len(want[-1])
    assert got[:start] == b''.join(want[:-1]) and set(got[start:]) == {0xAB}
    # lines that name what is not there count 0 bytes and are skipped by the fill: a protein or a label out of range, results that
    # are not the two proteins' rows, a counterpart beyond the other protein
    broken = [c.clone() for c in cols]
    broken[0][1], broken[1][2], broken[4][3], broken[5][5] = 5, -1, 21, -2
    off_bad = torch.as_tensor(row_off, device=dev).clone()
    off_bad[7] += 1                                             # (line 6: one entry too many; line 7: one short)
    arg_bad = arg.clone()
    arg_bad[int(row_off[4])] = 9                                # (line 4, all nine rows matched: row 0 names row 9 of a nine-row protein)
    assert lines[4][6][0] <= bound and lines[4][:2] == (2, 1)
    skipped = {1, 2, 3, 4, 5, 6, 7}
    bad_common = (*broken, *common[6:10], off_bad, l1, arg_bad, bound)
    count = pair_map_line_lengths(*bad_common).cpu().tolist()
    assert count == [0 if n in skipped else len(w) for n, w in enumerate(want)]
    buf = torch.full((total,), 0xAB, dtype=torch.uint8, device=dev)
    pair_map_lines(*bad_common, off, buf)
    got = buf.cpu().numpy().tobytes()
    starts = off.cpu().tolist()
    for n, w in enumerate(want):
        assert got[starts[n]:starts[n + 1]] == (b'\xab' * len(w) if n in skipped else w), n
    with pytest.raises(ValueError):
        pair_map_line_lengths(*common[:-1], 17000)              # (similarity 0 never matches)
    with pytest.raises(ValueError):
        pair_map_lines(*common, off.int(), buf)


# ---- end to end

def _main(tmp_path, argv) -> list:
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    dct_sim.main(argv + ['--output', out])
    with open(out, encoding='utf8') as fh:
        text = fh.read()
    assert text.endswith('\n')
    return text.split('\n')[:-1]


def _with_rule(domain_lines, sid_a, idx_a, dct_a, names_a, sid_b, idx_b, dct_b, names_b, bound, text, z_fields=0):
    """The lines of a --domains run with the rule's field behind ``dom1 dom2`` (before the last ``z_fields`` fields); the proteins of
    a line found by id (unique in the fixtures)."""
    wa, wb = {s: k for k, s in enumerate(sid_a)}, {s: k for k, s in enumerate(sid_b)}
    head = domain_lines[0].split(' ')
    out = [' '.join(head[:6] + ['domain-map'] + head[6:])]
    assert len(head) == 6 + z_fields
    for line in domain_lines[1:]:
        f = line.split(' ')
        assert len(f) == 6 + z_fields
        field = rule.file_field(dct_a, idx_a, names_a, dct_b, idx_b, names_b, wa[f[0]], wb[f[1]], bound, text)
        out.append(' '.join(f[:6] + [field] + f[6:]))
    return out


def test_pair_mode_on_g6pd(tmp_path):
    from dctdomain_amd import dct_sim
    pair = os.path.join(FIX, 'G6PD.pair')
    sid, idx, dct = _load(G6PD)
    with open(os.path.join(FIX, 'G6PD-dctsim.txt'), encoding='utf8') as fh:
        reference = fh.read().split('\n')[:-1]
    named = _main(tmp_path, ['--dct', G6PD, '--pair', pair, '--domains'])
    got = _main(tmp_path, ['--dct', G6PD, '--pair', pair, '--domain-map', '0.5'])
    assert len(got) == 352 and [' '.join(x.split(' ')[:4]) for x in got] == reference
    assert got[0] == dct_sim.DOMAIN_HEADER + ' domain-map'
    assert got == _with_rule(named, sid, idx, dct, None, sid, idx, dct, None, 8500, rule.pair_text)
    # the best pair's entry repeats the line's own sim-domain text
    for line in got[1:]:
        f = line.split(' ')
        assert f'{f[4]}={f[5]}:{f[2]}' in f[6].split('/')[0].split(';')
    # the default X, and a report the mode function opens itself
    out = str(tmp_path / 'lib.txt')
    dct_sim.pair_sim(G6PD, pair, None, out, domain_map=True)
    with open(out, encoding='utf8') as fh:
        assert fh.read().split('\n')[:-1] == _with_rule(named, sid, idx, dct, None, sid, idx, dct, None, 12750, rule.pair_text)


@pytest.mark.parametrize('small', [False, True])
def test_db_and_rbh_modes_on_the_example(tmp_path, monkeypatch, small):
    from dctdomain_amd import dct_sim
    sid, idx, dct = _load(EXAMPLE)
    dom = os.path.join(FIX, 'example.dom')
    names = dct_sim.fingerprint_labels(sid, idx, dct_sim.read_dom_file(dom))
    if small:                                                   # several database groups and query chunks
        monkeypatch.setattr(dct_sim.ProteinSearch, 'COL_ROWS', 9)
        monkeypatch.setattr(dct_sim.ProteinSearch, 'TILE_INTS', 20)
    plain = _main(tmp_path, ['--dct', EXAMPLE, '--db', EXAMPLE, '--rank', 'domain'])
    for base, z in ((['--rank', 'domain', '--zscore'], 1), (['--rbh', '--zscore'], 2), (['--rbh'], 0), (['--top', '8', '--threshold', '2'], 0)):
        base = ['--dct', EXAMPLE, '--db', EXAMPLE] + base
        for extra, labels, x, bound in (([], None, [], 12750), (['--dom', dom, '--db-dom', dom], names, ['0.5'], 8500)):
            named = _main(tmp_path, base + ['--domains'] + extra)
            got = _main(tmp_path, base + extra + ['--domain-map'] + x)
            assert got == _with_rule(named, sid, idx, dct, labels, sid, idx, dct, labels, bound, rule.pair_text, z), (base, extra)
            assert len(got) > 8 and got[0].split(' ')[6] == 'domain-map'
            if z == 1:
                assert [' '.join(x.split(' ')[:4]) for x in got] == plain and got[0].endswith(' domain-map z-domain')
            if z == 2:
                assert got[0].endswith(' domain-map z-query z-db')
    assert len(got) == 1 + 64 and sum(' -/-' in x for x in got) > 20      # (every protein against every protein: most share nothing)


def _all_case(tmp_path, monkeypatch, small):
    from dctdomain_amd import dct_sim
    if small:                                                   # single-row stripes, column groups, split ranges, the file not resident
        monkeypatch.setattr(dct_sim.FilteredPairs, 'TEXT_BYTES', 3000)
        monkeypatch.setattr(dct_sim.FilteredPairs, 'COL_ROWS', 40)
        monkeypatch.setattr(dct_sim.FilteredPairs, 'TILE_INTS', 100)


@pytest.mark.parametrize('small', [False, True])
def test_all_against_all_on_g6pd(tmp_path, monkeypatch, small):
    from dctdomain_amd import dct_sim
    sid, idx, dct = _load(G6PD)
    _all_case(tmp_path, monkeypatch, small)
    writes = []
    compose = dct_sim._PairText.write
    monkeypatch.setattr(dct_sim._PairText, 'write', lambda self, *a: (writes.append(len(a[0])), compose(self, *a))[1])
    if small:                                                   # (several stripes of several rows, each in several ranges)
        job = dct_sim.FilteredPairs(sid, idx, dct, min_domain=0.5, labels=rule.index_names(221)).with_map(8500)
        stripes = list(job.stripes())
        assert job.resident_rows() is None and 5 < len(stripes) < 20
        _main(tmp_path, ['--dct', G6PD, '--min-domain', '0.5', '--domain-map'])
        assert len(writes) > len(stripes)

    def refuse(*a, **k):
        raise AssertionError('--domain-map composes its lines through FilteredPairs')
    monkeypatch.setattr(dct_sim.AllPairs, 'write', refuse)
    for cut, x, bound in ((['--min-domain', '0.5'], [], 8500), (['--min-domain', '0.5'], ['0.25'], 12750), ([], [], 12750),
                          (['--min-global', '0.5'], ['1e-9'], 16999)):
        named = _main(tmp_path, ['--dct', G6PD, '--domains'] + cut)
        got = _main(tmp_path, ['--dct', G6PD, '--domain-map'] + x + cut)
        assert got == _with_rule(named, sid, idx, dct, None, sid, idx, dct, None, bound, rule.all_text), (cut, x)
        assert len(got) > 100
    assert len(got) < 352 == len(_main(tmp_path, ['--dct', G6PD, '--domain-map']))
    # the line of the README, with the ranges of the npz's own dom array as labels
    with np.load(G6PD) as data:
        doms = {}
        for p, s in enumerate(sid):
            doms[s] = [str(v) for v in data['dom'][idx[p]:idx[p + 1] - 1]]
    dom = str(tmp_path / 'g6pd.dom')
    with open(dom, 'w', encoding='utf8') as fh:
        fh.writelines(f'{s} {len(v)} {";".join(v)}\n' for s, v in doms.items())
    got = _main(tmp_path, ['--dct', G6PD, '--min-domain', '0.5', '--domain-map', '--dom', dom])
    line = [x for x in got if x.startswith('A0A2K6GTL0 A0A341BUD1 ')][0].split(' ')
    assert line[2:6] == ['0.884', '0.805', '35-219', '28-211']
    assert line[6].split('/')[0] == '1-34=1-27:0.504;35-219=28-211:0.884;220-407=212-366:0.641;533-781=594-840:0.876;whole=whole:0.805'


@pytest.mark.parametrize('small', [False, True])
def test_the_map_and_the_coverage_agree_on_what_is_matched(tmp_path, monkeypatch, small):
    """--min-coverage 0.8 --cov-unit domains: every printed pair's matched rows reach the coverage's need on both sides."""
    from dctdomain_amd import dct_sim
    sid, idx, dct = _load(G6PD)
    _all_case(tmp_path, monkeypatch, small)
    base = ['--dct', G6PD, '--min-domain', '0.5', '--min-coverage', '0.8', '--cov-unit', 'domains']
    named = _main(tmp_path, base + ['--domains'])
    got = _main(tmp_path, base + ['--domain-map'])
    assert got == _with_rule(named, sid, idx, dct, None, sid, idx, dct, None, 8500, rule.all_text)
    assert 10 < len(got) < len(_main(tmp_path, base[:4] + ['--domain-map']))
    weights = dct_sim.coverage_weights(sid, idx, None, 'domains')
    where = {s: k for k, s in enumerate(sid)}
    for line in got[1:]:
        f = line.split(' ')
        for p, side in zip((where[f[0]], where[f[1]]), f[6].split('/')):
            rows = [int(e.split('=')[0]) - 1 for e in side.split(';')] if side != '-' else []
            w = weights[idx[p]:idx[p + 1]]                      # (the whole-protein row weighs the protein: it stands for all rows)
            assert int(sum(w[r] for r in rows)) >= dct_sim.coverage_need(int(w[-1]), 0.8) > 0, line
