"""query_db's GPU path against the plain CPU reference of tests/query_reference.py (not against other GPU kernels): the fused
k-nearest kernel (dctfp_l1_knn) at the k, widths, tiles, slice counts, col0 and layouts where it can go wrong, the ranking and
line kernels called directly, and QuerySearch on every route, up to the production shape where knn='auto' takes the fused
kernel."""

import time

import numpy as np
import pytest

from query_reference import ref_knn, ref_lines, score_text

pytestmark = pytest.mark.gpu

D480 = 480


def _ctx():
    from dctdomain_amd import _lib
    return _lib.get_context(0)


def _knn(q, b, k, col0=0):
    """l1_knn's (dist, idx) as int64 numpy, the slices of its last dctfp_l1_knn call and how many calls it made."""
    from dctdomain_amd.similarity import l1_knn
    ctx = _ctx()
    calls = ctx.get_option('knn_calls')
    v, i = l1_knn(q, b, k, col0)
    return v, i, ctx.get_option('last_knn_slices'), ctx.get_option('knn_calls') - calls


def _host(x):
    import torch
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _check(q, b, k, ref=None, col0=0, slices=None, msg=''):
    """l1_knn(q, b, k, col0) == the reference (``ref``: ref_knn of at least k columns, a prefix of which is the answer)."""
    rd, ri = ref if ref is not None else ref_knn(_host(q), _host(b), k)
    kk = min(k, _host(b).shape[0])
    v, i, s, calls = _knn(q, b, k, col0)
    np.testing.assert_array_equal(v, rd[:, :kk], err_msg=msg)
    np.testing.assert_array_equal(i, ri[:, :kk] + col0, err_msg=msg)
    if slices is not None:
        assert s == slices, f'{msg}: {s} slices, meant {slices}'
    return calls


def _falling_db(nb, d, rng, dup=0.1):
    """Database rows whose first half sums to P_c and second half to -P_c, P_c strictly falling along the columns: the zero
    query row sees every column closer than all before it (each enters the list: the ring overflows on every tile), a
    constant -128 or 127 row sees all columns at one distance (pure ties).  The last ``dup`` of the rows repeat earlier ones."""
    h = d // 2
    cap = h * 127
    assert nb <= cap, (nb, d)
    p = (np.arange(nb)[::-1] + 1) * (cap // nb)
    b = np.zeros((nb, d), np.int16)
    full, rest = p // 127, p % 127
    cols = np.arange(h)
    b[:, :h] = np.where(cols < full[:, None], 127, np.where(cols == full[:, None], rest[:, None], 0))
    b[:, h:2 * h] = -b[:, :h]
    b = b.astype(np.int8)
    n_dup = int(nb * dup)
    if n_dup:
        src = rng.integers(0, nb - n_dup, n_dup)
        b[nb - n_dup:] = b[src]
    return b


def _tile_queries(b, nq, rng):
    """Query rows that behave differently within one 128-row tile: zero (falling distances), constant -128 and 127 (pure
    ties), a copy of a database row (distance 0, and a tie with its duplicate), a random row."""
    d = b.shape[1]
    q = np.zeros((nq, d), np.int8)
    for r in range(nq):
        kind = (r * 7 + r // 128) % 5
        if kind == 1:
            q[r] = -128
        elif kind == 2:
            q[r] = b[rng.integers(0, b.shape[0])]
        elif kind == 3:
            q[r] = rng.integers(-128, 128, d)
        elif kind == 4:
            q[r] = 127
    if nq > 1:                                                        # a duplicated database row: the lower one must win
        q[nq - 1] = b[-1]
    return q


# ---- dctfp_l1_knn against ref_knn

def test_l1_knn_k_and_tiles():
    """k around the 32-slot ring and the 64-lane wave, k = nb and k > nb, and query sets of 1 ... 300 rows, all against one
    exact reference (the k nearest are a prefix of the full order)."""
    rng = np.random.default_rng(20)
    nb = 1100
    b = _falling_db(nb, D480, rng)
    q = _tile_queries(b, 300, rng)
    ref = ref_knn(q, b, nb)
    assert (ref[0][np.all(q == -128, axis=1)] == 128 * D480).all()   # (the pure-tie rows are what they claim to be)
    for nq in (1, 127, 128, 129, 300):
        for k in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024):
            _check(q[:nq], b, k, ref=(ref[0][:nq], ref[1][:nq]), slices=1, msg=f'nq {nq}, k {k}')
    small = b[:500]
    ref = ref_knn(q, small, 500)
    for k in (500, 507):                                              # k = nb and k > nb: every column, k_eff = nb
        _check(q, small, k, ref=ref, slices=1, msg=f'500 columns, k {k}')


@pytest.mark.parametrize('d', [1, 2, 15, 16, 17, 127, 128, 129, 440, 480, 496, 510, 512, 513])
def test_l1_knn_widths(d):
    """Every width class: only the 1..15-byte tail (d < 16), whole 16-byte groups, a tail behind them, chunk edges, the
    512-byte limit, and 513 (the l1_matrix fallback, no dctfp_l1_knn call).  -128 against 127 gives 255 d."""
    rng = np.random.default_rng(21 + d)
    nb = 700
    if d >= 16:
        b = _falling_db(nb, d, rng)
    else:                                                             # (too narrow to balance: few levels, many ties)
        b = rng.integers(-2, 3, size=(nb, d)).astype(np.int8)
        b[nb // 2:] = b[:nb - nb // 2]
    q = _tile_queries(b, 129, rng)
    ref = ref_knn(q, b, nb)
    for k in (1, 33, 129, 1024):
        calls = _check(q, b, k, ref=ref, msg=f'd {d}, k {k}')
        assert calls == (0 if d > 512 else 1), (d, k, calls)
    bx = np.stack([np.full(d, 127), np.full(d, -128), np.full(d, 127), np.zeros(d)]).astype(np.int8)
    qx = np.stack([np.full(d, -128), np.full(d, 127)]).astype(np.int8)
    ref = ref_knn(qx, bx, 4)
    assert ref[0][0].tolist() == [0, 128 * d, 255 * d, 255 * d] and ref[1][0].tolist() == [1, 3, 0, 2]
    _check(qx, bx, 4, ref=ref, msg=f'd {d}, extreme bytes')


def _random_db(nb, d, rng):
    return rng.integers(-128, 128, size=(nb, d), dtype=np.int8)


def _sliced_case(nb, rng, nq=3):
    """Random rows (L1 ~ 41 000 +- 1 300: many equal distances among tens of thousands of columns), with rows repeated at the
    far end of the database and queries equal to them: distance-0 ties across slices, the lower row first."""
    b = _random_db(nb, D480, rng)
    for src, dst in ((0, nb - 1), (1, nb // 2), (2, nb // 2 + 1), (1, nb - 2)):
        b[dst] = b[src]
    q = np.concatenate([b[:2], _random_db(nq - 2, D480, rng)])
    return q, b


@pytest.mark.parametrize('nb,slices', [(10000, 1), (16384, 2), (24576, 3), (32768, 4), (40960, 5), (57344, 7),
                                       (4160 * 128 + 1, 65), (4160 * 128 + 77, 65)])
def test_l1_knn_slices_and_merge_tree(nb, slices):
    """One slice (no merge), even and odd slice counts (an unpaired list at some merge level), and 65 slices whose last owns 1
    or 77 columns: seven merge levels of 65 -> 33 -> 17 -> 9 -> 5 -> 3 -> 2 -> 1 lists."""
    rng = np.random.default_rng(nb)
    q, b = _sliced_case(nb, rng)
    ks = (1, 64, 100) if slices < 65 else (1, 129, 512)
    ref = ref_knn(q, b, max(ks))
    for k in ks:
        _check(q, b, k, ref=ref, slices=slices, msg=f'{nb} columns, k {k}')


def test_l1_knn_col0_one_and_several_slices():
    """col0 is added at two sites: the one-slice output of l1_knn_kernel and the last merge.  Up to nb + col0 = 2^31 - 1;
    one past that is DCTFP_ERR_LIMIT."""
    import torch
    from dctdomain_amd import _lib
    rng = np.random.default_rng(22)
    ctx = _ctx()
    for nb, slices in ((1100, 1), (24576, 3)):
        q, b = _sliced_case(nb, rng, nq=5)
        ref = ref_knn(q, b, 100)
        for col0 in (0, 123456789, (1 << 31) - 1 - nb):
            _check(q, b, 100, ref=ref, col0=col0, slices=slices, msg=f'{nb} columns, col0 {col0}')
        tq, tb = torch.from_numpy(q).cuda(), torch.from_numpy(b).cuda()
        out = torch.full((5, 100), -3, dtype=torch.int32, device='cuda')
        rc = ctx._lib.dctfp_l1_knn(ctx.handle, tq.data_ptr(), 5, D480, tb.data_ptr(), nb, D480, D480, 100, (1 << 31) - nb,
                                   out.data_ptr(), out.data_ptr(), None)
        assert rc == _lib.DCTFP_ERR_LIMIT
        assert (out.cpu().numpy() == -3).all()


def test_l1_knn_strided_and_unaligned_layouts():
    """Row strides above the width (read in place), and rows that do not start on 16-byte boundaries (copied by _rows16)."""
    import torch
    rng = np.random.default_rng(23)
    b = _falling_db(900, D480, rng)
    q = _tile_queries(b, 130, rng)
    ref = ref_knn(q, b, 200)
    for ld, off in ((512, 0), (528, 16), (500, 0), (512, 3), (481, 1)):
        wq = torch.zeros((130, ld + off), dtype=torch.int8, device='cuda')
        wb = torch.zeros((900, ld + off), dtype=torch.int8, device='cuda')
        wq[:, off:off + D480] = torch.from_numpy(q)
        wb[:, off:off + D480] = torch.from_numpy(b)
        for k in (1, 65, 200):
            _check(wq[:, off:off + D480], wb[:, off:off + D480], k, ref=ref, slices=1, msg=f'ld {ld}, offset {off}, k {k}')


def test_l1_knn_query_chunks():
    """k = 1024: l1_knn_device's step is 65 536 query rows, so 65 836 rows take two dctfp_l1_knn calls."""
    rng = np.random.default_rng(24)
    b = rng.integers(-3, 4, size=(1030, 16), dtype=np.int8)
    q = rng.integers(-3, 4, size=(65536 + 300, 16), dtype=np.int8)
    q[65530:65540] = b[:10]
    assert _check(q, b, 1024, slices=1, msg='two query chunks') == 2


# ---- dctfp_query_rank and dctfp_query_lines, called directly

def _dev(a, dtype):
    import torch
    return torch.as_tensor(np.array(a, dtype=dtype), device='cuda')


@pytest.mark.parametrize('k', [128, 1])
def test_query_rank_kernel_against_stable_sort(k):
    """Sorted per-row lists with heavy ties across a protein's fingerprints; proteins of 1 ... 128 fingerprints (f k up to
    RANK_CAP at k = 128), some left to the host (prot_of_row = -1, interleaved): the kernel writes numpy's stable order of the
    protein's (f, k) block at line_base[p] + rank and nothing in the host proteins' slots."""
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.query_db import QuerySearch
    rng = np.random.default_rng(25 + k)
    f = np.array([1, 128, 3, 1, 5, 2, 17, 128, 1, 4] if k > 1 else [1, 128, 3, 1, 5, 2, 17, 300, 1, 4])
    host = np.array([0, 0, 1, 0, 0, 1, 0, 1, 0, 1], bool)
    n_rows = int(f.sum())
    val = np.sort(rng.integers(0, 4, size=(n_rows, k)) * 11, axis=1).astype(np.int32)
    val[:3] = 0                                                       # (whole lists equal)
    idx = rng.permutation(n_rows * k).reshape(n_rows, k).astype(np.int32)
    qoff = np.zeros(len(f) + 1, np.int64)
    np.cumsum(f, out=qoff[1:])
    prot_of_row = np.repeat(np.where(host, -1, np.arange(len(f))), f).astype(np.int32)
    assert k != 128 or f.max() * k == QuerySearch.RANK_CAP
    ctx = _ctx()
    for khits in (1, 100, int(f.max()) * k, int(f.max()) * k + 5):
        n_lines = np.minimum(khits, f * k)
        base = np.zeros(len(f) + 1, np.int64)
        np.cumsum(n_lines, out=base[1:])
        total = int(base[-1])
        outs = [torch.full((total,), -77, dtype=torch.int32, device='cuda') for _ in range(3)]
        dv, di, dq, dp, db = _dev(val, np.int32), _dev(idx, np.int32), _dev(qoff, np.int64), _dev(prot_of_row, np.int32), _dev(base, np.int64)
        _lib.check(ctx._lib.dctfp_query_rank(ctx.handle, dv.data_ptr(), di.data_ptr(), n_rows, k, dq.data_ptr(), dp.data_ptr(),
                                             db.data_ptr(), int(khits), *(o.data_ptr() for o in outs), None))
        torch.cuda.synchronize()
        got = np.stack([o.cpu().numpy() for o in outs])
        exp = np.full((3, total), -77, np.int64)
        for p in np.flatnonzero(~host):
            blk = val[qoff[p]:qoff[p + 1]].ravel()
            sel = np.argsort(blk, kind='stable')[:khits]
            ii, jj = np.divmod(sel, k)
            at = slice(base[p], base[p] + len(sel))
            exp[0, at] = qoff[p] + ii
            exp[1, at] = idx[qoff[p] + ii, jj]
            exp[2, at] = val[qoff[p] + ii, jj]
        np.testing.assert_array_equal(got, exp, err_msg=f'k {k}, khits {khits}')


def _string_table(strs):
    enc = [s.encode('utf8') for s in strs]
    off = np.zeros(len(enc) + 1, np.int64)
    np.cumsum([len(e) for e in enc], out=off[1:])
    return b''.join(enc), off


@pytest.mark.parametrize('width', [1, 480, 512])
def test_query_lines_kernel_against_fstrings(width):
    """Empty pids and domains, 2-, 3- and 4-byte UTF-8, ranks of 1 to 10 digits, distance 0 and 255 d (both ends of the score
    table), line counts that are not a multiple of 256, and runs whose line offsets start inside the buffer."""
    import torch
    from dctdomain_amd import _lib
    from dctdomain_amd.query_db import score_table
    rng = np.random.default_rng(26 + width)
    qp = ['', 'q1', 'é', 'ß€', '𝄞x', 'Q' * 70]
    qd = ['1-50', '', 'λ-λ', '€', '1-9,20-𝄞', '']
    dp = ['d0', '', '€€€', '𝄞', 'é' * 9, 'db5', 'x']
    dd = ['', '1-1', '2-200', 'ü', '𝄞𝄞', '5-6,8-9', '']
    q_txt, q_off = _string_table(qp + qd)
    d_txt, d_off = _string_table(dp + dd)
    score_txt, score_off = score_table(width)
    top = 255 * width
    ctx = _ctx()
    for n in (1, 255, 257, 300):
        qrow = rng.integers(0, len(qp), n)
        drow = rng.integers(0, len(dp), n)
        dist = rng.integers(0, top + 1, n)
        dist[0] = 0
        dist[-1] = top
        rank = 10 ** rng.integers(0, 10, n) + rng.integers(0, 10, n)
        rank[0] = 1
        rank[-1] = 2147483647
        lines = [f'Query: {qp[a]} {qd[a]}, Result {r}: {dp[c]} {dd[c]}, Similarity: {score_text(x)}\n'.encode('utf8')
                 for a, c, x, r in zip(qrow, drow, dist, rank)]
        off = np.zeros(n + 1, np.int64)
        np.cumsum([len(x) for x in lines], out=off[1:])
        cols = [_dev(x, np.int32) for x in (qrow, drow, dist, rank)]
        strs = [_dev(np.frombuffer(q_txt, np.uint8), np.uint8), _dev(q_off[:len(qp) + 1], np.int64),
                _dev(q_off[len(qp):], np.int64), _dev(np.frombuffer(d_txt, np.uint8), np.uint8), _dev(d_off[:len(dp) + 1], np.int64),
                _dev(d_off[len(dp):], np.int64), _dev(np.frombuffer(score_txt, np.uint8), np.uint8), _dev(score_off, np.int64)]
        for a, start in ((0, 0), (n // 3, 37)):                      # lines a ... n, written from byte `start`
            out = torch.full((int(off[n] - off[a]) + start + 64,), 0xEE, dtype=torch.uint8, device='cuda')
            rel = _dev(off[a:] - off[a] + start, np.int64)
            _lib.check(ctx._lib.dctfp_query_lines(ctx.handle, n - a, *(c[a:].data_ptr() for c in cols), *(s.data_ptr() for s in strs),
                                                  rel.data_ptr(), out.data_ptr(), None))
            torch.cuda.synchronize()
            got = out.cpu().numpy().tobytes()
            assert got[:start] == b'\xee' * start and got[len(got) - 64:] == b'\xee' * 64
            assert got[start:len(got) - 64] == b''.join(lines[a:]), (width, n, a)


# ---- QuerySearch against ref_lines

def _table(pids, doms, fps):
    from dctdomain_amd.query_db import Table
    return Table(list(pids), list(doms), np.ascontiguousarray(fps, dtype=np.int8))


def _tables(rng, n_prot_q, n_prot_d, d=D480, levels=3, fmax=5):
    def one(n_prot, tag):
        pids, doms, rows = [], [], []
        for p in range(n_prot):
            f = int(rng.integers(1, fmax + 1))
            for j in range(f):
                pids.append(f'{tag}{p}' if p % 4 else f'{tag}-é{p}')
                doms.append(f'{j + 1}-{j + 40},{j + 60}-{j + 90}' if j % 2 else f'1-{j + 50}')
                rows.append(rng.integers(0, levels, size=d))
        order = rng.permutation(len(pids))                          # a protein's rows need not be adjacent in the table
        return [pids[i] for i in order], [doms[i] for i in order], np.array(rows)[order]
    return one(n_prot_q, 'q'), one(n_prot_d, 'd')


def _run(qt, dt, khits, **kw):
    from dctdomain_amd.query_db import QuerySearch
    out = []
    init = {x: kw.pop(x) for x in ('block_rows', 'device_budget', 'knn') if x in kw}
    kw.setdefault('text_bytes', 1 << 20)
    QuerySearch(dt, **init).search(qt, khits, out.append, **kw)
    return b''.join(out)


def _max_fk(qt, k):
    return int(np.bincount(qt.pid_code).max()) * k


def test_query_search_routes_against_reference():
    """knn auto / fused / matrix; a resident database and one streamed in blocks, with duplicated rows straddling the block
    boundaries (the lower row wins across blocks); rank_cap at f k - 1, f k, f k + 1 of the largest protein; batches smaller
    than one protein; a text buffer of exactly the longest line, and the ValueError one byte below it."""
    rng = np.random.default_rng(30)
    (qp, qd, qf), (dp, dd, df) = _tables(rng, 24, 160, fmax=6)
    for blk in (37, 64, 128):                                         # equal rows on both sides of every block boundary
        for c in range(blk, len(dp), blk):
            df[c] = df[c - 1]
    qf[:6] = df[[36, 37, 63, 64, 127, 128]]                           # ... and queries that hit them at distance 0
    qt, dt = _table(qp, qd, qf), _table(dp, dd, df)
    khits = 40
    exp = ref_lines(qt, dt, khits)
    longest = max(len(x) + 1 for x in exp.split(b'\n')[:-1])
    fk = _max_fk(qt, khits)
    for knn in ('auto', 'fused', 'matrix'):
        assert _run(qt, dt, khits, knn=knn) == exp, knn
        for blk in (37, 64, 128):
            assert _run(qt, dt, khits, knn=knn, block_rows=blk, device_budget=0) == exp, (knn, blk)
        assert _run(qt, dt, khits, knn=knn, block_rows=64) == exp, knn
        for cap in (fk - 1, fk, fk + 1):
            assert _run(qt, dt, khits, knn=knn, rank_cap=cap) == exp, (knn, cap)
        assert _run(qt, dt, khits, knn=knn, batch_rows=2, block_rows=37, device_budget=0, rank_cap=fk - 1) == exp, knn
        assert _run(qt, dt, khits, knn=knn, text_bytes=longest) == exp, knn
        with pytest.raises(ValueError):
            _run(qt, dt, khits, knn=knn, text_bytes=longest - 1)


@pytest.mark.parametrize('d', [440, 480, 510])
def test_query_search_small_databases_and_shared_rows(d):
    """khits above the database size, a one-row database, and a query table that shares rows (and pids) with the database."""
    rng = np.random.default_rng(31 + d)
    (qp, qd, qf), (dp, dd, df) = _tables(rng, 10, 40, d=d, levels=4)
    n = min(len(qf[::2]), len(df))
    qf[::2][:n] = df[:n]
    qp[1] = dp[0]
    qt, dt = _table(qp, qd, qf), _table(dp, dd, df)
    for knn in ('auto', 'fused', 'matrix'):
        for khits in (1, 7, 100, 1000):
            assert _run(qt, dt, khits, knn=knn) == ref_lines(qt, dt, khits), (knn, khits)
        small = _table(dp[:7], dd[:7], df[:7])
        assert _run(qt, small, 50, knn=knn, block_rows=3, device_budget=0) == ref_lines(qt, small, 50), knn
        one = _table(dp[:1], dd[:1], df[:1])
        assert _run(qt, one, 5, knn=knn) == ref_lines(qt, one, 5), knn


# ---- the production route at its own shape

def _fast_table(pids_of_row, pid_names, doms, fps):
    """A query_db.Table of millions of rows without a Python string per row: ``pids_of_row`` = index into the sorted
    ``pid_names``; ``doms`` = one domain string per row (short ASCII)."""
    from dctdomain_amd.query_db import Table
    t = Table.__new__(Table)
    enc = np.array([p.encode() for p in pid_names], dtype=object)
    plen = np.fromiter((len(e) for e in enc), np.int64, len(enc))
    t.n = len(pids_of_row)
    t.fps = fps
    t.pid = b''.join(enc[pids_of_row])
    t.pid_off = np.zeros(t.n + 1, np.int64)
    np.cumsum(plen[pids_of_row], out=t.pid_off[1:])
    t.dom = ''.join(doms).encode()
    t.dom_off = np.zeros(t.n + 1, np.int64)
    np.cumsum(np.fromiter(map(len, doms), np.int64, t.n), out=t.dom_off[1:])
    t.pids = list(pid_names)
    t.pid_code = np.asarray(pids_of_row, np.int64)
    return t


def _subtable(t, rows):
    from dctdomain_amd.query_db import Table
    text = lambda txt, off, r: txt[off[r]:off[r + 1]].decode('utf8')
    return Table([text(t.pid, t.pid_off, r) for r in rows], [text(t.dom, t.dom_off, r) for r in rows], np.ascontiguousarray(t.fps[rows]))


def test_query_search_production_shape_fused_route():
    """16 384 query fingerprints against 2 200 000 database rows of 480 bytes, khits = 100, knn='auto': the fused kernel.  The
    answer for a sample of query proteins is planted: 120 perturbed copies of each of their fingerprints at L1 < 3 000 (random
    rows lie at 41 000 +- 1 300), spread over every database slice and both sides of the slice boundaries, with duplicated
    copies in different slices.  ref_lines over the planted rows alone must equal QuerySearch's lines for those proteins;
    a few unplanted rows are checked by brute force."""
    from dctdomain_amd.query_db import knn_route
    t0 = time.time()
    rng = np.random.default_rng(40)
    nq, nb, khits = 16384, 2_200_000, 100
    db = np.frombuffer(rng.bytes(nb * D480), np.int8).reshape(nb, D480).copy()
    qf = np.frombuffer(rng.bytes(nq * D480), np.int8).reshape(nq, D480).copy()
    f = np.full(nq // 4, 4)                                          # 4 096 proteins of 2 ... 6 fingerprints
    f[::3] = 2
    f[1::3] = 6
    f = f[:np.searchsorted(np.cumsum(f), nq, side='right')]
    f[-1] += nq - f.sum()
    qoff = np.concatenate([[0], np.cumsum(f)])
    n_prot = len(f)
    names = [f'Q{p:05d}' for p in range(n_prot)]                     # sorted = table order: query row r = batch row r
    q_of_row = np.repeat(np.arange(n_prot), f)
    qt = _fast_table(q_of_row, names, [f'{r % 7 + 1}-{r % 300 + 40}' for r in range(nq)], qf)
    assert knn_route(nq, nb, khits)

    # planted proteins: those owning rows at both ends of 128-row tiles, the first and the last, and a few more
    tile_rows = [0, 127, 128, 255, 256, 8191, 8192, 16255, 16256, nq - 1]
    sample = sorted(set(int(np.searchsorted(qoff, r, side='right')) - 1 for r in tile_rows) | {1, 500, 2000, 3333})
    prow = np.concatenate([np.arange(qoff[p], qoff[p + 1]) for p in sample])
    n_copy = khits + 20
    blocks = (nb + 127) // 128
    slice_cols = (blocks + 3) // 4 * 128                              # knn_slices: 4 slices at this shape
    bounds = [slice_cols * s for s in range(1, 4)]
    # copy slots: around every slice boundary and scattered everywhere else, no slot twice
    near = np.concatenate([np.arange(b0 - 40, b0 + 40) for b0 in bounds] + [np.arange(0, 20), np.arange(nb - 20, nb)])
    spread = rng.choice(np.setdiff1d(np.arange(nb), near), len(prow) * n_copy - len(near), replace=False)
    slots = rng.permutation(np.concatenate([near, spread])).reshape(len(prow), n_copy)
    for j, r in enumerate(prow):
        pert = np.zeros((n_copy, D480), np.int16)
        amount = rng.integers(0, 2900, n_copy)
        amount[:6] = (0, 0, 1, 1, 500, 500)                           # equal distances in different slots (slices)
        for c in range(n_copy):
            cols = rng.choice(D480, 200, replace=False)
            per = np.full(200, amount[c] // 200)
            per[:amount[c] % 200] += 1
            sign = np.where(qf[r, cols] >= 0, -1, 1)                  # towards zero: no clipping, |change| = amount
            pert[c, cols] = sign * per
        db[slots[j]] = (qf[r].astype(np.int16) + pert).astype(np.int8)
    slices_of = np.searchsorted(bounds, slots, side='right')
    assert set(np.unique(slices_of)) == {0, 1, 2, 3}
    assert (slices_of[:, 0] != slices_of[:, 1]).sum() > len(prow) // 2
    dt = _fast_table(np.arange(nb) // 4, [f'D{c:06d}' for c in range((nb + 3) // 4)],
                     ['1-9' if c % 3 else '5-60,70-99' for c in range(nb)], db)
    t_setup = time.time() - t0

    from dctdomain_amd.query_db import QuerySearch
    ctx = _ctx()
    calls = ctx.get_option('knn_calls')
    out = []
    t1 = time.time()
    QuerySearch(dt).search(qt, khits, out.append)
    t_gpu = time.time() - t1
    assert ctx.get_option('knn_calls') - calls == 1 and ctx.get_option('last_knn_slices') == 4
    lines = b''.join(out).split(b'\n')
    assert lines[-1] == b'' and len(lines) - 1 == n_prot * khits    # (f k >= khits: every protein prints khits lines)
    of_prot = lambda ps: b''.join(x + b'\n' for p in ps for x in lines[p * khits:(p + 1) * khits])

    # planted proteins: their lines, from the planted rows alone (every other row is far beyond 3 000)
    planted = np.sort(slots.ravel())
    sub_q = _subtable(qt, prow)
    sub_d = _subtable(dt, planted)
    exp = ref_lines(sub_q, sub_d, khits)
    assert of_prot(sample) == exp
    assert exp.count(b'Similarity: 1.0\n') >= 2 * len(prow) and b'Similarity: 0.9706\n' in exp   # distance 0 twice, 500
    # two unplanted proteins (2 and 6 fingerprints): their k nearest by brute force over the whole database
    others = [p for p in (300, 301) if p not in sample]
    assert sorted(f[others]) == [2, 6]
    orow = np.concatenate([np.arange(qoff[p], qoff[p + 1]) for p in others])
    rd, ri = ref_knn(qf[orow], db, khits)
    hit_rows, ri_sub = np.unique(ri, return_inverse=True)
    exp = ref_lines(_subtable(qt, orow), _subtable(dt, hit_rows), khits, knn=(rd, ri_sub.reshape(ri.shape)))
    assert of_prot(others) == exp
    print(f'setup {t_setup:.1f} s, QuerySearch {t_gpu:.1f} s, checks {time.time() - t1 - t_gpu:.1f} s')
