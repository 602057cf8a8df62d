"""Contact top-k (dctfp_contact_topk) and its order (dctfp_contact_sort) on every route and every map layout, entry by entry
against the oracle's selection (oracle.contacts_oracle.top_contacts, the reference's stable sort).

Routes: the experiments library's option topk_kernel -- 0 (one read, two reads, radix select behind each other), 1 (the
radix select alone), 2 (two reads first) -- and the product library through reccut.top_contacts_batch.  The long chain
(2^18 candidate pairs and more: striped over many workgroups on a side stream) runs beside whichever route the short ones
take.

Layouts: contiguous maps, and views base[b, :L, :L] of a (B, W, W) tensor as Batch.embed_parallel hands them over (row
stride W, data pointer b W^2 floats into the tensor) for every W mod 4 and L mod 4; the tensor is pre-filled with 2.0, above
every value of the maps below but the infinities, so that a read past row or column L - 1 which is counted shows in the
answer.  W mod 4 == 0 with L mod 4 != 0 sends the one-read kernel's 16-byte loads across the end of the row's buffer
descriptor; an odd W puts every other map 4 bytes off a 16-byte boundary (its 4-byte loads)."""

import ctypes as C

import numpy as np
import pytest

from oracle import contacts_oracle as co
from recipes_contacts import make_contacts

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

LONG_PAIRS = 1 << 18          # dctfp_contact_topk: a protein with this many candidate pairs or more takes the striped chain
K_BOUNDS = {                  # k on both sides of every limit of the kernels (dctfp.hip / kernels.hip.h)
    'small': (0, 1, 2),
    'topk1 <8> / <16>': (1400, 1401),
    'one-read limit': (3000, 3001),
    'two-read limit': (6144, 6145),
    'sort network 2048': (2048, 2049),
    'sort network 4096': (4096, 4097),
    'sort network 8192': (8192, 8193),
    'sort network 16384 / host order': (16384, 16385),
}


def _cand(L):
    return (L - 5) * (L - 4) // 2 if L >= 6 else 0


def _k_of(L, t):
    return min(max(int(t * L), 0), _cand(L))


def _t_for(k, L):
    """t with int(t * L) == k exactly."""
    t = (k + 0.5) / L if L > 0 else 1.0
    assert L == 0 or int(t * L) == k
    return t


# ------------------------------------------------------------------ the values of a map
def _band(rng, L):
    i, j = np.indices((L, L))
    return np.exp(-np.abs(i - j) / 6.0) * (0.6 + 0.4 * rng.random((L, L)))


def _special(rng, L):
    """+-inf, subnormals, exact 1.0 and mixed +-0.0 among band values."""
    m = _band(rng, L).astype(np.float32)
    u = rng.random((L, L))
    sub = np.float32(1.5e-41) * rng.integers(1, 50, size=(L, L)).astype(np.float32)
    m = np.where(u < 0.04, np.float32(np.inf), m)
    m = np.where((u >= 0.04) & (u < 0.07), np.float32(-np.inf), m)
    m = np.where((u >= 0.07) & (u < 0.15), sub, m)
    m = np.where((u >= 0.15) & (u < 0.20), -sub, m)
    m = np.where((u >= 0.20) & (u < 0.28), np.float32(1.0), m)
    m = np.where((u >= 0.28) & (u < 0.36), np.float32(0.0), m)
    m = np.where((u >= 0.36) & (u < 0.44), np.float32(-0.0), m)
    return m


RECIPES = {
    'blocks': lambda rng, L: make_contacts('blocks', L, int(rng.integers(1 << 30))),
    'interleaved': lambda rng, L: make_contacts('interleaved', L, int(rng.integers(1 << 30))),
    'ties': lambda rng, L: make_contacts('ties', L, int(rng.integers(1 << 30))),
    'sparse': lambda rng, L: make_contacts('sparse', L, int(rng.integers(1 << 30))),
    'flat': lambda rng, L: make_contacts('flat', L, int(rng.integers(1 << 30))),
    'negzero': lambda rng, L: make_contacts('negzero', L, int(rng.integers(1 << 30))),
    'band': _band,
    'seven': lambda rng, L: np.floor(rng.random((L, L)) * 7) / 7,
    'f16': lambda rng, L: torch.from_numpy(_band(rng, L).astype(np.float32)).to(torch.float16).float().numpy(),
    'bf16': lambda rng, L: torch.from_numpy(_band(rng, L).astype(np.float32)).to(torch.bfloat16).float().numpy(),
    'special': _special,
}
NAMES = sorted(RECIPES)


def _map(name, L, seed):
    return np.ascontiguousarray(RECIPES[name](np.random.default_rng(seed), L), dtype=np.float32).reshape(L, L)


def _corpus():
    """Groups of maps that share t: [(t, [(name, map), ...])].  Every k limit on both sides with L of every residue mod 4, at
    lengths where the k is an ordinary share of the candidates (the one-read kernel samples the map), and a few where the
    whole map is in its sample; L = 728 / 729 (short / long); long proteins with k above the two-read limit."""
    plan = []                                                   # (k, L)
    for k in K_BOUNDS['small']:
        plan += [(k, L) for L in range(8)]
    for k, L0 in ((1400, 538), (1401, 538), (1400, 120), (1401, 120), (3000, 700), (3001, 700), (6144, 720), (6145, 720),
                  (2048, 600), (2049, 600), (4096, 650), (4097, 650), (8192, 700), (8193, 700), (16384, 700), (16385, 700)):
        plan += [(k, L0 + r) for r in range(4)]
    plan += [(2000, 728), (2000, 729), (1893, 728), (1895, 729), (3001, 729), (7000, 729), (7001, 730), (6500, 731), (9000, 732)]
    groups = []
    for g, (k, L) in enumerate(plan):
        assert k <= 2 or _cand(L) >= k, (k, L)
        n = 3 if L >= 6 else 1
        maps = [(NAMES[(3 * g + q) % len(NAMES)], None) for q in range(n)]
        maps = [(name, _map(name, L, 1000 * g + q)) for q, (name, _) in enumerate(maps)]
        groups.append((_t_for(k, L), maps))
    return groups


# ------------------------------------------------------------------ the oracle (cached: it dominates the run time)
_ORACLE = {}


def _oracle(key, m, t):
    got = _ORACLE.get(key)
    if got is None:
        got = _ORACLE[key] = co.top_contacts(np.ascontiguousarray(m, dtype=np.float32), t)
    return got


def _assert_same(got, exp, what):
    gi, gj, gv = got
    oi, oj, ov = exp
    np.testing.assert_array_equal(gi, oi, err_msg=what)
    np.testing.assert_array_equal(gj, oj, err_msg=what)
    np.testing.assert_array_equal(np.asarray(gv, np.float32).view(np.uint32), np.asarray(ov, np.float32).view(np.uint32), err_msg=what)


# ------------------------------------------------------------------ the two calls through ctypes, on a given context
def _topk_sorted(ctx, views, t):
    """dctfp_contact_topk then dctfp_contact_sort on ``ctx``; proteins the sort leaves (sorted[p] == 0) ordered on the host as
    reccut.top_contacts_batch orders them.  Returns per protein (i, j, v) as numpy arrays."""
    from dctdomain_amd import _lib
    n = len(views)
    dev = views[0].device
    n_res = np.array([v.shape[0] for v in views], dtype=np.int32)
    counts = np.array([_k_of(int(L), t) for L in n_res], dtype=np.int64)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=offs[1:])
    total = max(int(offs[-1]), 1)
    oi = torch.full((total,), -7, dtype=torch.int32, device=dev)
    oj = torch.full((total,), -7, dtype=torch.int32, device=dev)
    ov = torch.full((total,), -7.0, dtype=torch.float32, device=dev)
    on = torch.zeros(n, dtype=torch.int32, device=dev)
    ptrs = np.array([v.data_ptr() for v in views], dtype=np.uint64)
    lds = np.array([v.stride(0) if v.shape[0] > 1 else max(v.shape[0], 1) for v in views], dtype=np.int64)
    sorted_ = np.ones(n, dtype=np.uint8)
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lib = ctx._lib
    _lib.check(lib.dctfp_contact_topk(ctx.handle, ptrs.ctypes.data, lds.ctypes.data, n_res.ctypes.data, n, float(t), oi.data_ptr(),
                                      oj.data_ptr(), ov.data_ptr(), offs.ctypes.data, on.data_ptr(), sp), lib)
    _lib.check(lib.dctfp_contact_sort(ctx.handle, ptrs.ctypes.data, lds.ctypes.data, n_res.ctypes.data, n, float(t), oi.data_ptr(),
                                      oj.data_ptr(), ov.data_ptr(), offs.ctypes.data, sorted_.ctypes.data, sp), lib)
    torch.cuda.current_stream(dev).synchronize()
    np.testing.assert_array_equal(on.cpu().numpy(), counts)
    hi, hj, hv = oi.cpu().numpy(), oj.cpu().numpy(), ov.cpu().numpy()
    out = []
    for p in range(n):
        a, b = int(offs[p]), int(offs[p + 1])
        i, j, v = hi[a:b], hj[a:b], hv[a:b]
        if not sorted_[p]:
            assert counts[p] > 16384 or n_res[p] > 65536
            order = np.lexsort((j, i, -v.astype(np.float64)))
            i, j, v = i[order], j[order], v[order]
        out.append((i, j, v))
    return out


def _product(views, t):
    from dctdomain_amd import reccut
    offs, ci, cj, cv = reccut.top_contacts_batch(views, t)
    return [(ci[offs[p]:offs[p + 1]], cj[offs[p]:offs[p + 1]], cv[offs[p]:offs[p + 1]]) for p in range(len(views))]


def _routes(device):
    """(name, run(views, t)) of every route; the experiments context's option is restored by the caller."""
    from dctdomain_amd import _lib
    ectx = _lib.experiments_context(device)
    out = []
    for which in (0, 1, 2):
        def run(views, t, which=which):
            ectx.set_option('topk_kernel', which)
            return _topk_sorted(ectx, views, t)
        out.append((f'topk_kernel={which}', run))
    out.append(('product', _product))
    return ectx, out


# ------------------------------------------------------------------ layouts
def _contiguous(groups, dev):
    return [[torch.from_numpy(m).to(dev) for _, m in maps] for _, maps in groups]


def _padded(groups, dev, wmod):
    """All maps of the corpus as views base[b, :L, :L] of one (B, W, W) tensor filled with 2.0, W = wmod mod 4 and > every L."""
    flat = [m for _, maps in groups for _, m in maps]
    W = max(m.shape[0] for m in flat) + 1
    W += (wmod - W) % 4
    base = torch.full((len(flat), W, W), 2.0, dtype=torch.float32, device=dev)
    views, b = [], 0
    for _, maps in groups:
        vs = []
        for _, m in maps:
            L = m.shape[0]
            v = base[b, :L, :L]
            v.copy_(torch.from_numpy(m))
            assert L < 2 or v.stride(0) == W
            vs.append(v)
            b += 1
        views.append(vs)
    return base, views


def test_contact_topk_every_route_and_layout():
    from dctdomain_amd import _lib
    dev = torch.device('cuda', torch.cuda.current_device())
    groups = _corpus()
    # the corpus covers every limit, from the host-side k and L alone (a later edit must not drop a route silently)
    ks = {(_k_of(m.shape[0], t)) for t, maps in groups for _, m in maps}
    Ls = {m.shape[0] for _, maps in groups for _, m in maps}
    for what, want in K_BOUNDS.items():
        assert set(want) <= ks, (what, sorted(set(want) - ks))
    assert set(range(8)) <= Ls and {728, 729} <= Ls
    long_k = [_k_of(m.shape[0], t) for t, maps in groups for _, m in maps if _cand(m.shape[0]) >= LONG_PAIRS]
    short_max = max(_cand(m.shape[0]) for _, maps in groups for _, m in maps if _cand(m.shape[0]) < LONG_PAIRS)
    assert max(long_k) > 6144 and short_max >= LONG_PAIRS - 1000
    for k in (1400, 1401, 3000, 3001, 6144, 6145, 2048, 4096, 8192, 16384):   # every L mod 4 at every limit but the smallest
        assert {m.shape[0] % 4 for t, maps in groups for _, m in maps if _k_of(m.shape[0], t) == k} == {0, 1, 2, 3}, k
    assert {name for _, maps in groups for name, _ in maps} == set(NAMES)

    ectx, routes = _routes(dev.index)
    seen = {}
    try:
        layouts = [('contiguous', None, _contiguous(groups, dev))]
        for wmod in range(4):
            layouts.append((f'W%4={wmod}',) + _padded(groups, dev, wmod))
        for lname, base, views in layouts:
            for rname, run in routes:
                for g, ((t, maps), vs) in enumerate(zip(groups, views)):
                    got = run(vs, t)
                    for q, ((name, m), v) in enumerate(zip(maps, vs)):
                        L = m.shape[0]
                        _assert_same(got[q], _oracle((g, q), m, t), f'{rname}, {lname}, map {name} L={L} k={_k_of(L, t)} '
                                                                     f'ld={v.stride(0)} ptr%16={v.data_ptr() % 16}')
                        cell = (rname, lname, L % 4 if lname != 'contiguous' else None, L >= 6 and _cand(L) >= LONG_PAIRS)
                        seen[cell] = seen.get(cell, 0) + 1
            del base, views
    finally:
        ectx.set_option('topk_kernel', 0)
    # every cell of route x layout (x L mod 4 on the padded ones) x short / long was reached
    for rname, _ in routes:
        for long_ in (False, True):
            assert seen.get((rname, 'contiguous', None, long_), 0) > 0
            for wmod in range(4):
                for lmod in range(4):
                    assert seen.get((rname, f'W%4={wmod}', lmod, long_), 0) > 0, (rname, wmod, lmod, long_)


def test_contact_topk_huge_row_stride_goes_to_the_radix_select():
    """A view whose n_res * ld reaches 2^29 floats (beyond the 32-bit byte offsets of the one- and two-read kernels' buffer
    loads): handed to the radix select, which must read it right (about 2.1 GB)."""
    from dctdomain_amd import reccut
    dev = torch.device('cuda', torch.cuda.current_device())
    L, ld = 64, (1 << 23) + 4
    assert L * ld >= 1 << 29
    store = torch.full(((L - 1) * ld + L,), 2.0, dtype=torch.float32, device=dev)
    view = store.as_strided((L, L), (ld, 1))
    for name in ('band', 'ties', 'special'):
        m = _map(name, L, 31)
        view.copy_(torch.from_numpy(m))
        for k in (1, 150, _cand(L)):
            t = _t_for(k, L)
            offs, ci, cj, cv = reccut.top_contacts_batch([view], t)
            _assert_same((ci, cj, cv), co.top_contacts(m, t), f'{name} k={k}')
    del view, store
    torch.cuda.empty_cache()


def _mixed_batch(n=320, seed=4):
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.gamma(2.0, 170.0, size=n).astype(int), 0, 728).tolist()
    lens += [729, 733, 760, 810, 905, 1010, 1160, 1201]                 # long: the striped chain, beside the short ones
    rng.shuffle(lens)
    names = [NAMES[q % len(NAMES)] for q in range(len(lens))]
    return [(nm, _map(nm, L, 50_000 + q)) for q, (nm, L) in enumerate(zip(names, lens))]


def test_contact_topk_mixed_batch_on_a_side_stream_and_padded_views():
    """Several hundred shuffled proteins, short and long in one call, on a torch stream of its own; then the same proteins as
    views of a padded batch: bit for bit what contiguous copies give, and the same multiset without the order."""
    from dctdomain_amd import reccut
    dev = torch.device('cuda', torch.cuda.current_device())
    t = 2.6
    maps = _mixed_batch()
    assert sum(_cand(m.shape[0]) >= LONG_PAIRS for _, m in maps) >= 8 and len(maps) > 300
    dense = [torch.from_numpy(m).to(dev) for _, m in maps]
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        offs, ci, cj, cv = reccut.top_contacts_batch(dense, t)
    torch.cuda.current_stream(dev).wait_stream(side)
    for p, (name, m) in enumerate(maps):
        a, b = offs[p], offs[p + 1]
        _assert_same((ci[a:b], cj[a:b], cv[a:b]), co.top_contacts(m, t), f'side stream: map {p} {name} L={m.shape[0]}')
    unsorted = reccut.top_contacts_batch(dense, t, sort=False)
    for wmod in range(4):
        W = max(m.shape[0] for _, m in maps) + 1
        W += (wmod - W) % 4
        base = torch.full((len(maps), W, W), 2.0, dtype=torch.float32, device=dev)
        views = []
        for b_, (_, m) in enumerate(maps):
            v = base[b_, :m.shape[0], :m.shape[0]]
            v.copy_(torch.from_numpy(m))
            views.append(v)
        got = reccut.top_contacts_batch(views, t)
        for x, y in zip(got, (offs, ci, cj, cv)):
            np.testing.assert_array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8), err_msg=f'W%4={wmod}')
        u_offs, u_i, u_j, u_v = reccut.top_contacts_batch(views, t, sort=False)
        np.testing.assert_array_equal(u_offs, unsorted[0])
        for p in range(len(maps)):
            a, b = u_offs[p], u_offs[p + 1]
            mine = sorted(zip(u_i[a:b].tolist(), u_j[a:b].tolist(), u_v[a:b].view(np.uint32).tolist()))
            theirs = sorted(zip(unsorted[1][a:b].tolist(), unsorted[2][a:b].tolist(), unsorted[3][a:b].view(np.uint32).tolist()))
            assert mine == theirs, (wmod, p, maps[p][1].shape[0])
        del base, views


def test_contact_topk_keys_spanning_the_whole_range():
    """+inf and -inf in one map, every candidate wanted (k = cand, the -inf entry the k-th): the bisection over keys spans
    nearly 2^32 and its top bin ends at the top of the key space (its upper end once wrapped round below its lower end, and
    the one-read kernel left one output slot unwritten) -- on every route, with huge finite values too."""
    dev = torch.device('cuda', torch.cuda.current_device())
    rng = np.random.default_rng(8)
    ectx, routes = _routes(dev.index)
    try:
        for L in (8, 11, 12, 40, 100, 300):
            maps = []
            for lo_v, hi_v in ((-np.inf, np.inf), (-3.0e38, np.inf), (-np.inf, 3.0e38), (-3.0e38, 3.0e38)):
                m = rng.random((L, L)).astype(np.float32)
                m[0, 7 if L > 7 else 5] = hi_v
                m[L - 6, L - 1] = lo_v
                maps.append(m)
            for k in (_cand(L), _cand(L) - 1):
                t = _t_for(k, L)
                for rname, run in routes:
                    got = run([torch.from_numpy(m).to(dev) for m in maps], t)
                    for q, m in enumerate(maps):
                        _assert_same(got[q], co.top_contacts(m, t), f'{rname}: L={L} k={k} map {q}')
    finally:
        ectx.set_option('topk_kernel', 0)
