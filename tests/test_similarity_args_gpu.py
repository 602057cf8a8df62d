"""What dctdomain_amd/similarity.py refuses before it launches anything, as a table: one row per (public function, kind of wrong
argument) -> the exception type.  The library bounds no index on the device, so these checks are what stands between a wrong
argument and a memory fault.  The kinds: a wrong dtype, a wrong length, a tensor that is not contiguous, a CPU tensor where a
device one is required, a wrong number of dimensions, an index or range outside the nodes.  The types were read off the module
as it was when every function spelt its own checks.  The shapes are the smallest that reach a check: 3 x 16 int8 fingerprints
with the prefix array [0, 1, 3], a 2 x 3 int32 tile at row0 = 0, col0 = 1 over 4 nodes, 4-entry node arrays, a 4 x 4 linkage
matrix.  Below the table: the views the checks must go on accepting, each held to the result of its contiguous copy."""

from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

I32, I64, U8, I8 = torch.int32, torch.int64, torch.uint8, torch.int8
N, BOUND, IDX = 4, 9000, [0, 1, 3]
ALL = ('dtype', 'length', 'strided', 'cpu', 'ndim')
NO_NDIM = ALL[:4]                                # the line writers take their columns in any shape


def wrong(kind: str, good: torch.Tensor) -> torch.Tensor:
    """``good`` (a contiguous device vector) made wrong in one way."""
    n = good.numel()
    if kind == 'dtype':
        return good.to(I64 if good.dtype != I64 else I32)
    if kind == 'length':
        return torch.cat([good, good[:1]])
    if kind == 'strided':
        return torch.cat([good, good]).view(n, 2).t()[0] if n > 1 else pytest.fail('one entry is always contiguous')
    if kind == 'cpu':
        return good.cpu()
    return good.view(n, 1)


@pytest.fixture(scope='module')
def e():
    """The good arguments, never written to: a refusal launches nothing."""
    from dctdomain_amd import similarity as sim
    dev = torch.device('cuda', torch.cuda.current_device())
    rng = np.random.default_rng(5)
    vec = lambda n=N, dtype=I32: torch.zeros(n, dtype=dtype, device=dev)          # noqa: E731
    ids, labels = sim.LineIds(['a', 'bb', 'c', 'dd'], dev), sim.LineIds(['x', 'y', 'z', '-'], dev)
    pi, pj = torch.tensor([0, 1], dtype=I32, device=dev), torch.tensor([1, 2], dtype=I32, device=dev)
    return SimpleNamespace(
        sim=sim, dev=dev, vec=vec,
        fa=torch.as_tensor(rng.integers(-128, 128, (3, 16)).astype(np.int8), device=dev),
        fb=torch.as_tensor(rng.integers(-128, 128, (3, 16)).astype(np.int8), device=dev),
        idx=torch.tensor(IDX, dtype=I64, device=dev), pairs=torch.tensor([[0, 1], [1, 0]], dtype=I32, device=dev),
        tile=torch.as_tensor(rng.integers(0, 17000, (2, 3)).astype(np.int32), device=dev),
        mat=torch.zeros((N, N), dtype=I32, device=dev), size=torch.ones(N, dtype=I32, device=dev),
        live=torch.arange(N, dtype=I32, device=dev), ids=ids, labels=labels, pi=pi, pj=pj,
        table=torch.zeros((2, 17002, 5), dtype=U8, device=dev), text=torch.zeros(400, dtype=U8, device=dev),
        line_off=sim.pair_line_offsets(pi, pj, ids), hist=torch.zeros((1, 17001), dtype=I64, device=dev))


def tree(e, **bad):
    ts = e.sim.TreeState(N, e.dev)
    for name, kind in bad.items():
        setattr(ts, name, kind if isinstance(kind, torch.Tensor) else wrong(kind, getattr(ts, name)))
    return ts


def greedy(e, n=N, **bad):
    gs = e.sim.GreedyState(n, e.dev)
    for name, kind in bad.items():
        setattr(gs, name, wrong(kind, getattr(gs, name)))
    return gs


def best(e, n_a=N, n_b=N, **bad):
    state = e.sim.BestState(n_a, n_b, e.dev)
    for name, kind in bad.items():
        setattr(state, name, wrong(kind, getattr(state, name)))
    return state


def map_args(e, bound=100, **put):
    """The arguments of pair_map_line_lengths, with ``put`` in place of the good ones."""
    args = dict(pi=e.pi, pj=e.pj, mn=e.vec(2), last=e.vec(2), la=e.vec(2), lb=e.vec(2), ids=e.ids, labels=e.labels, table=e.table,
                first_row=e.vec(5, I64), row_off=e.vec(3, I64), row_l1=e.vec(4), row_arg=e.vec(4), bound=bound)
    args.update(put)
    return tuple(args.values())


CASES = []


def refuse(name, error, call):
    CASES.append(pytest.param(error, call, id=name))


def vectors(name, kinds, good, call):
    """A row per kind: ``call(e, t)`` with the vector ``good(e)`` made wrong must raise ValueError."""
    for kind in kinds:
        refuse(f'{name}-{kind}', ValueError, lambda e, kind=kind: call(e, wrong(kind, good(e))))


# ---- the tile every tile scan starts with (tri_filter_count stands for all: one function describes the tile)
for what, make in (('dtype', lambda e: e.tile.long()), ('cpu', lambda e: e.tile.cpu()), ('ndim', lambda e: e.tile[0]),
                   ('column-stride', lambda e: torch.zeros((2, 6), dtype=I32, device=e.dev)[:, ::2])):
    refuse(f'tri_filter_count-tile-{what}', ValueError, lambda e, make=make: e.sim.tri_filter_count(make(e), 0, 1, BOUND))
refuse('tri_filter_count-negative-row0', ValueError, lambda e: e.sim.tri_filter_count(e.tile, -1, 1, BOUND))
refuse('tri_filter_count-row_empty-length', ValueError, lambda e: e.sim.tri_filter_count(e.tile, 0, 1, BOUND, row_empty=[0, 0, 0]))
refuse('tri_filter_count-col_empty-length', ValueError, lambda e: e.sim.tri_filter_count(e.tile, 0, 1, BOUND, col_empty=[0, 0]))
for kind in ('dtype', 'length', 'cpu'):
    refuse(f'tri_filter_fill-count-{kind}', ValueError, lambda e, kind=kind: e.sim.tri_filter_fill(e.tile, 0, 1, BOUND, wrong(kind, e.vec(2)), 0))

# ---- union-find forests
vectors('tri_link-parent', ALL[:1] + ALL[2:], lambda e: e.vec(), lambda e, t: e.sim.tri_link(e.tile, 0, 1, BOUND, t))
refuse('tri_link-tile-outside-the-nodes', IndexError, lambda e: e.sim.tri_link(e.tile, 0, 1, BOUND, e.vec(3)))
refuse('tri_link-tile-outside-the-nodes-rows', IndexError, lambda e: e.sim.tri_link(e.tile, 3, 0, BOUND, e.vec()))
refuse('tri_link-tile-dtype', ValueError, lambda e: e.sim.tri_link(e.tile.long(), 0, 1, BOUND, e.vec()))
vectors('link_pairs-pi', ALL, lambda e: e.pi, lambda e, t: e.sim.link_pairs(t, e.pj, e.vec()))
vectors('link_pairs-pj', ALL, lambda e: e.pj, lambda e, t: e.sim.link_pairs(e.pi, t, e.vec()))
vectors('link_pairs-parent', ALL[:1] + ALL[2:], lambda e: e.vec(), lambda e, t: e.sim.link_pairs(e.pi, e.pj, t))
vectors('cluster_labels-parent', ALL[:1] + ALL[2:], lambda e: e.vec(), lambda e, t: e.sim.cluster_labels(t))
vectors('rows_link-owner', ALL, lambda e: e.vec(), lambda e, t: e.sim.rows_link(e.fa, 0, e.fb, 0, t, e.vec(), BOUND))
vectors('rows_link-parent', ALL[:1] + ALL[2:], lambda e: e.vec(), lambda e, t: e.sim.rows_link(e.fa, 0, e.fb, 0, e.vec(), t, BOUND))
refuse('rows_link-parent-length', ValueError, lambda e: e.sim.rows_link(e.fa, 0, e.fb, 0, e.vec(), e.vec(5), BOUND))     # (owner: one per node)
refuse('rows_link-skip-length', ValueError, lambda e: e.sim.rows_link(e.fa, 0, e.fb, 0, e.vec(), e.vec(), BOUND, skip=[0, 0, 0]))
refuse('rows_link-rows-ndim', ValueError, lambda e: e.sim.rows_link(e.fa[0], 0, e.fb, 0, e.vec(), e.vec(), BOUND))
refuse('rows_link-rows-width', ValueError, lambda e: e.sim.rows_link(e.fa[:, :8], 0, e.fb, 0, e.vec(), e.vec(), BOUND))
vectors('rows_assign-assign', ALL[:1] + ALL[2:], lambda e: e.vec(), lambda e, t: e.sim.rows_assign(e.fa, e.fb, t, BOUND))
vectors('rows_assign-value_a', ALL, lambda e: e.vec(3), lambda e, t: e.sim.rows_assign(e.fa, e.fb, e.vec(), BOUND, value_a=t))
vectors('rows_assign-slot_b', ALL, lambda e: e.vec(3), lambda e, t: e.sim.rows_assign(e.fa, e.fb, e.vec(), BOUND, slot_b=t))
refuse('rows_assign-value_a-numpy', ValueError, lambda e: e.sim.rows_assign(e.fa, e.fb, e.vec(), BOUND, value_a=np.zeros(3, np.int32)))
refuse('rows_assign-rows-width', ValueError, lambda e: e.sim.rows_assign(e.fa, e.fb[:, :8], e.vec(), BOUND))

# ---- the single-linkage tree
for field in ('comp', 'parent', 'best'):
    for kind in ALL:
        if (field, kind) != ('comp', 'length'):       # (comp sets the length the others are held to)
            refuse(f'tri_nearest-{field}-{kind}', ValueError, lambda e, f=field, k=kind: e.sim.tri_nearest(e.tile, 0, 1, BOUND, tree(e, **{f: k})))
refuse('tri_nearest-tile-outside-the-nodes', IndexError, lambda e: e.sim.tri_nearest(e.tile, 0, 1, BOUND, e.sim.TreeState(3, e.dev)))
refuse('tree_hook-best-dtype', ValueError, lambda e: e.sim.tree_hook(tree(e, best='dtype')))
for field in ('edge_i', 'edge_j', 'edge_key'):
    for kind in ALL:
        if (field, kind) != ('edge_i', 'length'):
            refuse(f'tree_hook-{field}-{kind}', ValueError, lambda e, f=field, k=kind: e.sim.tree_hook(tree(e, **{f: k})))
refuse('tree_hook-counter-dtype', ValueError, lambda e: e.sim.tree_hook(tree(e, counter='dtype')))
refuse('tree_hook-counter-length', ValueError, lambda e: e.sim.tree_hook(tree(e, counter='length')))
refuse('tree_hook-counter-cpu', ValueError, lambda e: e.sim.tree_hook(tree(e, counter='cpu')))

# ---- complete / average linkage
for what, make in (('dtype', lambda e: e.mat.float()), ('cpu', lambda e: e.mat.cpu()), ('ndim', lambda e: e.mat[0]),
                   ('column-stride', lambda e: torch.zeros((N, 2 * N), dtype=I32, device=e.dev)[:, ::2]),
                   ('columns', lambda e: e.mat[:, :3]), ('rows', lambda e: torch.zeros((N + 1, N), dtype=I32, device=e.dev))):
    refuse(f'linkage_nearest-mat-{what}', ValueError, lambda e, make=make: e.sim.linkage_nearest(make(e), e.size, e.live, BOUND))
vectors('linkage_nearest-size', ALL[:1] + ALL[2:], lambda e: e.size, lambda e, t: e.sim.linkage_nearest(e.mat, t, e.live, BOUND))
vectors('linkage_nearest-live', ALL, lambda e: e.live, lambda e, t: e.sim.linkage_nearest(e.mat, e.size, t, BOUND))
vectors('linkage_nearest-nn', ALL, lambda e: e.vec(), lambda e, t: e.sim.linkage_nearest(e.mat, e.size, e.live, BOUND, t))
refuse('linkage_nearest-live-outside-the-rows', IndexError, lambda e: e.sim.linkage_nearest(e.mat[:2], e.size, e.live, BOUND))
refuse('linkage_merge-mat-not-square', ValueError, lambda e: e.sim.linkage_merge(e.mat[:2], e.size, e.vec(), e.vec(1)))
vectors('linkage_merge-partner', ALL, lambda e: e.vec(), lambda e, t: e.sim.linkage_merge(e.mat, e.size, t, e.vec(1)))
vectors('linkage_merge-keep', ALL[:1] + ALL[2:], lambda e: e.vec(2), lambda e, t: e.sim.linkage_merge(e.mat, e.size, e.vec(), t))
refuse('linkage_merge-keep-too-many', ValueError, lambda e: e.sim.linkage_merge(e.mat, e.size, e.vec(), e.vec(3)))

# ---- reciprocal best hits and moments: rectangles
for field in ('best_row', 'best_col'):
    for kind in ALL[:1] + ALL[2:]:
        refuse(f'rect_best-{field}-{kind}', ValueError, lambda e, f=field, k=kind: e.sim.rect_best(e.tile, 0, 1, BOUND, best(e, **{f: k})))
refuse('rect_best-tile-outside-the-rows', IndexError, lambda e: e.sim.rect_best(e.tile, 0, 1, BOUND, best(e, n_a=1)))
refuse('rect_best-tile-outside-the-columns', IndexError, lambda e: e.sim.rect_best(e.tile, 0, 1, BOUND, best(e, n_b=3)))


def moments(e, n_a=N, n_b=N, **put):
    state = e.sim.MomentState(n_a, n_b, device=e.dev)
    for name, t in put.items():
        setattr(state, name, t(state) if callable(t) else t)
    return state


for what, put in (('dtype', lambda s: s.row.int()), ('shape', lambda s: s.row[:, :3]), ('strided', lambda s: s.row.t().contiguous().t()),
                  ('cpu', lambda s: s.row.cpu())):
    refuse(f'rect_moments-row-{what}', ValueError, lambda e, put=put: e.sim.rect_moments(e.tile, 0, 1, moments(e, row=put)))
refuse('rect_moments-neither-side', ValueError, lambda e: e.sim.rect_moments(e.tile, 0, 1, moments(e, row=None, col=None)))
refuse('rect_moments-tile-outside-the-rows', IndexError, lambda e: e.sim.rect_moments(e.tile, 0, 1, moments(e, n_a=1)))
refuse('rect_moments-tile-outside-the-columns', IndexError, lambda e: e.sim.rect_moments(e.tile, 0, 1, moments(e, n_b=3)))

# ---- the passes over a tile of one file with per-protein arrays
vectors('label_sums-labels', ALL[:1] + ALL[2:], lambda e: e.vec(), lambda e, t: e.sim.label_sums(e.tile, 0, 1, t, e.vec(N, I64)))
vectors('label_sums-sums', ALL, lambda e: e.vec(N, I64), lambda e, t: e.sim.label_sums(e.tile, 0, 1, e.vec(), t))
refuse('label_sums-tile-outside-the-nodes', IndexError, lambda e: e.sim.label_sums(e.tile, 0, 1, e.vec(3), e.vec(3, I64)))
vectors('tri_degree-deg', ALL[:1] + ALL[2:], lambda e: e.vec(), lambda e, t: e.sim.tri_degree(e.tile, 0, 1, BOUND, t))
refuse('tri_degree-tile-outside-the-nodes', IndexError, lambda e: e.sim.tri_degree(e.tile, 0, 1, BOUND, e.vec(3)))
vectors('tri_link_core-core', ALL[:1] + ALL[2:], lambda e: e.vec(N, U8), lambda e, t: e.sim.tri_link_core(e.tile, 0, 1, BOUND, t, e.vec(), e.vec()))
vectors('tri_link_core-parent', ALL, lambda e: e.vec(), lambda e, t: e.sim.tri_link_core(e.tile, 0, 1, BOUND, e.vec(N, U8), t, e.vec()))
vectors('tri_link_core-nearest', ALL, lambda e: e.vec(), lambda e, t: e.sim.tri_link_core(e.tile, 0, 1, BOUND, e.vec(N, U8), e.vec(), t))
vectors('tri_first_fp-fam', ALL[:1] + ALL[2:], lambda e: e.vec(), lambda e, t: e.sim.tri_first_fp(e.tile, 0, 1, BOUND, t, e.vec(N, I64)))
vectors('tri_first_fp-first', ALL, lambda e: e.vec(N, I64), lambda e, t: e.sim.tri_first_fp(e.tile, 0, 1, BOUND, e.vec(), t))
vectors('tri_tp_before-first', ALL, lambda e: e.vec(N, I64), lambda e, t: e.sim.tri_tp_before(e.tile, 0, 1, BOUND, e.vec(), t, e.vec()))
vectors('tri_tp_before-tp', ALL, lambda e: e.vec(), lambda e, t: e.sim.tri_tp_before(e.tile, 0, 1, BOUND, e.vec(), e.vec(N, I64), t))
refuse('tri_tp_before-tile-outside-the-nodes', IndexError,
       lambda e: e.sim.tri_tp_before(e.tile, 0, 1, BOUND, e.vec(3), e.vec(3, I64), e.vec(3)))
for what, make in (('dtype', lambda e: e.hist.int()), ('width', lambda e: e.hist[:, :17000].contiguous()), ('ndim', lambda e: e.hist[0]),
                   ('strided', lambda e: torch.zeros((17001, 2), dtype=I64, device=e.dev).t()[:1]), ('cpu', lambda e: e.hist.cpu()),
                   ('rows', lambda e: torch.zeros((2, 17001), dtype=I64, device=e.dev))):
    refuse(f'tri_hist-hist-{what}', ValueError, lambda e, make=make: e.sim.tri_hist(e.tile, 0, 1, BOUND, make(e)))
refuse('tri_hist-one-row-with-fam', ValueError, lambda e: e.sim.tri_hist(e.tile, 0, 1, BOUND, e.hist, e.vec()))
vectors('tri_hist-fam', ALL[:1] + ALL[2:], lambda e: e.vec(),
        lambda e, t: e.sim.tri_hist(e.tile, 0, 1, BOUND, torch.zeros((2, 17001), dtype=I64, device=e.dev), t))
refuse('tri_hist-tile-outside-the-nodes', IndexError,
       lambda e: e.sim.tri_hist(e.tile, 0, 1, BOUND, torch.zeros((2, 17001), dtype=I64, device=e.dev), e.vec(3)))

# ---- greedy clusters
for field in ('assign', 'state', 'blocked'):
    for kind in ALL:
        if (field, kind) != ('assign', 'length'):
            refuse(f'greedy_decide-{field}-{kind}', ValueError, lambda e, f=field, k=kind: e.sim.greedy_decide(greedy(e, **{f: k}), 0, N, 0))
for what, (i0, i1) in (('end', (0, N + 1)), ('start', (-1, 2)), ('order', (3, 2))):
    refuse(f'greedy_decide-range-{what}', IndexError, lambda e, i0=i0, i1=i1: e.sim.greedy_decide(greedy(e), i0, i1, 0))
refuse('greedy_tri_mark-state-dtype', ValueError, lambda e: e.sim.greedy_tri_mark(e.tile, 0, 1, BOUND, greedy(e, state='dtype'), N, 1))
refuse('greedy_tri_mark-tile-outside-the-nodes', IndexError, lambda e: e.sim.greedy_tri_mark(e.tile, 0, 1, BOUND, greedy(e, 3), 3, 1))
refuse('greedy_tri_mark-range-end', IndexError, lambda e: e.sim.greedy_tri_mark(e.tile, 0, 1, BOUND, greedy(e), N + 1, 1))
refuse('greedy_tri_mark-range-negative', IndexError, lambda e: e.sim.greedy_tri_mark(e.tile, 0, 1, BOUND, greedy(e), -1, 1))
vectors('greedy_pairs_mark-pi', ALL, lambda e: e.pi, lambda e, t: e.sim.greedy_pairs_mark(t, e.pj, greedy(e), N, 1))
vectors('greedy_pairs_mark-pj', ALL, lambda e: e.pj, lambda e, t: e.sim.greedy_pairs_mark(e.pi, t, greedy(e), N, 1))
refuse('greedy_pairs_mark-blocked-strided', ValueError, lambda e: e.sim.greedy_pairs_mark(e.pi, e.pj, greedy(e, blocked='strided'), N, 1))
refuse('greedy_pairs_mark-range-end', IndexError, lambda e: e.sim.greedy_pairs_mark(e.pi, e.pj, greedy(e), N + 1, 1))

# ---- distances straight from the fingerprints
for what, make in (('dtype', lambda e: torch.zeros((3, 3), dtype=I64, device=e.dev)), ('shape', lambda e: torch.zeros((3, 2), dtype=I32, device=e.dev)),
                   ('ndim', lambda e: torch.zeros(9, dtype=I32, device=e.dev)), ('cpu', lambda e: torch.zeros((3, 3), dtype=I32)),
                   ('column-stride', lambda e: torch.zeros((3, 6), dtype=I32, device=e.dev)[:, ::2])):
    refuse(f'l1_matrix-out-{what}', ValueError, lambda e, make=make: e.sim.l1_matrix(e.fa, e.fb, out=make(e)))
refuse('l1_matrix-rows-ndim', ValueError, lambda e: e.sim.l1_matrix(e.fa[0], e.fb))
refuse('l1_matrix-rows-width', ValueError, lambda e: e.sim.l1_matrix(e.fa, e.fb[:, :8]))
refuse('l1_knn_device-rows-width', ValueError, lambda e: e.sim.l1_knn_device(e.fa, e.fb[:, :8], 2))
BAD_PREFIX = (('decreasing', [0, 2, 1]), ('beyond-the-rows', [0, 1, 4]), ('negative', [-1, 1, 3]), ('empty', []))
for what, make in (('dtype', lambda e: torch.zeros((2, 2), dtype=I64, device=e.dev)), ('shape', lambda e: torch.zeros((2, 3), dtype=I32, device=e.dev)),
                   ('cpu', lambda e: torch.zeros((2, 2), dtype=I32)), ('column-stride', lambda e: torch.zeros((2, 4), dtype=I32, device=e.dev)[:, ::2])):
    refuse(f'protein_min-out-{what}', ValueError, lambda e, make=make: e.sim.protein_min(e.fa, IDX, e.fb, IDX, out=make(e)))
    refuse(f'protein_cover-out-{what}', ValueError,
           lambda e, make=make: e.sim.protein_cover(e.fa, IDX, [1] * 3, [0] * 2, e.fb, IDX, [1] * 3, [0] * 2, BOUND, out=make(e)))
for what, idx in BAD_PREFIX:
    refuse(f'protein_min-idx_a-{what}', ValueError, lambda e, idx=idx: e.sim.protein_min(e.fa, idx, e.fb, IDX))
    refuse(f'protein_min-idx_b-{what}', ValueError, lambda e, idx=idx: e.sim.protein_min(e.fa, IDX, e.fb, idx))
    refuse(f'protein_cover-idx_b-{what}', ValueError,
           lambda e, idx=idx: e.sim.protein_cover(e.fa, IDX, [1] * 3, [0] * 2, e.fb, idx, [1] * 3, [0] * 2, BOUND))
    refuse(f'pair_min-idx_a-{what}', ValueError, lambda e, idx=idx: e.sim.pair_min(e.fa, idx, e.fb, IDX, [[0, 0]]))
    refuse(f'pair_row_best-idx_b-{what}', ValueError, lambda e, idx=idx: e.sim.pair_row_best(e.fa, IDX, e.fb, idx, [[0, 0]]))
refuse('protein_min-rows-width', ValueError, lambda e: e.sim.protein_min(e.fa, IDX, e.fb[:, :8], IDX))
refuse('protein_cover-rows-too-wide', ValueError, lambda e: e.sim.protein_cover(
    torch.zeros((3, 528), dtype=I8, device=e.dev), IDX, [1] * 3, [0] * 2, torch.zeros((3, 528), dtype=I8, device=e.dev), IDX, [1] * 3, [0] * 2, BOUND))
for name, n, place in (('w_a', 3, 0), ('need_a', 2, 1), ('w_b', 3, 2), ('need_b', 2, 3)):
    def cover(e, t, place=place):
        args = [[1] * 3, [0] * 2, [1] * 3, [0] * 2]
        args[place] = t
        return e.sim.protein_cover(e.fa, IDX, args[0], args[1], e.fb, IDX, args[2], args[3], BOUND)
    vectors(f'protein_cover-{name}', ('dtype', 'length', 'ndim'), lambda e, n=n: e.vec(n), cover)       # (a host list or a strided tensor is copied)
    refuse(f'protein_cover-{name}-host-length', ValueError, lambda e, n=n, cover=cover: cover(e, [1] * (n + 1)))
for fn in ('pair_min', 'pair_argmin', 'pair_row_best'):
    for what, pairs in (('beyond-a', [[2, 0]]), ('beyond-b', [[0, 2]]), ('negative', [[0, -1]])):
        refuse(f'{fn}-pairs-{what}', IndexError, lambda e, fn=fn, pairs=pairs: getattr(e.sim, fn)(e.fa, IDX, e.fb, IDX, pairs))
    refuse(f'{fn}-pairs-odd', ValueError, lambda e, fn=fn: getattr(e.sim, fn)(e.fa, IDX, e.fb, IDX, [0, 1, 0]))
    refuse(f'{fn}-rows-width', ValueError, lambda e, fn=fn: getattr(e.sim, fn)(e.fa, IDX, e.fb[:, :8], IDX, [[0, 0]]))
for fn in ('pair_min_device', 'pair_argmin_device', 'pair_row_best_device'):
    for what, make in (('dtype', lambda e: e.pairs.long()), ('columns', lambda e: torch.zeros((2, 3), dtype=I32, device=e.dev)),
                       ('ndim', lambda e: e.pairs.reshape(-1)), ('strided', lambda e: torch.zeros((2, 4), dtype=I32, device=e.dev)[:, ::2])):
        refuse(f'{fn}-pairs-{what}', ValueError, lambda e, fn=fn, make=make: getattr(e.sim, fn)(e.fa, e.idx, e.fb, e.idx, make(e)))
    for what, make in (('dtype', lambda e: e.fa.int()), ('ndim', lambda e: e.fa[0]), ('width', lambda e: e.fa[:, :8])):
        refuse(f'{fn}-a-{what}', ValueError, lambda e, fn=fn, make=make: getattr(e.sim, fn)(make(e), e.idx, e.fb, e.idx, e.pairs))
    refuse(f'{fn}-idx_a-dtype', ValueError, lambda e, fn=fn: getattr(e.sim, fn)(e.fa, e.idx.int(), e.fb, e.idx, e.pairs))
    refuse(f'{fn}-idx_b-strided', ValueError, lambda e, fn=fn: getattr(e.sim, fn)(e.fa, e.idx, e.fb, wrong('strided', e.idx), e.pairs))
vectors('pair_row_best_device-row_off', NO_NDIM, lambda e: e.vec(3, I64),
        lambda e, t: e.sim.pair_row_best_device(e.fa, e.idx, e.fb, e.idx, e.pairs, t))

# ---- the line writers
refuse('sim_lines-last-shape', ValueError, lambda e: e.sim.sim_lines(e.tile, e.tile[:, :2].contiguous(), 0, 1, e.ids, e.table, [0, 100], e.text))
refuse('sim_lines-mn-dtype', ValueError, lambda e: e.sim.sim_lines(e.tile.long(), e.tile, 0, 1, e.ids, e.table, [0, 100], e.text))
refuse('sim_lines-mn-strided', ValueError,
       lambda e: e.sim.sim_lines(torch.zeros((2, 6), dtype=I32, device=e.dev)[:, :3], e.tile, 0, 1, e.ids, e.table, [0, 100], e.text))
refuse('sim_lines-row_base-length', ValueError, lambda e: e.sim.sim_lines(e.tile, e.tile, 0, 1, e.ids, e.table, [0], e.text))
refuse('sim_lines-table-dtype', ValueError, lambda e: e.sim.sim_lines(e.tile, e.tile, 0, 1, e.ids, e.table.view(I8), [0, 100], e.text))
refuse('sim_lines-table-length', ValueError, lambda e: e.sim.sim_lines(e.tile, e.tile, 0, 1, e.ids, e.table[:, :17001].contiguous(), [0, 100], e.text))
refuse('sim_lines-out-dtype', ValueError, lambda e: e.sim.sim_lines(e.tile, e.tile, 0, 1, e.ids, e.table, [0, 100], e.text.view(I8)))
refuse('sim_lines-out-strided', ValueError, lambda e: e.sim.sim_lines(e.tile, e.tile, 0, 1, e.ids, e.table, [0, 100], e.text[::2]))
refuse('sim_lines-tile-outside-the-ids', IndexError, lambda e: e.sim.sim_lines(e.tile, e.tile, 0, 2, e.ids, e.table, [0, 100], e.text))
refuse('sim_lines-negative-row0', IndexError, lambda e: e.sim.sim_lines(e.tile, e.tile, -1, 1, e.ids, e.table, [0, 100], e.text))
refuse('sim_lines-lines-beyond-out', ValueError, lambda e: e.sim.sim_lines(e.tile, e.tile, 0, 1, e.ids, e.table, [0, 100], e.text[:64]))
refuse('sim_lines-negative-row_base', ValueError, lambda e: e.sim.sim_lines(e.tile, e.tile, 0, 1, e.ids, e.table, [-1, 100], e.text))
for place, name in enumerate(('pi', 'pj', 'mn', 'last')):
    def lines(e, t, place=place):
        cols = [e.pi, e.pj, e.vec(2), e.vec(2)]
        cols[place] = t
        return e.sim.pair_lines(*cols, e.ids, e.table, e.line_off, e.text)
    vectors(f'pair_lines-{name}', NO_NDIM, lambda e: e.vec(2), lines)
for place, name in enumerate(('la', 'lb')):
    def label_lines(e, t, place=place):
        cols = [e.vec(2), e.vec(2)]
        cols[place] = t
        return e.sim.pair_lines(e.pi, e.pj, e.vec(2), e.vec(2), e.ids, e.table, e.line_off, e.text, *cols, e.labels)
    vectors(f'pair_lines-{name}', NO_NDIM, lambda e: e.vec(2), label_lines)
for kind in ('dtype', 'strided', 'cpu'):
    refuse(f'pair_lines-line_off-{kind}', ValueError,
           lambda e, kind=kind: e.sim.pair_lines(e.pi, e.pj, e.vec(2), e.vec(2), e.ids, e.table, wrong(kind, e.line_off), e.text))
refuse('pair_lines-line_off-short', ValueError, lambda e: e.sim.pair_lines(e.pi, e.pj, e.vec(2), e.vec(2), e.ids, e.table, e.line_off[:1], e.text))
refuse('pair_lines-table-dtype', ValueError, lambda e: e.sim.pair_lines(e.pi, e.pj, e.vec(2), e.vec(2), e.ids, e.table.view(I8), e.line_off, e.text))
refuse('pair_lines-table-length', ValueError, lambda e: e.sim.pair_lines(e.pi, e.pj, e.vec(2), e.vec(2), e.ids, e.table[:1], e.line_off, e.text))
refuse('pair_lines-out-dtype', ValueError, lambda e: e.sim.pair_lines(e.pi, e.pj, e.vec(2), e.vec(2), e.ids, e.table, e.line_off, e.text.view(I8)))
refuse('pair_lines-out-strided', ValueError, lambda e: e.sim.pair_lines(e.pi, e.pj, e.vec(2), e.vec(2), e.ids, e.table, e.line_off, e.text[::2]))
for name, n, dtype in (('pi', 2, I32), ('pj', 2, I32), ('mn', 2, I32), ('last', 2, I32), ('la', 2, I32), ('lb', 2, I32), ('row_off', 3, I64),
                       ('first_row', 5, I64), ('row_arg', 4, I32)):
    vectors(f'pair_map_line_lengths-{name}', NO_NDIM, lambda e, n=n, dtype=dtype: e.vec(n, dtype),
            lambda e, t, name=name: e.sim.pair_map_line_lengths(*map_args(e, **{name: t})))
refuse('pair_map_line_lengths-table-dtype', ValueError, lambda e: e.sim.pair_map_line_lengths(*map_args(e, table=e.table.view(I8))))
refuse('pair_map_line_lengths-table-length', ValueError, lambda e: e.sim.pair_map_line_lengths(*map_args(e, table=e.table[:1])))
refuse('pair_map_line_lengths-table-strided', ValueError,
       lambda e: e.sim.pair_map_line_lengths(*map_args(e, table=torch.zeros((5, 17002, 2), dtype=U8, device=e.dev).permute(2, 1, 0))))
refuse('pair_map_line_lengths-bound-cap', ValueError, lambda e: e.sim.pair_map_line_lengths(*map_args(e, bound=17000)))
refuse('pair_map_line_lengths-bound-negative', ValueError, lambda e: e.sim.pair_map_line_lengths(*map_args(e, bound=-2)))
for kind in ('dtype', 'strided', 'cpu'):
    refuse(f'pair_map_lines-line_off-{kind}', ValueError, lambda e, kind=kind: e.sim.pair_map_lines(*map_args(e), wrong(kind, e.line_off), e.text))
refuse('pair_map_lines-line_off-short', ValueError, lambda e: e.sim.pair_map_lines(*map_args(e), e.line_off[:1], e.text))
refuse('pair_map_lines-row_l1-length', ValueError, lambda e: e.sim.pair_map_lines(*map_args(e, row_l1=e.vec(5)), e.line_off, e.text))
refuse('pair_map_lines-out-dtype', ValueError, lambda e: e.sim.pair_map_lines(*map_args(e), e.line_off, e.text.view(I8)))
refuse('pair_map_lines-out-strided', ValueError, lambda e: e.sim.pair_map_lines(*map_args(e), e.line_off, e.text[::2]))
refuse('pair_map_lines-out-cpu', ValueError, lambda e: e.sim.pair_map_lines(*map_args(e), e.line_off, e.text.cpu()))


@pytest.mark.parametrize('error, call', CASES)
def test_a_wrong_argument_is_refused_before_anything_is_launched(e, monkeypatch, error, call):
    def launched(device, name, *args):
        raise AssertionError(f'{name} was launched')
    monkeypatch.setattr(e.sim, '_launch', launched)
    with pytest.raises(error) as caught:
        call(e)
    assert type(caught.value) is error                    # the type itself, not a subclass of it


def test_the_good_arguments_of_the_table_are_accepted(e):
    """The refusals above are the wrong argument's doing: the same calls go through with the good ones."""
    sim = e.sim
    assert sim.tri_filter_count(e.tile, 0, 1, BOUND).shape == (2,)
    sim.tri_link(e.tile, 0, 1, BOUND, e.vec())
    sim.link_pairs(e.pi, e.pj, e.vec())
    sim.rows_link(e.fa, 0, e.fb, 1, e.vec(), e.vec(), BOUND)
    sim.rows_assign(e.fa, e.fb, e.vec(), BOUND, value_a=e.vec(3), slot_b=e.vec(3))
    sim.tri_nearest(e.tile, 0, 1, BOUND, tree(e))
    sim.tree_hook(tree(e))
    sim.linkage_nearest(e.mat, e.size, e.live, BOUND, e.vec())
    sim.linkage_merge(e.mat.clone(), e.size, torch.tensor([1, 0, -1, -1], dtype=I32, device=e.dev), e.vec(1))
    sim.rect_best(e.tile, 0, 1, BOUND, best(e))
    sim.rect_moments(e.tile, 0, 1, moments(e))
    sim.label_sums(e.tile, 0, 1, e.vec(), e.vec(N, I64))
    sim.tri_link_core(e.tile, 0, 1, BOUND, e.vec(N, U8), torch.arange(N, dtype=I32, device=e.dev), e.vec())
    sim.tri_tp_before(e.tile, 0, 1, BOUND, e.vec(), e.vec(N, I64), e.vec())
    sim.tri_hist(e.tile, 0, 1, BOUND, torch.zeros((2, 17001), dtype=I64, device=e.dev), e.vec())
    sim.greedy_decide(greedy(e), 0, N, 0)
    sim.greedy_tri_mark(e.tile, 0, 1, BOUND, greedy(e), N, 1)
    sim.greedy_pairs_mark(e.pi, e.pj, greedy(e), N, 1)
    sim.protein_cover(e.fa, IDX, [1] * 3, [0] * 2, e.fb, IDX, [1] * 3, [0] * 2, BOUND)
    sim.pair_row_best_device(e.fa, e.idx, e.fb, e.idx, e.pairs)
    text = torch.zeros(400, dtype=U8, device=e.dev)
    sim.sim_lines(e.tile, e.tile, 0, 1, e.ids, e.table, [0, 100], text)
    sim.pair_lines(e.pi, e.pj, e.vec(2), e.vec(2), e.ids, e.table, e.line_off, text)
    count = sim.pair_map_line_lengths(*map_args(e))
    assert count.shape == (2,)
    torch.cuda.synchronize()


# ---- views the checks go on accepting, each against its contiguous copy

def test_a_tile_that_is_a_column_range_of_a_wider_tensor(e):
    sim = e.sim
    rng = np.random.default_rng(11)
    wide = torch.as_tensor(rng.integers(0, 17000, (3, 9)).astype(np.int32), device=e.dev)
    tile = wide[:, 2:6]                                        # row stride 9 > width 4, off a 16-byte boundary
    assert tile.stride() == (9, 1) and not tile.is_contiguous()
    for t in (tile, tile[:1]):                                 # (and its first row alone: a one-row tile may carry any stride)
        n_rows = t.shape[0]
        got, want = sim.tri_filter(t, 0, 1, BOUND), sim.tri_filter(t.contiguous(), 0, 1, BOUND)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and want[0].sum() > 0
        parents = [torch.arange(5, dtype=I32, device=e.dev) for _ in range(2)]
        sim.tri_link(t, 0, 1, BOUND, parents[0])
        sim.tri_link(t.contiguous(), 0, 1, BOUND, parents[1])
        assert torch.equal(sim.cluster_labels(parents[0]), sim.cluster_labels(parents[1]))
        states = [sim.BestState(n_rows, 5, e.dev) for _ in range(2)]
        sim.rect_best(t, 0, 1, BOUND, states[0])
        sim.rect_best(t.contiguous(), 0, 1, BOUND, states[1])
        assert torch.equal(states[0].best_row, states[1].best_row) and torch.equal(states[0].best_col, states[1].best_col)
        assert (states[1].best_row != sim.BEST_NONE).any()


def test_one_row_of_fingerprints_with_a_stride_of_its_own(e):
    sim = e.sim
    rng = np.random.default_rng(12)
    wide = torch.as_tensor(rng.integers(-128, 128, (3, 40)).astype(np.int8), device=e.dev)
    one = wide[1:2, 3:19]                                      # one row of 16 bytes, row stride 40, not on a 16-byte boundary
    assert one.stride(0) == 40 and one.shape == (1, 16)
    copy = one.clone()
    assert torch.equal(sim.l1_matrix(one, e.fb), sim.l1_matrix(copy, e.fb)) and torch.equal(sim.l1_matrix(e.fa, one), sim.l1_matrix(e.fa, copy))
    assert torch.equal(sim.protein_min(one, [0, 1], e.fb, IDX), sim.protein_min(copy, [0, 1], e.fb, IDX))
    ref = (sim.l1_matrix(copy, e.fb)).cpu().numpy()
    assert sim.protein_min(one, [0, 1], e.fb, IDX).cpu().numpy().tolist() == [[ref[0, :1].min(), ref[0, 1:3].min()]]
    for got, want in zip(sim.l1_knn_device(one, e.fb, 2), sim.l1_knn_device(copy, e.fb, 2)):
        assert torch.equal(got, want)
    rows = wide[:, 3:19]                                       # three rows, row stride 40: read in place by rows_assign
    slots = [torch.full((3,), sim.GREEDY_NONE, dtype=I32, device=e.dev) for _ in range(2)]
    sim.rows_assign(rows, e.fb, slots[0], 17000)
    sim.rows_assign(rows.contiguous(), e.fb, slots[1], 17000)
    assert torch.equal(slots[0], slots[1]) and (slots[1] != sim.GREEDY_NONE).all()


def test_out_as_a_column_range_of_a_wider_tile(e):
    sim = e.sim
    for fn, args, shape in ((sim.l1_matrix, (e.fa, e.fb), (3, 3)), (sim.protein_min, (e.fa, IDX, e.fb, IDX), (2, 2))):
        want = fn(*args)
        assert tuple(want.shape) == shape
        wide = torch.full((shape[0], shape[1] + 3), -7, dtype=I32, device=e.dev)
        out = wide[:, 1:1 + shape[1]]
        assert fn(*args, out=out) is out and torch.equal(out, want)
        assert (wide[:, :1] == -7).all() and (wide[:, 1 + shape[1]:] == -7).all()
        one = torch.full((1, 8), -7, dtype=I32, device=e.dev)[:, 2:2 + shape[1]]      # a one-row out: any stride
        first = fn(args[0][:1], *(([0, 1],) if fn is sim.protein_min else ()), *args[2 if fn is sim.protein_min else 1:], out=one)
        assert torch.equal(first, want[:1])
