"""The six entry points that reduce an int32 L1 tile onto per-protein arrays (rect_best, label_sums, tri_degree, tri_link_core,
tri_first_fp, tri_tp_before; one TriTile and the band walk of csrc/band_walk.hip.h, rect_best in a loop of its own) against ONE numpy
keep / key matrix of one tile:
all_sim_filter_rule.tile_keep.

The tile has 70 rows x 1030 columns -- two bands of 64 rows, the second of 6, and two steps of 1024 columns, the second of 6: the
smallest shape that crosses both edges of a job -- and is a view into a larger tensor with an odd row stride and a column offset of
1 .. 3.  Values on both sides of the bound and of the cap, 0x7fffffff and negative ones; both flag arrays set.  Three placements: the
diagonal inside the tile, the tile wholly right of it, and wholly left of it -- where the five kernels of the triangle write nothing
and rect_best, which knows no diagonal, scans everything."""

import numpy as np
import pytest

import all_sim_filter_rule as rule
import cluster_rule as crule

pytestmark = pytest.mark.gpu
N_ROWS, N_COLS, BOUND, CAP = 70, 1030, 8500, 17000
PLACES = {'diagonal_inside': (5, 10, 3), 'right_of_diagonal': (3, 100, 1), 'left_of_diagonal': (1100, 0, 2)}    # row0, col0, column offset of the view
NONE64 = ~np.uint64(0)


def lowest(n_nodes, at, key, other):
    """Per node the smallest word key << 32 | other over the entries listed for it; all ones where there is none."""
    out = np.full(n_nodes, NONE64, dtype=np.uint64)
    np.minimum.at(out, at, key.astype(np.uint64) << np.uint64(32) | other.astype(np.uint64))
    return out


class Case:
    def __init__(self, name):
        import torch
        self.name = name
        self.row0, self.col0, offset = PLACES[name]
        self.n_nodes = max(self.row0 + N_ROWS, self.col0 + N_COLS) + 7
        rng = np.random.default_rng(len(name))
        t = rule.random_tile(rng, N_ROWS, N_COLS, BOUND)
        self.flags = (rng.random(N_ROWS) < 0.2, rng.random(N_COLS) < 0.2)
        big = torch.full((N_ROWS, (N_COLS + offset + 8) | 1), -1, dtype=torch.int32, device='cuda')    # (what lies beside the view is never a hit)
        assert big.stride(0) % 2 == 1
        self.tile = big[:, offset:offset + N_COLS]
        self.tile.copy_(torch.as_tensor(t, device='cuda'))
        # the one matrix: keep = the entries of the triangle within the bound, upper = all of the triangle, hit = the rectangle's
        self.keep, self.key = rule.tile_keep(t, self.row0, self.col0, BOUND, *self.flags, cap=CAP)
        self.upper = rule.tile_keep(t, self.row0, self.col0, CAP, *self.flags, cap=CAP)[0]
        self.hit = self.key <= BOUND
        assert (t > CAP).any() and (t < 0).any() and (self.key == CAP).any() and (self.key == BOUND).any() and (self.key == BOUND + 1).any()
        left = name == 'left_of_diagonal'
        assert self.keep.any() != left and self.upper.any() != left and np.array_equal(self.keep, self.hit) == (name == 'right_of_diagonal')
        assert (self.row0 + N_ROWS > self.col0 and not left) == (name == 'diagonal_inside')
        for m in (self.hit,) if left else (self.hit, self.keep):
            assert m[64:].any() and m[:, 1024:].any() and not m[64:].all() and not m[:, 1024:].all()
        r, c = np.nonzero(self.keep)
        self.i, self.j, self.edge_key = self.row0 + r, self.col0 + c, self.key[r, c]

    def args(self):
        return self.tile, self.row0, self.col0, BOUND

    def per_node(self, matrix):
        """Row sums + column sums of a matrix of the tile's shape, at the nodes of its rows and columns."""
        out = np.zeros(self.n_nodes, dtype=np.int64)
        np.add.at(out, self.row0 + np.arange(N_ROWS), matrix.sum(axis=1))
        np.add.at(out, self.col0 + np.arange(N_COLS), matrix.sum(axis=0))
        return out

    def nontrivial(self, want, none):
        """Some node has a value and some has none -- but left of the diagonal, where nothing may be written."""
        assert (want == none).any() and (want != none).any() == (self.name != 'left_of_diagonal')
        return want


@pytest.fixture(scope='module', params=sorted(PLACES))
def case(request):
    return Case(request.param)


def run_rect_best(case):
    from dctdomain_amd.similarity import BestState, rect_best
    state = BestState(case.n_nodes, case.n_nodes)
    rect_best(*case.args(), state, *case.flags, cap=CAP)
    return state.best_row.cpu().numpy().view(np.uint64), state.best_col.cpu().numpy().view(np.uint64)


def run_first_fp(case, fam):
    import torch
    from dctdomain_amd.similarity import BEST_NONE, tri_first_fp
    first = torch.full((case.n_nodes,), BEST_NONE, dtype=torch.int64, device='cuda')
    tri_first_fp(*case.args(), torch.as_tensor(fam, dtype=torch.int32, device='cuda'), first, *case.flags, cap=CAP)
    return first


def test_rect_best_gives_every_row_and_column_of_the_rectangle_its_lowest_hit(case):
    r, c = np.nonzero(case.hit)                                       # (no diagonal: every placement scans all of it)
    rows = lowest(case.n_nodes, case.row0 + r, case.key[r, c], case.col0 + c)
    cols = lowest(case.n_nodes, case.col0 + c, case.key[r, c], case.row0 + r)
    assert (rows == NONE64).any() and (rows != NONE64).any() and len(set((cols >> np.uint64(32)).tolist())) > 3
    best_row, best_col = run_rect_best(case)
    assert np.array_equal(best_row, rows) and np.array_equal(best_col, cols)


def test_degree_is_the_row_sums_plus_the_column_sums_of_keep(case):
    import torch
    from dctdomain_amd.similarity import tri_degree
    deg = torch.zeros(case.n_nodes, dtype=torch.int32, device='cuda')
    tri_degree(*case.args(), deg, *case.flags, cap=CAP)
    want = case.nontrivial(case.per_node(case.keep), 0)
    assert np.array_equal(deg.cpu().numpy(), want)


def test_label_sums_with_one_label_is_the_key_sums_of_the_triangle_whatever_the_bound(case):
    import torch
    from dctdomain_amd.similarity import label_sums
    labels = torch.zeros(case.n_nodes, dtype=torch.int32, device='cuda')
    sums = torch.zeros(case.n_nodes, dtype=torch.int64, device='cuda')
    label_sums(case.tile, case.row0, case.col0, labels, sums, *case.flags, cap=CAP)
    want = case.nontrivial(case.per_node(np.where(case.upper, case.key, 0)), 0)
    assert np.array_equal(want, case.per_node(np.where(case.keep, case.key, 0))) == (case.name == 'left_of_diagonal')   # (keys above the bound count)
    assert np.array_equal(sums.cpu().numpy(), want)


def test_first_fp_with_all_different_families_is_the_lowest_hit_of_either_side_above_the_diagonal(case):
    want = np.minimum(lowest(case.n_nodes, case.i, case.edge_key, case.j), lowest(case.n_nodes, case.j, case.edge_key, case.i))
    case.nontrivial(want, NONE64)
    first = run_first_fp(case, np.arange(case.n_nodes)).cpu().numpy().view(np.uint64)
    assert np.array_equal(first, want)
    if case.name == 'right_of_diagonal':                              # (keep is the whole rectangle: rect_best's two arrays, merged per node)
        assert np.array_equal(first, np.minimum(*run_rect_best(case)))
    # one family: nothing is a false positive
    assert (run_first_fp(case, np.zeros(case.n_nodes)).cpu().numpy().view(np.uint64) == NONE64).all()


def test_tp_before_with_one_family_and_no_false_positive_is_the_degree(case):
    import torch
    from dctdomain_amd.similarity import BEST_NONE, tri_tp_before
    fam = torch.zeros(case.n_nodes, dtype=torch.int32, device='cuda')
    first = torch.full((case.n_nodes,), BEST_NONE, dtype=torch.int64, device='cuda')
    tp = torch.zeros(case.n_nodes, dtype=torch.int32, device='cuda')
    tri_tp_before(*case.args(), fam, first, tp, *case.flags, cap=CAP)
    assert np.array_equal(tp.cpu().numpy(), case.per_node(case.keep))
    # with the first of all-different families every entry IS that first or ranks behind it: nothing counts
    tp.zero_()
    tri_tp_before(*case.args(), fam, run_first_fp(case, np.arange(case.n_nodes)), tp, *case.flags, cap=CAP)
    assert not tp.any().item()


def test_link_core_with_all_cores_gives_the_components_of_keep(case):
    import torch
    from dctdomain_amd.similarity import NEAREST_NONE, cluster_labels, tri_link_core
    core = torch.ones(case.n_nodes, dtype=torch.uint8, device='cuda')
    parent = torch.arange(case.n_nodes, dtype=torch.int32, device='cuda')
    nearest = torch.full((case.n_nodes,), NEAREST_NONE, dtype=torch.int32, device='cuda')
    tri_link_core(*case.args(), core, parent, nearest, *case.flags, cap=CAP)
    want = crule.components(case.n_nodes, case.i, case.j)
    assert (len(set(want.tolist())) < case.n_nodes) == (case.name != 'left_of_diagonal')
    assert np.array_equal(cluster_labels(parent).cpu().numpy(), want)
    assert (nearest == NEAREST_NONE).all().item()                    # (no entry has exactly one core end)
