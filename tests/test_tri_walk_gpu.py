"""The five entry points that scan an int32 L1 tile (tri_filter_count, tri_filter_fill, tri_link, greedy_tri_mark, tri_nearest; one
TriTile and one row walk, csrc/tri_walk.hip.h) against ONE numpy keep-matrix of one tile: all_sim_filter_rule.tile_keep.

The tile has 70 rows x 1030 columns -- two bands of 64 rows for tri_nearest, the second partial, and two steps of 1024 columns for
all five -- and is a view into a larger tensor with an odd row stride and a column offset of 1 .. 3, so that successive rows have
different 16-byte shifts and the last quad of a row is read entry by entry.  Values on both sides of the bound and of the cap,
0x7fffffff and negative ones; both flag arrays set.  Two placements: the diagonal inside the tile, and the tile wholly right of it."""

import numpy as np
import pytest

import all_sim_filter_rule as rule
import cluster_rule as crule

pytestmark = pytest.mark.gpu
N_ROWS, N_COLS, BOUND, CAP = 70, 1030, 8500, 17000
PLACES = {'diagonal_inside': (5, 10, 3), 'right_of_diagonal': (3, 100, 1)}    # row0, col0, column offset of the view


class Case:
    def __init__(self, name):
        import torch
        self.row0, self.col0, offset = PLACES[name]
        self.n_nodes = self.col0 + N_COLS + 7
        rng = np.random.default_rng(len(name))
        t = rule.random_tile(rng, N_ROWS, N_COLS, BOUND)
        self.flags = (rng.random(N_ROWS) < 0.2, rng.random(N_COLS) < 0.2)
        big = torch.full((N_ROWS, N_COLS + offset + 8), -1, dtype=torch.int32, device='cuda')    # (-1 would be kept if it were read)
        assert big.stride(0) % 2 == 1 and big.data_ptr() % 16 == 0
        self.tile = big[:, offset:offset + N_COLS]
        self.tile.copy_(torch.as_tensor(t, device='cuda'))
        assert len({(self.tile[r].data_ptr() >> 2) & 3 for r in range(4)}) == 4          # every 16-byte shift occurs
        self.keep, self.key = rule.tile_keep(t, self.row0, self.col0, BOUND, *self.flags, cap=CAP)
        r, c = np.nonzero(self.keep)                                                     # (row-major)
        self.i, self.j, self.edge_key = self.row0 + r, self.col0 + c, self.key[r, c]
        assert len(r) > 0 and self.keep[64:].any() and self.keep[:, 1024:].any()
        assert (self.row0 + N_ROWS > self.col0) == (name == 'diagonal_inside')

    def args(self):
        return self.tile, self.row0, self.col0, BOUND

    def columns(self, value_of_row, none):
        """Per node: the smallest value_of_row[r] over the rows r with a kept entry in the node's column; `none` where there is none."""
        out = np.full(self.n_nodes, none, dtype=np.int64)
        r, c = np.nonzero(self.keep)
        np.minimum.at(out, self.col0 + c, value_of_row[r])
        return out


@pytest.fixture(scope='module', params=sorted(PLACES))
def case(request):
    return Case(request.param)


def test_count_is_the_row_sums_and_fill_the_nonzeros_in_row_major_order(case):
    from dctdomain_amd.similarity import tri_filter
    count, i, j = tri_filter(*case.args(), *case.flags, cap=CAP)
    assert np.array_equal(count, case.keep.sum(axis=1))
    assert np.array_equal(i, case.i) and np.array_equal(j, case.j)


def test_link_gives_the_components_of_the_matrix(case):
    import torch
    from dctdomain_amd.similarity import cluster_labels, tri_link
    parent = torch.arange(case.n_nodes, dtype=torch.int32, device='cuda')
    tri_link(*case.args(), parent, *case.flags, cap=CAP)
    want = crule.components(case.n_nodes, case.i, case.j)
    assert len(set(want.tolist())) < case.n_nodes
    assert np.array_equal(cluster_labels(parent).cpu().numpy(), want)


def test_mark_of_new_representatives_lowers_assign_to_the_first_row_of_every_kept_column(case):
    from dctdomain_amd.similarity import GREEDY_NEW, GREEDY_NONE, GreedyState, greedy_tri_mark
    gs = GreedyState(case.n_nodes)
    gs.state.fill_(GREEDY_NEW)
    greedy_tri_mark(*case.args(), gs, case.n_nodes, 1, *case.flags, cap=CAP)
    want = case.columns(case.row0 + np.arange(N_ROWS), GREEDY_NONE)
    assert (want != GREEDY_NONE).any() and (want == GREEDY_NONE).any()
    assert np.array_equal(gs.assign.cpu().numpy(), want)
    assert not gs.blocked.any().item()


def test_mark_of_undecided_rows_stamps_the_kept_columns_below_the_range_end_and_nothing_else(case):
    from dctdomain_amd.similarity import GREEDY_NONE, GreedyState, greedy_tri_mark
    gs = GreedyState(case.n_nodes)                            # (every row GREEDY_UNDECIDED)
    range_end, next_round = case.col0 + N_COLS // 2, 3
    greedy_tri_mark(*case.args(), gs, range_end, next_round, *case.flags, cap=CAP)
    kept_column = case.columns(np.zeros(N_ROWS, dtype=np.int64), 1) == 0
    want = np.where(kept_column & (np.arange(case.n_nodes) < range_end), next_round, 0)
    assert want.any() and kept_column[range_end:].any()
    assert np.array_equal(gs.blocked.cpu().numpy(), want)
    assert (gs.assign == GREEDY_NONE).all().item()


def test_nearest_gives_every_node_its_smallest_packed_edge(case):
    from dctdomain_amd.similarity import TreeState, tri_nearest
    ts = TreeState(case.n_nodes)                              # (comp = arange: every kept entry joins two components)
    tri_nearest(*case.args(), ts, *case.flags, cap=CAP)
    edge = case.edge_key.astype(np.uint64) << np.uint64(48) | case.i.astype(np.uint64) << np.uint64(24) | case.j.astype(np.uint64)
    want = np.full(case.n_nodes, ~np.uint64(0), dtype=np.uint64)
    np.minimum.at(want, case.i, edge)
    np.minimum.at(want, case.j, edge)
    assert (want == ~np.uint64(0)).any() and len(set((want >> np.uint64(48)).tolist())) > 3
    assert np.array_equal(ts.best.cpu().numpy().view(np.uint64), want)
