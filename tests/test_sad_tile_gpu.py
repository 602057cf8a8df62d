"""The five kernels built on the 128 x 128 SAD tile pinned to each other on one input: l1_matrix16_kernel, protein_min_kernel and
rows_link_kernel, which call sad_tile (csrc/sad_tile.hip.h), and l1_knn_kernel and rows_assign_kernel, which keep a copy of it, must
all see the int64 numpy L1 matrix of the same rows.

Rows: a is 129 x d, b is 257 x d -- a partial last tile on both sides, three tiles of b -- uniform int8 over the full range, some
rows holding both -128 and 127 (the sign flip is the shared part), some rows of b exact or near copies of rows of a.  Widths:
7 (the narrow round only), 16 (exactly one 16-byte segment), 475 (29 segments and an 11-byte round), 480 (whole segments only).
The rows are handed over as views on 16-byte boundaries with a row stride of the next multiple of 16, straight through the C ABI
where the Python layer would copy them, so that every kernel meets d itself.  Every comparison is exact integer equality."""

import ctypes as C

import numpy as np
import pytest

import cluster_rule as crule
from test_assign_gpu import _view

pytestmark = pytest.mark.gpu
NA, NB = 129, 257
NONE = 0x7fffffff
NO_CAP = 1 << 30                                               # (the bound is the matrix's median: above 17000 at d = 475, 480)


def _call(name, *args):
    import torch
    from dctdomain_amd import _lib
    ctx = _lib.get_context(0)
    _lib.check(getattr(ctx._lib, name)(ctx.handle, *args, C.c_void_p(torch.cuda.current_stream().cuda_stream)))


class Case:
    def __init__(self, d):
        rng = np.random.default_rng(4200 + d)
        a = rng.integers(-128, 128, size=(NA, d)).astype(np.int8)
        b = rng.integers(-128, 128, size=(NB, d)).astype(np.int8)
        for r in (0, 77, NA - 1):                              # both ends of the range in one row, on either side of a pair
            a[r, 0::2], a[r, 1::2] = -128, 127
        b[1, 0::2], b[1, 1::2] = 127, -128
        b[200, 0::2], b[200, 1::2] = -128, 127
        b[NB - 1] = -128
        b[NB - 2] = 127
        for c, r in ((5, 3), (130, NA - 1), (255, 0), (64, 64), (128, 127)):      # exact copies, across tiles and tile edges
            b[c] = a[r]
        for c in rng.choice(np.arange(8, 250), size=40, replace=False):            # near copies
            if c not in (64, 128, 130, 200):
                b[c] = np.clip(a[rng.integers(0, NA)].astype(np.int64) + rng.integers(-3, 4, size=d), -128, 127)
        self.d, self.a, self.b = d, a, b
        self.dist = np.abs(a.astype(np.int16)[:, None, :] - b.astype(np.int16)[None, :, :]).sum(axis=2, dtype=np.int64)
        assert self.dist[0, 1] == 255 * d and self.dist[3, 5] == 0 and self.dist[NA - 1, 130] == 0
        self.bound = int(np.median(self.dist))
        assert 0 < int((self.dist <= self.bound).sum()) < NA * NB
        self.views = {}

    def view(self, arm):
        if arm not in self.views:
            self.views[arm] = (_view(self.a, self.d, arm), _view(self.b, self.d, arm))
        return self.views[arm]


@pytest.fixture(scope='module', params=[7, 16, 475, 480])
def case(request):
    return Case(request.param)


def test_l1_matrix(case):
    import torch
    va, vb = case.view(16)
    out = torch.full((NA, NB + 3), -1, dtype=torch.int32, device='cuda')
    _call('dctfp_l1_matrix', va.data_ptr(), NA, va.stride(0), vb.data_ptr(), NB, vb.stride(0), case.d, out.data_ptr(), out.stride(0))
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :NB], case.dist) and (got[:, NB:] == -1).all()


def test_protein_min_one_protein_per_row(case):
    from dctdomain_amd.similarity import protein_min
    va, vb = case.view(16)
    got = protein_min(va, np.arange(NA + 1), vb, np.arange(NB + 1))
    assert np.array_equal(got.cpu().numpy(), case.dist)


def test_protein_min_ragged(case):
    """Proteins of 0 rows, of a few, and of more than 128 (a block of its own, walked in two sub-tiles)."""
    from dctdomain_amd.similarity import protein_min
    va, vb = case.view(16)
    idx_a, idx_b = np.array([0, 3, 3, 10, NA]), np.array([0, 130, 130, 200, 201, NB])
    want = np.full((len(idx_a) - 1, len(idx_b) - 1), NONE, dtype=np.int64)
    for i in range(len(idx_a) - 1):
        for j in range(len(idx_b) - 1):
            block = case.dist[idx_a[i]:idx_a[i + 1], idx_b[j]:idx_b[j + 1]]
            if block.size:
                want[i, j] = block.min()
    assert (want[1] == NONE).all() and (want[:, 1] == NONE).all() and want[3, 0] == 0
    assert np.array_equal(protein_min(va, idx_a, vb, idx_b).cpu().numpy(), want)


def test_k_nearest(case):
    import torch
    k = 8
    va, vb = case.view(16)
    val = torch.full((NA, k), -1, dtype=torch.int32, device='cuda')
    idx = torch.full((NA, k), -1, dtype=torch.int32, device='cuda')
    _call('dctfp_l1_knn', va.data_ptr(), NA, va.stride(0), vb.data_ptr(), NB, vb.stride(0), case.d, k, 0, val.data_ptr(), idx.data_ptr())
    order = np.argsort(case.dist, axis=1, kind='stable')[:, :k]                    # by (distance, column)
    assert np.array_equal(idx.cpu().numpy(), order)
    assert np.array_equal(val.cpu().numpy(), np.take_along_axis(case.dist, order, axis=1))


@pytest.fixture(scope='module')
def linked(case):
    """The rule of rows_link (domain_cluster_rule: rows of different owners within the bound are joined, label = the smallest row
    of the component) on nodes 0 .. 128 = the rows of a, 129 .. 385 = the rows of b, every row its own owner."""
    r, c = np.nonzero(case.dist <= case.bound)
    return crule.components(NA + NB, r, NA + c)


def _rows_link(case, arm):
    import torch
    from dctdomain_amd.similarity import cluster_labels
    va, vb = case.view(arm)
    owner = torch.arange(NA + NB, dtype=torch.int32, device='cuda')
    parent = torch.arange(NA + NB, dtype=torch.int32, device='cuda')
    _call('dctfp_rows_link', va.data_ptr(), NA, va.stride(0), 0, vb.data_ptr(), NB, vb.stride(0), NA, case.d, owner.data_ptr(), None, NO_CAP,
          case.bound, parent.data_ptr(), NA + NB)
    return cluster_labels(parent).cpu().numpy()


def _rows_assign(case, arm):
    import torch
    from dctdomain_amd.similarity import rows_assign
    va, vb = case.view(arm)
    assign = torch.full((NB,), NONE, dtype=torch.int32, device='cuda')
    rows_assign(va, vb, assign, case.bound, cap=NO_CAP)
    return assign.cpu().numpy()


def test_rows_link(case, linked):
    assert np.array_equal(_rows_link(case, 16), linked)


def test_rows_assign(case):
    """Per row of b the lowest row of a within the bound (assign_rule's cover pass with value = the row, slot = the column)."""
    within = case.dist <= case.bound
    want = np.where(within.any(axis=0), within.argmax(axis=0), NONE)
    assert len(np.unique(want)) > 2                            # (the lowest row differs from column to column)
    assert np.array_equal(_rows_assign(case, 16), want)


@pytest.mark.parametrize('arm', [4, 1])
def test_rows_on_4_byte_and_1_byte_boundaries_give_the_same(case, linked, arm):
    within = case.dist <= case.bound
    assert np.array_equal(_rows_link(case, arm), linked)
    assert np.array_equal(_rows_assign(case, arm), np.where(within.any(axis=0), within.argmax(axis=0), NONE))
