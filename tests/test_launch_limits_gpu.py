"""The rows of one launch, on the GPU: dctfp_row_order, dctfp_select_count and dctfp_cluster_labels at the largest size
include/dctfp.h accepts (cluster_labels: at 2^26 nodes, its limit of 2^31 - 1 does not fit a test), where the workgroup of the last
row is the last one a launch can hold -- HIP launches nothing whose gridDim.x * blockDim.x reaches 2^32.  tests/test_host_asan.py
proves on the CPU that these sizes launch and that one more is refused before anything is launched; here the kernels run, and the
last rows, where an index that wrapped or a grid that was cut short would show, are compared with numpy.  One size above the limit
comes back as the library's DCTFP_ERR_LIMIT with the buffers (allocated in full: nothing here could write outside them) untouched."""
import numpy as np
import pytest

import cluster_rule as crule

pytestmark = pytest.mark.gpu

ROW_ORDER_MAX_ROWS = 0xffffffff // 512       # include/dctfp.h, dctfp_row_order: a workgroup of up to 512 threads per row
SELECT_MAX_ROWS = 0xffffffff // 1024         # dctfp_select_count: one 1024-thread workgroup per row
TAIL = 1000


@pytest.fixture(scope='module')
def sim():
    import torch
    from dctdomain_amd import _lib, similarity
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch, _lib, similarity


def _sample(n, rng):
    """The last TAIL rows, the first ten and 4096 of the rest."""
    return np.unique(np.concatenate([np.arange(n - TAIL, n), np.arange(10), rng.integers(0, n, 4096)]))


def test_row_order_at_its_largest_accepted_size(sim):
    torch, _lib, similarity = sim
    dev = torch.device('cuda', 0)
    n, k = ROW_ORDER_MAX_ROWS, 2                                   # k = 2: row_order_kernel<128>, 64 threads per row
    g = torch.Generator(device=dev).manual_seed(5)
    val = torch.randint(0, 50, (n, k), dtype=torch.int32, device=dev, generator=g)       # (few values: ties, broken by the column)
    idx = torch.randint(0, 1000, (n, k), dtype=torch.int32, device=dev, generator=g)
    val[:-TAIL] = val[:-TAIL].sort(dim=1).values                   # in order but for ties ...
    val[-TAIL:, 0] = 60                                            # ... and every one of the last rows out of order
    rows = _sample(n, np.random.default_rng(6))
    pick = torch.from_numpy(rows).to(dev)
    v0, i0 = val[pick].cpu().numpy().astype(np.int64), idx[pick].cpu().numpy().astype(np.int64)
    assert (v0[-TAIL:, 0] > v0[-TAIL:, 1]).all()
    similarity._launch(dev, 'dctfp_row_order', val.data_ptr(), idx.data_ptr(), n, k)
    torch.cuda.synchronize(dev)
    order = np.lexsort((i0, v0), axis=1)                           # by value, ties by column
    want_v, want_i = np.take_along_axis(v0, order, 1), np.take_along_axis(i0, order, 1)
    got_v, got_i = val[pick].cpu().numpy(), idx[pick].cpu().numpy()
    assert np.array_equal(got_v, want_v) and np.array_equal(got_i, want_i)
    assert bool((val[:, 0] <= val[:, 1]).all())                    # every row of the launch, the cheap half of the property


def test_row_order_refuses_one_row_more(sim):
    torch, _lib, similarity = sim
    dev = torch.device('cuda', 0)
    n = ROW_ORDER_MAX_ROWS + 1
    val = torch.ones((n, 2), dtype=torch.int32, device=dev)
    val[:, 1] = 0                                                  # out of order everywhere: a launch would show
    idx = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    with pytest.raises(_lib.DctfpError) as err:
        similarity._launch(dev, 'dctfp_row_order', val.data_ptr(), idx.data_ptr(), n, 2)
    assert err.value.code == _lib.DCTFP_ERR_LIMIT and str(ROW_ORDER_MAX_ROWS) in str(err.value)
    torch.cuda.synchronize(dev)
    assert int(val[:, 0].sum()) == n and int(val[:, 1].sum()) == 0


@pytest.mark.parametrize('n_cols', [1, 3])
def test_select_count_at_its_largest_accepted_size(sim, n_cols):
    torch, _lib, similarity = sim
    dev = torch.device('cuda', 0)
    n, cap, bound, top = SELECT_MAX_ROWS, 17000, 5000, 1
    g = torch.Generator(device=dev).manual_seed(7 + n_cols)
    dist = torch.randint(0, 30000, (n, n_cols), dtype=torch.int32, device=dev, generator=g)
    count = torch.full((n,), -1, dtype=torch.int32, device=dev)
    cut = torch.empty((n, 2), dtype=torch.int32, device=dev)
    similarity._launch(dev, 'dctfp_select_count', dist.data_ptr(), n, n_cols, n_cols, None, None, cap, bound, top, count.data_ptr(), cut.data_ptr())
    torch.cuda.synchronize(dev)
    rows = _sample(n, np.random.default_rng(8))
    pick = torch.from_numpy(rows).to(dev)
    key = np.minimum(dist[pick].cpu().numpy().astype(np.int64), cap)
    want = np.minimum(n_cols, np.maximum(top, (key <= bound).sum(axis=1)))      # include/dctfp.h: m = min(n_cols, max(top, #(key <= bound)))
    assert np.array_equal(count[pick].cpu().numpy(), want)
    whole = torch.clamp((torch.clamp(dist, max=cap) <= bound).sum(dim=1), min=top, max=n_cols)
    assert torch.equal(count.long(), whole)                        # ... and every row of the launch


def test_select_count_refuses_one_row_more(sim):
    torch, _lib, similarity = sim
    dev = torch.device('cuda', 0)
    n = SELECT_MAX_ROWS + 1
    dist = torch.zeros((n, 1), dtype=torch.int32, device=dev)
    count = torch.full((n,), -1, dtype=torch.int32, device=dev)
    cut = torch.empty((n, 2), dtype=torch.int32, device=dev)
    with pytest.raises(_lib.DctfpError) as err:
        similarity._launch(dev, 'dctfp_select_count', dist.data_ptr(), n, 1, 1, None, None, 17000, 5000, 1, count.data_ptr(), cut.data_ptr())
    assert err.value.code == _lib.DCTFP_ERR_LIMIT and str(SELECT_MAX_ROWS) in str(err.value)
    torch.cuda.synchronize(dev)
    assert int(count.sum()) == -n


def test_cluster_labels_with_chains_into_the_last_nodes(sim):
    torch, _lib, similarity = sim
    dev = torch.device('cuda', 0)
    n, chains, length = 1 << 26, 3, 100000
    tail = chains * length
    parent = torch.arange(n, dtype=torch.int32, device=dev)
    # three interleaved chains over the last `tail` nodes, each 100 000 deep and ending in one of the last three nodes: parent[x] = x - 3
    x = torch.arange(n - tail + chains, n, dtype=torch.int64, device=dev)
    parent[x] = (x - chains).to(torch.int32)
    edges_i = np.arange(n - tail + chains, n, dtype=np.int64) - (n - tail)
    want_tail = crule.components(tail, edges_i, edges_i - chains).astype(np.int64) + (n - tail)      # the sequential union-find, on the tail
    assert set(want_tail[-chains:]) == {n - tail, n - tail + 1, n - tail + 2}
    labels = similarity.cluster_labels(parent)
    torch.cuda.synchronize(dev)
    assert np.array_equal(labels[n - tail:].cpu().numpy(), want_tail)
    head = torch.arange(n - tail, dtype=torch.int32, device=dev)
    assert torch.equal(labels[:n - tail], head)                    # every node before the chains is its own root
    rows = _sample(n - tail, np.random.default_rng(9))
    assert np.array_equal(labels[torch.from_numpy(rows).to(dev)].cpu().numpy(), rows)
    assert torch.equal(parent[n - tail:].long(), torch.from_numpy(want_tail).to(dev))   # left flattened: a forest of the same components
