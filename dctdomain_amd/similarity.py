"""GPU L1 distances between int8 fingerprints (``dctfp_l1_matrix`` / ``dctfp_block_min``): the
arithmetic under the reference's two consumers, ``src/dct-sim.py`` and ``src/query_db.py``."""

from __future__ import annotations

import threading

import numpy as np
import torch

from . import _lib


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError('dctdomain_amd needs an MI355X GPU; there is no CPU fallback')
    return torch.device('cuda', torch.cuda.current_device())


def to_device_int8(fps) -> torch.Tensor:
    t = fps if isinstance(fps, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(fps, dtype=np.int8)))
    if t.dtype != torch.int8:
        t = t.to(torch.int8)
    if t.device.type != 'cuda':
        t = t.to(_dev())
    return t.contiguous()


def _launch(device, name: str, *args):
    """Calls the library's export ``name`` with the context of ``device``, ``args`` and the device's current stream (every
    export's first and last argument: ``_lib.Context.call``); a failure raises what ``_lib.check`` maps its code to."""
    _lib.get_context(device.index).call(name, *args)


def _ld(t: torch.Tensor) -> int:
    """The row stride of a 2-D tensor in elements; its width where there is at most one row (a size-1 axis may carry any stride)."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


# ---- the argument checks, each written once: the library bounds no index on the device, its kernels trust what these let through

def _vector(t: torch.Tensor, dtype, device, what: str, n: int = None, flat: bool = True) -> int:
    """The length of ``t``, which must be a contiguous 1-D tensor of ``dtype`` on ``device`` -- of ``n`` entries, if given.
    ``flat=False``: any shape of that many entries (the columns of the line writers, which never asked for one dimension)."""
    if t.dtype != dtype or (flat and t.dim() != 1) or not t.is_contiguous() or t.device != device or (n is not None and t.numel() != n):
        raise ValueError(f'{what} must be a contiguous {"1-D " if flat else ""}{dtype} tensor'
                         f'{"" if n is None else f" of {n} entries"} on the device of the other arguments')
    return t.numel()


def _check_pair(ta: torch.Tensor, tb: torch.Tensor):
    if ta.dim() != 2 or tb.dim() != 2 or ta.shape[1] != tb.shape[1]:
        raise ValueError('fingerprint sets must be 2-D with equal width')


def _check_prefix(idx: np.ndarray, rows: int):
    """The kernels trust the prefix arrays: checked here."""
    if len(idx) < 1 or idx[0] < 0 or idx[-1] > rows or (np.diff(idx) < 0).any():
        raise ValueError('idx must be a non-decreasing prefix array within its fingerprint matrix')


def _prefix_sides(ta: torch.Tensor, idx_a, tb: torch.Tensor, idx_b):
    """(ia, ib): the prefix arrays of two device fingerprint matrices as int64 numpy arrays, matrices and arrays checked."""
    ia, ib = np.asarray(idx_a, dtype=np.int64), np.asarray(idx_b, dtype=np.int64)
    _check_pair(ta, tb)
    _check_prefix(ia, ta.shape[0])
    _check_prefix(ib, tb.shape[0])
    return ia, ib


def _out_tile(out, n_rows: int, n_cols: int, device) -> torch.Tensor:
    """``out``, or a fresh tile where it is None: int32 (n_rows, n_cols) on ``device`` with unit column stride (any row stride: a
    column range of a wider tile)."""
    if out is None:
        return torch.empty((n_rows, n_cols), dtype=torch.int32, device=device)
    if out.dtype != torch.int32 or tuple(out.shape) != (n_rows, n_cols) or out.device != device or (n_cols > 1 and out.stride(1) != 1):
        raise ValueError(f'out must be an int32 ({n_rows}, {n_cols}) tensor on the fingerprints\' device with unit column stride')
    return out


def _text_buffer(out: torch.Tensor, device):
    """The buffer the line writers fill: contiguous uint8 on ``device``."""
    if out.dtype != torch.uint8 or not out.is_contiguous() or out.device != device:
        raise ValueError('out must be a contiguous uint8 buffer on the device of the other arguments')


def _line_offsets(line_off: torch.Tensor, n: int, device):
    """Where the lines start: contiguous int64 on ``device``, an entry per line at least (a prefix sum has one more)."""
    _vector(line_off, torch.int64, device, 'line_off', flat=False)
    if line_off.numel() < n:
        raise ValueError('line_off must have an entry per line')


def _score_table(table: torch.Tensor):
    """``dct_sim.score_table`` on the device, as the line writers read it: 2 x 17002 rows of 5 bytes, one after the other."""
    if table.dtype != torch.uint8 or table.numel() != 2 * 17002 * 5 or not table.is_contiguous():
        raise ValueError('table must be a contiguous uint8 (2, 17002, 5) tensor')


def l1_matrix(a, b, out: torch.Tensor = None) -> torch.Tensor:
    """int32 (na, nb) matrix of L1 distances, on the GPU.  ``out``: an int32 (na, nb) device tensor with unit column stride to
    write into (any row stride: a column range of a wider tile)."""
    ta, tb = to_device_int8(a), to_device_int8(b)
    _check_pair(ta, tb)
    out = _out_tile(out, ta.shape[0], tb.shape[0], ta.device)
    if out.numel():
        _launch(ta.device, 'dctfp_l1_matrix', ta.data_ptr(), ta.shape[0], _ld(ta), tb.data_ptr(), tb.shape[0], _ld(tb), ta.shape[1],
                out.data_ptr(), _ld(out))
    return out


def block_min(dist: torch.Tensor, idx_a, idx_b):
    """(min, last) int32 arrays of shape (npa, npb) over the protein blocks of ``dist``."""
    ia = torch.as_tensor(np.asarray(idx_a, dtype=np.int64), device=dist.device)
    ib = torch.as_tensor(np.asarray(idx_b, dtype=np.int64), device=dist.device)
    npa, npb = len(ia) - 1, len(ib) - 1
    if dist.numel() == 0:       # proteins without a single fingerprint on either side: every block is empty
        empty = np.full((npa, npb), 0x7fffffff, dtype=np.int32)     # what block_min_kernel writes for an empty block
        return empty, empty.copy()
    return _pair_to_host(*_block_min_launch(dist, ia, ib), np.int32)


def _block_min_launch(dist: torch.Tensor, ia: torch.Tensor, ib: torch.Tensor):
    npa, npb = len(ia) - 1, len(ib) - 1
    mn = torch.empty((npa, npb), dtype=torch.int32, device=dist.device)
    last = torch.empty((npa, npb), dtype=torch.int32, device=dist.device)
    if mn.numel():
        _launch(dist.device, 'dctfp_block_min', dist.data_ptr(), _ld(dist), ia.data_ptr(), npa, ib.data_ptr(), npb, mn.data_ptr(),
                last.data_ptr())
    return mn, last


def block_min_device(dist: torch.Tensor, idx_a, idx_b):
    """``block_min`` with its two (npa, npb) int32 outputs left on the device (contiguous, row stride npb)."""
    ia = torch.as_tensor(np.asarray(idx_a, dtype=np.int64), device=dist.device)
    ib = torch.as_tensor(np.asarray(idx_b, dtype=np.int64), device=dist.device)
    if dist.numel() == 0:       # (block_min_kernel's fill for empty blocks)
        shape = (len(ia) - 1, len(ib) - 1)
        return (torch.full(shape, 0x7fffffff, dtype=torch.int32, device=dist.device),
                torch.full(shape, 0x7fffffff, dtype=torch.int32, device=dist.device))
    return _block_min_launch(dist, ia, ib)


def order_pairs(v: np.ndarray, i: np.ndarray):
    """(values, indices) with every row ordered by (value, index): one sort of packed 64-bit keys instead of ``np.lexsort``
    along an axis (134 ms for 6 700 x 100 pairs, and as long again to apply; this: 5 ms).  int32-range values, indices < 2^32."""
    key = ((v.astype(np.int64) + (1 << 31)).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)
    key.sort(axis=1)
    return (key >> np.uint64(32)).astype(np.int64) - (1 << 31), (key & np.uint64(0xffffffff)).astype(np.int64)


def row_select(dist: torch.Tensor, k: int):
    """(values, indices) numpy arrays (n_rows, k): the k smallest entries of each row, ascending, ties
    to the lower column -- selected (``dctfp_row_select``) and ordered (``dctfp_row_order``, k <= 1024) on the GPU."""
    n_rows, n_cols = dist.shape
    k = min(int(k), n_cols)
    val = torch.empty((n_rows, k), dtype=torch.int32, device=dist.device)
    idx = torch.empty((n_rows, k), dtype=torch.int32, device=dist.device)
    on_device = k <= 1024
    if n_rows:
        _launch(dist.device, 'dctfp_row_select', dist.data_ptr(), n_rows, n_cols, _ld(dist), k, val.data_ptr(), idx.data_ptr())
        if on_device:
            _launch(dist.device, 'dctfp_row_order', val.data_ptr(), idx.data_ptr(), n_rows, k)
    v, i = _pair_to_host(val, idx)
    return (v, i) if on_device else order_pairs(v, i)


_PINNED = threading.local()


def _pair_to_host(val: torch.Tensor, idx: torch.Tensor, dtype=np.int64):
    """Two int32 device tensors of one shape -> numpy arrays through one page-locked staging buffer of this thread (a pageable
    ``.cpu()`` of a tile's 2 x 2.7 MB took 18 ms each on the GPU boxes; this: both in under a millisecond)."""
    n = val.numel()
    pin = getattr(_PINNED, 'buf', None)
    if pin is None or pin.numel() < 2 * n:
        pin = torch.empty(max(2 * n + n // 2, 1 << 18), dtype=torch.int32, pin_memory=True)
        _PINNED.buf = pin
    pin[:n].view(val.shape).copy_(val, non_blocking=True)
    pin[n:2 * n].view(idx.shape).copy_(idx, non_blocking=True)
    torch.cuda.current_stream(val.device).synchronize()
    host = pin[:2 * n].numpy().astype(dtype)                    # (the copy out of the staging buffer, and the widening, in one)
    return host[:n].reshape(val.shape), host[n:].reshape(idx.shape)


class TextStream:
    """Device text out to a host ``sink`` through two pinned buffers: ``hand_over`` starts the copy of a chunk into buffer k % 2 and,
    while it runs, gives ``sink`` the chunk before (a memoryview of the pinned bytes, good for the length of the call);
    ``close`` gives it the last one.  ``room(nbytes)``: the size of a buffer made for a chunk of ``nbytes`` -- one is made when
    the chunk does not fit in what is there."""

    def __init__(self, sink, room=lambda nbytes: nbytes):
        self.sink, self.room = sink, room
        self.pinned, self.held, self.k = [None, None], None, 0

    def hand_over(self, text: torch.Tensor, nbytes: int):
        """The first ``nbytes`` of the device uint8 tensor ``text``, as the current stream leaves them."""
        pin = self.pinned[self.k % 2]                           # (written out by the host two chunks ago)
        if pin is None or pin.numel() < nbytes:
            pin = self.pinned[self.k % 2] = torch.empty(self.room(nbytes), dtype=torch.uint8, pin_memory=True)
        pin[:nbytes].copy_(text[:nbytes], non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(text.device))
        self.close()                                            # the previous chunk goes out while the device works on this one
        self.held = (pin, nbytes, done)
        self.k += 1

    def close(self):
        if self.held is not None:
            (pin, nbytes, done), self.held = self.held, None
            done.synchronize()
            self.sink(memoryview(pin.numpy())[:nbytes])


def _utf8_binary(stream):
    """The binary layer under a text stream whose encoding is UTF-8, else None: where a ``TextStream`` sink may write its bytes."""
    buf = getattr(stream, 'buffer', None)
    enc = (getattr(stream, 'encoding', None) or '').lower().replace('-', '').replace('_', '')
    return buf if buf is not None and enc == 'utf8' else None


def _device_int64(a, device) -> torch.Tensor:
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.int64)), device=device)


def _pair_device_args(a: torch.Tensor, idx_a: torch.Tensor, b: torch.Tensor, idx_b: torch.Tensor, pairs: torch.Tensor):
    """(n, device) of ``pairs``: what the ``*_device`` pair functions ask of arguments that are on the device already."""
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2 or not pairs.is_contiguous():
        raise ValueError('pairs must be a contiguous int32 (n, 2) device tensor')
    if a.dtype != torch.int8 or b.dtype != torch.int8 or a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError('fingerprint sets a / b must be 2-D int8 with equal width')
    if idx_a.dtype != torch.int64 or idx_b.dtype != torch.int64 or not (idx_a.is_contiguous() and idx_b.is_contiguous()):
        raise ValueError('prefix arrays idx_a / idx_b must be contiguous int64 device tensors')
    return pairs.shape[0], pairs.device


def _pair_host_args(a, idx_a, b, idx_b, pairs):
    """(ta, ia, tb, ib, pairs) of the host pair functions: the fingerprints as device int8, the prefix arrays and the (n, 2) pairs
    as int64 numpy arrays -- prefix arrays within their matrices, pair indices within the proteins."""
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    ta, tb = to_device_int8(a), to_device_int8(b)
    ia, ib = _prefix_sides(ta, idx_a, tb, idx_b)
    if len(pairs) and (pairs[:, 0].min() < 0 or pairs[:, 0].max() >= len(ia) - 1 or pairs[:, 1].min() < 0 or pairs[:, 1].max() >= len(ib) - 1):
        raise IndexError('protein index of pairs out of range')
    return ta, ia, tb, ib, pairs


def _pair_scores_device(a: torch.Tensor, idx_a: torch.Tensor, b: torch.Tensor, idx_b: torch.Tensor, pairs: torch.Tensor, arg: bool):
    """The device int32 tensors (min, last) -- with ``arg`` also (arg_a, arg_b) -- of ``pair_min_device`` / ``pair_argmin_device``:
    ``dctfp_pair_min``, or ``dctfp_pair_argmin`` with its two more outputs."""
    n, dev = _pair_device_args(a, idx_a, b, idx_b, pairs)
    out = [torch.full((n,), fill, dtype=torch.int32, device=dev) for fill in (0x7fffffff, 0x7fffffff) + ((-1, -1) if arg else ())]
    if n and a.shape[0] and b.shape[0]:                         # (no fingerprint on a side: every pair is empty)
        _launch(dev, 'dctfp_pair_argmin' if arg else 'dctfp_pair_min', pairs.data_ptr(), n, a.data_ptr(), _ld(a), idx_a.data_ptr(),
                idx_a.numel() - 1, b.data_ptr(), _ld(b), idx_b.data_ptr(), idx_b.numel() - 1, a.shape[1], *(t.data_ptr() for t in out))
    return tuple(out)


def _pair_scores_host(a, idx_a, b, idx_b, pairs, arg: bool):
    """``_pair_scores_device`` for host arguments, which are checked here, as int64 numpy arrays."""
    ta, ia, tb, ib, pairs = _pair_host_args(a, idx_a, b, idx_b, pairs)
    n = len(pairs)
    if n == 0 or ta.shape[0] == 0 or tb.shape[0] == 0:          # (no fingerprint on a side: every pair is empty)
        return tuple(np.full(n, fill, dtype=np.int64) for fill in (0x7fffffff, 0x7fffffff) + ((-1, -1) if arg else ()))
    dev = ta.device
    out = _pair_scores_device(ta, _device_int64(ia, dev), tb, _device_int64(ib, dev), torch.as_tensor(pairs.astype(np.int32), device=dev), arg)
    return _pair_to_host(*out[:2]) + (_pair_to_host(*out[2:]) if arg else ())


def pair_min(a, idx_a, b, idx_b, pairs):
    """(min, last) int64 numpy arrays, one entry per row (protein of ``a``, protein of ``b``) of ``pairs``: the smallest L1 over
    all fingerprint pairs of the two proteins and the L1 of their last rows (``dctfp_pair_min``; no distance matrix).
    ``idx_a`` / ``idx_b``: the npz prefix arrays of the two fingerprint matrices.  A protein without fingerprints gives
    0x7fffffff in both, as ``block_min``."""
    return _pair_scores_host(a, idx_a, b, idx_b, pairs, False)


def pair_min_device(a: torch.Tensor, idx_a: torch.Tensor, b: torch.Tensor, idx_b: torch.Tensor, pairs: torch.Tensor):
    """``pair_min`` with everything on the device already: int8 fingerprint matrices, int64 prefix arrays (the caller's guarantee:
    non-decreasing, within their matrices), ``pairs`` int32 (n, 2) contiguous.  Returns device int32 (min, last); a pair index out
    of range gives -1 in both (the kernel's check)."""
    return _pair_scores_device(a, idx_a, b, idx_b, pairs, False)


def pair_argmin(a, idx_a, b, idx_b, pairs):
    """``pair_min`` with the fingerprint pair the minimum came from (``dctfp_pair_argmin``): (min, last, arg_a, arg_b) int64 numpy
    arrays, ``arg_a`` / ``arg_b`` = rows counted from 0 within the two proteins, ties to the lowest ``arg_a``, then the lowest
    ``arg_b``; -1 in both when the minimum is 17000 or more or a protein has no fingerprints (the reference's loop keeps no pair
    there, src/dct-sim.py:42-50)."""
    return _pair_scores_host(a, idx_a, b, idx_b, pairs, True)


def pair_argmin_device(a: torch.Tensor, idx_a: torch.Tensor, b: torch.Tensor, idx_b: torch.Tensor, pairs: torch.Tensor):
    """``pair_argmin`` with everything on the device already (``pair_min_device``'s arguments and guarantees).  Returns device int32
    (min, last, arg_a, arg_b); a pair index out of range gives -1 in all four (the kernel's check)."""
    return _pair_scores_device(a, idx_a, b, idx_b, pairs, True)


def pair_row_offsets(idx_a, idx_b, pairs) -> np.ndarray:
    """int64 (n + 1): the prefix sum of k + m over the pairs -- where ``pair_row_best`` puts the rows of each pair."""
    ia, ib = np.asarray(idx_a, dtype=np.int64), np.asarray(idx_b, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    off = np.zeros(len(pairs) + 1, dtype=np.int64)
    np.cumsum((ia[pairs[:, 0] + 1] - ia[pairs[:, 0]]) + (ib[pairs[:, 1] + 1] - ib[pairs[:, 1]]), out=off[1:])
    return off


def pair_row_best(a, idx_a, b, idx_b, pairs):
    """Every fingerprint row's counterpart, for the pairs (protein of ``a``, protein of ``b``) of ``pairs`` (``dctfp_pair_row_best``):
    (row_off, l1, arg) numpy int64.  The rows of pair p lie at [row_off[p], row_off[p + 1]): first those of the protein of ``a``,
    then those of the protein of ``b``; ``l1`` = the smallest L1 to any row of the other protein, raw, ``arg`` = that row within the
    other protein, ties to the lowest; 0x7fffffff and -1 where the other protein has no rows.  ``pair_argmin``'s arguments and
    checks."""
    ta, ia, tb, ib, pairs = _pair_host_args(a, idx_a, b, idx_b, pairs)
    off = pair_row_offsets(ia, ib, pairs)
    total = int(off[-1])
    if len(pairs) == 0 or ta.shape[0] == 0 or tb.shape[0] == 0:  # (no fingerprint on a side: no row has a counterpart)
        return off, np.full(total, 0x7fffffff, dtype=np.int64), np.full(total, -1, dtype=np.int64)
    dev = ta.device
    _, l1, arg = pair_row_best_device(ta, _device_int64(ia, dev), tb, _device_int64(ib, dev), torch.as_tensor(pairs.astype(np.int32), device=dev),
                                      _device_int64(off, dev))
    return (off,) + _pair_to_host(l1, arg)


def pair_row_best_device(a: torch.Tensor, idx_a: torch.Tensor, b: torch.Tensor, idx_b: torch.Tensor, pairs: torch.Tensor,
                         row_off: torch.Tensor = None):
    """``pair_row_best`` with everything on the device already (``pair_argmin_device``'s arguments and guarantees).  ``row_off``:
    device int64 (n + 1), made here from the prefix arrays when None.  Returns device (row_off int64, l1 int32, arg int32); the
    kernel leaves the fill, 0x7fffffff and -1, in the rows of a pair whose index is out of range or whose ``row_off`` range is not
    its two proteins' rows."""
    n, dev = _pair_device_args(a, idx_a, b, idx_b, pairs)
    if row_off is None:
        pa, pb = pairs[:, 0].long(), pairs[:, 1].long()
        row_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        if n:
            torch.cumsum((idx_a[pa + 1] - idx_a[pa]) + (idx_b[pb + 1] - idx_b[pb]), 0, out=row_off[1:])
    _vector(row_off, torch.int64, dev, 'row_off (an entry per pair and one more)', n + 1, flat=False)
    total = int(row_off[-1]) if n else 0
    l1 = torch.full((max(total, 0),), 0x7fffffff, dtype=torch.int32, device=dev)
    arg = torch.full((max(total, 0),), -1, dtype=torch.int32, device=dev)
    if n and total > 0 and a.shape[0] and b.shape[0]:           # (no fingerprint on a side: no row has a counterpart)
        _launch(dev, 'dctfp_pair_row_best', pairs.data_ptr(), n, a.data_ptr(), _ld(a), idx_a.data_ptr(), idx_a.numel() - 1, b.data_ptr(),
                _ld(b), idx_b.data_ptr(), idx_b.numel() - 1, a.shape[1], row_off.data_ptr(), total, l1.data_ptr(), arg.data_ptr())
    return row_off, l1, arg


def _rows_view(t) -> torch.Tensor:
    """``to_device_int8`` that leaves a device int8 view with unit column stride and rows that do not overlap as it is (any row
    stride from the width up, any alignment); anything else becomes a contiguous copy."""
    if isinstance(t, torch.Tensor) and t.dtype == torch.int8 and t.device.type == 'cuda' and t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1) \
            and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]):
        return t
    return to_device_int8(t)


def _protein_out(out, ia: np.ndarray, ib: np.ndarray, device):
    """(out, done) for the proteins of ``ia`` x ``ib``: ``out`` checked, or made (``_out_tile``); ``done`` = there is nothing to
    launch -- no protein pair, or no fingerprint on a side: every pair is empty and has its 0x7fffffff from here."""
    out = _out_tile(out, len(ia) - 1, len(ib) - 1, device)
    if out.numel() == 0:
        return out, True
    if ia[-1] == ia[0] or ib[-1] == ib[0]:
        return out.fill_(0x7fffffff), True
    return out, False


def protein_min(a, idx_a, b, idx_b, out: torch.Tensor = None) -> torch.Tensor:
    """int32 (npa, npb) on the device: the smallest L1 over all fingerprint pairs of every (protein of ``a``, protein of ``b``)
    -- DCTdomain's distance, ``block_min(l1_matrix(a, b), idx_a, idx_b)[0]`` without the distance matrix
    (``dctfp_protein_min``).  ``idx_a`` / ``idx_b``: the npz prefix arrays; a protein without fingerprints gives 0x7fffffff.
    ``out``: an int32 (npa, npb) device tensor with unit column stride to write into (any row stride).  Rows not on 16-byte
    boundaries are copied into padded ones; rows wider than 512 bytes (the kernel's limit) take l1_matrix + block_min."""
    ta, tb = _rows_view(a), _rows_view(b)
    ia, ib = _prefix_sides(ta, idx_a, tb, idx_b)
    npa, npb, dev, d = len(ia) - 1, len(ib) - 1, ta.device, ta.shape[1]
    out, done = _protein_out(out, ia, ib, dev)
    if done:
        return out
    if d <= PROTEIN_MIN_MAX_D:
        ta, tb = _rows_on_16(ta, tb)
    da, db = _device_int64(ia, dev), _device_int64(ib, dev)
    try:
        _launch(dev, 'dctfp_protein_min', ta.data_ptr(), _ld(ta), da.data_ptr(), npa, tb.data_ptr(), _ld(tb), db.data_ptr(), npb, d,
                out.data_ptr(), _ld(out))
    except _lib.DctfpError as e:
        if e.code != _lib.DCTFP_ERR_LIMIT:
            raise
        out.copy_(block_min_device(l1_matrix(ta[:, :d], tb[:, :d]), ia, ib)[0])
    return out


COVER_ALL = 0x7ffffffe     # dctfp_protein_cover's largest bound: every row of a pair with rows on both sides is matched


def _device_int32(v, n: int, what: str, device) -> torch.Tensor:
    """``v`` (host values, or a device int32 tensor, copied only where it is not contiguous) as a contiguous device int32 vector of
    ``n`` entries."""
    if isinstance(v, torch.Tensor) and v.device.type == 'cuda':
        t = v.contiguous()
    else:
        t = torch.as_tensor(np.ascontiguousarray(np.asarray(v, dtype=np.int64).astype(np.int32)), device=device)
    _vector(t, torch.int32, device, what, n)
    return t


def protein_cover(a, idx_a, w_a, need_a, b, idx_b, w_b, need_b, bound: int, out: torch.Tensor = None, cap: int = 17000) -> torch.Tensor:
    """``protein_min`` with a coverage requirement (``dctfp_protein_cover``; dct-sim --min-coverage): int32 (npa, npb) on the
    device, the smallest L1 over all fingerprint pairs where the rows of the protein of ``a`` that have a row of the other protein
    within ``bound`` weigh at least ``need_a`` of it (``w_a``: one int32 weight per row of ``a``; ``need_a``: one int32 per
    protein, 0 = no requirement) and likewise for the protein of ``b``; 0x7fffffff where they do not, and for a protein without
    fingerprints.  A row is matched when min(L1, ``cap``) <= ``bound``: a bound of ``cap`` or more goes to the kernel as
    ``COVER_ALL``, a negative one matches no row.  ``out`` and the 16-byte padding of rows as in ``protein_min``; rows wider than
    512 bytes raise ValueError: there is no other route (fingerprints are 480 bytes)."""
    ta, tb = _rows_view(a), _rows_view(b)
    ia, ib = _prefix_sides(ta, idx_a, tb, idx_b)
    npa, npb, dev, d = len(ia) - 1, len(ib) - 1, ta.device, ta.shape[1]
    if d > PROTEIN_MIN_MAX_D:
        raise ValueError(f'protein_cover takes rows of at most {PROTEIN_MIN_MAX_D} bytes, not {d}')
    wa, wb = _device_int32(w_a, ta.shape[0], 'w_a', dev), _device_int32(w_b, tb.shape[0], 'w_b', dev)
    na, nb = _device_int32(need_a, npa, 'need_a', dev), _device_int32(need_b, npb, 'need_b', dev)
    out, done = _protein_out(out, ia, ib, dev)
    if done:
        return out
    ta, tb = _rows_on_16(ta, tb)
    da, db = _device_int64(ia, dev), _device_int64(ib, dev)
    _launch(dev, 'dctfp_protein_cover', ta.data_ptr(), _ld(ta), da.data_ptr(), npa, wa.data_ptr(), na.data_ptr(), tb.data_ptr(), _ld(tb),
            db.data_ptr(), npb, wb.data_ptr(), nb.data_ptr(), d, COVER_ALL if bound >= cap else max(int(bound), -1), out.data_ptr(), _ld(out))
    return out


def threshold_select(dist: torch.Tensor, top: int, bound: int, row_empty=None, col_empty=None, cap: int = 17000):
    """The hits of every row of a last-row distance tile in db_search's order (src/dct-sim.py:146-156): key = min(L1, cap)
    (``cap`` for a row / column flagged empty), ascending, ties to the lower column; the first max(top, #(key <= bound))
    of them.  Counted and selected on the GPU (``dctfp_select_count`` / ``dctfp_select_fill``), rows of up to 1024 hits
    ordered there too.  Returns numpy (offsets int64 (n_rows + 1), keys, columns): row r's hits are [offsets[r], offsets[r+1])."""
    n_rows, n_cols = dist.shape
    if n_rows == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    dev = dist.device
    ld = dist.stride(0) if n_rows > 1 else n_cols
    flags = _empty_flags(row_empty, n_rows, dev), _empty_flags(col_empty, n_cols, dev)
    ptr = [_ptr(f) for f in flags]
    bound = int(max(-1, min(int(bound), cap)))
    count = torch.empty(n_rows, dtype=torch.int32, device=dev)
    cut = torch.empty((n_rows, 2), dtype=torch.int32, device=dev)
    _launch(dev, 'dctfp_select_count', dist.data_ptr(), n_rows, n_cols, ld, ptr[0], ptr[1], cap, bound, max(1, int(top)), count.data_ptr(),
            cut.data_ptr())
    m = count.cpu().numpy().astype(np.int64)
    offsets = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(m, out=offsets[1:])
    key = torch.empty(int(offsets[-1]), dtype=torch.int32, device=dev)
    col = torch.empty(int(offsets[-1]), dtype=torch.int32, device=dev)
    _launch(dev, 'dctfp_select_fill', dist.data_ptr(), n_rows, n_cols, ld, ptr[0], ptr[1], cap, cut.data_ptr(),
            _device_int64(offsets, dev).data_ptr(), int(m.max()), key.data_ptr(), col.data_ptr())
    k, c = _pair_to_host(key, col)
    for r in np.flatnonzero(m > 1024):                             # (rows the device left in column order)
        s = slice(offsets[r], offsets[r + 1])
        o = np.argsort(k[s], kind='stable')
        k[s], c[s] = k[s][o], c[s][o]
    return offsets, k, c


def _empty_flags(flags, n: int, dev):
    """A row / column flag array (or None) as a contiguous device uint8 tensor of ``n`` entries."""
    if flags is None:
        return None
    f = torch.as_tensor(np.asarray(flags, dtype=np.uint8) if not isinstance(flags, torch.Tensor) else flags, device=dev).to(torch.uint8).contiguous()
    if f.numel() != n:
        raise ValueError('empty flags must have one entry per row / column')
    return f


def _ptr(t):
    """The address of an optional device tensor (None: the library's NULL)."""
    return t.data_ptr() if t is not None else None


def _tri_filter_args(tile: torch.Tensor, row0: int, col0: int, bound: int, row_empty, col_empty, cap: int, n_nodes: int = None,
                     range_end: int = None):
    """(n_rows, n_cols, lead, flags) of an L1 tile: ``lead`` = the ten arguments every export that scans a tile starts with (the
    library's ``TriTile``), ``flags`` = the device copies of the flag arrays, which the caller holds until its launch is queued.
    ``n_nodes``: the length of the node arrays beside the tile, which the tile (and ``range_end``, if given) must lie inside."""
    if tile.dtype != torch.int32 or tile.dim() != 2 or tile.device.type != 'cuda' or (tile.shape[1] > 1 and tile.stride(1) != 1):
        raise ValueError('tile must be a 2-D int32 device tensor with unit column stride')
    if row0 < 0 or col0 < 0:
        raise ValueError('row0 / col0 must not be negative')
    n_rows, n_cols = tile.shape
    ld = tile.stride(0) if n_rows > 1 else max(n_cols, 1)
    re, ce = _empty_flags(row_empty, n_rows, tile.device), _empty_flags(col_empty, n_cols, tile.device)
    if n_nodes is not None and (row0 + n_rows > n_nodes or col0 + n_cols > n_nodes or (range_end is not None and not 0 <= range_end <= n_nodes)):
        raise IndexError('tile or range outside the nodes')
    lead = (tile.data_ptr(), n_rows, n_cols, ld, int(row0), int(col0), _ptr(re), _ptr(ce), cap, int(max(-1, min(int(bound), cap))))
    return n_rows, n_cols, lead, (re, ce)


def tri_filter_count(tile: torch.Tensor, row0: int, col0: int, bound: int, row_empty=None, col_empty=None, cap: int = 17000) -> torch.Tensor:
    """Device int32 (n_rows): per row of an L1 tile (entry (r, c) = proteins row0 + r, col0 + c) the entries with
    col0 + c > row0 + r and min(L1, cap) <= bound -- ``cap`` for a row / column flagged empty (``dctfp_tri_filter_count``)."""
    n_rows, n_cols, lead, _flags = _tri_filter_args(tile, row0, col0, bound, row_empty, col_empty, cap)
    count = torch.zeros(n_rows, dtype=torch.int32, device=tile.device)
    if n_rows and n_cols:
        _launch(tile.device, 'dctfp_tri_filter_count', *lead, count.data_ptr())
    return count


def tri_filter_fill(tile: torch.Tensor, row0: int, col0: int, bound: int, count: torch.Tensor, total: int, row_empty=None, col_empty=None,
                    cap: int = 17000):
    """(i, j): device int32 (total) -- the entries ``tri_filter_count`` counted (``count`` = its result for this tile, ``total``
    its sum) as global protein indices, i ascending, then j ascending (``dctfp_tri_filter_fill``; the prefix sum of the counts
    is taken here, on the device)."""
    n_rows, n_cols, lead, _flags = _tri_filter_args(tile, row0, col0, bound, row_empty, col_empty, cap)
    if count.dtype != torch.int32 or count.numel() != n_rows or count.device != tile.device:
        raise ValueError('count must be the int32 device result of tri_filter_count for this tile')
    total = int(total)
    out_i = torch.empty(total, dtype=torch.int32, device=tile.device)
    out_j = torch.empty(total, dtype=torch.int32, device=tile.device)
    if total and n_rows and n_cols:
        offsets = torch.zeros(n_rows + 1, dtype=torch.int64, device=tile.device)
        torch.cumsum(count, 0, out=offsets[1:])
        _launch(tile.device, 'dctfp_tri_filter_fill', *lead, offsets.data_ptr(), total, out_i.data_ptr(), out_j.data_ptr())
    return out_i, out_j


def tri_filter(tile: torch.Tensor, row0: int, col0: int, bound: int, row_empty=None, col_empty=None, cap: int = 17000):
    """(count, i, j) as int64 numpy arrays: ``tri_filter_count`` and ``tri_filter_fill`` on one tile."""
    count = tri_filter_count(tile, row0, col0, bound, row_empty, col_empty, cap)
    m = count.cpu().numpy().astype(np.int64)
    i, j = tri_filter_fill(tile, row0, col0, bound, count, int(m.sum()), row_empty, col_empty, cap)
    return m, i.cpu().numpy().astype(np.int64), j.cpu().numpy().astype(np.int64)


def tri_link(tile: torch.Tensor, row0: int, col0: int, bound: int, parent: torch.Tensor, row_empty=None, col_empty=None, cap: int = 17000):
    """Joins, in the union-find forest ``parent`` (device int32, started as ``torch.arange(n)``), proteins row0 + r and col0 + c
    for every entry of an L1 tile that ``tri_filter_count`` would count (``dctfp_tri_link``).  Nothing comes back: the forest is
    read with ``cluster_labels`` once every tile has been linked."""
    n_nodes = _vector(parent, torch.int32, tile.device, 'parent')
    n_rows, n_cols, lead, _flags = _tri_filter_args(tile, row0, col0, bound, row_empty, col_empty, cap, n_nodes)
    if n_rows and n_cols:
        _launch(tile.device, 'dctfp_tri_link', *lead, parent.data_ptr(), n_nodes)


def link_pairs(pi: torch.Tensor, pj: torch.Tensor, parent: torch.Tensor):
    """Joins proteins pi[n] and pj[n] (device int32, ``tri_filter_fill``'s output) in the forest ``parent`` (``dctfp_link_pairs``);
    the kernel skips a pair that names a node outside it."""
    n_nodes = _vector(parent, torch.int32, pi.device, 'parent')
    for t, what in ((pi, 'pi'), (pj, 'pj')):
        _vector(t, torch.int32, parent.device, what, pi.numel())
    if pi.numel() and n_nodes:
        _launch(parent.device, 'dctfp_link_pairs', pi.data_ptr(), pj.data_ptr(), pi.numel(), parent.data_ptr(), n_nodes)


def rows_link(a, a0: int, b, b0: int, owner: torch.Tensor, parent: torch.Tensor, bound: int, skip=None, cap: int = 17000):
    """Joins, in the forest ``parent`` (one node per fingerprint row of a file), row r of ``a`` (node a0 + r) and row c of ``b``
    (node b0 + c) wherever a0 + r < b0 + c, ``owner`` (device int32, one protein index per node) differs, neither node is flagged
    in ``skip`` (uint8 per node, or None) and min(L1, cap) <= bound (``dctfp_rows_link``): ``l1_matrix``'s contraction with the
    comparison in registers -- no distance is stored.  The library checks the shapes; its codes come back as ``DctfpError``."""
    ta, tb = to_device_int8(a), to_device_int8(b)
    _check_pair(ta, tb)
    n_nodes = _vector(parent, torch.int32, ta.device, 'parent')
    _vector(owner, torch.int32, ta.device, 'owner (one entry per node of parent)', n_nodes)
    flags = _empty_flags(skip, n_nodes, ta.device)
    if ta.shape[0] == 0 or tb.shape[0] == 0:
        return
    _launch(ta.device, 'dctfp_rows_link', ta.data_ptr(), ta.shape[0], _ld(ta), int(a0), tb.data_ptr(), tb.shape[0], _ld(tb), int(b0),
            ta.shape[1], owner.data_ptr(), _ptr(flags), int(cap), int(bound), parent.data_ptr(), n_nodes)


def _row_map(m, n: int, device, what: str):
    if m is None:
        return None
    if not isinstance(m, torch.Tensor):                         # (the one argument that is refused by name where it is a host array)
        raise ValueError(f'{what} must be a device tensor')
    _vector(m, torch.int32, device, f'{what} (one entry per row)', n)
    return m


def rows_assign(a, b, assign: torch.Tensor, bound: int, value_a=None, slot_b=None, a0: int = 0, b0: int = 0, cap: int = 17000):
    """Lowers ``assign[slot]`` (device int32, started as ``GREEDY_NONE``) to ``value`` for every row r of ``a`` and row c of ``b``
    with min(L1, cap) <= bound, where value = ``value_a[r]`` (device int32 per row; None: a0 + r) and slot = ``slot_b[c]`` (None:
    b0 + c) (``dctfp_rows_assign``): ``l1_matrix``'s contraction over the full rectangle with the comparison in registers -- no
    distance is stored.  ``a`` / ``b`` may be views with any row stride and alignment.  The kernel skips a slot outside ``assign``
    and a negative value; the library checks the shapes, its codes come back as ``DctfpError``."""
    ta, tb = _rows_view(a), _rows_view(b)
    _check_pair(ta, tb)
    _vector(assign, torch.int32, ta.device, 'assign')
    va = _row_map(value_a, ta.shape[0], ta.device, 'value_a')
    sb = _row_map(slot_b, tb.shape[0], ta.device, 'slot_b')
    if ta.shape[0] == 0 or tb.shape[0] == 0 or assign.numel() == 0:
        return
    _launch(ta.device, 'dctfp_rows_assign', ta.data_ptr(), ta.shape[0], _ld(ta), _ptr(va), int(a0), tb.data_ptr(), tb.shape[0], _ld(tb), _ptr(sb),
            int(b0), ta.shape[1], int(cap), int(bound), assign.data_ptr(), assign.numel())


def cluster_labels(parent: torch.Tensor) -> torch.Tensor:
    """A new device int32 tensor: labels[x] = the root of x in the forest ``parent`` = the smallest member of x's component
    (``dctfp_cluster_labels``).  ``parent`` stays a forest of the same components (flattened): linking may go on."""
    if parent.device.type != 'cuda':
        raise ValueError('parent must be a device tensor')
    n_nodes = _vector(parent, torch.int32, parent.device, 'parent')
    labels = torch.empty(n_nodes, dtype=torch.int32, device=parent.device)
    if n_nodes:
        _launch(parent.device, 'dctfp_cluster_labels', parent.data_ptr(), n_nodes, labels.data_ptr())
    return labels


TREE_NONE = -1                                 # best as torch shows it: int64 -1 = all 64 bits set = no edge
TREE_MAX_NODES = 1 << 24                       # i and j take 24 bits each of a packed edge


class TreeState:
    """The device arrays of the single-linkage tree over ``n`` nodes (``dctfp_tri_nearest`` / ``dctfp_tree_hook``): ``comp`` (int32,
    this round's labels: ``arange(n)`` at the start), ``best`` (int64 as torch has no uint64 arithmetic: the packed edge
    ``key << 48 | i << 24 | j`` per label, ``TREE_NONE`` = none), ``parent`` (the union-find forest of ``tri_link``), the edge list
    ``edge_i`` / ``edge_j`` / ``edge_key`` (int32, ``max_edges`` = n - 1 slots unless given) and ``counter`` (int32: the edges
    appended so far)."""

    def __init__(self, n: int, device=None, max_edges: int = None):
        device = device if device is not None else _dev()
        self.comp = torch.arange(n, dtype=torch.int32, device=device)
        self.parent = torch.arange(n, dtype=torch.int32, device=device)
        self.best = torch.full((n,), TREE_NONE, dtype=torch.int64, device=device)
        m = max(n - 1, 0) if max_edges is None else int(max_edges)
        self.edge_i, self.edge_j, self.edge_key = (torch.zeros(m, dtype=torch.int32, device=device) for _ in range(3))
        self.counter = torch.zeros(1, dtype=torch.int32, device=device)

    def arrays(self, device) -> int:
        n = self.comp.numel()
        for t, dtype, what in ((self.comp, torch.int32, 'comp'), (self.parent, torch.int32, 'parent'), (self.best, torch.int64, 'best')):
            _vector(t, dtype, device, what, n)
        return n

    def edges(self):
        """(i, j, key): the edges appended so far as int64 numpy arrays, in the order of their slots (one copy; the host waits)."""
        m = min(int(self.counter.item()), self.edge_i.numel())
        return tuple(t[:m].cpu().numpy().astype(np.int64) for t in (self.edge_i, self.edge_j, self.edge_key))


def tri_nearest(tile: torch.Tensor, row0: int, col0: int, bound: int, ts: TreeState, row_empty=None, col_empty=None, cap: int = 17000):
    """Lowers ``ts.best`` of both labels to the packed edge of every entry of an L1 tile that ``tri_filter_count`` would count and
    whose two proteins carry different labels in ``ts.comp`` (``dctfp_tri_nearest``): one round's candidates for the lightest
    edge out of every component.  ``tree_hook`` ends the round once every tile has been through."""
    n_nodes = ts.arrays(tile.device)
    n_rows, n_cols, lead, _flags = _tri_filter_args(tile, row0, col0, bound, row_empty, col_empty, cap, n_nodes)
    if n_rows and n_cols:
        _launch(tile.device, 'dctfp_tri_nearest', *lead, ts.comp.data_ptr(), ts.best.data_ptr(), n_nodes)


def tree_hook(ts: TreeState):
    """Ends a round (``dctfp_tree_hook``): every label of ``ts.comp`` appends the edge ``ts.best`` holds for it to the edge list
    (``ts.counter`` grows; an edge chosen from both sides once) and joins its ends in ``ts.parent``; ``ts.best`` is none again
    afterwards.  ``ts.comp`` is the caller's to renew: ``ts.comp = cluster_labels(ts.parent)``."""
    n_nodes = ts.arrays(ts.comp.device)
    edges = (ts.edge_i, ts.edge_j, ts.edge_key)
    for t, what in zip(edges, ('edge_i', 'edge_j', 'edge_key')):
        _vector(t, torch.int32, ts.comp.device, what, ts.edge_i.numel())
    if ts.counter.dtype != torch.int32 or ts.counter.numel() != 1 or ts.counter.device != ts.comp.device:
        raise ValueError('counter must be one int32 on the device')
    if n_nodes:
        _launch(ts.comp.device, 'dctfp_tree_hook', ts.comp.data_ptr(), ts.best.data_ptr(), ts.parent.data_ptr(), n_nodes,
                *(t.data_ptr() if t.numel() else None for t in edges), ts.counter.data_ptr(), ts.edge_i.numel())


LINKAGE_MAX_N = _lib.LINKAGE_MAX_N             # dctfp_linkage_*'s limit: n * n fits 31 bits and S * c fits 63
LINKAGE_NONE = {torch.int32: 0x7fffffff, torch.int64: 0x7fffffffffffffff}     # the diagonal: passes no bound test


def _linkage_args(mat: torch.Tensor, size: torch.Tensor, arrays):
    """(n, lead) of a linkage matrix: ``lead`` = (address, wide, n, ld), the arguments both exports of include/dctfp_linkage.h take
    first.  ``mat``: 2-D device int32 (complete linkage) or int64 (average), unit column stride, n = ``len(size)`` columns and
    at most n rows; ``arrays``: the int32 node arrays beside it."""
    if mat.dtype not in LINKAGE_NONE or mat.dim() != 2 or mat.device.type != 'cuda' or (mat.shape[1] > 1 and mat.stride(1) != 1):
        raise ValueError('the matrix must be a 2-D int32 or int64 device tensor with unit column stride')
    n = size.numel()
    if mat.shape[1] != n or mat.shape[0] > n:
        raise ValueError('the matrix has one column per entry of size and no more rows than columns')
    if n > LINKAGE_MAX_N:
        raise ValueError(f'at most {LINKAGE_MAX_N} nodes')
    for t in (size, *arrays):
        _vector(t, torch.int32, mat.device, 'size and each array beside it')
    return n, (mat.data_ptr(), int(mat.dtype == torch.int64), n, mat.stride(0) if mat.shape[0] > 1 else max(n, 1))


def linkage_nearest(mat: torch.Tensor, size: torch.Tensor, live: torch.Tensor, bound: int, nn: torch.Tensor = None) -> torch.Tensor:
    """Step 1 of a round of complete (int32 ``mat``) or average (int64) linkage (``dctfp_linkage_nearest``): device int32 ``nn``, for
    every a of ``live`` the x != a with ``size[x] > 0`` and D(a, x) <= ``bound`` that minimises (D(a, x), x), -1 = none; D is the
    entry, or for int64 the entry over ``size[a] * size[x]`` as an exact fraction.  The entries of ``nn`` (made here, all -1, unless
    given) for ids outside ``live`` are left alone.  ``mat`` may hold the first rows of the matrix only when ``live`` names no other."""
    n, lead = _linkage_args(mat, size, (live,) if nn is None else (live, nn))
    if nn is None:
        nn = torch.full((n,), -1, dtype=torch.int32, device=mat.device)
    if nn.numel() != n or live.numel() > n:
        raise ValueError('nn has one entry per node and live at most as many')
    if live.numel() and mat.shape[0] < n and not 0 <= int(live.min()) <= int(live.max()) < mat.shape[0]:
        raise IndexError('a live id outside the rows of the matrix')
    if n and live.numel():
        _launch(mat.device, 'dctfp_linkage_nearest', *lead, size.data_ptr(), live.data_ptr(), live.numel(), int(max(-1, bound)), nn.data_ptr())
    return nn


def linkage_merge(mat: torch.Tensor, size: torch.Tensor, partner: torch.Tensor, keep: torch.Tensor):
    """Step 2 of a round, in place (``dctfp_linkage_merge``): ``partner[x]`` = the other cluster of x's pair, -1 = none; ``keep`` = the
    lower id of every pair.  Every entry between a cluster of ``keep`` and a cluster that lives on becomes the maximum (int32) or
    the sum (int64) of the up to four entries of the clusters they consist of, on both sides of the diagonal.  Rows and columns of
    the absorbed clusters keep their values: the caller sets their ``size`` to 0, which masks them in ``linkage_nearest``."""
    n, lead = _linkage_args(mat, size, (partner, keep))
    if mat.shape[0] != n or partner.numel() != n or 2 * keep.numel() > n:
        raise ValueError('a square matrix, one partner per node and at most n / 2 pairs')
    if n and keep.numel():
        _launch(mat.device, 'dctfp_linkage_merge', *lead, size.data_ptr(), partner.data_ptr(), keep.data_ptr(), keep.numel())


BEST_NONE = -1                                 # best_row / best_col as torch shows them: int64 -1 = all 64 bits set = no hit


class BestState:
    """The device arrays of the reciprocal best hits of ``n_a`` x ``n_b`` proteins (``dctfp_rect_best``): ``best_row`` (one entry per
    protein of A) and ``best_col`` (per protein of B), int64 as torch has no uint64 arithmetic: the packed hit
    ``key << 32 | index on the other side``, ``BEST_NONE`` = none."""

    def __init__(self, n_a: int, n_b: int, device=None):
        device = device if device is not None else _dev()
        self.best_row = torch.full((n_a,), BEST_NONE, dtype=torch.int64, device=device)
        self.best_col = torch.full((n_b,), BEST_NONE, dtype=torch.int64, device=device)

    def arrays(self, device):
        """(n_a, n_b), the arrays checked."""
        return _vector(self.best_row, torch.int64, device, 'best_row'), _vector(self.best_col, torch.int64, device, 'best_col')

    def hits(self):
        """((index, key) per protein of A, (index, key) per protein of B) as int64 numpy arrays: the best hit on the other side and
        its key, -1 in both where there is none (two copies of 8 bytes per protein; the host waits)."""
        out = []
        for t in (self.best_row, self.best_col):
            v = t.cpu().numpy()
            none = v == BEST_NONE
            out.append((np.where(none, -1, v & 0xffffffff), np.where(none, -1, v >> 32)))
        return tuple(out)


def rect_best(tile: torch.Tensor, row0: int, col0: int, bound: int, state: BestState, row_empty=None, col_empty=None, cap: int = 17000):
    """Lowers ``state.best_row[row0 + r]`` to ``key << 32 | (col0 + c)`` and ``state.best_col[col0 + c]`` to ``key << 32 | (row0 + r)``
    for every entry (r, c) of an L1 tile -- the full rectangle, protein row0 + r of one file against protein col0 + c of another --
    with key = min(L1, cap) <= bound, ``cap`` for a row / column flagged empty (``dctfp_rect_best``).  Packed that way, the
    minimum is the best hit with ties to the lower index; it does not depend on how the rectangle is cut into tiles."""
    n_a, n_b = state.arrays(tile.device)
    n_rows, n_cols, lead, _flags = _tri_filter_args(tile, row0, col0, bound, row_empty, col_empty, cap)
    if row0 + n_rows > n_a or col0 + n_cols > n_b:
        raise IndexError('tile outside the proteins of the state')
    if n_rows and n_cols:
        _launch(tile.device, 'dctfp_rect_best', *lead, state.best_row.data_ptr(), n_a, state.best_col.data_ptr(), n_b)


MOMENT_LIMIT = 255 * 480 + 1                   # above every L1 of two int8 fingerprints of the widest kind (480 columns)


class MomentState:
    """The device arrays of the background moments of ``n_a`` x ``n_b`` proteins (``dctfp_rect_moments``): ``row`` (3, n_a) for the
    proteins of A and ``col`` (3, n_b) for those of B, zeroed -- the planes count, sum and sum of squares of the L1s that counted.
    int64 as torch has no uint64 arithmetic: a sum of squares of 2^63 or more shows negative here and is the same 64 bits.
    ``rows=False`` / ``cols=False``: that side is None and ``rect_moments`` does not compute it."""

    def __init__(self, n_a: int, n_b: int, rows: bool = True, cols: bool = True, device=None):
        device = device if device is not None else _dev()
        self.n_a, self.n_b = int(n_a), int(n_b)
        self.row = torch.zeros((3, self.n_a), dtype=torch.int64, device=device) if rows else None
        self.col = torch.zeros((3, self.n_b), dtype=torch.int64, device=device) if cols else None

    def arrays(self, device):
        """(n_a, n_b), the arrays checked."""
        if self.row is None and self.col is None:
            raise ValueError('a MomentState without rows and without cols has nothing to add to')
        for t, n in ((self.row, self.n_a), (self.col, self.n_b)):
            if t is not None and (t.dtype != torch.int64 or t.shape != (3, n) or not t.is_contiguous() or t.device != device):
                raise ValueError('row / col must be contiguous int64 tensors of shape (3, n) on the device of the other arguments')
        return self.n_a, self.n_b

    def moments(self):
        """(row, col): the numpy int64 arrays (3, n), None for a side the state does not have (one copy per side; the host waits)."""
        return tuple(t.cpu().numpy() if t is not None else None for t in (self.row, self.col))


def rect_moments(tile: torch.Tensor, row0: int, col0: int, state: MomentState, row_empty=None, col_empty=None, limit: int = MOMENT_LIMIT):
    """Adds (1, x, x^2) to ``state.row[:, row0 + r]`` and to ``state.col[:, col0 + c]`` for every entry (r, c) of an L1 tile -- the full
    rectangle, protein row0 + r of one file against protein col0 + c of another -- whose row and column are not flagged empty and
    whose value x lies in 0 .. limit - 1 (``dctfp_rect_moments``).  ``limit`` excludes, it does not cap: ``protein_min``'s 0x7fffffff
    and a negative value are left out, every other value counts raw.  The words are exact integers and add up over tiles and
    calls; they do not depend on how the rectangle is cut into tiles or on the order of the calls."""
    n_a, n_b = state.arrays(tile.device)
    n_rows, n_cols, lead, _flags = _tri_filter_args(tile, row0, col0, limit, row_empty, col_empty, int(limit))
    if (state.row is not None and row0 + n_rows > n_a) or (state.col is not None and col0 + n_cols > n_b):
        raise IndexError('tile outside the proteins of the state')
    if n_rows and n_cols:
        _launch(tile.device, 'dctfp_rect_moments', *lead, _ptr(state.row), n_a, _ptr(state.col), n_b)


SILHOUETTE_PASS_CLUSTERS = _lib.DCTFP_SILHOUETTE_MAX_PASS_CLUSTERS     # cluster sums in the LDS of a workgroup at a time: the default


def silhouette_rows(tile: torch.Tensor, row0: int, col0: int, cid: torch.Tensor, size: torch.Tensor, first: torch.Tensor,
                    own_sum: torch.Tensor, near_sum: torch.Tensor, near_size: torch.Tensor, near_first: torch.Tensor, row_empty=None,
                    col_empty=None, cap: int = 17000, pass_clusters: int = SILHOUETTE_PASS_CLUSTERS):
    """The sums behind the silhouette of the rows of an L1 tile of ONE file (``dctfp_silhouette_rows``; include/dctfp_silhouette.h
    has the rule): entry (r, c) = proteins row0 + r and col0 + c, the columns being the whole file.  ``cid`` (device int32, one per
    protein): the dense id of the protein's cluster if that has two or more members, -1 for a singleton; ``size`` / ``first``
    (device int32, one per id): the members of every such cluster and the first of them.  For every row i = row0 + r, with key =
    min(L1, cap) -- ``cap`` for a row / column flagged empty -- over the columns j != i: ``own_sum[i]`` = the summed key over i's own
    cluster, and (``near_sum[i]``, ``near_size[i]``, ``near_first[i]``) = (sum, members, first member) of the other cluster with the
    smallest mean key, an exact comparison with ties to the lower first member; (0, 0, -1) where there is no other cluster.  The
    sums are device int64 (the library's uint64; they stay below 2^53), one entry per protein like the two int32 arrays; only the
    entries of the tile's rows are written.  ``pass_clusters``: the cluster sums a workgroup keeps at a time (the row is read once
    per that many clusters; the results do not depend on it).  The library cannot check ``cid`` against the arrays it indexes:
    that is done here, on the host, at one small device reduction per call."""
    dev = tile.device
    n_nodes = _vector(cid, torch.int32, dev, 'cid (one entry per protein)')
    n_clusters = _vector(size, torch.int32, dev, 'size (one entry per cluster)')
    _vector(first, torch.int32, dev, 'first (one entry per cluster)', n_clusters)
    for t, dtype, what in ((own_sum, torch.int64, 'own_sum'), (near_sum, torch.int64, 'near_sum'), (near_size, torch.int32, 'near_size'),
                           (near_first, torch.int32, 'near_first')):
        _vector(t, dtype, dev, f'{what} (one entry per protein)', n_nodes)
    n_rows, n_cols, lead, _flags = _tri_filter_args(tile, row0, col0, cap, row_empty, col_empty, cap, n_nodes)
    if n_nodes and not -1 <= int(cid.min()) <= int(cid.max()) < n_clusters:
        raise IndexError('a cluster id outside -1 .. the number of clusters - 1')
    if n_rows and n_cols:
        _launch(dev, 'dctfp_silhouette_rows', *lead[:-1], cid.data_ptr(), _ptr(size if n_clusters else None),
                _ptr(first if n_clusters else None), n_clusters, int(pass_clusters), own_sum.data_ptr(), near_sum.data_ptr(),
                near_size.data_ptr(), near_first.data_ptr(), n_nodes)


def _node_arrays(tile: torch.Tensor, arrays) -> int:
    """n_nodes of the per-protein arrays beside a tile -- ``arrays`` = (tensor, dtype, name): contiguous 1-D device tensors of one
    length on the tile's device."""
    n_nodes = arrays[0][0].numel()
    for t, dtype, what in arrays:
        _vector(t, dtype, tile.device, f'{what} (one entry per protein)', n_nodes)
    return n_nodes


def _band_pass(export: str, tile: torch.Tensor, row0: int, col0: int, bound: int, row_empty, col_empty, cap: int, arrays):
    """What the passes over a tile of ONE file share: the per-protein ``arrays`` checked (``_node_arrays``), the tile described with
    them as its nodes (``_tri_filter_args``), and ``export`` launched -- the tile, the arrays in their order, n_nodes -- unless the
    tile is empty."""
    n_nodes = _node_arrays(tile, arrays)
    n_rows, n_cols, lead, _flags = _tri_filter_args(tile, row0, col0, bound, row_empty, col_empty, cap, n_nodes)
    if n_rows and n_cols:
        _launch(tile.device, export, *lead, *(t.data_ptr() for t, _dtype, _what in arrays), n_nodes)


def label_sums(tile: torch.Tensor, row0: int, col0: int, labels: torch.Tensor, sums: torch.Tensor, row_empty=None, col_empty=None,
               cap: int = 17000):
    """Adds key = min(L1, cap) -- ``cap`` for a row / column flagged empty -- of every entry (r, c) of an L1 tile of ONE file with
    col0 + c > row0 + r and ``labels[row0 + r] == labels[col0 + c]`` to ``sums[row0 + r]`` and to ``sums[col0 + c]``
    (``dctfp_label_sums``).  ``labels``: device int32, one per protein (``cluster_labels``); ``sums``: device int64 of the same
    length (torch has no uint64 arithmetic; the sums stay far below 2^63), zeroed by the caller before the first tile.  After every
    tile of the triangle ``sums[x]`` is the summed distance of x to the other members of its cluster; integer addition commutes, so
    it does not depend on how the triangle is cut into tiles or on the order of the calls."""
    _band_pass('dctfp_label_sums', tile, row0, col0, cap, row_empty, col_empty, cap,
                ((labels, torch.int32, 'labels'), (sums, torch.int64, 'sums')))


NEAREST_NONE = 0x7fffffff                      # nearest: no core neighbour


def tri_degree(tile: torch.Tensor, row0: int, col0: int, bound: int, deg: torch.Tensor, row_empty=None, col_empty=None, cap: int = 17000):
    """Adds 1 to ``deg[row0 + r]`` and to ``deg[col0 + c]`` for every entry (r, c) of an L1 tile of ONE file that ``tri_filter_count``
    would count: col0 + c > row0 + r and min(L1, cap) <= bound, ``cap`` for a row / column flagged empty (``dctfp_tri_degree``).
    ``deg``: device int32, one per protein (the library's uint32: a degree stays below 2^31), zeroed by the caller before the first
    tile.  After every tile of the triangle ``deg[x]`` is the number of pairs within the bound that x is in; a count does not depend
    on how the triangle is cut into tiles or on the order of the calls."""
    _band_pass('dctfp_tri_degree', tile, row0, col0, bound, row_empty, col_empty, cap, ((deg, torch.int32, 'deg'),))


def tri_link_core(tile: torch.Tensor, row0: int, col0: int, bound: int, core: torch.Tensor, parent: torch.Tensor, nearest: torch.Tensor,
                  row_empty=None, col_empty=None, cap: int = 17000):
    """The second pass of the density clusters over an L1 tile (``dctfp_tri_link_core``): of the entries ``tri_degree`` counted, one
    whose two proteins are both flagged in ``core`` (device uint8, one per protein) joins them in the forest ``parent`` (as
    ``tri_link``; read with ``cluster_labels``), one with exactly one core end lowers ``nearest`` of the other end (device int32,
    ``NEAREST_NONE`` at the start) to the core's index, one without a core end does nothing.  After every tile ``nearest[x]`` of a
    non-core x is its lowest core neighbour; neither result depends on the tiling or on the order of the calls."""
    _band_pass('dctfp_tri_link_core', tile, row0, col0, bound, row_empty, col_empty, cap,
                ((core, torch.uint8, 'core'), (parent, torch.int32, 'parent'), (nearest, torch.int32, 'nearest')))


def tri_first_fp(tile: torch.Tensor, row0: int, col0: int, bound: int, fam: torch.Tensor, first: torch.Tensor, row_empty=None,
                 col_empty=None, cap: int = 17000):
    """The first pass of ``dct-sim --auc1`` over an L1 tile of ONE file (``dctfp_tri_first_fp``): every entry (r, c) that
    ``tri_degree`` would count -- col0 + c > row0 + r and key = min(L1, cap) <= bound, ``cap`` for a row / column flagged empty --
    whose proteins i = row0 + r and j = col0 + c are of two families (``fam``: device int32, one per protein) lowers ``first[i]`` to
    ``key << 32 | j`` and ``first[j]`` to ``key << 32 | i``.  ``first``: device int64, one per protein, held as ``BestState`` holds
    its words (torch has no uint64 arithmetic) and filled with ``BEST_NONE`` by the caller before the first tile.  After every tile
    of the triangle ``first[x]`` is the best-ranked hit of x from another family, ties to the lower index; a minimum does not
    depend on how the triangle is cut into tiles or on the order of the calls."""
    _band_pass('dctfp_tri_first_fp', tile, row0, col0, bound, row_empty, col_empty, cap,
                ((fam, torch.int32, 'fam'), (first, torch.int64, 'first')))


def tri_tp_before(tile: torch.Tensor, row0: int, col0: int, bound: int, fam: torch.Tensor, first: torch.Tensor, tp: torch.Tensor,
                  row_empty=None, col_empty=None, cap: int = 17000):
    """The second pass of ``dct-sim --auc1`` (``dctfp_tri_tp_before``), with the ``first`` that ``tri_first_fp`` left after every
    tile: an entry ``tri_degree`` would count whose two proteins are of one family adds 1 to ``tp[i]`` when ``key << 32 | j`` is
    below ``first[i]`` (as unsigned words) and, decided on its own, 1 to ``tp[j]`` when ``key << 32 | i`` is below ``first[j]``.
    ``tp``: device int32, one per protein (the library's uint32), zeroed by the caller before the first tile.  After every tile
    ``tp[x]`` is the number of hits of x's own family ranked before its first false positive; a count does not depend on the tiling
    or on the order of the calls."""
    _band_pass('dctfp_tri_tp_before', tile, row0, col0, bound, row_empty, col_empty, cap,
                ((fam, torch.int32, 'fam'), (first, torch.int64, 'first'), (tp, torch.int32, 'tp')))


def tri_hist(tile: torch.Tensor, row0: int, col0: int, bound: int, hist: torch.Tensor, fam: torch.Tensor = None, row_empty=None,
             col_empty=None, cap: int = 17000):
    """Adds 1 to ``hist[cls, key]`` for every entry (r, c) of an L1 tile of ONE file that ``tri_degree`` would count -- col0 + c >
    row0 + r and key = min(L1, cap) <= bound, ``cap`` for a row / column flagged empty (``dctfp_tri_hist``).  ``hist``: a contiguous
    device int64 tensor (the library's uint64; a count stays far below 2^63) of shape (1 or 2, cap + 1), zeroed by the caller before
    the first tile.  Without ``fam`` there is one class, ``cls = 0``, and one row; with ``fam`` (device int32, one family per
    protein) ``cls = (fam[row0 + r] != fam[col0 + c])`` and ``hist`` has two rows: the pairs of one family, then the pairs of two.
    The counts add up over the tiles of the triangle and over calls; integer addition commutes, so they do not depend on how the
    triangle is cut into tiles or on the order of the calls."""
    if hist.dtype != torch.int64 or hist.dim() != 2 or not hist.is_contiguous() or hist.device != tile.device or hist.shape[1] != cap + 1:
        raise ValueError('hist must be a contiguous int64 tensor of shape (classes, cap + 1) on the device of the tile')
    if hist.shape[0] != (1 if fam is None else 2):
        raise ValueError('hist has one row without fam and two rows with it')
    if fam is not None:
        n_nodes = _node_arrays(tile, ((fam, torch.int32, 'fam'),))
    else:
        n_nodes = max(int(row0) + tile.shape[0], int(col0) + tile.shape[1]) if tile.dim() == 2 else 0
    n_rows, n_cols, lead, _flags = _tri_filter_args(tile, row0, col0, bound, row_empty, col_empty, cap, n_nodes)
    if n_rows and n_cols:
        _launch(tile.device, 'dctfp_tri_hist', *lead, _ptr(fam), n_nodes, hist.data_ptr())


GREEDY_NONE = 0x7fffffff                       # assign: no representative yet
GREEDY_UNDECIDED, GREEDY_MEMBER, GREEDY_NEW, GREEDY_DONE = 0, 1, 2, 3


class GreedyState:
    """The device arrays of the greedy linkage over ``n`` nodes (``dctfp_greedy_decide``): ``assign`` (the lowest representative
    seen so far, ``GREEDY_NONE`` at the start), ``state`` (``GREEDY_UNDECIDED`` at the start) and ``blocked`` (round stamps), int32
    each, and ``undecided``, the int64 word the decide launches add the nodes they leave undecided to."""

    def __init__(self, n: int, device=None):
        device = device if device is not None else _dev()
        self.assign = torch.full((n,), GREEDY_NONE, dtype=torch.int32, device=device)
        self.state = torch.zeros(n, dtype=torch.int32, device=device)
        self.blocked = torch.zeros(n, dtype=torch.int32, device=device)
        self.undecided = torch.zeros(1, dtype=torch.int64, device=device)
        self._read = 0

    def left(self) -> int:
        """The nodes the decide launches since the last call left undecided (one copy of 8 bytes: the host waits here)."""
        total = int(self.undecided.item())
        new, self._read = total - self._read, total
        return new

    def arrays(self, device) -> int:
        for t, what in ((self.assign, 'assign'), (self.state, 'state'), (self.blocked, 'blocked')):
            _vector(t, torch.int32, device, what, self.assign.numel())
        return self.assign.numel()


def greedy_decide(gs: GreedyState, i0: int, i1: int, round: int):
    """One decide launch over the nodes [i0, i1) (``dctfp_greedy_decide``): round 0 makes members only; ``gs.left()`` then says how
    many nodes of the range are still undecided."""
    n_nodes = gs.arrays(gs.assign.device)
    if not 0 <= i0 <= i1 <= n_nodes:
        raise IndexError('range outside the nodes')
    if i1 > i0:
        _launch(gs.assign.device, 'dctfp_greedy_decide', gs.assign.data_ptr(), gs.state.data_ptr(), gs.blocked.data_ptr(), n_nodes, int(i0), int(i1),
                int(round), gs.undecided.data_ptr())


def greedy_tri_mark(tile: torch.Tensor, row0: int, col0: int, bound: int, gs: GreedyState, range_end: int, next_round: int, row_empty=None,
                    col_empty=None, cap: int = 17000):
    """The mark launch of a round from an L1 tile (``dctfp_greedy_tri_mark``): over the entries ``tri_filter_count`` would count, a
    row that is a new representative lowers ``assign`` of its columns, an undecided row stamps ``blocked`` of its columns below
    ``range_end`` with ``next_round``."""
    n_nodes = gs.arrays(tile.device)
    n_rows, n_cols, lead, _flags = _tri_filter_args(tile, row0, col0, bound, row_empty, col_empty, cap, n_nodes, range_end)
    if n_rows and n_cols:
        _launch(tile.device, 'dctfp_greedy_tri_mark', *lead, gs.assign.data_ptr(), gs.state.data_ptr(), gs.blocked.data_ptr(), n_nodes,
                int(range_end), int(next_round))


def greedy_pairs_mark(pi: torch.Tensor, pj: torch.Tensor, gs: GreedyState, range_end: int, next_round: int):
    """The mark launch of a round from pairs (pi[n], pj[n]) (device int32, ``tri_filter_fill``'s output; ``dctfp_greedy_pairs_mark``);
    the kernel skips a pair that names a node outside the state."""
    n_nodes = gs.arrays(pi.device)
    for t, what in ((pi, 'pi'), (pj, 'pj')):
        _vector(t, torch.int32, gs.assign.device, what, pi.numel())
    if not 0 <= range_end <= n_nodes:
        raise IndexError('range outside the nodes')
    if pi.numel() and n_nodes:
        _launch(pi.device, 'dctfp_greedy_pairs_mark', pi.data_ptr(), pj.data_ptr(), pi.numel(), gs.assign.data_ptr(), gs.state.data_ptr(),
                gs.blocked.data_ptr(), n_nodes, int(range_end), int(next_round))


class LineIds:
    """The protein ids of a file as ``dctfp_sim_lines`` reads them: ``off`` = int64 prefix offsets of their UTF-8 bytes (host),
    ``bytes_dev`` / ``off_dev`` = the concatenated bytes and the offsets on the device."""

    def __init__(self, names, device=None):
        device = device if device is not None else _dev()
        enc = [str(s).encode('utf8') for s in names]
        self.lens = np.fromiter((len(e) for e in enc), dtype=np.int64, count=len(enc))
        self.off = np.zeros(len(enc) + 1, dtype=np.int64)
        np.cumsum(self.lens, out=self.off[1:])
        raw = np.frombuffer(bytearray(b''.join(enc)), dtype=np.uint8)
        self.bytes_dev = torch.as_tensor(raw if len(raw) else np.zeros(1, dtype=np.uint8), device=device)
        self.off_dev = _device_int64(self.off, device)
        self.lens_dev = _device_int64(self.lens, device)


def sim_lines(mn: torch.Tensor, last: torch.Tensor, row0: int, col0: int, ids: LineIds, table: torch.Tensor, row_base, out: torch.Tensor):
    """all_sim's text for a (min, last) device tile (``block_min_device``): the lines (row0 + r, col0 + c) with column > row, row
    r's lines from byte ``row_base[r]`` of the device uint8 buffer ``out`` (``dctfp_sim_lines``; include/dctfp.h has the
    layout).  ``table``: device uint8 (2, 17002, 5), ``dct_sim.score_table``.  Every line must fit in ``out``: checked here."""
    n_rows, n_cols = mn.shape
    row_base = np.asarray(row_base, dtype=np.int64)
    n = len(ids.off) - 1
    if last.shape != mn.shape or len(row_base) != n_rows or mn.dtype != torch.int32 or last.dtype != torch.int32:
        raise ValueError('mn / last must be int32 tiles of one shape, one row base per row')
    if not (mn.is_contiguous() and last.is_contiguous()):
        raise ValueError('mn / last must be contiguous')
    _score_table(table)
    _text_buffer(out, out.device)
    if n_rows == 0 or n_cols == 0:
        return
    if row0 < 0 or col0 < 0 or row0 + n_rows > n or col0 + n_cols > n:
        raise IndexError('tile outside the proteins of the id list')
    i = row0 + np.arange(n_rows, dtype=np.int64)              # (the kernel trusts its offsets: bound every row's last line here)
    j_hi = col0 + n_cols
    live = j_hi > i + 1
    ends = row_base[live] + (j_hi - i[live] - 1) * (ids.lens[i[live]] + 14) + (ids.off[j_hi] - ids.off[i[live] + 1])
    if (row_base < 0).any() or (len(ends) and ends.max() > out.numel()):
        raise ValueError('the lines do not fit in the output buffer')
    base = _device_int64(row_base, mn.device)
    _launch(mn.device, 'dctfp_sim_lines', mn.data_ptr(), last.data_ptr(), n_cols, n_rows, int(row0), int(col0), n_cols,
            ids.bytes_dev.data_ptr(), ids.off_dev.data_ptr(), table.data_ptr(), base.data_ptr(), out.data_ptr())


def pair_line_offsets(pi: torch.Tensor, pj: torch.Tensor, ids: LineIds, la: torch.Tensor = None, lb: torch.Tensor = None,
                      labels: LineIds = None) -> torch.Tensor:
    """Device int64 (n + 1): where the ``pair_lines`` lines of the pairs (pi[n], pj[n]) start -- the prefix sum of len_i + len_j + 14,
    with ``labels`` (and the label indices la[n], lb[n]) + len_label_a + len_label_b + 2; the last entry is the text's size."""
    off = torch.zeros(pi.numel() + 1, dtype=torch.int64, device=pi.device)
    if pi.numel():
        lens = ids.lens_dev[pi.long()] + ids.lens_dev[pj.long()] + 14
        if labels is not None:
            lens += labels.lens_dev[la.long()] + labels.lens_dev[lb.long()] + 2
        torch.cumsum(lens, 0, out=off[1:])
    return off


def pair_lines(pi: torch.Tensor, pj: torch.Tensor, mn: torch.Tensor, last: torch.Tensor, ids: LineIds, table: torch.Tensor,
               line_off: torch.Tensor, out: torch.Tensor, la: torch.Tensor = None, lb: torch.Tensor = None, labels: LineIds = None):
    """all_sim's text for a list of pairs: line n = ``"{id of pi[n]} {id of pj[n]} {a} {b}\\n"`` from byte ``line_off[n]`` of the
    device uint8 buffer ``out`` (``dctfp_pair_lines``), a / b from ``table`` (``dct_sim.score_table`` on the device) by ``mn`` /
    ``last``.  All device tensors: int32 pairs and values, int64 offsets (``pair_line_offsets``).  The kernel skips a line that
    names a protein outside ``ids`` or that ends beyond ``out``.

    ``labels`` adds the domain pair behind the scores: ``"... {a} {b} {label la[n]} {label lb[n]}\\n"``
    (``dctfp_pair_domain_lines``).  ``labels``: the label table of the file as a ``LineIds`` -- one entry per fingerprint row, then
    the "no pair" entry; ``la`` / ``lb``: device int32 indices into it, also given to ``pair_line_offsets``.  A line that names a
    label outside ``labels`` is skipped too."""
    n = pi.numel()
    cols = (pi, pj, mn, last) + ((la, lb) if labels is not None else ())
    for t, what in zip(cols, ('pi', 'pj', 'mn', 'last', 'la', 'lb')):
        _vector(t, torch.int32, out.device, what, n, flat=False)
    _line_offsets(line_off, n, out.device)
    _score_table(table)
    _text_buffer(out, out.device)
    if n == 0:
        return
    tail = (table.data_ptr(), line_off.data_ptr(), out.data_ptr(), out.numel())
    if labels is None:
        _launch(out.device, 'dctfp_pair_lines', n, *(t.data_ptr() for t in cols), ids.bytes_dev.data_ptr(), ids.off_dev.data_ptr(),
                len(ids.off) - 1, *tail)
    else:
        _launch(out.device, 'dctfp_pair_domain_lines', n, *(t.data_ptr() for t in cols), ids.bytes_dev.data_ptr(), ids.off_dev.data_ptr(),
                len(ids.off) - 1, labels.bytes_dev.data_ptr(), labels.off_dev.data_ptr(), len(labels.off) - 1, *tail)


def pair_domain_line_offsets(pi: torch.Tensor, pj: torch.Tensor, la: torch.Tensor, lb: torch.Tensor, ids: LineIds,
                             labels: LineIds) -> torch.Tensor:
    """``pair_line_offsets`` with labels, in the argument order of ``pair_domain_lines``."""
    return pair_line_offsets(pi, pj, ids, la, lb, labels)


def pair_domain_lines(pi: torch.Tensor, pj: torch.Tensor, mn: torch.Tensor, last: torch.Tensor, la: torch.Tensor, lb: torch.Tensor,
                      ids: LineIds, labels: LineIds, table: torch.Tensor, line_off: torch.Tensor, out: torch.Tensor):
    """``pair_lines`` with labels (``line_off``: ``pair_domain_line_offsets``)."""
    pair_lines(pi, pj, mn, last, ids, table, line_off, out, la, lb, labels)


def _pair_map_args(pi, pj, mn, last, la, lb, ids: LineIds, labels: LineIds, table, first_row, row_off, row_l1, row_arg, bound: int):
    """The checked arguments the two passes of ``dctfp_pair_map_lines`` share, as (head, tail): the line buffer goes between them."""
    n, dev = pi.numel(), pi.device
    for t, what in zip((pi, pj, mn, last, la, lb), ('pi', 'pj', 'mn', 'last', 'la', 'lb')):
        _vector(t, torch.int32, dev, what, n, flat=False)
    _score_table(table)
    _vector(row_off, torch.int64, dev, 'row_off (an entry per line and one more)', n + 1, flat=False)
    _vector(first_row, torch.int64, dev, 'first_row (an entry per protein and one more)', len(ids.off), flat=False)
    for t, what in ((row_l1, 'row_l1'), (row_arg, 'row_arg')):
        _vector(t, torch.int32, dev, what, row_l1.numel(), flat=False)
    if not -1 <= int(bound) < 17000:
        raise ValueError('the bound of a map is an L1 of similarity above 0: -1 .. 16999')
    head = (n, pi.data_ptr(), pj.data_ptr(), mn.data_ptr(), last.data_ptr(), la.data_ptr(), lb.data_ptr(), ids.bytes_dev.data_ptr(),
            ids.off_dev.data_ptr(), len(ids.off) - 1, labels.bytes_dev.data_ptr(), labels.off_dev.data_ptr(), len(labels.off) - 1,
            table.data_ptr())
    tail = (row_off.data_ptr(), row_l1.numel(), _ptr(row_l1) or row_off.data_ptr(), _ptr(row_arg) or row_off.data_ptr(), first_row.data_ptr(),
            int(bound))
    return head, tail


def pair_map_line_lengths(pi, pj, mn, last, la, lb, ids: LineIds, labels: LineIds, table, first_row, row_off, row_l1, row_arg,
                          bound: int) -> torch.Tensor:
    """Device int64 (n): the bytes of every ``pair_map_lines`` line -- the count pass of ``dctfp_pair_map_lines``, the same kernel
    body as the text; 0 for a line the fill would skip."""
    head, tail = _pair_map_args(pi, pj, mn, last, la, lb, ids, labels, table, first_row, row_off, row_l1, row_arg, bound)
    count = torch.zeros(pi.numel(), dtype=torch.int64, device=pi.device)
    if pi.numel():
        _launch(pi.device, 'dctfp_pair_map_lines', *head, None, None, 0, *tail, count.data_ptr())
    return count


def pair_map_lines(pi, pj, mn, last, la, lb, ids: LineIds, labels: LineIds, table, first_row, row_off, row_l1, row_arg, bound: int,
                   line_off: torch.Tensor, out: torch.Tensor):
    """``pair_lines`` with labels and the domain map of every pair: line n = ``"... {label la[n]} {label lb[n]} {side}/{side}\\n"``
    from byte ``line_off[n]`` of ``out`` (the fill pass of ``dctfp_pair_map_lines``).  ``row_off`` / ``row_l1`` / ``row_arg``:
    ``pair_row_best_device`` of the pairs; ``first_row``: device int64, the prefix array of the file whose rows ``labels`` names;
    ``bound``: a row is matched when its L1 is at most this.  ``line_off``: the prefix sum of ``pair_map_line_lengths``."""
    head, tail = _pair_map_args(pi, pj, mn, last, la, lb, ids, labels, table, first_row, row_off, row_l1, row_arg, bound)
    _line_offsets(line_off, pi.numel(), out.device)
    _text_buffer(out, pi.device)
    if pi.numel() and out.numel():
        _launch(out.device, 'dctfp_pair_map_lines', *head, line_off.data_ptr(), out.data_ptr(), out.numel(), *tail, None)


KNN_MAX_K = 1024     # dctfp_l1_knn's limits: larger k or wider rows take l1_matrix + row_select
KNN_MAX_D = 512
KNN_SCRATCH_BYTES = 1 << 31
PROTEIN_MIN_MAX_D = 512   # dctfp_protein_min's limit: wider rows take l1_matrix + block_min


def _aligned16(t: torch.Tensor) -> bool:
    return (t.data_ptr() | _ld(t)) & 15 == 0 and t.stride(1) == 1


def _rows16(t: torch.Tensor, w: int) -> torch.Tensor:
    """``t`` copied into zero-padded rows of ``w`` bytes (what dctfp_l1_knn reads: rows on 16-byte boundaries; zeros on both
    sides add nothing to an L1 distance)."""
    out = torch.zeros((t.shape[0], w), dtype=torch.int8, device=t.device)
    out[:, :t.shape[1]] = t
    return out


def _rows_on_16(ta: torch.Tensor, tb: torch.Tensor):
    """Both matrices with their rows on 16-byte boundaries: as they are, or both as padded copies of one width."""
    if _aligned16(ta) and _aligned16(tb):
        return ta, tb
    w = (ta.shape[1] + 15) // 16 * 16
    return _rows16(ta, w), _rows16(tb, w)


def l1_knn_device(q, db, k: int, col0: int = 0):
    """(values, indices): device int32 (nq, min(k, nb)) -- each query row's k nearest database rows by L1, ascending, ties to the
    lower row, ``col0`` added to the indices (``dctfp_l1_knn``: distances and selection in one kernel, no distance matrix).
    What ``row_select(l1_matrix(q, db), k)`` returns; k > 1024 or rows wider than 512 bytes go that way."""
    tq, tb = to_device_int8(q), to_device_int8(db)
    _check_pair(tq, tb)
    nq, nb, d = tq.shape[0], tb.shape[0], tq.shape[1]
    k = min(int(k), nb)
    dev = tq.device
    if nq == 0 or k <= 0:
        return (torch.empty((nq, max(k, 0)), dtype=torch.int32, device=dev), torch.empty((nq, max(k, 0)), dtype=torch.int32, device=dev))
    if k > KNN_MAX_K or d > KNN_MAX_D:
        v, i = row_select(l1_matrix(tq, tb), k)
        return (torch.as_tensor(v.astype(np.int32), device=dev), torch.as_tensor((i + col0).astype(np.int32), device=dev))
    tq, tb = _rows_on_16(tq, tb)
    val = torch.empty((nq, k), dtype=torch.int32, device=dev)
    idx = torch.empty((nq, k), dtype=torch.int32, device=dev)
    # query rows per call sized by the scratch they take: 2 k-lists of k 8-byte keys per (row, database slice), and with several
    # slices (only when there are few row tiles) the slices' lists once more and a half -- about 2 GiB at most per call
    step = max(128, KNN_SCRATCH_BYTES // (32 * k) // 128 * 128)
    for q0 in range(0, nq, step):
        qs = tq[q0:q0 + step]
        _launch(dev, 'dctfp_l1_knn', qs.data_ptr(), qs.shape[0], _ld(qs), tb.data_ptr(), nb, _ld(tb), tq.shape[1], k, int(col0),
                val[q0:].data_ptr(), idx[q0:].data_ptr())
    return val, idx


def l1_knn(q, db, k: int, col0: int = 0):
    """``l1_knn_device`` as int64 numpy arrays: the same pair as ``row_select(l1_matrix(q, db), k)`` (indices + ``col0``)."""
    val, idx = l1_knn_device(q, db, k, col0)
    if val.numel() == 0:
        return np.zeros(tuple(val.shape), np.int64), np.zeros(tuple(idx.shape), np.int64)
    return _pair_to_host(val, idx)
