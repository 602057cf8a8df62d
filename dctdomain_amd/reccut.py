"""Domain prediction step of the reference's ``Fingerprint`` (mgtools/DCTdomain
src/fingerprint.py:45-107) without the Python pair list, the .ce temp file and the RecCut
subprocess:

* the top ``int(t * L)`` contacts with ``j >= i + 5`` are selected on the GPU
  (``dctfp_contact_topk``; the reference builds and sorts an O(L^2) Python list, :54-67);
* the domain boundaries come from ``libreccut.so`` in-process (include/reccut.h; the
  reference spawns ``src/RecCut`` on a text file, :92-100).

``write_ce`` still writes the byte-identical .ce text for users of that file format."""

from __future__ import annotations

import threading
from typing import List, Sequence

import numpy as np
import torch

from itertools import repeat

from . import _lib

CUT1_DEFAULT = 0.08      # src/RecCut.cpp:12
CUT2_DEFAULT = 0.07      # src/RecCut.cpp:13


def _contact_tensor(contacts, n_res: int, device=None) -> torch.Tensor:
    if isinstance(contacts, torch.Tensor):
        t = contacts
        if t.dtype == torch.float32 and t.is_cuda and t.dim() == 2 and t.shape[0] == n_res and t.shape[1] == n_res \
                and t.stride(1) == 1:
            return t                            # straight off the language model: nothing to do
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(contacts, dtype=np.float32)))
    t = t.reshape(n_res, n_res)                 # cta = self.contacts.reshape(slen, slen)
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.device.type != 'cuda':
        if not torch.cuda.is_available():
            raise RuntimeError('dctdomain_amd needs an MI355X GPU; there is no CPU fallback')
        t = t.to(device if device is not None else torch.device('cuda', torch.cuda.current_device()))
    if t.stride(1) != 1:
        t = t.contiguous()
    return t


_PINNED = threading.local()


def _pinned(name: str, dtype, n: int) -> torch.Tensor:
    """A page-locked staging buffer of this thread (grown geometrically): device -> host copies of a flush's contacts run
    at the PCIe rate instead of the pageable one."""
    buf = getattr(_PINNED, name, None)
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(n + n // 2, 1 << 16), dtype=dtype, pin_memory=True)
        setattr(_PINNED, name, buf)
    return buf[:n]


def _pinned_take(name: str, dtype, n: int) -> torch.Tensor:
    """A page-locked buffer of at least ``n`` elements from this thread's free list ``name`` (grown as ``_pinned`` grows its
    own), owned by the caller until ``_pinned_give`` puts it back."""
    free = _PINNED.__dict__.setdefault('free_' + name, [])
    buf = free.pop() if free else None
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(n + n // 2, 1 << 16), dtype=dtype, pin_memory=True)
    return buf


def _pinned_give(name: str, buf: torch.Tensor):
    _PINNED.__dict__.setdefault('free_' + name, []).append(buf)


def contact_counts(n_res, t: float):
    """(counts, offs) of ``dctfp_contact_count`` for all proteins at once: ``min(int(t * L), (L-5)(L-4)/2)`` contacts with
    j >= i + 5 each; protein p's are ``[offs[p], offs[p+1])``."""
    L64 = np.asarray(n_res, dtype=np.int64)
    cand = np.where(L64 >= 6, (L64 - 5) * (L64 - 4) // 2, 0)
    counts = np.minimum(np.maximum((float(t) * L64.astype(np.float64)).astype(np.int64), 0), cand)
    offs = np.zeros(len(L64) + 1, dtype=np.int64)
    np.cumsum(counts, out=offs[1:])
    return counts, offs


def map_geometry(maps: Sequence[torch.Tensor]):
    """(ptrs, lds, n_res) of a list of contact maps, as ``dctfp_contact_topk`` takes them (C-level passes over the list:
    three generator passes over 4 096 maps cost 3 ms)."""
    n = len(maps)
    n_res = np.fromiter(map(len, maps), dtype=np.int32, count=n)
    ptrs = np.fromiter(map(torch.Tensor.data_ptr, maps), dtype=np.uint64, count=n)
    lds = np.fromiter(map(torch.Tensor.stride, maps, repeat(0)), dtype=np.int64, count=n)
    lds = np.where(n_res > 1, lds, np.maximum(n_res.astype(np.int64), 1))      # (a one-row map may carry any stride)
    return ptrs, lds, n_res


def enqueue_topk(ptrs, lds, n_res, t: float, device, stream):
    """``dctfp_contact_topk`` on ``stream``, everything left on the device: (counts, offs [host], oi, oj, ov, on [device]);
    ``on[p]`` is what the kernel wrote for protein p, to be held to ``counts``."""
    n = len(n_res)
    counts, offs = contact_counts(n_res, t)
    total = max(int(offs[-1]), 1)
    with torch.cuda.stream(stream):
        oi = torch.empty(total, dtype=torch.int32, device=device)
        oj = torch.empty(total, dtype=torch.int32, device=device)
        ov = torch.empty(total, dtype=torch.float32, device=device)
        on = torch.zeros(n, dtype=torch.int32, device=device)
    _lib.get_context(device.index).call('dctfp_contact_topk', ptrs.ctypes.data, lds.ctypes.data, n_res.ctypes.data, n, float(t),
                                        oi.data_ptr(), oj.data_ptr(), ov.data_ptr(), offs.ctypes.data, on.data_ptr(), stream=stream)
    return counts, offs, oi, oj, ov, on


def _check_counts(written: np.ndarray, counts: np.ndarray):
    if not (written == counts).all():
        raise RuntimeError('dctfp_contact_topk wrote a different number of contacts than dctfp_contact_count says')


def top_contacts_batch(maps: Sequence[torch.Tensor], t: float, sort: bool = True, own: bool = True):
    """Top ``int(t*L)`` contacts of each map.  Returns (offs, i, j, v) as numpy arrays: protein
    p's contacts are ``[offs[p], offs[p+1])``; with ``sort`` they are ordered by (-v, i, j) -- the
    order of the reference's CON line (the domain cutter itself does not care about the order).

    Selection (``dctfp_contact_topk``) and order (``dctfp_contact_sort``) both happen on the GPU; what comes back is one
    copy of the selected entries through page-locked buffers.  ``own=False`` returns views of those buffers instead of
    copies of them (64 MB for 4 096 proteins of 500 residues: 5 of the call's 12 ms): valid until this thread's next call."""
    n = len(maps)
    if n == 0:
        return np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    device = maps[0].device
    stream = torch.cuda.current_stream(device)
    ptrs, lds, n_res = map_geometry(maps)
    counts, offs, oi, oj, ov, on = enqueue_topk(ptrs, lds, n_res, t, device, stream)
    total = int(offs[-1])
    on_device = np.ones(n, dtype=np.uint8)
    if sort:
        _lib.get_context(device.index).call('dctfp_contact_sort', ptrs.ctypes.data, lds.ctypes.data, n_res.ctypes.data, n, float(t),
                                            oi.data_ptr(), oj.data_ptr(), ov.data_ptr(), offs.ctypes.data, on_device.ctypes.data,
                                            stream=stream)
    pi, pj, pv, pn = (_pinned('i', torch.int32, total), _pinned('j', torch.int32, total), _pinned('v', torch.float32, total),
                      _pinned('n', torch.int32, n))
    pi.copy_(oi[:total], non_blocking=True)
    pj.copy_(oj[:total], non_blocking=True)
    pv.copy_(ov[:total], non_blocking=True)
    pn.copy_(on, non_blocking=True)
    stream.synchronize()
    hi, hj, hv = pi.numpy(), pj.numpy(), pv.numpy()
    if own:
        hi, hj, hv = hi.copy(), hj.copy(), hv.copy()
    _check_counts(pn.numpy(), counts)
    for p in (np.flatnonzero(on_device == 0) if sort else ()):       # longer than the device network holds (L > 6 301)
        a, b = offs[p], offs[p + 1]
        order = np.lexsort((hj[a:b], hi[a:b], -hv[a:b].astype(np.float64)))
        hi[a:b], hj[a:b], hv[a:b] = hi[a:b][order], hj[a:b][order], hv[a:b][order]
    return offs, hi, hj, hv


#: proteins of this thread's last ``CutInFlight.wait`` (``domains_from_maps``, ``domains_from_contacts_gpu``, a database flush)
#: that went through the host library (``host_redo``), and the GPU's own times of the last timed one (``gpu_ms``: top-k, cutter,
#: copies) -- tests and profiles read them
LAST = threading.local()


def reccut_room(n_res: np.ndarray) -> np.ndarray:
    """``dctfp_reccut_room`` for an array of lengths (the C function is the definition; tests hold this to it)."""
    n = np.asarray(n_res, dtype=np.int64)
    doms = np.where(n > 0, n // 22 + 1, 1)
    return 2 + doms + 2 * (2 * doms + 1)


class CutInFlight:
    """The domain cutter of a batch (``dctfp_reccut``), enqueued on ``stream``, the encoded results on their way into a
    page-locked buffer; ``wait()`` picks them up.  The one GPU cut pipeline: a database flush starts it early and waits for it
    when it needs the domains (``make_db.Flush``), ``domains_from_maps`` / ``domains_from_contacts_gpu`` wait at once.

    ``CutInFlight(ptrs, lds, n_res, device, t, ...)`` selects the contacts first (``dctfp_contact_topk``) from the contact
    maps' geometry (``map_geometry`` / ``_geom.tensor_table``); ``CutInFlight.from_contacts`` cuts contact lists already on the
    device.  Its page-locked result buffers are its own, from this thread's free list, until ``release()``: any number of
    batches may be in flight at once."""

    def __init__(self, ptrs, lds, n_res, device, t: float, cut1=CUT1_DEFAULT, cut2=CUT2_DEFAULT, stream=None,
                 timing: bool = False):
        self._setup(n_res, device, cut1, cut2, stream, timing)
        self._record(0)
        self.counts, self.offs, self.oi, self.oj, self.ov, on = enqueue_topk(
            np.ascontiguousarray(ptrs, dtype=np.uint64), np.ascontiguousarray(lds, dtype=np.int64), self.n_res, t, device,
            self.stream)
        self._record(1)
        self._enqueue_cut(device, on)

    @classmethod
    def from_contacts(cls, n_res, offs, oi, oj, ov, device, cut1=CUT1_DEFAULT, cut2=CUT2_DEFAULT, stream=None):
        """The cutter alone on contact lists on the device: protein p's are ``[offs[p], offs[p+1])`` of ``oi`` / ``oj`` / ``ov``."""
        self = cls.__new__(cls)
        self._setup(n_res, device, cut1, cut2, stream, False)
        self.offs = np.ascontiguousarray(offs, dtype=np.int64)
        self.counts = np.diff(self.offs)
        self.oi, self.oj, self.ov = oi, oj, ov
        self._enqueue_cut(device, None)
        return self

    def _setup(self, n_res, device, cut1, cut2, stream, timing):
        self.n_res = np.ascontiguousarray(n_res, dtype=np.int32)
        self.n = len(self.n_res)
        self.cut1, self.cut2 = float(cut1), float(cut2)
        self.stream = stream if stream is not None else torch.cuda.current_stream(device)
        self.events = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if timing else None    # (tools/flush_timeline.py)

    def _record(self, i):
        if self.events is not None:
            self.events[i].record(self.stream)

    def _enqueue_cut(self, device, on):
        """``dctfp_reccut`` behind whatever is on the stream, then the copies of its results (and of ``on``, the contacts top-k
        wrote) into page-locked buffers of this batch's own."""
        n = self.n
        self.enc_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(reccut_room(self.n_res), out=self.enc_off[1:])
        n_enc = int(self.enc_off[-1])
        with torch.cuda.stream(self.stream):
            enc = torch.empty(n_enc, dtype=torch.int32, device=device)
            _lib.get_context(device.index).call('dctfp_reccut', self.n_res.ctypes.data, n, self.oi.data_ptr(), self.oj.data_ptr(),
                                                self.ov.data_ptr(), self.offs.ctypes.data, self.cut1, self.cut2, enc.data_ptr(),
                                                self.enc_off.ctypes.data, stream=self.stream)
            self._record(2)
            self._pins = (_pinned_take('enc', torch.int32, n_enc), _pinned_take('n', torch.int32, n) if on is not None else None)
            self.penc = self._pins[0][:n_enc]
            self.penc.copy_(enc, non_blocking=True)
            self.pn = None
            if on is not None:
                self.pn = self._pins[1][:n]
                self.pn.copy_(on, non_blocking=True)
            self._record(3)
            self.done = torch.cuda.Event()
            self.done.record(self.stream)
        self._keep = (enc, on)

    def wait(self, threads: int = 1, strings: bool = False):
        """Waits for the results and redoes in the host library (on ``threads`` threads, with each protein's own contacts) what
        the GPU cutter handed back.  Without ``strings``: the encoded results (host view, valid until ``release()``), the
        proteins with status < 1 redone and written into the same encoding (where a record does not fit, the status stays -1
        and the caller sees it).  With ``strings``: per protein the binary's domain strings (``reccut_format_packed``), every
        protein the format flags redone -- status < 1 or a record it cannot read."""
        self.done.synchronize()
        if self.events is not None:
            e = self.events
            LAST.gpu_ms = (e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e[2].elapsed_time(e[3]))   # top-k, cutter, copies
        if self.pn is not None:
            _check_counts(self.pn.numpy(), self.counts)
        enc = self.penc.numpy()
        if strings:
            doms, redo = _format_packed(self.n, enc, self.enc_off, self.n_res)
        else:
            redo = np.flatnonzero(enc[self.enc_off[:-1]] < 1)
        LAST.host_redo = redo.tolist()
        if len(redo):      # the host library on these proteins' own contacts (copied over now: they are few)
            sel_off = np.zeros(len(redo) + 1, dtype=np.int64)
            np.cumsum(self.counts[redo], out=sel_off[1:])
            pick = np.concatenate([np.arange(self.offs[p], self.offs[p + 1]) for p in redo]) if sel_off[-1] else np.zeros(0, np.int64)
            pick_t = torch.from_numpy(pick).to(self.oi.device)
            hi, hj, hv = (x[pick_t].cpu().numpy() for x in (self.oi, self.oj, self.ov))
            for p, d in zip(redo.tolist(), domains_from_contacts(self.n_res[redo], sel_off, hi, hj, hv, self.cut1, self.cut2,
                                                                 threads=threads)):
                if strings:
                    doms[p] = d
                    continue
                rec = _encode_domains(d)
                a, b = int(self.enc_off[p]), int(self.enc_off[p + 1])
                if rec is not None and len(rec) <= b - a:
                    enc[a:a + len(rec)] = rec
        return doms if strings else enc

    def release(self):
        """Waits for the copies into the page-locked result buffers and puts those back on this thread's free list."""
        if self._pins is not None:
            self.done.synchronize()
            _pinned_give('enc', self._pins[0])
            if self._pins[1] is not None:
                _pinned_give('n', self._pins[1])
            self._pins = self.penc = self.pn = None


def _format_packed(n: int, enc: np.ndarray, enc_off: np.ndarray, n_res: np.ndarray):
    """``reccut_format_packed``: (per protein the domain strings, proteins it flags for the host library)."""
    rlib = _lib.load_reccut()
    cap = 64 * n + 16 * int(n_res.astype(np.int64).sum())
    buf = np.empty(cap, dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.int64)
    nd = np.zeros(n, dtype=np.int32)
    needs = np.zeros(n, dtype=np.uint8)
    ret = rlib.reccut_format_packed(n, enc.ctypes.data, enc_off.ctypes.data, buf.ctypes.data, cap, out_off.ctypes.data,
                                    nd.ctypes.data, needs.ctypes.data)
    if ret != 0:
        raise RuntimeError(f'reccut_format_packed failed: {ret}')
    text = buf[:int(out_off[-1])].tobytes().decode('ascii')
    bounds = out_off.tolist()
    return [text[a:b].split(';')[:-1] for a, b in zip(bounds[:-1], bounds[1:])], np.flatnonzero(needs)


def _encode_domains(doms: List[str]):
    """Domain strings of the binary ("b-e[,b-e]*", 1-based inclusive) in ``dctfp_reccut``'s encoding, or None for anything else."""
    rec = [len(doms)]
    try:
        for d in doms:
            segs = d.split(',')
            rec.append(len(segs))
            for sg in segs:
                b, e = sg.split('-')
                if not (b.isdigit() and e.isdigit()):
                    return None
                rec += [int(b) - 1, int(e) - 1]
    except ValueError:
        return None
    return np.asarray(rec, dtype=np.int32) if doms else None


def _wait_strings(cut: CutInFlight, threads: int, before_wait=None) -> List[List[str]]:
    try:
        if before_wait is not None:
            before_wait()
        return cut.wait(threads, strings=True)
    finally:
        cut.release()


def domains_from_maps(maps: Sequence[torch.Tensor], t: float, cut1=CUT1_DEFAULT, cut2=CUT2_DEFAULT, threads: int = 1,
                      before_wait=None) -> List[List[str]]:
    """``Fingerprint.reccut``'s domain lists for a batch of contact maps with NOTHING but the answer leaving the GPU: the contact
    selection (``dctfp_contact_topk``) and the domain cutter's recursion (``dctfp_reccut``: src/RecCut.cpp:150-351, one
    workgroup per protein) run back to back on the device; what comes over is a few ints per domain, which libreccut formats
    into the binary's strings.  Proteins the GPU cutter hands back (status -1: longer than its tables, or a step the
    reference leaves undefined) go through the host library on their own contacts.  ``before_wait`` (a callable) runs after
    the kernels are enqueued and before this thread waits for them."""
    if len(maps) == 0:
        return []
    ptrs, lds, n_res = map_geometry(maps)
    return _wait_strings(CutInFlight(ptrs, lds, n_res, maps[0].device, t, cut1, cut2), threads, before_wait)


def domains_from_contacts_gpu(n_res: Sequence[int], offs, ci, cj, cv, cut1=CUT1_DEFAULT, cut2=CUT2_DEFAULT, threads: int = 1,
                              device=None) -> List[List[str]]:
    """``domains_from_contacts`` with the recursion on the GPU (``dctfp_reccut``): the same contact lists (host arrays, pairs
    distinct) -> the same strings."""
    n_res = np.ascontiguousarray(n_res, dtype=np.int32)
    if len(n_res) == 0:
        return []
    device = device if device is not None else torch.device('cuda', torch.cuda.current_device())
    oi = torch.from_numpy(np.ascontiguousarray(ci, dtype=np.int32)).to(device)
    oj = torch.from_numpy(np.ascontiguousarray(cj, dtype=np.int32)).to(device)
    ov = torch.from_numpy(np.ascontiguousarray(cv, dtype=np.float32)).to(device)
    if oi.numel() == 0:
        oi, oj, ov = (torch.zeros(1, dtype=d, device=device) for d in (torch.int32, torch.int32, torch.float32))
    return _wait_strings(CutInFlight.from_contacts(n_res, offs, oi, oj, ov, device, cut1, cut2), threads)


def ce_text(pid: str, seq: str, ci, cj, cv) -> str:
    """The .ce file body of src/fingerprint.py:69-80."""
    slen = len(seq)
    sout = ''
    if len(ci):
        sout = 'CON   ' + ','.join(f'{int(i)} {int(j)} {float(v):.6f}' for i, j, v in zip(ci, cj, cv))
    return f'INF   {pid} {slen}\nSEQ   {seq}\nSS    {"C" * slen}\n{sout}\n'


def write_ce(fp, outfile: str, t: float):
    """``Fingerprint.writece`` (src/fingerprint.py:45-80): same file, byte for byte."""
    slen = len(fp.seq)
    cmap = _contact_tensor(fp.contacts, slen)
    offs, ci, cj, cv = top_contacts_batch([cmap], t)
    with open(outfile, 'w', encoding='utf8') as out_f:
        out_f.write(ce_text(fp.pid, fp.seq, ci, cj, cv))


def domains_from_contacts(n_res: Sequence[int], offs, ci, cj, cv, cut1=CUT1_DEFAULT, cut2=CUT2_DEFAULT,
                          threads: int = 1) -> List[List[str]]:
    """libreccut on a batch: per protein the list the reference gets from
    ``stdout.strip().split()[2].split(';')[:-1]`` (src/fingerprint.py:103)."""
    lib = _lib.load_reccut()
    n = len(n_res)
    n_res = np.ascontiguousarray(n_res, dtype=np.int32)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    ci = np.ascontiguousarray(ci, dtype=np.int32)
    cj = np.ascontiguousarray(cj, dtype=np.int32)
    cv = np.ascontiguousarray(cv, dtype=np.float32)
    if n == 0:
        return []
    cap = 64 * n + 16 * int(n_res.astype(np.int64).sum())      # a domain piece "b-e," is at most 12 bytes per residue it holds
    buf = np.empty(cap, dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.int64)
    nd = np.zeros(n, dtype=np.int32)
    rc = np.zeros(n, dtype=np.int32)
    ret = lib.reccut_predict_packed(n, n_res.ctypes.data, offs.ctypes.data, ci.ctypes.data, cj.ctypes.data,
                                    cv.ctypes.data, float(cut1), float(cut2), buf.ctypes.data, cap, out_off.ctypes.data,
                                    nd.ctypes.data, rc.ctypes.data, int(threads))
    if ret != 0:
        raise RuntimeError(f'reccut_predict_packed failed: {ret}')
    if rc.any():
        p = int(np.flatnonzero(rc)[0])
        # the reference would raise CalledProcessError (RecCut exit != 0) or crash
        raise RuntimeError(f'reccut: protein {p}: error {int(rc[p])} '
                           f'({"undefined behaviour in the reference at this input" if rc[p] == -3 else "invalid input"})')
    text = buf[:int(out_off[-1])].tobytes().decode('ascii')
    bounds = out_off.tolist()
    return [text[a:b].split(';')[:-1] for a, b in zip(bounds[:-1], bounds[1:])]


def predict_domains(fp, threshold: float) -> List[str]:
    """The domain list ``Fingerprint.reccut`` appends (src/fingerprint.py:83-104), without the
    trailing whole-protein entry (the caller adds it when there are several domains)."""
    slen = len(fp.seq)
    cmap = _contact_tensor(fp.contacts, slen)
    offs, ci, cj, cv = top_contacts_batch([cmap], threshold, sort=False, own=False)
    return domains_from_contacts([slen], offs, ci, cj, cv)[0]
