"""Drop-in for the search half of mgtools/DCTdomain ``src/query_db.py`` (:17-91): for every query
protein the ``khits`` nearest database fingerprints by L1 distance, printed as
``round(1 - L1/17000, 4)``.  The reference uses a FAISS flat index forced to METRIC_L1 (:75-76);
here the exact L1 matrix comes from the GPU kernel and needs no index file.

    python -m dctdomain_amd.query_db --query Q.fasta|Q.db --db X.db [--out F] [--khits 100]
                                     [--maxlen 500] [--cpu N] [--gpu G] [--model esm|synthetic]
"""

from __future__ import annotations

import argparse
import logging
import os
from io import BytesIO

import numpy as np
import torch

from . import _lib
from .database import Database, _npy_vector
from .similarity import (TextStream, _device_int64, _pair_to_host, _utf8_binary, l1_knn_device, l1_matrix, order_pairs, row_select,
                         to_device_int8)


def _load_all(db: Database):
    """Every fingerprint row of a database as ((vid, pid, domain) tuples, int8 matrix), table order."""
    meta, blobs = [], []
    for vid, pid, domain, blob in db.cur.execute('SELECT vid, pid, domain, fingerprint FROM fingerprints'):
        meta.append((vid, pid, domain))
        blobs.append(np.load(BytesIO(blob), allow_pickle=False))      # plain int8 vectors: no reason to unpickle a user's file
    return meta, np.array(blobs, dtype=np.int8)


COL_ROWS = 1 << 22      # database fingerprints on the device at a time (2 GB of int8 at 480 columns)
TILE_INTS = 1 << 28     # int32 entries of one distance matrix (1 GiB)


def ranked_hits(d_rows: np.ndarray, khits: int):
    """The first ``khits`` of all hits of one query protein -- ``d_rows[i, j]`` = distance of hit j of its fingerprint i --
    ranked by distance, stable in (fingerprint, hit) order: the reference's ``sorted(top_hits.items(), key=distance)`` over
    the items as it inserts them (src/query_db.py:33-40).  Returns (fingerprint index, hit index, score) lists, the scores
    as ``round(1 - (d / 17000), 4)`` of numpy scalars (:57), rounded all at once."""
    k = d_rows.shape[1]
    d_all = d_rows.ravel()
    sel = np.argsort(d_all, kind='stable')[:khits]
    scores = np.round(1 - (d_all[sel] / 17000), 4).tolist()
    ii, jj = np.divmod(sel, k)
    return ii.tolist(), jj.tolist(), scores


def search(query_rows, query_fps, db_rows, db_fps, khits: int):
    """Yields the reference's log lines.  Per query protein (pids in the order ``SELECT pid FROM
    sequences`` returns them: by primary key, i.e. sorted): the ``khits`` nearest database
    fingerprints of each of its fingerprints (ties: lower vid first, as a flat index scans), then
    all of those ranked by distance (stable) and the first ``khits`` printed (:33-59)."""
    # query fingerprints in tiles: the (tile, ndb) int32 distance matrix stays within ~1 GiB however large the database
    # is (the reference streams one query protein at a time, src/query_db.py:75-87)
    # ... and the database in column blocks of at most COL_ROWS fingerprints (uploaded one at a time): the k nearest of
    # every block are candidates, the k nearest of the candidates the answer (ties: lower database row first, as before)
    ndb = db_fps.shape[0]
    k = min(khits, ndb)
    nq = len(query_fps)
    cand_d, cand_i = [], []                                 # per column block: (nq, k_block) distances / database rows
    for c0 in range(0, ndb, COL_ROWS):
        db_dev = to_device_int8(db_fps[c0:c0 + COL_ROWS])
        kb = min(k, db_dev.shape[0])
        tile = max(1, min(8192, TILE_INTS // max(1, db_dev.shape[0])))
        dms, ims = [], []
        for q0 in range(0, nq, tile):
            dist = l1_matrix(query_fps[q0:q0 + tile], db_dev)            # (tile, block) int32 on the GPU
            dm_t, im_t = row_select(dist, kb)                             # k nearest per query fingerprint
            dms.append(dm_t)
            ims.append(im_t + c0)
            del dist
        cand_d.append(np.concatenate(dms) if dms else np.zeros((0, kb), np.int64))
        cand_i.append(np.concatenate(ims) if ims else np.zeros((0, kb), np.int64))
        del db_dev
    if len(cand_d) == 1:
        dm, im = cand_d[0], cand_i[0]
    elif cand_d:
        dm, im = order_pairs(np.concatenate(cand_d, axis=1), np.concatenate(cand_i, axis=1))
        dm, im = dm[:, :k], im[:, :k]
    else:
        dm, im = np.zeros((nq, 0), np.int64), np.zeros((nq, 0), np.int64)
    by_pid = {}
    for qi, r in enumerate(query_rows):
        by_pid.setdefault(r[1], []).append(qi)
    for pid in sorted(by_pid):
        qis = by_pid[pid]
        # all hits of the protein's fingerprints ranked by distance, stable in (fingerprint, hit) order -- the reference's
        # list.sort(key=distance) over the items as it appends them (:52-59)
        ii, jj, scores = ranked_hits(dm[qis], khits)
        for rank, (i, j, score) in enumerate(zip(ii, jj, scores)):
            qrow = query_rows[qis[i]]
            drow = db_rows[im[qis[i], j]]
            yield f'Query: {qrow[1]} {qrow[2]}, Result {rank + 1}: {drow[1]} {drow[2]}, Similarity: {score}'


class Table:
    """Every fingerprint row of a database in table order, without a Python object per row: ``fps`` (n, d) int8, ``pid`` /
    ``dom`` the UTF-8 bytes of the pids / domain strings with int64 prefix offsets ``pid_off`` / ``dom_off`` (n + 1), and
    ``pid_code`` = the row's index into ``pids`` (the distinct pids, sorted: the order search() prints them in)."""

    def __init__(self, pids, doms, fps):
        enc_p = [p.encode('utf8') for p in pids]
        enc_d = [x.encode('utf8') for x in doms]
        self.n = len(enc_p)
        self.fps = fps
        self.pid = b''.join(enc_p)
        self.dom = b''.join(enc_d)
        self.pid_off = np.zeros(self.n + 1, np.int64)
        self.dom_off = np.zeros(self.n + 1, np.int64)
        np.cumsum(np.fromiter(map(len, enc_p), np.int64, self.n), out=self.pid_off[1:])
        np.cumsum(np.fromiter(map(len, enc_d), np.int64, self.n), out=self.dom_off[1:])
        self.pids = sorted(set(pids))
        code = {p: i for i, p in enumerate(self.pids)}
        self.pid_code = np.fromiter(map(code.__getitem__, pids), np.int64, self.n)


def load_table(db: Database) -> Table:
    """``_load_all`` in bulk: ``vid, pid, domain, fingerprint`` in table order; blobs that all carry the header ``np.save`` writes
    for one int8 vector shape are cut out of one joined buffer (``database._npy_vector``'s fast path), any other blob goes
    through ``np.load(..., allow_pickle=False)`` one by one, as there -- a pickled object is refused the same way."""
    rows = db.cur.execute('SELECT vid, pid, domain, fingerprint FROM fingerprints').fetchall()
    if not rows:
        return Table([], [], np.zeros((0, 0), np.int8))
    _, pids, doms, blobs = zip(*rows)
    first = _npy_vector(blobs[0])
    head = blobs[0][:len(blobs[0]) - first.nbytes]
    size = len(blobs[0])
    if (first.dtype == np.int8 and first.ndim == 1 and all(len(b) == size for b in blobs)
            and all(b.startswith(head) for b in blobs)):
        fps = np.frombuffer(b''.join(blobs), np.int8).reshape(len(blobs), size)[:, len(head):]
        fps = np.ascontiguousarray(fps)
    else:
        fps = np.array([_npy_vector(b) for b in blobs], dtype=np.int8)
    return Table(pids, doms, fps)


SCORE_DIV = 17000


def score_table(width: int):
    """(bytes, int64 offsets): the string search() prints for every L1 distance 0 .. 255 * width -- ranked_hits' own
    expression, ``str`` of ``np.round(1 - (d / 17000), 4).tolist()`` -- looked up, not formatted, by the line kernel."""
    d = np.arange(255 * max(int(width), 1) + 1, dtype=np.int64)
    enc = [str(x).encode() for x in np.round(1 - (d / SCORE_DIV), 4).tolist()]
    off = np.zeros(len(enc) + 1, np.int64)
    np.cumsum(np.fromiter(map(len, enc), np.int64, len(enc)), out=off[1:])
    return b''.join(enc), off


LINE_FIXED = len('Query: ' ' ' ', Result ' ': ' ' ' ', Similarity: ' '\n')      # the bytes of a line that are not an id, a domain, a rank or a score


def line_lengths(q: Table, d: Table, score_off, qrow, drow, dist, rank):
    """Byte length of each line ``Query: {qpid} {qdom}, Result {rank}: {dpid} {ddom}, Similarity: {score}`` + newline, for
    query table rows ``qrow``, database rows ``drow``, distances ``dist`` and printed ranks ``rank`` (int arrays, one per line)."""
    qrow, drow, dist, rank = (np.asarray(x, np.int64) for x in (qrow, drow, dist, rank))
    digits = np.ones(len(rank), np.int64)
    for p in range(1, 19):
        digits += rank >= 10 ** p
    return (LINE_FIXED + np.diff(q.pid_off)[qrow] + np.diff(q.dom_off)[qrow] + np.diff(d.pid_off)[drow] + np.diff(d.dom_off)[drow]
            + digits + np.diff(score_off)[dist])


def _dev_bytes(b: bytes, device):
    a = np.frombuffer(b, np.uint8) if len(b) else np.zeros(1, np.uint8)
    return torch.as_tensor(a.copy(), device=device)


def knn_route(nq: int, nb: int, k: int) -> bool:
    """True where ``dctfp_l1_knn`` is taken over ``l1_matrix`` + ``row_select``.  Measured at 200 000 database
    rows, nq 5 ... 20 000, k 100 / 1 024, the matrix route won every shape (by 1.06x at 20 000 x 200 000, k = 100, by 8x and
    more for few rows).  It loses its footing when a distance tile of ``TILE_INTS`` holds fewer than 128 query rows (databases
    above 2M fingerprints: its 128-row workgroups then run partly empty and the database is re-read per tile), so the fused
    kernel is taken there, for many query rows and small k only."""
    return nq >= KNN_FUSED_MIN_ROWS and k <= KNN_FUSED_MAX_K and TILE_INTS // max(1, nb) < 128


KNN_FUSED_MIN_ROWS = 16384
KNN_FUSED_MAX_K = 128


class QuerySearch:
    """search() at database scale: the database fingerprints on the device (resident when they fit ``device_budget`` bytes,
    else uploaded block by block for every batch), per batch of query proteins their k nearest, the protein ranking
    (``dctfp_query_rank``; proteins with more than ``rank_cap`` hits go to ranked_hits) and the lines as text
    (``dctfp_query_lines``), handed to a sink as UTF-8 bytes.  Output = ``''.join(line + '\\n' for line in search(...))``, byte
    for byte.

    The k nearest come from one of two routes, both exact and equal: ``'fused'`` = ``dctfp_l1_knn`` (no distance matrix),
    ``'matrix'`` = ``l1_matrix`` + ``row_select`` on tiles of at most ``TILE_INTS`` distances.  ``knn='auto'`` takes the one
    measured faster for the shape (``knn_route``)."""

    RANK_CAP = 1 << 14          # f * k of a protein ranked on the device
    BATCH_ROWS = 1 << 16        # query fingerprints per batch
    TEXT_BYTES = 1 << 27        # device text buffer, and each of the two pinned ones
    BLOCK_ROWS = 1 << 24        # database fingerprints per kernel call
    DEVICE_BUDGET = 16 << 30    # database bytes kept resident on the device

    def __init__(self, db: Table, block_rows: int = None, device=None, device_budget: int = None, knn: str = 'auto'):
        if knn not in ('auto', 'fused', 'matrix'):
            raise ValueError("knn must be 'auto', 'fused' or 'matrix'")
        self.db = db
        self.knn = knn
        self.dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.block_rows = int(block_rows or self.BLOCK_ROWS)
        n = db.fps.shape[0]
        budget = self.DEVICE_BUDGET if device_budget is None else int(device_budget)
        self.resident = db.fps.nbytes <= budget
        self.blocks = [(c0, db.fps[c0:c0 + self.block_rows]) for c0 in range(0, n, self.block_rows)]
        if self.resident:
            self.blocks = [(c0, to_device_int8(blk).to(self.dev)) for c0, blk in self.blocks]
        width = db.fps.shape[1] if db.fps.ndim == 2 else 0
        self.score_txt, self.score_off = score_table(width)
        self.d_txt = _dev_bytes(db.pid + db.dom, self.dev)
        self.d_pid_off = _device_int64(db.pid_off, self.dev)
        self.d_dom_off = _device_int64(db.dom_off + len(db.pid), self.dev)
        self.score_txt_dev = _dev_bytes(self.score_txt, self.dev)
        self.score_off_dev = _device_int64(self.score_off, self.dev)

    def _block_knn(self, qf: torch.Tensor, blk: torch.Tensor, k: int, c0: int):
        if knn_route(qf.shape[0], blk.shape[0], k) if self.knn == 'auto' else self.knn == 'fused':
            return l1_knn_device(qf, blk, k, c0)
        kb = min(k, blk.shape[0])
        tile = max(1, min(8192, TILE_INTS // max(1, blk.shape[0])))
        vs, is_ = [], []
        for q0 in range(0, qf.shape[0], tile):
            v, i = row_select(l1_matrix(qf[q0:q0 + tile], blk), kb)
            vs.append(v)
            is_.append(i + c0)
        return (torch.as_tensor(np.concatenate(vs).astype(np.int32), device=self.dev),
                torch.as_tensor(np.concatenate(is_).astype(np.int32), device=self.dev))

    def _knn(self, qf: torch.Tensor, k: int):
        """(val, idx) device int32 (nq, k) over every block; blocks merged with order_pairs (ties: lower row)."""
        parts = []
        for c0, blk in self.blocks:
            dev_blk = blk if self.resident else to_device_int8(blk).to(self.dev)
            parts.append(self._block_knn(qf, dev_blk, k, c0))
            del dev_blk
        if len(parts) == 1:
            return parts[0]
        host = [_pair_to_host(v, i) for v, i in parts]
        v, i = order_pairs(np.concatenate([h[0] for h in host], axis=1), np.concatenate([h[1] for h in host], axis=1))
        return (torch.as_tensor(v[:, :k].astype(np.int32), device=self.dev), torch.as_tensor(i[:, :k].astype(np.int32), device=self.dev))

    def search(self, q: Table, khits: int, sink, batch_rows: int = None, text_bytes: int = None, rank_cap: int = None):
        """Writes the lines of ``search()`` for the query table ``q`` to ``sink`` (a callable taking bytes), in batches of query
        proteins of at most ``batch_rows`` fingerprints (one protein with more is a batch of its own).  The text of a run of
        lines is copied into one of two pinned buffers while the sink writes the other (``TextStream``)."""
        batch_rows = int(batch_rows or self.BATCH_ROWS)
        text_bytes = int(text_bytes or self.TEXT_BYTES)
        rank_cap = self.RANK_CAP if rank_cap is None else int(rank_cap)
        ndb = self.db.fps.shape[0]
        k = min(int(khits), ndb)
        if q.n == 0 or k <= 0:
            return
        dev = self.dev
        order = np.argsort(q.pid_code, kind='stable')                       # rows grouped by protein, pids sorted, table order
        n_prot = len(q.pids)
        counts = np.bincount(q.pid_code, minlength=n_prot)
        qoff = np.zeros(n_prot + 1, np.int64)
        np.cumsum(counts, out=qoff[1:])
        q_txt = _dev_bytes(q.pid + q.dom, dev)
        q_pid_off = _device_int64(q.pid_off, dev)
        q_dom_off = _device_int64(q.dom_off + len(q.pid), dev)
        text = torch.empty(max(1, text_bytes), dtype=torch.uint8, device=dev)
        out = TextStream(lambda view: sink(bytes(view)), room=lambda nbytes: max(1, text_bytes))      # (no run is longer than the text buffer)
        ctx = _lib.get_context(dev.index)
        stream = torch.cuda.current_stream(dev)
        p0 = 0
        while p0 < n_prot:
            p1 = max(p0 + 1, int(np.searchsorted(qoff, qoff[p0] + batch_rows, side='right')) - 1)
            p1 = min(p1, n_prot)
            r0, r1 = qoff[p0], qoff[p1]
            rows = order[r0:r1]                                             # query table rows of the batch, grouped
            val, idx = self._knn(to_device_int8(q.fps[rows]).to(dev), k)
            kk = val.shape[1]
            f = counts[p0:p1]
            n_lines = np.minimum(khits, f * kk)
            base = np.zeros(p1 - p0 + 1, np.int64)
            np.cumsum(n_lines, out=base[1:])
            total = int(base[-1])
            host = f * kk > rank_cap
            prot_of_row = np.repeat(np.where(host, -1, np.arange(p1 - p0)), f).astype(np.int32)
            lq = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            ld = torch.empty_like(lq)
            lx = torch.empty_like(lq)
            # (named: a temporary's memory would go back to the allocator, and to the next argument, before the kernel ran)
            qoff_dev, prot_dev, base_dev = _device_int64(qoff[p0:p1 + 1] - r0, dev), torch.as_tensor(prot_of_row, device=dev), _device_int64(base, dev)
            ctx.call('dctfp_query_rank', val.data_ptr(), idx.data_ptr(), len(rows), kk, qoff_dev.data_ptr(), prot_dev.data_ptr(),
                     base_dev.data_ptr(), int(khits), lq.data_ptr(), ld.data_ptr(), lx.data_ptr(), stream=stream)
            qr, dr, dx = (t.cpu().numpy().astype(np.int64)[:total] for t in (lq, ld, lx))
            if host.any():                                                  # proteins of many hits: ranked_hits on the host
                vh, ih = _pair_to_host(val, idx)
                for p in np.flatnonzero(host):
                    a, b = qoff[p0 + p] - r0, qoff[p0 + p + 1] - r0
                    ii, jj, _ = ranked_hits(vh[a:b], khits)
                    s = slice(base[p], base[p] + len(ii))
                    qr[s] = a + np.asarray(ii, np.int64)
                    dr[s] = ih[a:b][ii, jj]
                    dx[s] = vh[a:b][ii, jj]
            qrow = rows[qr]                                                 # query table rows of the lines
            rank = np.arange(total, dtype=np.int64) - np.repeat(base[:-1], n_lines) + 1
            lens = line_lengths(q, self.db, self.score_off, qrow, dr, dx, rank)
            off = np.zeros(total + 1, np.int64)
            np.cumsum(lens, out=off[1:])
            if off[-1] and lens.max() > text_bytes:
                raise ValueError('a result line is longer than the text buffer')
            dev_cols = [torch.as_tensor(x.astype(np.int32), device=dev) for x in (qrow, dr, dx, rank)]
            off_dev = _device_int64(off, dev)
            a = 0
            while a < total:                                                # runs of lines that fit the text buffer
                b = int(np.searchsorted(off, off[a] + text_bytes, side='right')) - 1
                b = max(b, a + 1)
                nbytes = int(off[b] - off[a])
                rel = off_dev[a:b + 1] - int(off[a])
                ctx.call('dctfp_query_lines', b - a, *(t[a:].data_ptr() for t in dev_cols), q_txt.data_ptr(), q_pid_off.data_ptr(),
                         q_dom_off.data_ptr(), self.d_txt.data_ptr(), self.d_pid_off.data_ptr(), self.d_dom_off.data_ptr(),
                         self.score_txt_dev.data_ptr(), self.score_off_dev.data_ptr(), rel.data_ptr(), text.data_ptr(), stream=stream)
                out.hand_over(text, nbytes)
                a = b
            p0 = p1
        out.close()


def search_db(args: argparse.Namespace, query_db: str, fp_db: str):
    qdb = Database(query_db)
    fdb = Database(fp_db)
    print('Querying database...\n')
    q, d = load_table(qdb), load_table(fdb)
    handlers = logging.getLogger().handlers
    stream = getattr(handlers[0], 'stream', None) if len(handlers) == 1 else None
    binary = _utf8_binary(stream) if stream is not None else None
    if binary is not None:              # the text straight to the binary layer under the handler's stream (flushed first)
        stream.flush()

        def sink(data):
            binary.write(data)
    else:                               # another encoding, or no single stream: the lines through logging, one by one
        def sink(data):
            for line in data.decode('utf8').split('\n')[:-1]:
                logging.info(line)
    QuerySearch(d).search(q, args.khits, sink)
    if binary is not None:
        binary.flush()
    qdb.close()
    fdb.close()


def build_parser() -> argparse.ArgumentParser:
    """Flags of src/query_db.py:94-110, plus ``--model`` (see make_db)."""
    ap = argparse.ArgumentParser(description='nearest database fingerprints of every query protein (GPU L1)')
    for flag, kind, default, text in (('--maxlen', int, 500, 'longest window given to the language model'),
                                      ('--khits', int, 100, 'hits reported per query protein'),
                                      ('--cpu', int, 1, 'host processes for RecCut'),
                                      ('--gpu', int, False, 'GPU worker processes')):
        ap.add_argument(flag, type=kind, default=default, help=text)
    ap.add_argument('--query', required=True, help='query proteins: FASTA (.fa/.fasta) or an existing .db')
    ap.add_argument('--db', required=True, help='database to search (.db)')
    ap.add_argument('--out', default=False, help='write the hit lines here instead of the console')
    ap.add_argument('--model', choices=['esm', 'synthetic'], default='esm')
    return ap


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.out:
        logging.basicConfig(level=logging.INFO, filename=args.out, filemode='w', format='%(message)s', force=True)
    else:
        logging.basicConfig(level=logging.INFO, format='%(message)s', force=True)
    query_db = os.path.splitext(args.query)[0] + '.db'
    if not args.query.endswith('.db'):
        from . import make_db
        ns = make_db.build_parser().parse_args(['--fafile', args.query, '--dbfile', os.path.splitext(args.query)[0],
                                                '--maxlen', str(args.maxlen), '--cpu', str(args.cpu), '--model', args.model,
                                                '--noindex', '--nonpz', '--nodom'] + (['--gpu', str(args.gpu)] if args.gpu else []))
        make_db.run(ns).close()
    search_db(args, query_db, args.db)


if __name__ == '__main__':
    main()
