"""A plain CPU reference of the reference's src/query_db.py search (:17-91), for the query_db tests: exact L1 k-nearest and the
hit lines, written out without any of the package's GPU code or its ranking helpers.  Only numpy and torch on the CPU."""

from __future__ import annotations

import numpy as np
import torch

SCORE_DIV = 17000


def l1_rows(q: np.ndarray, b: np.ndarray) -> np.ndarray:
    """(nq, nb) int64 L1 distances: float64 ``torch.cdist(p=1)`` on the CPU, exact for int8 rows (sums below 2^53)."""
    tq = torch.from_numpy(np.ascontiguousarray(q, dtype=np.int8)).to(torch.float64)
    tb = torch.from_numpy(np.ascontiguousarray(b, dtype=np.int8)).to(torch.float64)
    return torch.cdist(tq, tb, p=1).numpy().round().astype(np.int64)


def ref_knn(q, b, k: int, chunk_cells: int = 1 << 24, chunk_bytes: int = 1 << 28):
    """(dist, idx) int64 (nq, min(k, nb)): per query row the k nearest database rows by L1, ascending distance, ties to the
    lower database row.  Database rows in chunks of at most ``chunk_bytes`` as float64, query rows in chunks of about
    ``chunk_cells`` distances against one of them."""
    q = np.asarray(q, np.int8)
    b = np.asarray(b, np.int8)
    nq, nb = q.shape[0], b.shape[0]
    k = min(int(k), nb)
    out_d = np.zeros((nq, k), np.int64)
    out_i = np.zeros((nq, k), np.int64)
    if nq == 0 or k == 0:
        return out_d, out_i
    cols = max(k, min(nb, chunk_bytes // (8 * max(1, b.shape[1]))))
    rows = max(1, min(nq, chunk_cells // cols))
    for r0 in range(0, nq, rows):
        qc = q[r0:r0 + rows]
        best_d = np.zeros((len(qc), 0), np.int64)
        best_i = np.zeros((len(qc), 0), np.int64)
        for c0 in range(0, nb, cols):
            dist = l1_rows(qc, b[c0:c0 + cols])
            col = np.broadcast_to(np.arange(c0, c0 + dist.shape[1], dtype=np.int64), dist.shape)
            d_all = np.concatenate([best_d, dist], axis=1)
            i_all = np.concatenate([best_i, col], axis=1)
            keep = min(k, d_all.shape[1])
            if keep < d_all.shape[1]:       # (a partial selection; the full order comes from the lexsort below)
                key = d_all * (nb + 1) + i_all
                part = np.argpartition(key, keep - 1, axis=1)[:, :keep]
                d_all = np.take_along_axis(d_all, part, axis=1)
                i_all = np.take_along_axis(i_all, part, axis=1)
            best_d, best_i = d_all, i_all
        # ascending (distance, database row): np.lexsort((i, d)) of every row, as one sort of the unique key d (nb + 1) + i
        o = np.argsort(best_d * (nb + 1) + best_i, axis=1)
        out_d[r0:r0 + len(qc)] = np.take_along_axis(best_d, o, axis=1)
        out_i[r0:r0 + len(qc)] = np.take_along_axis(best_i, o, axis=1)
    return out_d, out_i


def strings(txt: bytes, off) -> list:
    return [txt[off[i]:off[i + 1]].decode('utf8') for i in range(len(off) - 1)]


def score_text(d) -> str:
    """What the reference prints for L1 distance ``d``: ``round(1 - d/17000, 4)`` of a numpy float, as ``str``."""
    return str(np.round(1 - np.float64(d) / SCORE_DIV, 4))


def ref_lines(qtable, dtable, khits: int, knn=None) -> bytes:
    """The reference's output for query table ``qtable`` against database table ``dtable`` (objects with ``fps``, ``pid`` /
    ``pid_off`` and ``dom`` / ``dom_off``, as ``query_db.Table``), as UTF-8 bytes:

    - query proteins in sorted-pid order (``SELECT pid FROM sequences``: the primary key);
    - ``min(khits, ndb)`` nearest database rows for each of the protein's fingerprints (table order);
    - all hits of the protein sorted stably by distance, in (fingerprint, hit) insertion order, the first ``khits`` printed as
      ``Query: {qpid} {qdom}, Result {rank}: {dpid} {ddom}, Similarity: {score}``.

    ``knn``: precomputed ``ref_knn(qtable.fps, dtable.fps, min(khits, ndb))``, if the caller has it."""
    qpid, qdom = strings(qtable.pid, qtable.pid_off), strings(qtable.dom, qtable.dom_off)
    dpid, ddom = strings(dtable.pid, dtable.pid_off), strings(dtable.dom, dtable.dom_off)
    ndb = len(dpid)
    k = min(int(khits), ndb)
    if not qpid or k <= 0:
        return b''
    dist, idx = knn if knn is not None else ref_knn(qtable.fps, dtable.fps, k)
    rows_of = {}
    for r, pid in enumerate(qpid):
        rows_of.setdefault(pid, []).append(r)       # the protein's fingerprints in table order
    out = []
    for pid in sorted(rows_of):
        hits = []                                   # (distance, query row, database row), in insertion order
        for r in rows_of[pid]:
            for j in range(k):
                hits.append((int(dist[r, j]), r, int(idx[r, j])))
        hits.sort(key=lambda h: h[0])               # list.sort is stable
        for rank, (d, r, c) in enumerate(hits[:khits]):
            out.append(f'Query: {qpid[r]} {qdom[r]}, Result {rank + 1}: {dpid[c]} {ddom[c]}, Similarity: {score_text(d)}\n')
    return ''.join(out).encode('utf8')
