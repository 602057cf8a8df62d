"""Host side of query_db at database scale: the score table, the line-length plan and the bulk loader (no GPU)."""

import sqlite3

import numpy as np
import pytest


def test_score_table_equals_ranked_hits_scores():
    from dctdomain_amd.query_db import ranked_hits, score_table
    txt, off = score_table(512)
    d = np.arange(255 * 512 + 1, dtype=np.int64)
    assert len(off) == len(d) + 1
    _, _, scores = ranked_hits(d.reshape(-1, 1), len(d))          # (one hit per "fingerprint": order = d)
    got = [txt[off[x]:off[x + 1]].decode() for x in range(len(d))]
    assert got == [str(s) for s in scores]
    assert got[0] == '1.0' and got[17000] == '0.0' and got[-1].startswith('-')


def _table(pids, doms, width=480):
    from dctdomain_amd.query_db import Table
    return Table(pids, doms, np.zeros((len(pids), width), np.int8))


def test_line_plan_matches_search_lines():
    from dctdomain_amd.query_db import line_lengths, ranked_hits, score_table
    rng = np.random.default_rng(0)
    q = _table(['q1', 'ßλ', 'x' * 300], ['1-50', '1-20,40-60', '1-9'])
    d = _table(['d', 'é' * 5, 'db3', 'd4'], ['1-1', '2-200', '5-6,8-9', '1-1000'])
    _, off = score_table(480)
    n = 500
    qrow = rng.integers(0, 3, n)
    drow = rng.integers(0, 4, n)
    dist = rng.integers(0, 255 * 480 + 1, n)
    rank = rng.integers(1, 100001, n)
    lens = line_lengths(q, d, off, qrow, drow, dist, rank)
    qp, qd = ['q1', 'ßλ', 'x' * 300], ['1-50', '1-20,40-60', '1-9']
    dp, dd = ['d', 'é' * 5, 'db3', 'd4'], ['1-1', '2-200', '5-6,8-9', '1-1000']
    for t in range(n):
        score = ranked_hits(np.array([[dist[t]]]), 1)[2][0]
        line = f'Query: {qp[qrow[t]]} {qd[qrow[t]]}, Result {rank[t]}: {dp[drow[t]]} {dd[drow[t]]}, Similarity: {score}\n'
        assert lens[t] == len(line.encode('utf8')), line


def _write_db(path, blobs):
    conn = sqlite3.connect(path)
    conn.execute('CREATE TABLE fingerprints (vid integer PRIMARY KEY, domain text NOT NULL, fingerprint blob NOT NULL, pid text NOT NULL)')
    conn.executemany('INSERT INTO fingerprints(vid, domain, fingerprint, pid) VALUES(?, ?, ?, ?)',
                     [(i, f'1-{i + 1}', b, f'p{i % 4}') for i, b in enumerate(blobs)])
    conn.commit()
    conn.close()


class _Db:
    def __init__(self, path):
        self.conn = sqlite3.connect(path)
        self.cur = self.conn.cursor()


def _npy(vec, version=None):
    from io import BytesIO
    buf = BytesIO()
    if version is None:
        np.save(buf, vec)
    else:
        np.lib.format.write_array(buf, vec, version=version)
    return buf.getvalue()


def test_bulk_loader_equals_np_load(tmp_path):
    from io import BytesIO
    from dctdomain_amd.query_db import _load_all, load_table
    rng = np.random.default_rng(1)
    vecs = [rng.integers(-128, 128, 480).astype(np.int8) for _ in range(30)]
    for name, blobs in (('same', [_npy(v) for v in vecs]),
                        ('mixed', [_npy(v, (2, 0) if i % 3 == 0 else None) for i, v in enumerate(vecs)])):
        path = str(tmp_path / f'{name}.db')
        _write_db(path, blobs)
        t = load_table(_Db(path))
        meta, fps = _load_all(_Db(path))
        exp = np.array([np.load(BytesIO(b), allow_pickle=False) for b in blobs], dtype=np.int8)
        np.testing.assert_array_equal(t.fps, exp)
        np.testing.assert_array_equal(t.fps, fps)
        assert [t.pid[t.pid_off[i]:t.pid_off[i + 1]].decode() for i in range(t.n)] == [m[1] for m in meta]
        assert [t.dom[t.dom_off[i]:t.dom_off[i + 1]].decode() for i in range(t.n)] == [m[2] for m in meta]
        assert t.pids == sorted(set(m[1] for m in meta))


def test_bulk_loader_refuses_pickled_blob(tmp_path):
    from dctdomain_amd.query_db import load_table
    rng = np.random.default_rng(2)
    blobs = [_npy(rng.integers(-128, 128, 480).astype(np.int8)) for _ in range(3)]
    blobs.append(_npy(np.array([{'a': 1}], dtype=object)))
    path = str(tmp_path / 'pickled.db')
    _write_db(path, blobs)
    with pytest.raises(ValueError):
        load_table(_Db(path))
