"""``dct_sim._field_lines``, the composer under ``cluster_lines`` / ``assign_lines`` (two fields) and ``domain_cluster_lines`` (four),
against ``' '.join`` in a Python loop, and ``cluster_lines``' two paths against each other."""

import numpy as np
import pytest

TABLE = ['', 'prot蛋é|', 'x' * 300, 'P12345', 'a b', '0']


@pytest.mark.parametrize('k', [1, 2, 4])
@pytest.mark.parametrize('chunk_bytes', [1, 1 << 24])
def test_field_lines_against_a_python_loop(k, chunk_bytes):
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(k)
    n = 57
    fields = [rng.integers(0, len(TABLE), n) for _ in range(k)]
    for f in fields:
        f[:len(TABLE)] = rng.permutation(len(TABLE))            # (every string in every field)
    fields[0][-1] = fields[-1][-1] = 0                          # (a line that opens and ends with the empty string)
    want = [(' '.join(TABLE[f[t]] for f in fields) + '\n').encode('utf8') for t in range(n)]
    got = list(dct_sim._field_lines(TABLE, fields, chunk_bytes))
    assert all(c.dtype == np.uint8 and c.ndim == 1 for c in got)
    assert b''.join(c.tobytes() for c in got) == b''.join(want)
    if chunk_bytes == 1:
        assert [c.tobytes() for c in got] == want               # (one line per chunk, however long)
    else:
        assert len(got) == 1
    assert list(dct_sim._field_lines(TABLE, [f[:0] for f in fields], chunk_bytes)) == []


def test_cluster_lines_general_path_equals_the_fixed_width_path(monkeypatch):
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(3)
    ids = [f'id{k}' + 'y' * int(rng.integers(0, 9)) for k in range(40)]
    labels = np.minimum(np.arange(40), rng.integers(0, 40, 40))
    labels = labels[labels]                                     # (not necessarily roots: cluster_lines takes any label in range)
    calls = []
    real = dct_sim._ascii_lines
    monkeypatch.setattr(dct_sim, '_ascii_lines', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for chunk_bytes in (1, 50, 1 << 24):
        general = b''.join(c.tobytes() for c in dct_sim.cluster_lines(ids, labels, chunk_bytes))
        assert not calls
        fixed = b''.join(c.tobytes() for c in dct_sim.cluster_lines(np.array(ids), labels, chunk_bytes))
        assert calls and general == fixed
        order = np.argsort(labels, kind='stable')
        assert general == ''.join(f'{ids[labels[m]]} {ids[m]}\n' for m in order).encode()
        calls.clear()
