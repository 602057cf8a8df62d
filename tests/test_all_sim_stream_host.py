"""CPU checks of all-against-all streaming (dct_sim.AllPairs): the score text table and the stripe planner."""

import numpy as np
import pytest

from dctdomain_amd import dct_sim


def test_score_table_is_the_printed_text_of_every_l1():
    tab = dct_sim.score_table()
    assert tab.shape == (2, dct_sim.SCORE_ROWS, 5) and tab.dtype == np.uint8
    for v in range(dct_sim.SCORE_ROWS):
        a, b = dct_sim._scores(np.int32(v), np.int32(v))
        assert tab[0, v].tobytes().decode() == f'{a:.3f}', v
        assert tab[1, v].tobytes().decode() == f'{b:.3f}', v
    for v in (17001, 17002, 30000, 0x7fffffff):             # the last row stands for every value above 17000
        a, b = dct_sim._scores(np.int32(v), np.int32(v))
        assert (f'{a:.3f}', f'{b:.3f}') == ('0.000', '0.000')
    assert len({tab[0, v].tobytes() for v in range(dct_sim.SCORE_ROWS)}) == 1001


def _brute_rows(lens):
    n = len(lens)
    return [sum(lens[i] + lens[j] + 14 for j in range(i + 1, n)) for i in range(n - 1)]


@pytest.mark.parametrize('seed', range(6))
def test_stripe_plan_matches_a_brute_force_count(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 90))
    lens = rng.integers(1, 400 if seed % 2 else 20, size=n)
    fps = rng.integers(0, 5, size=n)
    idx = np.concatenate([[0], np.cumsum(fps)])
    rows = _brute_rows([int(x) for x in lens])
    assert dct_sim.row_text_bytes(lens).tolist() == rows
    budget = int(rng.integers(1, 3 * max(rows)))
    fp_rows = int(rng.integers(1, 20))
    plan = dct_sim.plan_stripes(lens, idx, budget, fp_rows)
    assert plan[0][0] == 0 and plan[-1][1] == n - 1
    for (i0, i1, base, nbytes), nxt in zip(plan, plan[1:] + [None]):
        assert i1 > i0
        if nxt is not None:
            assert nxt[0] == i1
        assert base.tolist() == [sum(rows[i0:i]) for i in range(i0, i1)]
        assert nbytes == sum(rows[i0:i1])
        if i1 - i0 > 1:
            assert nbytes <= budget and idx[i1] - idx[i0] <= fp_rows
        if nxt is not None:                                  # (greedy: the next row did not fit)
            assert sum(rows[i0:i1 + 1]) > budget or idx[i1 + 1] - idx[i0] > fp_rows


def test_stripe_plan_of_tiny_files():
    assert dct_sim.plan_stripes([3], [0, 1], 100, 10) == []
    assert dct_sim.plan_stripes([], [0], 100, 10) == []
    (i0, i1, base, nbytes), = dct_sim.plan_stripes([1, 2], [0, 0, 0], 1, 1)
    assert (i0, i1, base.tolist(), nbytes) == (0, 1, [0], 17)


class _Binary:
    def __init__(self):
        import io
        self.buffer = io.BytesIO()
        self.text = []
        self.encoding = 'utf-8'

    def write(self, s):
        self.text.append(s)

    def flush(self):
        self.buffer.write(''.join(self.text).encode())
        self.text = []


def test_report_raw_keeps_the_order_and_falls_back_to_text(monkeypatch):
    import io
    out = _Binary()
    monkeypatch.setattr('sys.stdout', out)
    rep = dct_sim.Report()
    rep.line('a')
    rep.raw(memoryview('b é\n'.encode()))
    rep.line('c')
    rep.close()
    assert out.buffer.getvalue() == '#prot1 prot2 sim-domain sim-global\na\nb é\nc\n'.encode()
    sio = io.StringIO()
    monkeypatch.setattr('sys.stdout', sio)
    rep = dct_sim.Report()
    rep.raw(b'x \xc3\xa9\n')
    assert sio.getvalue() == dct_sim.HEADER + '\nx é\n'


@pytest.mark.parametrize('seed', range(4))
def test_protein_groups_are_the_greedy_ranges(seed):
    rng = np.random.default_rng(seed)
    for _ in range(300):
        n = int(rng.integers(0, 40))
        counts = rng.integers(0, 6, size=n)
        counts[rng.random(n) < 0.3] = 0
        idx = np.concatenate([[0], np.cumsum(counts)])
        max_rows = int(rng.integers(1, 15))
        groups = list(dct_sim._protein_groups(idx, max_rows))
        assert [g[0] for g in groups] == [0] * (n > 0) + [g[1] for g in groups[:-1]] and (groups[-1][1] == n if n else groups == [])
        for p0, p1 in groups:                                # at least one protein; otherwise as many as fit, and no more
            assert p1 > p0
            assert p1 - p0 == 1 or idx[p1] - idx[p0] <= max_rows
            assert p1 == n or idx[p1 + 1] - idx[p0] > max_rows
