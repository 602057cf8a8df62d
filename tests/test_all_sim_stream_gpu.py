"""All-against-all streamed from the device (dct_sim.AllPairs, dctfp_sim_lines): the reference's own output on a committed
synthetic golden, the block-matrix path (dct_sim.Blocks) on random ragged files, a file whose block matrix is never built,
the text kernel against Python formatting, and the two-buffer hand-over every device text goes out through."""

import gzip
import os

import numpy as np
import pytest

import golden_util as gu

pytestmark = pytest.mark.gpu
GOLD = os.path.join(gu.GOLD, 'all_sim')
NPZ = os.path.join(GOLD, 'all-dct.npz')


def _expected() -> bytes:
    with gzip.open(os.path.join(GOLD, 'expected.txt.gz'), 'rb') as fh:
        return fh.read()


def test_reference_golden_byte_for_byte(tmp_path):
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    dct_sim.main(['--dct', NPZ, '--output', out])
    assert open(out, 'rb').read() == _expected()


def test_stdout_keeps_the_order_of_its_lines(capfd):
    from dctdomain_amd import dct_sim
    dct_sim.main(['--dct', NPZ])
    lines = capfd.readouterr().out.split('\n')
    want = _expected().decode('utf8').split('\n')[:-1]
    assert lines[0] == dct_sim.HEADER == want[0]
    assert lines[1].startswith('dct loaded for 139 sequences, time used: ')
    assert lines[2:len(want) + 1] == want[1:]
    assert lines[len(want) + 1].startswith('total time used ')
    assert lines[len(want) + 2].startswith('distance calculation used ')
    assert lines[len(want) + 3:] == ['']


# ---- the block-matrix path as all_sim printed before AllPairs

def _blocks_all_sim(path) -> bytes:
    from dctdomain_amd import dct_sim
    blk = dct_sim.Blocks(path)
    lines = [dct_sim.HEADER]
    for i, j in zip(*np.triu_indices(len(blk.rows), k=1)):
        maxs, s = blk.scores(i, j)
        lines.append(f'{blk.rows[i]} {blk.rows[j]} {maxs:.3f} {s:.3f}')
    return ('\n'.join(lines) + '\n').encode('utf8')


_ALPHABET = list('abcdefghijklmnopqrstuvwxyz0123456789_|.-') + ['é', 'ß', 'α', '蛋', '😀']


def _ragged_file(path, seed, n):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 4, size=n)
    counts[rng.random(n) < 0.15] = 0                         # proteins without fingerprints
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    fam = rng.integers(-60, 61, size=(4, 480))
    dct = np.clip(fam[rng.integers(0, 4, size=int(idx[-1]))] + rng.integers(-20, 21, size=(int(idx[-1]), 480)), -127, 127).astype(np.int8)
    if idx[-1] > 3:
        dct[1] = dct[0]                                      # ties
    lens = rng.choice([1, 2, 5, 17, 40, 333], size=n, p=[.1, .1, .3, .3, .15, .05])
    names = [''.join(rng.choice(_ALPHABET, size=int(m))) for m in lens]
    np.savez(path, sid=np.array(names), idx=idx, dom=np.array(['1-9'] * len(dct)), dct=dct)


@pytest.mark.parametrize('seed,n,small', [(1, 60, False), (2, 45, True), (3, 2, False), (4, 1, False), (5, 33, True)])
def test_same_bytes_as_the_block_path(tmp_path, monkeypatch, seed, n, small):
    from dctdomain_amd import dct_sim
    path = str(tmp_path / 'r-dct.npz')
    _ragged_file(path, seed, n)
    want = _blocks_all_sim(path)
    if small:                                                # single-row stripes, many column groups, tiny tiles
        monkeypatch.setattr(dct_sim.AllPairs, 'TEXT_BYTES', 1 + seed * 40)
        monkeypatch.setattr(dct_sim.AllPairs, 'COL_ROWS', 3)
        monkeypatch.setattr(dct_sim.AllPairs, 'TILE_INTS', 5)
    out = str(tmp_path / 'out.txt')
    dct_sim.main(['--dct', path, '--output', out])
    assert open(out, 'rb').read() == want


def test_four_thousand_proteins_without_the_block_matrix(tmp_path, monkeypatch):
    from dctdomain_amd import dct_sim

    def refuse(*a, **k):
        raise AssertionError('all_sim must not build the block matrix')
    monkeypatch.setattr(dct_sim.Blocks, '__init__', refuse)
    rng = np.random.default_rng(17)
    n = 4000
    counts = rng.integers(1, 9, size=n)
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    dct = rng.integers(-40, 41, size=(int(idx[-1]), 480), dtype=np.int8)
    near = rng.choice(int(idx[-1]), size=2000)
    dct[near] = np.clip(dct[rng.choice(int(idx[-1]), size=2000)] + rng.integers(-6, 7, size=(2000, 480)), -127, 127)
    names = [f'prot{k}_' + 'x' * int(rng.integers(0, 12)) for k in range(n)]
    path = str(tmp_path / 'big-dct.npz')
    np.savez(path, sid=np.array(names), idx=idx, dom=np.array(['1-9'] * len(dct)), dct=dct)
    out = str(tmp_path / 'out.txt')
    monkeypatch.setattr(dct_sim.AllPairs, 'TEXT_BYTES', 1 << 24)   # (several stripes)
    dct_sim.main(['--dct', path, '--output', out])
    data = open(out, 'rb').read()
    assert data.count(b'\n') == 1 + n * (n - 1) // 2
    lens = np.array([len(s) for s in names], dtype=np.int64)
    starts = len(dct_sim.HEADER) + 1 + np.concatenate([[0], np.cumsum(dct_sim.row_text_bytes(lens))])
    rows = np.sort(rng.choice(n - 1, size=200, replace=False))
    rows[-1] = n - 2
    pairs = np.concatenate([np.stack([np.full(n - 1 - i, i), np.arange(i + 1, n)], axis=1) for i in rows])
    mn, last = dct_sim.pair_scores(dct, idx, pairs)
    k = 0
    for i in rows:
        got = data[starts[i]:starts[i + 1]].decode().split('\n')[:-1]
        want = []
        for j in range(i + 1, n):
            maxs, s = dct_sim._scores(mn[k], last[k])
            want.append(f'{names[i]} {names[j]} {maxs:.3f} {s:.3f}')
            k += 1
        assert got == want, i


def test_kernel_on_every_l1_value_with_unaligned_output():
    import torch
    from dctdomain_amd import dct_sim
    from dctdomain_amd.similarity import LineIds, sim_lines
    rng = np.random.default_rng(3)
    values = np.concatenate([np.arange(17002), [0x7fffffff]]).astype(np.int32)
    n_cols = len(values)
    n = n_cols + 1
    names = ['x', 'é', 'M' * 301] + [''.join(rng.choice(_ALPHABET, size=int(rng.integers(1, 30)))) for _ in range(n - 3)]
    ids = LineIds(names)
    row0, col0, n_rows = 0, 1, 3
    mn = np.stack([rng.permutation(values) for _ in range(n_rows)])
    last = np.stack([rng.permutation(values) for _ in range(n_rows)])
    enc = [s.encode() for s in names]
    table = dct_sim.score_table()
    want_rows = []
    for r in range(n_rows):
        i = row0 + r
        parts = []
        for c in range(n_cols):
            j = col0 + c
            if j > i:
                a = table[0, min(int(mn[r, c]), 17001)].tobytes()
                b = table[1, min(int(last[r, c]), 17001)].tobytes()
                parts.append(enc[i] + b' ' + enc[j] + b' ' + a + b' ' + b + b'\n')
        want_rows.append(b''.join(parts))
    base = np.zeros(n_rows, dtype=np.int64)
    pos = 3                                                  # unaligned starts, and gaps that must stay untouched
    for r in range(n_rows):
        base[r] = pos
        pos += len(want_rows[r]) + 5 + r
    out = torch.full((pos + 7,), 0xAB, dtype=torch.uint8, device='cuda')
    dev = lambda a: torch.as_tensor(a, device='cuda')       # noqa: E731
    # the columns in two calls, split at an odd place, like two column groups of a stripe
    split = 7777
    for c0, c1 in ((0, split), (split, n_cols)):
        sim_lines(dev(np.ascontiguousarray(mn[:, c0:c1])), dev(np.ascontiguousarray(last[:, c0:c1])), row0, col0 + c0, ids,
                  dev(table), base, out)
    got = out.cpu().numpy().tobytes()
    for r in range(n_rows):
        assert got[base[r]:base[r] + len(want_rows[r])] == want_rows[r], r
        gap_end = base[r + 1] if r + 1 < n_rows else len(got)
        assert set(got[base[r] + len(want_rows[r]):gap_end]) == {0xAB}
    assert set(got[:3]) == {0xAB}
    for v in (0, 8, 9, 12750, 17000, 17001, 0x7fffffff):
        a, b = dct_sim._scores(v, v)
        assert table[0, min(v, 17001)].tobytes().decode() == f'{a:.3f}'


def test_kernel_refuses_a_buffer_too_small():
    import torch
    from dctdomain_amd import dct_sim
    from dctdomain_amd.similarity import LineIds, sim_lines
    ids = LineIds(['a', 'bb', 'ccc'])
    mn = torch.zeros((1, 2), dtype=torch.int32, device='cuda')
    out = torch.zeros(20, dtype=torch.uint8, device='cuda')          # the row needs 2 * 15 + 5 = 35 bytes
    with pytest.raises(ValueError):
        sim_lines(mn, mn.clone(), 0, 1, ids, torch.as_tensor(dct_sim.score_table(), device='cuda'), [0], out)


# ---- similarity.TextStream

_TEXT_BYTES = 1 << 28       # AllPairs.TEXT_BYTES
_GROWTH = {
    'all_pairs': lambda nbytes: max(nbytes, min(_TEXT_BYTES, 2 * nbytes)),
    'filtered_pairs': lambda nbytes: max(nbytes, 1 << 16),
    'query_db': lambda nbytes: max(1, 70000),                # (fixed at the text buffer's size, which no chunk exceeds)
}


@pytest.mark.parametrize('rule', sorted(_GROWTH))
def test_text_stream_hands_every_chunk_over_once_and_one_behind(rule):
    import torch
    from dctdomain_amd.similarity import TextStream
    rng = np.random.default_rng(8)
    sizes = [1, 3, 70000, 5, 65536, 2]                          # (70 000: beyond a first buffer of 1 << 16 -- it has to grow)
    chunks = [rng.integers(0, 256, size=n, dtype=np.uint8) for n in sizes]
    got = []
    out = TextStream(lambda view: got.append(bytes(view)), room=_GROWTH[rule])
    for k, c in enumerate(chunks):
        text = torch.full((len(c) + 7,), 0xEE, dtype=torch.uint8, device='cuda')     # (a text buffer longer than its text)
        text[:len(c)] = torch.as_tensor(c, device='cuda')
        out.hand_over(text, len(c))
        assert len(got) == k                                    # chunk k + 1 handed over: the k before it have gone out
        text.fill_(0)                                           # (what the sink gets is the chunk as it was handed over)
    assert got == [c.tobytes() for c in chunks[:-1]]
    out.close()
    assert got == [c.tobytes() for c in chunks]
    out.close()                                                 # (nothing is held: nothing goes out twice)
    assert len(got) == len(chunks)
    assert all(p.is_pinned() for p in out.pinned)
