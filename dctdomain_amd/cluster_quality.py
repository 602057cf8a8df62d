"""How good a clustering of one ``-dct.npz`` file is, without knowing the answer: the silhouette of every protein, summed on the GPU.

    python -m dctdomain_amd.cluster_quality --dct X-dct.npz (--clusters FILE | --families FILE | --family-sep C)
                                            [--score {domain,global}] [--per {protein,cluster}] [--out FILE]

``--clusters`` reads ``representative member`` lines: what ``dct-sim --cluster``, ``--hac --flat`` and ``--assign`` print, or the
two-column table of another tool (MMseqs2's ``createtsv``, a converted CD-HIT table).  A command of its own, not a mode of ``dct-sim``,
whose command line is recorded token for token."""

from __future__ import annotations

import argparse
import math

import numpy as np

from .dct_sim import (L1_FULL_SCALE, SCORES, Report, _DeviceRows, _last_rows, _load_npz, _protein_groups, families_from_ids,
                      read_families)

PER = ('protein', 'cluster')
PROTEIN_HEADER = '#protein cluster size own other neighbour silhouette'
CLUSTER_HEADER = '#cluster size mean_silhouette min_silhouette negative'
UNDEFINED = '-'


def dense_clusters(labels):
    """(cluster, first, size) of one label per protein, of any hashable kind: ``cluster[i]`` = the index of protein i's cluster,
    the clusters numbered by their first member in the file; ``first[c]`` / ``size[c]`` = that member and the number of members.
    int64 numpy arrays, one pass over the labels."""
    index, cluster, first = {}, np.empty(len(labels), dtype=np.int64), []
    for i, label in enumerate(labels):
        c = index.setdefault(label, len(index))
        if c == len(first):
            first.append(i)
        cluster[i] = c
    return cluster, np.asarray(first, dtype=np.int64), np.bincount(cluster, minlength=len(first)).astype(np.int64)


def silhouette_value(own_sum: int, n_own: int, near_sum: int, n_near: int) -> float:
    """s = (Sb na - Sa nb) / max(Sa nb, Sb na) from Python integers with one division at the end; 0 when the maximum is 0 and for
    the member of a singleton cluster (na = 0: scikit-learn's convention)."""
    if n_own == 0:
        return 0.0
    a, b = int(own_sum) * int(n_near), int(near_sum) * int(n_own)
    return (b - a) / max(a, b) if max(a, b) else 0.0


def _mean_similarity(total: int, count: int) -> str:
    """1 - S / (n 17000) at four decimals; ``-`` where there is nothing to average."""
    return UNDEFINED if count == 0 else '%.4f' % (1 - int(total) / (int(count) * L1_FULL_SCALE))


def _fixed(value) -> str:
    return UNDEFINED if value is None or math.isnan(value) else '%.4f' % value


class Silhouette:
    """The silhouette of a clustering of one file on DCTdomain (``score='domain'``) or DCTglobal (``'global'``).

    These are exact integers.  key(i, j) = min(L1(i, j), 17000): under ``domain`` the protein minimum (what ``protein_min`` writes),
    under ``global`` the L1 of the two last rows; 17000 when either protein has no fingerprints; i == j never counts.  A clustering
    is one label per protein (``labels``: strings or ints).  For protein i in cluster A: Sa = the sum of key(i, j) over j in A,
    j != i, with na = |A| - 1; for every other cluster B, S(B) = the sum of key(i, j) over j in B, with nb = |B|.  The neighbour
    cluster minimises the fraction S(B) / |B|, compared exactly (cross-multiplied, no floating point), ties to the cluster whose
    first member comes first in the file.  s(i) = (Sb na - Sa nb) / max(Sa nb, Sb na), computed on the host from Python integers
    with one division at the end: 0 when the maximum is 0, 0 for the member of a singleton cluster (scikit-learn's convention),
    undefined (NaN, ``-`` in the text) for every protein when the file has fewer than two clusters.  With a precomputed matrix of
    the keys this is ``sklearn.metrics.silhouette_samples(metric='precomputed')``.

    The GPU returns only integers, so the text is the same on every machine: per protein Sa (uint64), Sb (uint64), |B| (int32)
    and the first member of B (int32, -1 for none), 24 bytes.  Dense ids, sizes and first members are computed on the host in
    O(n).  Rows go in stripes x all n columns (at most ``TILE_INTS`` entries), filled as ``Dendrogram._matrix`` fills its stripes --
    ``l1_matrix`` of the last rows, or ``protein_min`` over column groups of at most ``COL_ROWS`` fingerprints -- and scanned with
    one launch per stripe (``similarity.silhouette_rows``: a workgroup per row, the sums of a row's clusters in its LDS).  Nothing
    of size n x n or n x C exists anywhere.  The full square costs twice the fill of ``--cluster``'s triangle and nothing else: on
    the triangle a pair is seen once and would have to reach a sum of both its rows, an n x C accumulator in device memory."""

    COL_ROWS = 1 << 22      # fingerprints on the device at a time (the whole file stays there if it fits)
    TILE_INTS = 1 << 28     # int32 entries of one stripe's tile (1 GiB)
    PASS_CLUSTERS = 4096    # cluster sums a workgroup keeps at a time (``similarity.silhouette_rows``)

    def __init__(self, sid, idx, fps, labels, score: str = 'domain'):
        if score not in SCORES:
            raise ValueError(f'score must be one of {SCORES}')
        self.sid, self.fps, self.score = sid, fps, score
        self.idx = np.asarray(idx, dtype=np.int64) if idx is not None else None
        self.labels = list(labels)
        if len(self.labels) != len(sid) or (self.idx is not None and len(self.idx) - 1 != len(sid)):
            raise ValueError('labels must have one entry per protein')
        self.cluster, self.first, self.size = dense_clusters(self.labels)
        self._sums = None

    @property
    def n(self) -> int:
        return len(self.labels)

    def device_clusters(self):
        """(cid, size, first) as the kernel reads them, int32 numpy arrays: the dense id of every protein's cluster among those of
        two or more members (numbered by first member), -1 for a singleton; and the sizes and first members of those."""
        multi = self.size >= 2
        dense = np.where(multi, np.cumsum(multi) - 1, -1)
        return dense[self.cluster].astype(np.int32), self.size[multi].astype(np.int32), self.first[multi].astype(np.int32)

    def with_sums(self, own_sum, near_sum, near_size, near_first):
        """The object with the four arrays of ``sums()`` given instead of computed: everything behind them is host arithmetic."""
        sums = tuple(np.asarray(a, dtype=np.int64) for a in (own_sum, near_sum, near_size, near_first))
        if any(a.shape != (self.n,) for a in sums):
            raise ValueError('one entry per protein in each of the four arrays')
        self._sums = sums
        return self

    def sums(self):
        """(own_sum, near_sum, near_size, near_first): int64 numpy arrays, one entry per protein -- Sa, Sb, |B| and the first
        member of the neighbour cluster B (0, 0 and -1 where there is no other cluster).  Computed once, on the GPU."""
        if self._sums is None:
            self._sums = self._scan()
        return self._sums

    def _stripes(self):
        """[i0, i1) ranges of rows: stripes x all n columns within TILE_INTS, and (domain) their fingerprints within COL_ROWS."""
        n, step = self.n, max(1, self.TILE_INTS // max(1, self.n))
        if self.score == 'global':
            return [(i0, min(n, i0 + step)) for i0 in range(0, n, step)]
        return [(j0, min(i1, j0 + step)) for i0, i1 in _protein_groups(self.idx, self.COL_ROWS) for j0 in range(i0, i1, step)]

    def _scan(self):
        n, idx = self.n, self.idx
        if n == 0:
            return tuple(np.zeros(0, dtype=np.int64) for _ in range(4))
        import torch
        from .similarity import l1_matrix, protein_min, silhouette_rows, to_device_int8
        dev = torch.device('cuda', torch.cuda.current_device())
        cid, size, first = (torch.as_tensor(a, device=dev) for a in self.device_clusters())
        own_sum, near_sum = (torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(2))
        near_size, near_first = torch.zeros(n, dtype=torch.int32, device=dev), torch.full((n,), -1, dtype=torch.int32, device=dev)
        total = int(idx[-1])
        empty = torch.as_tensor((idx[1:] == idx[:-1]).astype(np.uint8), device=dev)
        if self.score == 'global':
            last = to_device_int8(_last_rows(self.fps[:total], idx)[0])
        else:
            rows = _DeviceRows(self.fps, idx, self.COL_ROWS)
        for i0, i1 in self._stripes():
            tile = torch.empty((i1 - i0, n), dtype=torch.int32, device=dev)
            if self.score == 'global':
                l1_matrix(last[i0:i1], last, out=tile)
            else:
                a, ia = rows(i0, i1), idx[i0:i1 + 1] - idx[i0]
                for q0, q1 in _protein_groups(idx, self.COL_ROWS):
                    protein_min(a, ia, rows(q0, q1), idx[q0:q1 + 1] - idx[q0], out=tile[:, q0:q1])
            # (the key is formed in the kernel: a protein without fingerprints is flagged, protein_min's 0x7fffffff is above the cap)
            silhouette_rows(tile, i0, 0, cid, size, first, own_sum, near_sum, near_size, near_first, empty[i0:i1], empty,
                            cap=L1_FULL_SCALE, pass_clusters=self.PASS_CLUSTERS)
            del tile
        back = torch.stack([own_sum, near_sum, near_size.to(torch.int64), near_first.to(torch.int64)]).cpu().numpy()    # 24 bytes of results per protein
        return tuple(back[k].copy() for k in range(4))

    def defined(self) -> bool:
        """Whether the file has two clusters at least: else no protein has a silhouette."""
        return len(self.size) >= 2

    def values(self) -> np.ndarray:
        """float64 (n): the silhouette of every protein, NaN for all of them when the file has fewer than two clusters."""
        if not self.defined():
            return np.full(self.n, np.nan)
        own_sum, near_sum, near_size, _ = self.sums()
        n_own = self.size[self.cluster] - 1
        return np.array([silhouette_value(own_sum[i], n_own[i], near_sum[i], near_size[i]) for i in range(self.n)], dtype=np.float64)

    def neighbours(self) -> np.ndarray:
        """int64 (n): the first member of every protein's neighbour cluster, -1 where there is no other cluster."""
        return self.sums()[3].copy()

    def summary(self) -> dict:
        """proteins, clusters, singletons, mean (None: undefined), negative, and per cluster in the order of their first members
        ``clusters_detail`` = (first member, size, mean, min, negatives) -- mean and min None where undefined."""
        values = self.values()
        ok = self.defined()
        detail = []
        order = np.argsort(self.cluster, kind='stable')
        bounds = np.concatenate([[0], np.cumsum(self.size)])
        for c in range(len(self.size)):
            v = values[order[bounds[c]:bounds[c + 1]]]
            detail.append((int(self.first[c]), int(self.size[c]), math.fsum(v) / len(v) if ok else None, float(v.min()) if ok else None,
                           int((v < 0).sum()) if ok else 0))
        return {'proteins': self.n, 'clusters': len(self.size), 'singletons': int((self.size == 1).sum()),
                'mean': math.fsum(values) / self.n if ok and self.n else None, 'negative': int((values < 0).sum()) if ok else 0,
                'clusters_detail': detail}

    def last_line(self, summary: dict = None) -> str:
        s = summary if summary is not None else self.summary()
        return (f'# proteins={s["proteins"]} clusters={s["clusters"]} singletons={s["singletons"]} mean_silhouette={_fixed(s["mean"])} '
                f'negative={s["negative"]}')

    def lines(self, per: str = 'protein'):
        """The result lines without the header, the summary line last.  ``per='protein'``: ``protein cluster size own other neighbour
        silhouette`` -- own and other are the mean similarities 1 - S / (n 17000) to the own and to the neighbour cluster, ``-``
        marks anything undefined; ``per='cluster'``: ``cluster size mean_silhouette min_silhouette negative``."""
        if per not in PER:
            raise ValueError(f'per must be one of {PER}')
        summary = self.summary()
        if per == 'cluster':
            for first, size, mean, low, negative in summary['clusters_detail']:
                yield f'{self.labels[first]} {size} {_fixed(mean)} {_fixed(low)} {negative}'
        else:
            own_sum, near_sum, near_size, near_first = self.sums()
            values = self.values()
            for i in range(self.n):
                size = int(self.size[self.cluster[i]])
                near = int(near_first[i])
                yield (f'{self.sid[i]} {self.labels[i]} {size} {_mean_similarity(own_sum[i], size - 1)} '
                       f'{_mean_similarity(near_sum[i], near_size[i] if near >= 0 else 0)} {self.labels[near] if near >= 0 else UNDEFINED} '
                       f'{_fixed(values[i])}')
        yield self.last_line(summary)

    def write(self, sink, per: str = 'protein', chunk_lines: int = 1 << 16):
        """Calls ``sink(bytes)`` with the text of ``lines(per)``, whole lines at a time, in order."""
        chunk = []
        for line in self.lines(per):
            chunk.append(line)
            if len(chunk) >= chunk_lines:
                sink(('\n'.join(chunk) + '\n').encode('utf8'))
                chunk = []
        if chunk:
            sink(('\n'.join(chunk) + '\n').encode('utf8'))


def read_clusters(path: str, sid) -> list:
    """The representative of every protein of ``sid`` from a file of ``representative member`` lines, separated by whitespace
    (``--clusters``): the output of ``dct-sim --cluster``, ``--hac --flat`` or ``--assign``, or another tool's two-column table.
    Blank lines and lines that start with ``#`` are skipped, members that are not in ``sid`` ignored.  ValueError for the
    four-field lines of ``--cluster --level domain`` (whose nodes are fingerprints, not proteins), for any other line that is not two
    fields, for a member given two representatives and for a protein of ``sid`` without a line (the first such id is named)."""
    wanted = {f'{s}' for s in sid}
    rep_of = {}
    with open(path, encoding='utf8') as fh:
        for number, line in enumerate(fh, 1):
            fields = line.split()
            if not fields or fields[0].startswith('#'):
                continue
            if len(fields) == 4:
                raise ValueError(f'{path}, line {number}: four fields, a line of dct-sim --cluster --level domain -- those clusters are of '
                                 f'domains, not of proteins, and have no protein silhouette')
            if len(fields) != 2:
                raise ValueError(f'{path}, line {number}: a line is "representative member", two fields separated by whitespace')
            rep, member = fields
            if member not in wanted:
                continue
            if rep_of.setdefault(member, rep) != rep:
                raise ValueError(f'{path}, line {number}: {member} is given two representatives, {rep_of[member]} and {rep}')
    for s in sid:
        if f'{s}' not in rep_of:
            raise ValueError(f'{path} has no line for {s}')
    return [rep_of[f'{s}'] for s in sid]


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog='python -m dctdomain_amd.cluster_quality',
                                     description='The silhouette of a clustering of one -dct.npz file: per protein, how much closer it '
                                                 'is to its own cluster than to the nearest other one.  No family labels are needed.')
    parser.add_argument('--dct', required=True, metavar='X-dct.npz', help='the fingerprints of the proteins that were clustered')
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument('--clusters', metavar='FILE', help='"representative member" lines: the output of dct-sim --cluster, --hac --flat '
                                                           'or --assign, or another tool\'s two-column table')
    source.add_argument('--families', metavar='FILE', help='"id family" lines, as for dct-sim --auc1: the families taken as the clusters')
    source.add_argument('--family-sep', metavar='C', help='the clusters are the text after the first C of every id')
    parser.add_argument('--score', choices=SCORES, default='domain', help='the distance: DCTdomain (default) or DCTglobal')
    parser.add_argument('--per', choices=PER, default='protein', help='one line per protein (default) or per cluster')
    parser.add_argument('--out', metavar='FILE', help='the result file (default: stdout)')
    return parser


def cluster_quality(npzfile: str, output=None, clusters: str = None, families: str = None, family_sep: str = None, score: str = 'domain',
                    per: str = 'protein'):
    """The command: the labels from exactly one of ``clusters`` / ``families`` / ``family_sep``, the text to ``output`` (a path, or
    None: stdout) through ``dct_sim.Report``."""
    if sum(x is not None for x in (clusters, families, family_sep)) != 1:
        raise ValueError('the clusters come from one place: clusters, families (files) or family_sep (the ids themselves)')
    if per not in PER:
        raise ValueError(f'per must be one of {PER}')
    sid, idx, fps = _load_npz(npzfile)
    if clusters is not None:
        labels = read_clusters(clusters, sid)
    else:
        labels = read_families(families, sid) if families is not None else families_from_ids(sid, family_sep)
    job = Silhouette(sid, idx, fps, labels, score=score)
    report = Report(output, PROTEIN_HEADER if per == 'protein' else CLUSTER_HEADER)
    try:
        job.write(report.raw, per=per)
    finally:
        report.close()


def main(argv=None):
    args = build_parser().parse_args(argv)
    cluster_quality(args.dct, args.out, clusters=args.clusters, families=args.families, family_sep=args.family_sep, score=args.score,
                    per=args.per)


if __name__ == '__main__':
    main()
