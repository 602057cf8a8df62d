#!/usr/bin/env python3
"""Writes tests/golden/silhouette/G6PD_{global,domain}.txt: the output of python -m dctdomain_amd.cluster_quality on the G6PD fixture
with the single-linkage clusters at --min-global 0.6, as tests/silhouette_rule.py states it (no GPU, no product code).
usage: python tests/golden/make_golden_silhouette.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cluster_rule  # noqa: E402
import silhouette_rule  # noqa: E402

OUT = os.path.join(HERE, 'silhouette')


def g6pd():
    """(sid, idx, dct, labels): the fixture and the representative id of every protein at --min-global 0.6."""
    with np.load(os.path.join(HERE, 'ref_fixtures', 'G6PD-dct.npz')) as data:
        sid, idx, dct = data['sid'], np.asarray(data['idx'], dtype=np.int64), data['dct']
    label, _ = cluster_rule.labels(dct, idx, min_global=0.6)
    return sid, idx, dct, [f'{sid[int(k)]}' for k in label]


def expected(score: str) -> bytes:
    sid, idx, dct, labels = g6pd()
    four = silhouette_rule.sums(silhouette_rule.key_matrix(dct, idx, score), labels)
    return silhouette_rule.PROTEIN_HEADER + silhouette_rule.text(sid, labels, four)


if __name__ == '__main__':
    os.makedirs(OUT, exist_ok=True)
    for score in ('global', 'domain'):
        with open(os.path.join(OUT, f'G6PD_{score}.txt'), 'wb') as fh:
            fh.write(expected(score))
