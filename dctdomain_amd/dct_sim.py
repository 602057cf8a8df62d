"""Drop-in for mgtools/DCTdomain ``src/dct-sim.py``: similarity between proteins from their DCT
fingerprints (``-dct.npz``), with the L1 distances computed on the GPU.

    python -m dctdomain_amd.dct_sim --dct X-dct.npz [--pair P | --db Y-dct.npz [--rank {global,domain}]] [--output F]
                                    [--pairfound F] [--top 5] [--threshold 0.25] [--min-domain X] [--min-global Y]
                                    [--min-coverage C [--cov-unit {residues,domains}]]
                                    [--cluster [--linkage {single,greedy}] [--level {protein,domain} [--no-whole]] [--rep {first,medoid}]
                                     [--min-neighbors M]]
                                    [--domains] [--domain-map [X]]
                                    [--dom X.dom] [--db-dom Y.dom]
    python -m dctdomain_amd.dct_sim --dct NEW-dct.npz --assign REPS-dct.npz --min-domain X [--min-global Y] [--reps-out ALL-dct.npz]
                                    [--output F]
    python -m dctdomain_amd.dct_sim --dct X-dct.npz --tree [domain|global] [--min-domain X | --min-global Y] [--output F]
    python -m dctdomain_amd.dct_sim --dct X-dct.npz --hac [domain|global] [--method {average,complete}] [--min-domain X | --min-global Y]
                                    [--flat] [--newick FILE] [--output F]
    python -m dctdomain_amd.dct_sim --dct A-dct.npz --db B-dct.npz --rbh [domain|global] [--min-domain X | --min-global Y] [--domains]
                                    [--dom A.dom] [--db-dom B.dom] [--output F]
    python -m dctdomain_amd.dct_sim --dct X-dct.npz --auc1 [domain|global] (--families FILE | --family-sep C)
                                    [--min-domain X | --min-global Y] [--output F]
    python -m dctdomain_amd.dct_sim --dct X-dct.npz --hist [domain|global] [--bins B] [--families FILE | --family-sep C]
                                    [--min-domain X | --min-global Y] [--output F]

Same flags, same output text (src/dct-sim.py:179-211); ``--rank domain`` (not in the reference) orders database hits by
DCTdomain instead of DCTglobal, and ``--min-domain`` / ``--min-global`` (not in the reference either, which ignores
``--threshold`` in that mode) keep only the all-against-all lines whose scores are not below the cut-offs.  DCTdomain = max over all domain pairs of
``1 - min(L1/17000, 1)``, DCTglobal = the same for the two last (whole-protein) fingerprints
(:12-50).

Where the reference loops over protein pairs and, inside, over domain pairs in Python:
- ``all_sim`` walks the upper triangle in stripes of proteins (``AllPairs``): the int8 L1 matrix of a stripe's fingerprints
  against those of the later proteins (``dctfp_l1_matrix``), reduced per protein x protein block to (minimum, last-last)
  (``dctfp_block_min``) and turned into the result text on the device (``dctfp_sim_lines``), which streams out through two
  pinned buffers (``similarity.TextStream``, as every text composed on the device does).  Host memory is the two buffers plus
  O(n), not the n x n block matrix (``Blocks``, kept for its callers);
- with a cut-off, ``all_sim`` never forms the other lines (``FilteredPairs``): per stripe one tile of protein-pair L1 values
  (``dctfp_protein_min``, or the last rows' ``dctfp_l1_matrix`` when DCTglobal is cut), the pairs of the triangle within the
  bound selected on the device in output order (``dctfp_tri_filter_count`` / ``dctfp_tri_filter_fill``), both scores for those
  (``dctfp_pair_min``) and their lines (``dctfp_pair_lines``);
- ``cluster_sim`` (``--cluster`` with a cut-off, not in the reference) joins those pairs into single-linkage clusters instead of
  printing them (``Clusters``): the same tiles, a lock-free union-find on the device (``dctfp_tri_link`` / ``dctfp_link_pairs``
  / ``dctfp_cluster_labels``), one ``representative member`` line per protein.  ``--linkage greedy`` takes the proteins in file
  order instead (``Representatives``; CD-HIT's rule): one that no earlier representative has an edge to becomes a representative,
  every other one goes to the lowest representative it has an edge to -- so every member is within the cut-off of its
  representative and no two representatives are within it of each other, decided on the device in rounds over the same tiles
  (``dctfp_greedy_decide`` / ``dctfp_greedy_tri_mark`` / ``dctfp_greedy_pairs_mark``);
- ``--cluster --rep medoid`` (``Clusters.medoids``; CD-HIT names a cluster by its longest member, MMseqs2 has ``result2repseq``)
  names every single-linkage cluster by its most central member instead of its first in the file: the member with the smallest
  summed distance min(L1, 17000) to the others, ties to the lowest index.  A second pass over the same tiles with the final labels
  on the device adds every pair of one cluster to the sums of both its proteins (``dctfp_label_sums``: exact 64-bit integer sums by
  atomic adds of per-workgroup partial sums); the choice per cluster is n-element work in torch, n int32 come back.  Under
  ``--min-coverage`` the coverage decides who is in a cluster and the plain distances decide its medoid.  The lines and their order
  stay, only the first field changes; ``--reps-out`` writes the medoids for a later ``--assign``;
- ``--cluster --min-neighbors M`` (``DensityClusters``; DBSCAN with the cut-off as its radius) keeps single linkage from chaining two
  families through one pair: only a protein with at least M pairs within the cut-offs -- a core -- passes a link on.  Clusters are
  the components of the core-core pairs; any other protein with a core neighbour joins the cluster of its lowest one, the rest are
  clusters of their own.  Two passes over the same tiles: the degrees (``dctfp_tri_degree``), then the unions of the core-core pairs
  and per non-core protein its lowest core neighbour (``dctfp_tri_link_core``); the rest is n-element work in torch.  M = 1 is
  ``--cluster`` itself;
- ``--min-coverage C`` (with ``--min-domain``, in the all-against-all and in ``--cluster`` at protein level; MMseqs2's ``-c``, CD-HIT's
  ``-aL`` / ``-aS``) keeps a pair only when it also covers the share C of BOTH proteins, so that one shared domain no longer links
  a six-domain protein to everything that carries it.  A fingerprint of one protein is matched when some fingerprint of the other
  is within the DCTdomain cut-off of it; the matched fingerprints' weights -- the residues ``make_db`` wrote for them
  (``--cov-unit residues``: the ``dom`` array of the npz, or ``--dom``) or 1 per domain (``domains``), the whole-protein fingerprint
  standing for all of them -- must reach ceil(C x the protein's weight).  The tiles then come from ``dctfp_protein_cover``:
  ``dctfp_protein_min``'s values, and 0x7fffffff for the pairs that fail, so the filter, the union-find and the greedy rounds run
  unchanged;
- ``--assign REPS`` (``Assignment``, not in the reference) goes on from such a run when proteins are added: every protein of
  ``REPS`` is a fixed representative, the proteins of ``--dct`` are taken in file order by the same rule.  The hot step compares
  every fingerprint of the representatives with every fingerprint of the new proteins and keeps, per new protein, the lowest
  representative within the cut-off (``dctfp_rows_assign``: ``dctfp_rows_link``'s contraction over the full rectangle, an atomic
  minimum instead of a union -- no distance is stored); the proteins left uncovered are clustered among themselves by
  ``Representatives``.  ``--reps-out`` writes the representatives as a ``-dct.npz`` (also with ``--cluster --linkage greedy``,
  which starts the chain): greedy on the first k proteins, then ``--assign`` of the rest, ends on the representatives of one
  greedy run over the whole file;
- ``--tree`` (``Tree``, not in the reference) answers ``--cluster`` for every cut-off at once: the single-linkage tree of the file,
  the minimum spanning forest of the pairs of similarity above 0 (or not below a cut-off) under the strict order (L1, i, j),
  printed as the all-against-all's own lines for its n - 1 pairs, most similar first -- the merge order of single linkage.  Cut at
  any score, its lines give the clusters ``--cluster`` finds there.  Boruvka's algorithm in at most ceil(log2 n) + 1 rounds over
  the same tiles: per component the lightest edge that leaves it (``dctfp_tri_nearest``), then one hook per component in the same
  union-find (``dctfp_tree_hook``) and the new labels (``dctfp_cluster_labels``);
- ``--hac`` (``Dendrogram``, not in the reference) gives the two hierarchical clusterings the modes above lack: complete linkage, whose
  clusters have a diameter -- every pair inside one is within the cut-off, where single linkage chains and the greedy rule only bounds
  the distance to the representative -- and average linkage, UPGMA.  The dense n x n matrix of the file stays on the device (n <= 46 340),
  filled by ``dctfp_protein_min`` / ``dctfp_l1_matrix``; in rounds, every live cluster takes its nearest live cluster within the bound
  (``dctfp_linkage_nearest``), the mutual pairs merge all at once, and the matrix is updated in place (``dctfp_linkage_merge``).
  Distances are exact integers -- maxima in int32, sums in int64 compared as fractions -- so the lines ``rep1 rep2 similarity size``,
  the ``--flat`` clusters and the ``--newick`` trees are the same on every machine;
- ``--auc1`` (``Auc1``) says how good the scores of a labelled file are, the number of the reference's own sensitivity benchmark
  (bench/cathdb/plot_results.py): every protein is searched against the file, and its AUC1 is the share of its family's other
  members ranked before the first hit of another family; the share of queries whose best hit is of their own family is the top-1
  rate.  Two scans over the same tiles with a family per protein on the device -- the first false positive of every protein as
  an atomic minimum of ``key << 32 | index`` (``dctfp_tri_first_fp``), then the true positives ranked before it
  (``dctfp_tri_tp_before``) -- and 12 bytes per protein come back; no ranked list is ever printed or parsed;
- ``--hist`` (``Histogram``) helps to choose the cut-off that every mode above asks for: the distribution of one score over all
  pairs of the file and, per cut-off of ``--bins``, how many pairs ``--min-domain`` / ``--min-global`` at that cut-off would keep;
  with a family per protein (``--families`` / ``--family-sep``) the pairs of one family and of two apart, so recall, precision and
  false-positive rate per cut-off, the ROC AUC and the cut-off of the best F1 -- what the reference's bench/G6PD/hist.py and
  bench/homo/results/AUC.py compute from the printed all-against-all.  One scan over the same tiles bins every pair's key on the
  device (``dctfp_tri_hist``: counters in LDS per workgroup, 64-bit atomic adds of the non-zero bins) and 8 bytes per bin and class
  come back, whatever the size of the file; the similarity-0 bin follows from the totals on the host;
- ``--cluster --level domain`` (``DomainClusters``) clusters the fingerprint ROWS of the file instead of its proteins -- the
  domain families: two rows of different proteins are joined when their own L1 passes ``--min-domain``, where the protein level
  joins two proteins as soon as any one of their fingerprint pairs does.  One kernel (``dctfp_rows_link``) takes a stripe of
  rows against the rows from the stripe's start onward: ``dctfp_l1_matrix``'s contraction, compared with the bound in registers
  and joined in the same union-find -- no distance is stored; then ``dctfp_cluster_labels`` and one
  ``representative member dom1 dom2`` line per row.  ``--no-whole`` leaves the whole-protein row of every multi-domain protein
  out; ``--dom`` names the rows by their residue ranges;
- ``db_search`` ranks on the whole-protein fingerprints only (one L1 per protein pair), selects the printed hits of
  every query on the GPU (``dctfp_select_count`` / ``dctfp_select_fill``) and computes DCTdomain for those pairs only
  (``dctfp_pair_min``): ``ProteinSearch``.  Host memory is what is printed plus one tile, not n_query x n_db.  With
  ``--rank domain`` it ranks on DCTdomain instead: the tiles hold every protein pair's minimum over all fingerprint pairs
  (``dctfp_protein_min``), selected the same way;
- ``--db Y --rbh`` (``ReciprocalBest``, not in the reference) prints the reciprocal best hits of the two files, the usual first-pass
  ortholog call: the pairs (a, b) where b is the best hit of a among the proteins of ``--db`` and a the best hit of b among those
  of ``--dct``, by DCTdomain (``domain``) or DCTglobal (``global``), ties to the lower index in the file, hits being the pairs of
  similarity above 0 (or not below that score's cut-off).  One search pass instead of two and a join by hand: ``ProteinSearch``'s
  tiles (``dctfp_protein_min``, or ``dctfp_l1_matrix`` of the last rows) go to one kernel that keeps the best column of every row
  and the best row of every column with atomic minima of ``key << 32 | index`` (``dctfp_rect_best``); 8 bytes per protein come
  back at the end, and the lines are ``db_search``'s lines for those pairs;
- ``--db Y --zscore`` (not in the reference) adds a z-score to every hit line, with or without ``--rbh``: the place of the hit's L1
  in the query's background, the raw L1s of the query against every protein of the database under the score that ranks
  (``zscore_of`` states the rule).  The tiles the search fills anyway are scanned once more before the hits are selected
  (``dctfp_rect_moments``: count, sum and sum of squares per protein, exact 64-bit integers) and 24 bytes per protein come back;
  z follows on the host from integers, the same on every machine.  ``--min-z Z`` drops the selected lines whose z is below Z;
- ``pair_sim`` uploads the fingerprints of the proteins its pairs name and runs ``dctfp_pair_min`` on the pairs.
``--domains`` (not in the reference) adds two fields to every result line: the fingerprint of each protein that DCTdomain came
from -- the pair the reference's double loop (:42-50) ends on: the smallest L1, ties to the lowest row of the first protein, then
of the second; ``-`` in both when no pair beats the loop's starting 0.  The scores then come from ``dctfp_pair_argmin`` instead
of ``dctfp_pair_min`` (the same reads, the position of the minimum kept); the all-against-all goes through ``FilteredPairs``
whatever the cut-offs and composes its lines with ``dctfp_pair_domain_lines``.  A fingerprint prints as its 1-based index within
the protein, or, with the ``.dom`` file of the npz (``--dom`` / ``--db-dom``), as the residue ranges ``make_db`` wrote there
(``whole`` for the unnamed whole-protein row).
``--domain-map [X]`` (not in the reference; implies ``--domains``) adds one more field behind those two: every matched domain pair
of the line, not only the best -- ``side/side``, the fingerprints of prot1 that have a counterpart in prot2, then those of prot2
that have one in prot1, each as ``label=label of its nearest fingerprint of the other protein:similarity``, joined by ``;`` (``-``
for none).  A fingerprint is matched when that L1 is at most ``map_bound``: ``sim_bound(X)`` -- X the option's value, else
``--min-domain``, else 0.25 -- and never an L1 of similarity 0; with ``--min-domain`` alone these are the fingerprints
``--min-coverage`` counts.  ``dctfp_pair_row_best`` keeps every row's nearest row of the other protein for the printed pairs
(``dctfp_pair_argmin``'s contraction, both ways); ``--pair``, ``--db`` and ``--rbh`` compose the field on the host
(``map_field``), the all-against-all on the device in two passes of one kernel (``dctfp_pair_map_lines``: the lines' lengths,
then the text at their cumulative sum).
Scores are formed from the integer L1 values with the reference's arithmetic (int64 / 17000 in float64), so the printed
floats are identical."""

from __future__ import annotations

import argparse
import contextlib
import math
import sys
import time
import typing

import numpy as np

from .similarity import (GREEDY_NONE, PROTEIN_MIN_MAX_D, GreedyState, LineIds, TextStream, _utf8_binary, block_min, block_min_device, cluster_labels,
                         greedy_decide, greedy_pairs_mark, greedy_tri_mark, l1_matrix, link_pairs, pair_argmin, pair_argmin_device, pair_line_offsets, pair_lines, pair_min, pair_min_device, protein_cover, protein_min,
                         rows_assign, rows_link, sim_lines, threshold_select, to_device_int8, tri_filter_count, tri_filter_fill, tri_link,
                         TREE_MAX_NODES, TreeState, tree_hook, tri_nearest, BestState, rect_best, label_sums, NEAREST_NONE, tri_degree,
                         tri_link_core, BEST_NONE, tri_first_fp, tri_tp_before, tri_hist, MomentState, rect_moments, pair_row_best,
                         pair_row_best_device, pair_row_offsets, pair_map_line_lengths, pair_map_lines)

L1_FULL_SCALE = 17000      # src/dct-sim.py:24
HEADER = '#prot1 prot2 sim-domain sim-global'
CLUSTER_HEADER = '#representative member'
DOMAIN_HEADER = HEADER + ' dom1 dom2'      # --domains
DOMAIN_CLUSTER_HEADER = CLUSTER_HEADER + ' dom1 dom2'      # --cluster --level domain
NO_DOMAIN = '-'                            # no fingerprint pair scores above 0
WHOLE = 'whole'                            # the whole-protein row a .dom file leaves unnamed
MAP_COLUMN = ' domain-map'                 # --domain-map: what it adds to DOMAIN_HEADER
MAP_SIMILARITY = 0.25                      # ... and the similarity from which a row is matched where neither it nor --min-domain says


def _z_spread(n: int, s1: int, s2: int):
    """sqrt(n s2 - s1^2) = n sigma of a background (Python integers: the radicand is exact, then one ``math.sqrt``); None where no z is
    defined against it: n < 2, or a radicand of 0."""
    radicand = n * s2 - s1 * s1
    return math.sqrt(radicand) if n >= 2 and radicand > 0 else None


def zscore_of(n, s1, s2, d):
    """The z-score of a hit with L1 ``d`` in a background of ``n`` L1s with sum ``s1`` and sum of squares ``s2`` (Python integers, or
    what ``int`` takes): z = (s1 - n d) / sqrt(n s2 - s1^2) = (mean - d) / sigma with the population sigma -- numerator and radicand
    exact integers, one ``math.sqrt``, one true division.  Positive = closer than the background.  The background of a query under a
    score is every protein of the database with which it has an L1 (neither is without fingerprints), the query itself included
    where the database holds it, each L1 raw (not capped at 17000).  None where z is undefined: ``d`` None (the pair has no L1),
    n < 2, or a radicand of 0."""
    if d is None:
        return None
    n, s1, s2, d = int(n), int(s1), int(s2), int(d)
    spread = _z_spread(n, s1, s2)
    return None if spread is None else (s1 - n * d) / spread


def zscores_of(mom, owner, d, has_l1=None) -> np.ndarray:
    """``zscore_of`` for many hits at once, to the same bits: float64, NaN where it has None.  ``mom`` = the (3, n) int64 array of
    ``MomentState.moments`` (the library's uint64 words), hit k lies in the background of protein ``owner[k]`` with L1 ``d[k]``, and
    ``has_l1[k]`` (default: all) says whether the pair has one.  The spread is taken per protein from Python integers
    (``_z_spread``); the numerator s1 - n d is exact in int64 (n < 2^31, d < 2^31, s1 < 2^55), its conversion to float64 rounds as
    Python's does, and the division is the same IEEE division."""
    owner, d = np.asarray(owner, dtype=np.int64), np.asarray(d, dtype=np.int64)
    used = np.unique(owner)
    words = np.ascontiguousarray(mom[:, used]).view(np.uint64).tolist()
    spread = np.full(mom.shape[1], np.nan)
    spread[used] = [v if v is not None else np.nan for v in (_z_spread(*w) for w in zip(*words))]
    with np.errstate(invalid='ignore'):
        z = (mom[1][owner] - mom[0][owner] * d) / spread[owner]
    if has_l1 is not None:
        z[~np.asarray(has_l1, dtype=bool)] = np.nan
    return z


def zscore_text(z) -> str:
    """The field of a z-score: two decimals, ``-`` where it is undefined (None or NaN)."""
    return '-' if z is None or z != z else f'{z:.2f}'


def _z_passes(min_z: float, *zs) -> bool:
    """``--min-z``: every z is defined (neither None nor NaN) and not below ``min_z``."""
    return all(z is not None and z >= min_z for z in zs)


def _moment_ints(mom):
    """[(n, s1, s2)] per protein as Python integers from a (3, n) int64 array of ``MomentState.moments`` (the library's uint64)."""
    return list(zip(*np.ascontiguousarray(mom).view(np.uint64).tolist()))


def _sim(l1):
    """1 - min(L1 / 17000, 1) for arrays of L1 values (ranking only; printing goes through ``_sim1``)."""
    return 1 - np.minimum(np.asarray(l1, dtype=np.int64) / L1_FULL_SCALE, 1)


def _sim1(l1):
    """The same for one value, with the reference's scalar arithmetic (src/dct-sim.py:24-26): Python's
    ``min`` hands back the int 1 once L1 exceeds 17000, so such a score prints as ``0``, not ``0.0``."""
    return 1 - min(np.int64(l1) / L1_FULL_SCALE, 1)


def _scores(mn, last):
    """(DCTdomain, DCTglobal) of one block.  The reference's running maximum starts at the int 0 and
    is replaced only by a strictly larger similarity (:42-50)."""
    best = _sim1(mn)
    return (best if best > 0 else 0), _sim1(last)


def prostSimilarity(emb1, emb2) -> float:
    """Similarity of two single fingerprints (src/dct-sim.py:12-26)."""
    d = l1_matrix(np.asarray(emb1)[None, :], np.asarray(emb2)[None, :]).cpu().numpy()[0, 0]
    return _sim1(d)


def domain_sim(dct_i: np.ndarray, dct_j: np.ndarray) -> tuple:
    """(DCTdomain, DCTglobal) of two proteins' fingerprint sets (src/dct-sim.py:28-50)."""
    mn, last = block_min(l1_matrix(dct_i, dct_j), [0, dct_i.shape[0]], [0, dct_j.shape[0]])
    return _scores(mn[0, 0], last[0, 0])


def best_domain_pair(dct_i: np.ndarray, dct_j: np.ndarray) -> tuple:
    """(DCTdomain, DCTglobal, pi, pj): ``domain_sim`` and the rows of ``dct_i`` / ``dct_j`` its loop ends on (src/dct-sim.py:42-50:
    the first pair, in (pi, pj) order, of the largest similarity); ``pi = pj = None`` when no pair scores above 0."""
    mn, last, arg_a, arg_b = pair_argmin(dct_i, [0, dct_i.shape[0]], dct_j, [0, dct_j.shape[0]], [(0, 0)])
    none = arg_a[0] < 0
    return _scores(mn[0], last[0]) + ((None, None) if none else (int(arg_a[0]), int(arg_b[0])))


def read_dom_file(path: str) -> dict:
    """{pid: [domain strings]} of a ``.dom`` file (``database.save_doms``: ``pid ndom d1;d2;...`` per line).  The last two
    whitespace-separated fields are the count and the list, whatever stands before them is the pid; a repeated pid: the later
    line.  ValueError for a line without those fields or whose count is not the length of its list."""
    doms = {}
    with open(path, encoding='utf8') as fh:
        for number, text in enumerate(fh, 1):
            if not text.strip():
                continue
            fields = text.rstrip('\r\n').rsplit(None, 2)
            if len(fields) != 3 or not fields[1].isdigit():
                raise ValueError(f'{path}:{number}: expected "pid ndom d1;d2;...", got {text.rstrip()!r}')
            names = fields[2].split(';')
            if len(names) != int(fields[1]):
                raise ValueError(f'{path}:{number}: {fields[0]} declares {fields[1]} domains and lists {len(names)}')
            doms[fields[0].lstrip()] = names
    return doms


def fingerprint_labels(sid, idx, doms: dict = None) -> list:
    """What ``--domains`` prints for every fingerprint row of an npz, in row order.  ``doms`` None: the 1-based index of the row
    within its protein.  Else (``read_dom_file`` of the npz's ``.dom``): the domain strings verbatim -- a protein of k > 0
    fingerprints must have k names, or k - 1 with the last row, the whole protein, printing ``whole``; ValueError naming the protein
    otherwise, also when it is absent from the file.  Proteins without fingerprints need no entry."""
    counts = np.diff(np.asarray(idx, dtype=np.int64))
    if doms is None:
        return [str(r + 1) for k in counts.tolist() for r in range(k)]
    labels = []
    for name, k in zip(sid, counts.tolist()):
        if k == 0:
            continue
        names = doms.get(f'{name}')
        if names is None:
            raise ValueError(f'protein {name} has {k} fingerprints and no line in the .dom file')
        if len(names) == k:
            labels += names
        elif len(names) == k - 1:
            labels += names + [WHOLE]
        else:
            raise ValueError(f'protein {name} has {k} fingerprints, the .dom file names {len(names)} domains (expected {k} or {k - 1})')
    return labels


def _labels_of(sid, idx, dom_path: str = None) -> list:
    return fingerprint_labels(sid, idx, read_dom_file(dom_path) if dom_path else None)


def _label(labels, first_row: int, arg: int) -> str:
    return NO_DOMAIN if arg < 0 else labels[first_row + arg]


def map_bound(x=None, min_domain=None) -> int:
    """B of ``--domain-map``: a fingerprint row is matched when its smallest L1 to the rows of the other protein is at most B =
    min(``sim_bound(X)``, 16999) -- a similarity of 0 never matches, ``NO_DOMAIN``'s rule.  X = ``x`` where a value is given (not
    None, not the bare flag's True), else ``min_domain`` where that is given, else MAP_SIMILARITY.  With X = ``--min-domain`` the
    matched rows are the rows ``--min-coverage`` counts."""
    given = x is not None and x is not True
    return min(sim_bound(x if given else min_domain if min_domain is not None else MAP_SIMILARITY), L1_FULL_SCALE - 1)


def map_entries(l1, arg, bound: int) -> list:
    """One side of a domain map: [(row, counterpart, L1)] of the rows whose ``l1`` is at most ``bound``, in row order, from one
    protein's slice of ``pair_row_best``'s (l1, arg)."""
    return [(r, int(c), int(v)) for r, (v, c) in enumerate(zip(l1, arg)) if 0 <= v <= bound]


def domain_map(dct_i: np.ndarray, dct_j: np.ndarray, x: float = MAP_SIMILARITY) -> tuple:
    """(rows of ``dct_i`` matched by ``dct_j``, rows of ``dct_j`` matched by ``dct_i``), each a list of (row, counterpart, L1): every
    row's nearest row of the other set (ties to the lowest) where that L1 is at most ``map_bound(x)``.  ``best_domain_pair``'s pair
    is the first entry of the smallest L1 of the first list."""
    k = dct_i.shape[0]
    _, l1, arg = pair_row_best(dct_i, [0, k], dct_j, [0, dct_j.shape[0]], [(0, 0)])
    bound = map_bound(x)
    return map_entries(l1[:k], arg[:k], bound), map_entries(l1[k:], arg[k:], bound)


def map_field(first, second, labels_i, labels_j, score=None) -> str:
    """The field ``--domain-map`` adds to a result line: ``side/side``, the first side the entries of ``first`` (rows of prot1
    against prot2), the second those of ``second`` (rows of prot2 against prot1); a side is ``-`` or its entries
    ``label=label of the counterpart:score`` joined by ``;``.  ``labels_i`` / ``labels_j``: the labels of the rows of the two
    proteins; ``score``: the text of an L1 -- by default the mode's own DCTdomain text outside the all-against-all,
    ``str(_sim1(L1))``; the all-against-all prints ``score_table()``'s five characters."""
    score = score or (lambda l1: str(_sim1(l1)))

    def side(entries, own, other):
        return ';'.join(f'{own[r]}={other[c]}:{score(v)}' for r, c, v in entries) or NO_DOMAIN
    return f'{side(first, labels_i, labels_j)}/{side(second, labels_j, labels_i)}'


def _map_fields(off, l1, arg, bound: int, pairs, labels, first_row, db_labels, db_first_row) -> list:
    """``map_field`` of every pair (i, j) of ``pairs`` from ``pair_row_best``'s arrays: protein i's rows are ``labels`` from
    ``first_row[i]``, protein j's ``db_labels`` from ``db_first_row[j]``."""
    out = []
    for p, (i, j) in enumerate(pairs):
        a0, a1, b0, b1 = int(first_row[i]), int(first_row[i + 1]), int(db_first_row[j]), int(db_first_row[j + 1])
        mid = int(off[p]) + a1 - a0
        out.append(map_field(map_entries(l1[off[p]:mid], arg[off[p]:mid], bound), map_entries(l1[mid:off[p + 1]], arg[mid:off[p + 1]], bound),
                             labels[a0:a1], db_labels[b0:b1]))
    return out


COV_UNITS = ('residues', 'domains')
MAX_COVERAGE_WEIGHT = 1 << 30      # a protein's weight stays below it: twice that still fits the int32 the kernel reads


def _residues(name: str) -> int:
    """The residues a domain string names (``"1-30,61-100"`` -> 70); 0 for anything that is not a list of ranges a-b, 1 <= a <= b."""
    total = 0
    for part in f'{name}'.split(','):
        ends = part.split('-')
        if len(ends) != 2 or not (ends[0].isdigit() and ends[1].isdigit()) or not 1 <= int(ends[0]) <= int(ends[1]):
            return 0
        total += int(ends[1]) - int(ends[0]) + 1
    return total


def coverage_weights(sid, idx, dom_names, unit: str = 'residues') -> np.ndarray:
    """What ``--min-coverage`` weighs: one int64 per fingerprint row of the file.  A protein of one row: that row carries the
    protein's weight W.  A protein of k > 1 rows: its domain rows 0 .. k - 2 carry their own weights, W is their sum, and the last
    row -- the whole-protein fingerprint -- carries W, so W is always the weight of a protein's last row.  ``unit='residues'``: a
    row weighs the residues its name covers (``dom_names``: one string per row, the ``dom`` array of the npz or
    ``fingerprint_labels`` of its ``.dom`` file; the name of a whole-protein row is not read); ValueError naming the protein
    where there are no names or one does not parse.  ``unit='domains'``: every domain row weighs 1 (W = max(1, k - 1)); no names
    needed.  ValueError for a W of 2^30 or more."""
    if unit not in COV_UNITS:
        raise ValueError(f'unit must be one of {COV_UNITS}')
    idx = np.asarray(idx, dtype=np.int64)
    counts = np.diff(idx)
    total = int(idx[-1]) if len(idx) else 0
    last = np.zeros(total, dtype=bool)
    last[idx[1:][counts > 0] - 1] = True
    whole = last & np.repeat(counts > 1, counts)                # the whole-protein rows: they get W
    if unit == 'domains':
        w = np.ones(total, dtype=np.int64)
    else:
        hint = 'use --cov-unit domains to count domains instead of residues'
        if dom_names is None or len(dom_names) != total:
            named = np.flatnonzero(counts > 0)
            who = f'protein {sid[named[0]]}' if len(named) else 'the file'
            raise ValueError(f'{who} has no domain names to count residues from (no dom array in the npz, no .dom file): {hint}')
        w = np.fromiter((0 if skip else _residues(name) for name, skip in zip(dom_names, whole)), dtype=np.int64, count=total)
        bad = np.flatnonzero((w <= 0) & ~whole)
        if len(bad):
            owner = int(np.searchsorted(idx, bad[0], 'right')) - 1
            raise ValueError(f'protein {sid[owner]}: {dom_names[bad[0]]!r} names no residue ranges: {hint}')
    w[whole] = 0
    sums = np.concatenate([[0], np.cumsum(w)])
    W = sums[idx[1:]] - sums[idx[:-1]]
    w[whole] = W[counts > 1]
    if len(W) and W.max() >= MAX_COVERAGE_WEIGHT:
        raise ValueError(f'protein {sid[int(np.argmax(W))]} weighs {int(W.max())}: the coverage takes weights below 2^30')
    return w


def coverage_need(W, c: float):
    """The weight of a protein of weight ``W`` that its matched rows must reach at coverage ``c``:
    min(W, max(1, ceil(c W - 1e-9))) -- an integer, so that 0.7 of 10 is 7 and not 8; 0 for W = 0.  Arrays or single values."""
    need = np.minimum(W, np.maximum(1, np.ceil(c * np.asarray(W, dtype=np.float64) - 1e-9))).astype(np.int64)
    return need if need.ndim else int(need)


def load_dct(filename: str, asmap=True) -> tuple:
    """npz -> ({sid: fingerprints} | [fingerprints], sid) (src/dct-sim.py:52-84)."""
    seqid, bounds, rows = _load_npz(filename)
    per_protein = [rows[a:b, :] for a, b in zip(bounds[:-1], bounds[1:])]
    return (dict(zip(seqid, per_protein)) if asmap else per_protein), seqid


def _protein_groups(idx, max_rows: int):
    """[p0, p1) ranges of consecutive proteins whose fingerprints (idx = prefix offsets) number at most ``max_rows``
    -- at least one protein per range, however many fingerprints it has."""
    idx = np.asarray(idx, dtype=np.int64)
    p0, n = 0, len(idx) - 1
    while p0 < n:       # (one search per range, not a step per protein: all_sim groups the later proteins once per stripe)
        p1 = min(n, max(p0 + 1, int(np.searchsorted(idx, idx[p0] + max_rows, 'right')) - 1))
        yield p0, p1
        p0 = p1


class Blocks:
    """All protein-vs-protein (minimum, last-last) L1 blocks between two ``-dct.npz`` files."""

    def __init__(self, file_a: str, file_b: str = None):
        self.rows, ia, da = _load_npz(file_a)               # (with the reference's progress line, one per file)
        self.cols, ib, dbm = (self.rows, ia, da) if file_b is None else _load_npz(file_b)
        # protein stripes of `a`: the int32 distance matrix of a stripe stays within ~1 GiB (the protein x protein result
        # is what is kept; the reference loops pair by pair, src/dct-sim.py:126-176)
        # ... and protein groups of `b` of at most COL_ROWS fingerprints, so that neither the uploaded part of `b` nor
        # the distance matrix grows with the size of the files
        na, nb = len(ia) - 1, len(ib) - 1
        self.mn = np.full((na, nb), 0x7fffffff, dtype=np.int32)      # (an empty block keeps this: block_min_kernel's fill)
        self.last = np.full((na, nb), 0x7fffffff, dtype=np.int32)
        for q0, q1 in _protein_groups(ib, self.COL_ROWS):
            db_dev = to_device_int8(dbm[ib[q0]:ib[q1]])
            budget = max(1, self.TILE_INTS // max(1, db_dev.shape[0]))
            for p0, p1 in _protein_groups(ia, budget):
                if ia[p1] > ia[p0] and db_dev.shape[0] > 0:           # (a stripe of proteins without fingerprints: nothing to launch)
                    mn_t, last_t = block_min(l1_matrix(da[ia[p0]:ia[p1]], db_dev), ia[p0:p1 + 1] - ia[p0], ib[q0:q1 + 1] - ib[q0])
                    self.mn[p0:p1, q0:q1] = mn_t
                    self.last[p0:p1, q0:q1] = last_t
            del db_dev

    COL_ROWS = 1 << 22      # fingerprints of `b` on the device at a time (2 GB of int8 at 480 columns)
    TILE_INTS = 1 << 28     # int32 entries of one distance matrix (1 GiB)

    def scores(self, i: int, j: int) -> tuple:
        return _scores(self.mn[i, j], self.last[i, j])


SCORE_ROWS = L1_FULL_SCALE + 2    # score table rows: L1 0 .. 17000, then one row for every larger value (0x7fffffff included)


def score_table() -> np.ndarray:
    """uint8 (2, SCORE_ROWS, 5): the text all_sim prints for each L1 value -- ``f'{v:.3f}'`` of ``_scores``' DCTdomain (by the
    block minimum) and DCTglobal (by the last-last value), evaluated for every L1 rather than derived: Python's correctly
    rounded ``.3f`` of the float64 is the definition.  Every one is five characters."""
    pairs = [_scores(v, v) for v in range(SCORE_ROWS)]
    text = ''.join(f'{a:.3f}' for a, _ in pairs) + ''.join(f'{b:.3f}' for _, b in pairs)
    if len(text) != 2 * SCORE_ROWS * 5:
        raise AssertionError('a score does not print as five characters')
    return np.frombuffer(bytearray(text.encode('ascii')), dtype=np.uint8).reshape(2, SCORE_ROWS, 5)


def row_text_bytes(id_lens) -> np.ndarray:
    """Bytes all_sim prints for row i (lines j = i + 1 .. n - 1, each len_i + len_j + 14), rows 0 .. n - 2."""
    lens = np.asarray(id_lens, dtype=np.int64)
    n = len(lens)
    if n < 2:
        return np.zeros(0, dtype=np.int64)
    after = np.cumsum(lens[::-1])[::-1]                      # after[k] = sum of lens[k:]
    i = np.arange(n - 1, dtype=np.int64)
    return (n - 1 - i) * (lens[:-1] + 14) + after[1:]


def plan_stripes(id_lens, idx, text_bytes: int, fp_rows: int):
    """Stripes [i0, i1) of rows 0 .. n - 2 in order, each as (i0, i1, row bases (int64, relative to the stripe's first byte),
    stripe bytes): as many rows as keep the text within ``text_bytes`` and the rows' fingerprints within ``fp_rows`` -- at
    least one row, however large."""
    size = row_text_bytes(id_lens)
    fps = np.diff(np.asarray(idx, dtype=np.int64))[:len(size)]
    cb = np.concatenate([[0], np.cumsum(size)])
    cf = np.concatenate([[0], np.cumsum(fps)])
    out, i0, m = [], 0, len(size)
    while i0 < m:
        i1 = min(int(np.searchsorted(cb, cb[i0] + text_bytes, 'right')), int(np.searchsorted(cf, cf[i0] + fp_rows, 'right'))) - 1
        i1 = min(m, max(i0 + 1, i1))
        out.append((i0, i1, cb[i0:i1] - cb[i0], int(cb[i1] - cb[i0])))
        i0 = i1
    return out


class _DeviceRows:
    """The fingerprints of proteins [p0, p1) of a file on the device: a slice of the whole file, which stays there (``resident``)
    when it has at most ``col_rows`` fingerprints, else uploaded per request."""

    def __init__(self, fps, idx, col_rows: int):
        self.fps, self.idx = fps, idx
        total = int(idx[-1]) if len(idx) else 0
        self.resident = to_device_int8(fps[:total]) if 0 < total <= col_rows else None
        self._idx_dev = None

    @property
    def idx_dev(self):
        """The prefix array beside ``resident`` (made when first asked for)."""
        if self._idx_dev is None:
            import torch
            self._idx_dev = torch.as_tensor(self.idx, device=self.resident.device)
        return self._idx_dev

    def __call__(self, p0: int, p1: int):
        if self.resident is not None:
            return self.resident[self.idx[p0]:self.idx[p1]]
        return to_device_int8(self.fps[self.idx[p0]:self.idx[p1]])


class AllPairs:
    """all_sim's text (src/dct-sim.py:158-176) for one file, upper triangle only, streamed: rows in stripes (``plan_stripes``)
    whose text fits in TEXT_BYTES and whose fingerprints times a column group fit in TILE_INTS; per stripe and group of at most
    COL_ROWS later fingerprints, ``l1_matrix`` -> ``block_min_device`` -> ``sim_lines`` into one device text buffer, copied
    to one of two pinned buffers while the host writes out the other.  No per-line Python; host memory beyond the data is the
    two buffers plus O(n)."""

    TEXT_BYTES = 1 << 28    # text of one stripe (a single row may exceed it: the buffers grow)
    COL_ROWS = 1 << 22      # fingerprints of the column side on the device at a time (the whole file stays there if it fits)
    TILE_INTS = 1 << 28     # int32 entries of one distance matrix (1 GiB)

    def __init__(self, sid, idx, fps):
        self.sid, self.idx, self.fps = sid, np.asarray(idx, dtype=np.int64), fps

    def stripes(self, id_lens):
        total = int(self.idx[-1]) if len(self.idx) else 0
        fp_rows = max(1, self.TILE_INTS // max(1, min(self.COL_ROWS, total)))
        return plan_stripes(id_lens, self.idx, self.TEXT_BYTES, fp_rows)

    def write(self, sink):
        """Calls ``sink(memoryview)`` with the text of each stripe, in order."""
        import torch
        n = len(self.idx) - 1
        if n < 2:
            return
        ids = LineIds([f'{s}' for s in self.sid])
        dev = ids.bytes_dev.device
        table = torch.as_tensor(score_table(), device=dev)
        rows = _DeviceRows(self.fps, self.idx, self.COL_ROWS)
        out = TextStream(sink, room=lambda nbytes: max(nbytes, min(self.TEXT_BYTES, 2 * nbytes)))
        text = None
        for i0, i1, base, nbytes in self.stripes(ids.lens):
            if text is None or text.numel() < nbytes:
                text = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            a = rows(i0, i1) if self.idx[i1] > self.idx[i0] else None
            ia = self.idx[i0:i1 + 1] - self.idx[i0]
            col0 = i0 + 1
            for q0, q1 in _protein_groups(self.idx[col0:] - self.idx[col0], self.COL_ROWS):
                q0, q1 = q0 + col0, q1 + col0
                b = rows(q0, q1) if a is not None and self.idx[q1] > self.idx[q0] else None
                dist = l1_matrix(a, b) if b is not None else torch.empty((0, 0), dtype=torch.int32, device=dev)
                mn, last = block_min_device(dist, ia, self.idx[q0:q1 + 1] - self.idx[q0])
                sim_lines(mn, last, i0, q0, ids, table, base, text)
                del dist, mn, last, b
            out.hand_over(text, nbytes)                         # (the previous stripe goes out while the device fills this one)
        out.close()


def _load_npz(filename: str) -> tuple:
    """(sid, idx, dct) of a ``-dct.npz``, with load_dct's progress line (src/dct-sim.py:52-84) -- without the per-protein
    list, which at a million proteins costs as much as the load."""
    t0 = time.time()
    with np.load(filename) as data:
        seqid, bounds, rows = data['sid'], np.asarray(data['idx'], dtype=np.int64), data['dct']
    print(f"dct loaded for {len(seqid)} sequences, time used: {time.time() - t0:.1f}s")
    return seqid, bounds, rows


def sim_bound(threshold: float) -> int:
    """The largest L1 in 0 .. 17000 whose similarity, with ``_sim``'s arithmetic, is not below ``threshold`` -- the
    reference keeps a hit past the first ``top`` unless ``sim < threshold`` (src/dct-sim.py:151) -- found by evaluating
    that expression on every L1, not by algebra.  -1 = none (threshold > 1); 17000 = every L1 (threshold <= 0, NaN).
    Similarity does not increase with L1, so the L1 values that pass are exactly 0 .. sim_bound."""
    ok = ~(_sim(np.arange(L1_FULL_SCALE + 1)) < threshold)
    return int(np.count_nonzero(ok)) - 1


def _last_rows(fps, idx):
    """(last fingerprint of every protein, a zero row where it has none; uint8 flag of the proteins without one)."""
    idx = np.asarray(idx, dtype=np.int64)
    empty = idx[1:] == idx[:-1]
    last = np.zeros((len(idx) - 1, fps.shape[1]), dtype=np.int8)
    last[~empty] = fps[idx[1:][~empty] - 1]
    return last, empty.astype(np.uint8)


def merge_candidates(parts, top: int, bound: int):
    """One query's hits from the hits of each database group: ``parts`` = [(keys, global columns)] of the groups, each the
    group's first max(top, #(key <= bound)) entries in (key, column) order.  Exact: the global entries with key <= bound are
    the union of the groups' ones, and the global first ``top`` lie within the union of the groups' first ``top``.
    Returns (keys, columns) of the first max(top, #(key <= bound)) entries of the union in (key, column) order."""
    if len(parts) == 1:
        return parts[0]
    keys = np.concatenate([k for k, _ in parts])
    cols = np.concatenate([c for _, c in parts])
    order = np.lexsort((cols, keys))
    m = min(len(order), max(top, int(np.count_nonzero(keys <= bound))))
    return keys[order[:m]], cols[order[:m]]


def _pair_chunks(idx, pairs, max_rows: int):
    """[start, end) ranges of ``pairs`` whose proteins (deduplicated) have at most ``max_rows`` fingerprints between them --
    at least one pair per range."""
    sizes = np.diff(np.asarray(idx, dtype=np.int64))
    start, seen, rows = 0, set(), 0
    for k, (i, j) in enumerate(pairs):
        new = [p for p in {int(i), int(j)} if p not in seen]
        more = int(sum(sizes[p] for p in new))
        if k > start and rows + more > max_rows:
            yield start, k
            start, seen, rows = k, set(), 0
            new = list({int(i), int(j)})
            more = int(sum(sizes[p] for p in new))
        seen.update(new)
        rows += more
    if start < len(pairs):
        yield start, len(pairs)


def _compact(fps, idx, proteins):
    """(fingerprint rows of ``proteins``, their prefix array): the part of an npz a pair list needs on the device."""
    idx = np.asarray(idx, dtype=np.int64)
    lens = idx[proteins + 1] - idx[proteins]
    sub_idx = np.zeros(len(proteins) + 1, dtype=np.int64)
    np.cumsum(lens, out=sub_idx[1:])
    rows = np.repeat(idx[proteins] - sub_idx[:-1], lens) + np.arange(sub_idx[-1])
    return fps[rows], sub_idx


def _score_arrays(n: int, domains: bool):
    """(the int64 arrays (min, last) -- ``domains``: (min, last, arg_a, arg_b) -- of ``n`` pairs, holding what a pair without
    fingerprints scores; ``pair_min`` -- ``pair_argmin`` -- which fills them)."""
    fills = (0x7fffffff, 0x7fffffff) + ((-1, -1) if domains else ())
    return [np.full(n, f, dtype=np.int64) for f in fills], (pair_argmin if domains else pair_min)


def pair_scores(fps, idx, pairs, max_rows: int = None, domains: bool = False):
    """(min, last) L1 of every (protein i, protein j) of ``pairs`` within one npz (``dctfp_pair_min``): only the fingerprints of
    the proteins the pairs name go to the device, at most ``max_rows`` (``ProteinSearch.COL_ROWS``) of them at a time.
    ``domains``: (min, last, arg_i, arg_j) -- with the rows of the minimum within the two proteins, -1 = none
    (``dctfp_pair_argmin``)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out, score = _score_arrays(len(pairs), domains)
    for k0, k1 in _pair_chunks(idx, pairs, max_rows or ProteinSearch.COL_ROWS):
        proteins, local = np.unique(pairs[k0:k1], return_inverse=True)
        rows, sub_idx = _compact(fps, idx, proteins)
        if len(rows):
            dev = to_device_int8(rows)
            for o, v in zip(out, score(dev, sub_idx, dev, sub_idx, local.reshape(-1, 2))):
                o[k0:k1] = v
    return tuple(out)


def _scatter_rows(out, off, sel, part_off, parts):
    """The ragged results ``parts`` of the pairs ``sel`` (rows of pair sel[k] at [part_off[k], part_off[k + 1])) to their places in
    the arrays ``out``, where pair p lies at [off[p], off[p + 1])."""
    to = np.repeat(off[sel] - part_off[:-1], np.diff(part_off)) + np.arange(part_off[-1])
    for o, v in zip(out, parts):
        o[to] = v


def pair_row_bests(fps, idx, pairs, max_rows: int = None):
    """(row_off, l1, arg) of ``pair_row_best`` for the pairs (protein i, protein j) of one npz, in ``pair_scores``' chunks: only the
    fingerprints of the proteins the pairs name go to the device, at most ``max_rows`` of them at a time."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    off = pair_row_offsets(idx, idx, pairs)
    out = np.full(off[-1], 0x7fffffff, dtype=np.int64), np.full(off[-1], -1, dtype=np.int64)
    for k0, k1 in _pair_chunks(idx, pairs, max_rows or ProteinSearch.COL_ROWS):
        proteins, local = np.unique(pairs[k0:k1], return_inverse=True)
        rows, sub_idx = _compact(fps, idx, proteins)
        if len(rows):
            dev = to_device_int8(rows)
            part_off, *parts = pair_row_best(dev, sub_idx, dev, sub_idx, local.reshape(-1, 2))
            _scatter_rows(out, off, np.arange(k0, k1), part_off, parts)
    return (off,) + out


class FilteredPairs:
    """all_sim's pairs whose scores are not below cut-offs -- DCTdomain >= ``min_domain`` and DCTglobal >= ``min_global``, either
    may be None -- without forming the others: ``AllPairs``' output with lines removed.  A cut-off is the integer bound
    ``sim_bound`` gives: a pair passes when min(L1, 17000) <= bound.  Per stripe of rows [i0, i1):

    1. one int32 tile, stripe x every later protein (at most TILE_INTS entries): DCTglobal's L1 (``l1_matrix`` of the last rows)
       when ``min_global`` excludes anything -- DCTglobal's fingerprint pair is one of DCTdomain's, so DCTdomain is never below
       it and nothing that fails here could be printed -- else DCTdomain's (``protein_min``); the later proteins' fingerprints
       go through the device in groups of at most COL_ROWS, each group filling its columns of the tile;
    2. the entries right of the diagonal within the bound, counted per row and compacted in (i, j) order on the device
       (``tri_filter_count`` / ``tri_filter_fill``).  Only the row counts come to the host; rows are then taken in ranges
       whose text cannot exceed TEXT_BYTES (a row's count times its longest possible line; a single row may exceed it);
    3. (min, last) of the survivors (``pair_min_device``; ``pair_scores``' chunks when the file does not stay on the device), and
       the other cut-off, if any, on those;
    4. the lines of what is left (``pair_lines``), out through two pinned buffers.

    Nothing of size n x n exists anywhere; host memory beyond the data is O(n), one range's survivors and the two buffers.

    ``labels`` (``--domains``: ``fingerprint_labels`` of the file) adds the domain pair to every line: step 3 takes
    ``pair_argmin_device`` and keeps the two rows of the minimum, step 4 gives ``pair_lines`` the labels on the device (one
    per fingerprint row and ``-``).  Without cut-offs both bounds keep every pair and the output is ``AllPairs``' with the two
    fields added -- by the slower route: a protein-minimum tile, a filter that drops nothing and a second read of every pair's
    fingerprints for the scores, where ``AllPairs`` reduces one distance matrix.

    ``min_coverage`` (``--min-coverage``; needs ``min_domain`` and ``weights``, ``coverage_weights`` of the file) also asks that
    the pair covers enough of BOTH proteins.  Row r of protein p is matched by protein q when min(L1(r, s), 17000) <= the DCTdomain
    bound for some row s of q; cov(p by q) = the weights of the matched rows of p; the pair stays when cov(p by q) >=
    ``coverage_need(W_p, min_coverage)`` and likewise for q.  The tile is then always DCTdomain's and comes from ``protein_cover``,
    which writes 0x7fffffff for the pairs that fail: the filter, the union-find and the greedy rounds read it as they read
    ``protein_min``'s, and ``min_global`` is applied to the survivors' last-row L1.  At a bound of 17000 every row is matched and
    below 0 none is: the coverage then changes nothing and is not computed.

    ``with_map(bound)`` (``--domain-map``; needs ``labels``) adds the domain map to every line: after step 3, for the pairs that are
    printed and no others, ``pair_row_best_device`` gives every row's nearest row of the other protein, and step 4 becomes two
    passes of ``pair_map_lines`` -- the byte length of every line, a cumulative sum on the device, then the text.  The ranges of
    rows are then sized by an upper bound of a line with its map: every row of both proteins matched, each entry with the longest
    label of the file as its counterpart."""

    TEXT_BYTES = 1 << 28    # text of one range of rows
    COL_ROWS = 1 << 22      # fingerprints on the device at a time (the whole file stays there if it fits)
    TILE_INTS = 1 << 28     # int32 entries of one stripe's tile (1 GiB)

    def __init__(self, sid, idx, fps, min_domain=None, min_global=None, labels=None, min_coverage=None, weights=None):
        self.sid, self.idx, self.fps = sid, np.asarray(idx, dtype=np.int64), fps
        self.row_labels = labels                                # (not `labels`: Clusters.labels() is a method)
        if labels is not None and len(labels) != int(self.idx[-1]):
            raise ValueError('labels must have one entry per fingerprint row')
        self.bound_domain = L1_FULL_SCALE if min_domain is None else sim_bound(min_domain)
        self.bound_global = L1_FULL_SCALE if min_global is None else sim_bound(min_global)
        self.route = 'global' if self.bound_global < L1_FULL_SCALE else 'domain'
        self.cover = None                                       # (row weights, protein needs) where a coverage can exclude a pair
        self.map_l1 = None                                      # the bound of the domain map where the lines carry one
        if min_coverage is not None:
            if min_domain is None:
                raise ValueError('min_coverage needs min_domain: it counts the fingerprints within that cut-off')
            self.with_coverage(min_coverage, weights)

    def with_coverage(self, min_coverage: float, weights):
        """Adds the coverage cut-off of the class text to a job that has a DCTdomain cut-off: ``weights`` = ``coverage_weights`` of
        the file.  Returns the job (``Clusters(...).with_coverage(...)``: the cluster classes' constructors take the two cut-offs)."""
        if weights is None or not 0 < min_coverage <= 1:
            raise ValueError('a coverage is above 0 and at most 1 and needs the weights of the fingerprint rows')
        w = np.asarray(weights, dtype=np.int64)
        if len(w) != int(self.idx[-1]):
            raise ValueError('weights must have one entry per fingerprint row')
        if 0 <= self.bound_domain < L1_FULL_SCALE:              # (else every row is matched, or none: nothing to compute)
            W = np.zeros(len(self.idx) - 1, dtype=np.int64)
            has = np.diff(self.idx) > 0
            W[has] = w[self.idx[1:][has] - 1]                   # (a protein's weight is its last row's)
            self.cover = (w.astype(np.int32), coverage_need(W, min_coverage).astype(np.int32))
            self.route = 'domain'
        return self

    def with_map(self, bound: int):
        """Adds the domain map of the class text to a job that has ``labels``: ``bound`` = ``map_bound`` of the run.  Returns the job."""
        if self.row_labels is None:
            raise ValueError('a domain map names fingerprint rows: it needs labels')
        if not -1 <= int(bound) < L1_FULL_SCALE:
            raise ValueError('the bound of a domain map is an L1 of similarity above 0: at most 16999')
        self.map_l1 = int(bound)
        return self

    def _map_room(self) -> np.ndarray:
        """Per protein, an upper bound of what its rows add to the map of a line: every row matched, each entry its own label, the
        longest label of the file, ``=``, ``:``, five characters of score and a separator."""
        lens = np.fromiter((len(f'{s}'.encode('utf8')) for s in self.row_labels), dtype=np.int64, count=len(self.row_labels))
        own = np.concatenate([[0], np.cumsum(lens)])[self.idx]
        return np.diff(own) + np.diff(self.idx) * (int(lens.max(initial=0)) + 8) + 1

    def stripes(self):
        """[i0, i1) over rows 0 .. n - 2: as many rows as keep rows x later proteins within TILE_INTS and the rows' fingerprints
        within COL_ROWS (within an ``AllPairs`` distance tile where ``protein_min`` falls back to one) -- at least one row."""
        n = len(self.idx) - 1
        total = int(self.idx[-1])
        fp_rows = self.COL_ROWS
        if self.route == 'domain' and self.fps.shape[1] > PROTEIN_MIN_MAX_D:
            fp_rows = max(1, self.TILE_INTS // max(1, min(self.COL_ROWS, total)))
        i0 = 0
        while i0 < n - 1:
            by_tile = i0 + max(1, self.TILE_INTS // (n - 1 - i0))
            by_rows = int(np.searchsorted(self.idx, self.idx[i0] + fp_rows, 'right')) - 1
            i1 = min(n - 1, max(i0 + 1, min(by_tile, by_rows)))
            yield i0, i1
            i0 = i1

    @property
    def bound(self) -> int:
        """The bound of the route's tile: DCTglobal's when it excludes anything, else DCTdomain's."""
        return self.bound_global if self.route == 'global' else self.bound_domain

    def device_rows(self) -> _DeviceRows:
        return _DeviceRows(self.fps, self.idx, self.COL_ROWS)

    def resident_rows(self):
        """The file's fingerprints on the device when they fit there (at most COL_ROWS), else None."""
        return self.device_rows().resident

    def tiles(self, rows: _DeviceRows = None, cover: bool = True):
        """Yields, per stripe, (i0, i1, tile, (row flags, column flags)): step 1 of the class text.  The tile is device int32,
        rows [i0, i1) x proteins i0 + 1 .. n - 1; the flags mark the proteins without fingerprints on the DCTglobal route (None on
        the other: ``protein_min`` leaves 0x7fffffff there, and so does ``protein_cover``, which takes its place under a coverage).  ``rows``: ``device_rows()`` of a caller that needs the
        fingerprints itself; taken here otherwise.  ``cover=False``: ``protein_min``'s tile even under a coverage -- the plain distances, for a
        caller that has the pairs' fate already (``Clusters.medoids``)."""
        import torch
        covered = self.cover if cover else None
        n = len(self.idx) - 1
        dev = torch.device('cuda', torch.cuda.current_device())
        total = int(self.idx[-1])
        if rows is None:
            rows = self.device_rows()
        if self.route == 'global':
            last_rows, empty = _last_rows(self.fps[:total], self.idx)
            last_dev = to_device_int8(last_rows) if n <= self.COL_ROWS else None
            empty_dev = torch.as_tensor(empty, device=dev)
        if covered is not None:
            w_dev, need_dev = (torch.as_tensor(v, device=dev) for v in covered)

        def lasts(p0, p1):
            return last_dev[p0:p1] if last_dev is not None else to_device_int8(last_rows[p0:p1])

        for i0, i1 in self.stripes():
            col0 = i0 + 1
            tile = torch.empty((i1 - i0, n - col0), dtype=torch.int32, device=dev)
            if self.route == 'global':
                a = lasts(i0, i1)
                for q0 in range(col0, n, self.COL_ROWS):
                    q1 = min(n, q0 + self.COL_ROWS)
                    l1_matrix(a, lasts(q0, q1), out=tile[:, q0 - col0:q1 - col0])
                flags = (empty_dev[i0:i1], empty_dev[col0:])
            else:
                a, ia = rows(i0, i1), self.idx[i0:i1 + 1] - self.idx[i0]
                for q0, q1 in _protein_groups(self.idx[col0:] - self.idx[col0], self.COL_ROWS):
                    q0, q1 = q0 + col0, q1 + col0
                    b, ib, out = rows(q0, q1), self.idx[q0:q1 + 1] - self.idx[q0], tile[:, q0 - col0:q1 - col0]
                    if covered is None:
                        protein_min(a, ia, b, ib, out=out)
                    else:
                        protein_cover(a, ia, w_dev[self.idx[i0]:self.idx[i1]], need_dev[i0:i1], b, ib, w_dev[self.idx[q0]:self.idx[q1]],
                                      need_dev[q0:q1], self.bound_domain, out=out, cap=L1_FULL_SCALE)
                flags = (None, None)
            yield i0, i1, tile, flags
            del tile                                            # (before the next one is made; the caller drops its own too)

    def tile_pass(self, rows: _DeviceRows = None, cover: bool = True, hold: list = None):
        """Yields (i0, tile, flags) per stripe of ``tiles(rows, cover)``, each tile dropped before the next is made.  ``hold``: a list that
        gets the one tile when the triangle is one stripe -- a later pass then iterates ``held or self.tile_pass(...)``."""
        one = hold is not None and len(list(self.stripes())) == 1
        for i0, _, tile, flags in self.tiles(rows, cover):
            if one:
                hold.append((i0, tile, flags))
            yield i0, tile, flags
            del tile

    def _scores_of(self, pi, pj, domains: bool = False, rows: _DeviceRows = None):
        """Step 3 of the class text: device int32 (min L1, last L1) of the pairs (pi[k], pj[k]) (device int32) -- ``domains``: also
        (arg_i, arg_j).  ``pair_min_device`` / ``pair_argmin_device`` on the file where it stays on the device, else
        ``pair_scores``' chunks of at most COL_ROWS fingerprints, copied back.  ``rows``: as in ``tiles``."""
        import torch
        if rows is None:
            rows = self.device_rows()
        pairs = torch.stack([pi, pj], dim=1)
        if rows.resident is not None:
            score = pair_argmin_device if domains else pair_min_device
            return score(rows.resident, rows.idx_dev, rows.resident, rows.idx_dev, pairs.contiguous())
        return tuple(torch.as_tensor(v.astype(np.int32), device=pi.device)
                     for v in pair_scores(self.fps, self.idx, pairs.cpu().numpy(), self.COL_ROWS, domains=domains))

    def chunks(self, rows: _DeviceRows = None):
        """Yields device int32 tensors (i, j, min L1, last L1) of the surviving pairs, range of rows by range, in output order; with
        ``labels`` also (arg_i, arg_j), the rows of the minimum within the two proteins (-1: none).  ``rows``: as in ``tiles``."""
        n = len(self.idx) - 1
        if n < 2 or min(self.bound_domain, self.bound_global) < 0:
            return
        id_lens = np.fromiter((len(f'{s}'.encode('utf8')) for s in self.sid), dtype=np.int64, count=n)
        longest = int(id_lens.max())
        line = id_lens + 14 + longest                           # (a line of row i is at most this long)
        if self.map_l1 is not None:                             # (... and with its map: the two label fields, " ", "/", both sides)
            side = self._map_room()
            label = max((len(f'{s}'.encode('utf8')) for s in self.row_labels), default=0)
            line = line + 2 * max(label, len(NO_DOMAIN)) + 4 + side + int(side.max())
        bound = self.bound
        if rows is None:
            rows = self.device_rows()
        for i0, i1, tile, flags in self.tiles(rows):
            col0 = i0 + 1
            count_dev = tri_filter_count(tile, i0, col0, bound, *flags)
            count = count_dev.cpu().numpy().astype(np.int64)
            # ranges of rows by the text they can make: count x the longest line of the row
            room = np.concatenate([[0], np.cumsum(count * line[i0:i1])])
            r0 = 0
            while r0 < i1 - i0:
                r1 = min(i1 - i0, max(r0 + 1, int(np.searchsorted(room, room[r0] + self.TEXT_BYTES, 'right')) - 1))
                m = int(count[r0:r1].sum())
                if m:
                    pi, pj = tri_filter_fill(tile[r0:r1], i0 + r0, col0, bound, count_dev[r0:r1], m,
                                             flags[0][r0:r1] if flags[0] is not None else None, flags[1])
                    chunk = (pi, pj) + tuple(self._scores_of(pi, pj, self.row_labels is not None, rows))
                    # the other cut-off (the order stays): DCTdomain's on the min L1, or under a coverage DCTglobal's on the last-row L1
                    score, other = (2, self.bound_domain) if self.route == 'global' else (3, self.bound_global)
                    if other < L1_FULL_SCALE:
                        keep = chunk[score].clamp(max=L1_FULL_SCALE) <= other
                        chunk = tuple(t[keep].contiguous() for t in chunk)
                    if chunk[0].numel():
                        yield chunk
                r0 = r1
            del tile

    def pairs(self):
        """(i, j, min L1, last L1): int64 numpy arrays of the surviving pairs in output order (i ascending, then j); with ``labels``
        also (arg_i, arg_j)."""
        import torch
        parts = [torch.stack(c, dim=0).cpu().numpy().astype(np.int64) for c in self.chunks()]
        width = 4 if self.row_labels is None else 6
        both = np.concatenate(parts, axis=1) if parts else np.zeros((width, 0), dtype=np.int64)
        return tuple(both[k] for k in range(width))

    def _row_best_of(self, pi, pj, rows: _DeviceRows):
        """Device (row_off int64, l1 int32, arg int32) of ``pair_row_best_device`` for the pairs (pi[k], pj[k]) (device int32): on
        the file where it stays on the device, else ``pair_row_bests``' chunks, copied back -- ``_scores_of``'s two routes."""
        import torch
        pairs = torch.stack([pi, pj], dim=1).contiguous()
        if rows.resident is not None:
            return pair_row_best_device(rows.resident, rows.idx_dev, rows.resident, rows.idx_dev, pairs)
        off, l1, arg = pair_row_bests(self.fps, self.idx, pairs.cpu().numpy(), self.COL_ROWS)
        return (torch.as_tensor(off, device=pi.device),) + tuple(torch.as_tensor(v.astype(np.int32), device=pi.device) for v in (l1, arg))

    def write(self, sink):
        """Calls ``sink(memoryview)`` with the text of each range of rows that has any, in order."""
        out = TextStream(sink, room=lambda nbytes: max(nbytes, 1 << 16))
        lines = None
        rows = self.device_rows() if self.map_l1 is not None else None    # (the map reads the fingerprints of the printed pairs again)
        for chunk in self.chunks(rows):
            lines = lines or _PairText(self, out, chunk[0].device, rows)
            lines.write(*chunk)                                 # (the previous range goes out while the device works on this one)
        out.close()


class _PairText:
    """The pair lines of one ``write`` of a ``FilteredPairs``: the ids, the score table and, with ``row_labels``, the label ids and
    every protein's first row go to the device once; ``write`` composes the lines of one list of pairs there (step 4 of the class
    text) and hands them to the stream.  With a domain map (``job.map_l1``; ``rows`` = the job's ``device_rows()``) the lines come
    from ``pair_map_lines`` at the cumulative sum of ``pair_map_line_lengths``."""

    def __init__(self, job, out: TextStream, dev, rows: _DeviceRows = None):
        import torch
        self.out = out
        self.job, self.rows = job, rows
        self.idx_dev = torch.as_tensor(job.idx, device=dev) if job.map_l1 is not None else None
        self.ids = LineIds([f'{s}' for s in job.sid])
        self.table = torch.as_tensor(score_table(), device=dev)
        self.labels = self.first_row = None
        if job.row_labels is not None:                          # (one label per fingerprint row, then the "no pair" entry)
            self.labels = LineIds(list(job.row_labels) + [NO_DOMAIN], device=dev)
            self.first_row = torch.as_tensor(job.idx[:-1].astype(np.int32), device=dev)
            self.none = len(job.row_labels)

    def write(self, pi, pj, mn, last, *args):
        import torch
        la = lb = None
        if self.labels is not None:
            la, lb = (torch.where(arg >= 0, self.first_row[p.long()] + arg, torch.full_like(arg, self.none)).contiguous()
                      for p, arg in zip((pi, pj), args))
        if self.job.map_l1 is not None:
            best = self.job._row_best_of(pi, pj, self.rows)
            common = (pi, pj, mn, last, la, lb, self.ids, self.labels, self.table, self.idx_dev, *best, self.job.map_l1)
            off = torch.zeros(pi.numel() + 1, dtype=torch.int64, device=pi.device)
            torch.cumsum(pair_map_line_lengths(*common), 0, out=off[1:])
            nbytes = int(off[-1])
            text = torch.empty(nbytes, dtype=torch.uint8, device=pi.device)
            pair_map_lines(*common, off, text)
            self.out.hand_over(text, nbytes)
            return
        off = pair_line_offsets(pi, pj, self.ids, la, lb, self.labels)
        nbytes = int(off[-1])
        text = torch.empty(nbytes, dtype=torch.uint8, device=pi.device)
        pair_lines(pi, pj, mn, last, self.ids, self.table, off, text, la, lb, self.labels)
        self.out.hand_over(text, nbytes)


def _ragged_gather(raw: np.ndarray, starts: np.ndarray, lens: np.ndarray) -> np.ndarray:
    """raw[starts[k]:starts[k] + lens[k]] for every k, concatenated (``_compact``'s index arithmetic, for bytes)."""
    ends = np.cumsum(lens)
    return raw[np.repeat(starts - (ends - lens), lens) + np.arange(int(ends[-1]) if len(ends) else 0, dtype=np.int64)]


def _ascii_id_rows(sid):
    """(uint8 (n, width) of the ids' bytes, their lengths) for a numpy unicode array whose ids are all ASCII -- what a
    ``-dct.npz`` usually holds: a code point is a byte, every id padded to one width -- or None for anything else."""
    if not (isinstance(sid, np.ndarray) and sid.dtype.kind == 'U' and sid.ndim == 1 and sid.dtype.itemsize and sid.dtype.isnative):
        return None
    points = np.ascontiguousarray(sid).view(np.uint32).reshape(len(sid), -1)
    if points.max() >= 128:
        return None
    used = points != 0                                          # (numpy drops trailing NULs only: an id ends at its last other one)
    lens = np.where(used.any(axis=1), points.shape[1] - np.argmax(used[:, ::-1], axis=1), 0)
    return points.astype(np.uint8), lens


def _ascii_lines(wide, lens, rep, member, chunk_bytes: int):
    """``cluster_lines``' text from fixed-width id rows: a line is a row [representative, ' ', member, '\n'] with each id cut at
    its length -- one masked copy per chunk of lines."""
    width = wide.shape[1]
    col = np.arange(width)[None, :]
    per = max(1, chunk_bytes // (2 * width + 2))
    for t0 in range(0, len(member), per):
        r, m = rep[t0:t0 + per], member[t0:t0 + per]
        sep = np.ones((len(r), 1), dtype=bool)
        rows = np.concatenate([wide[r], np.full((len(r), 1), 32, np.uint8), wide[m], np.full((len(r), 1), 10, np.uint8)], axis=1)
        yield rows[np.concatenate([col < lens[r, None], sep, col < lens[m, None], sep], axis=1)]


def cluster_lines(sid, labels, chunk_bytes: int = 1 << 24, rep=None):
    """The text of ``--cluster`` for given labels (``labels[i]`` = index of the representative of protein i), as uint8 arrays of
    whole lines of about ``chunk_bytes`` each: one line ``"{id of representative} {id of member}\n"`` per protein in the order of
    a stable sort of the proteins by label -- clusters by representative index, members by index inside a cluster, so a
    representative's own line comes first.  Composed from the ids' bytes by index arithmetic: no Python loop per line.
    ``rep`` (``--rep medoid``: ``Clusters.medoids``): the protein that names the cluster of protein i in the first field instead of
    ``labels[i]`` -- the lines and their order stay, so a medoid's own line need not come first."""
    labels = np.asarray(labels, dtype=np.int64)
    n = len(labels)
    if n != len(sid):
        raise ValueError('one label per protein')
    if n == 0:
        return
    if labels.min() < 0 or labels.max() >= n:
        raise IndexError('a label outside the proteins of the file')
    member = np.argsort(labels, kind='stable')
    first = labels
    if rep is not None:
        first = np.asarray(rep, dtype=np.int64)
        if len(first) != n:
            raise ValueError('one representative per protein')
        if first.min() < 0 or first.max() >= n:
            raise IndexError('a representative outside the proteins of the file')
    yield from _id_lines(sid, first[member], member, chunk_bytes)


def medoid_cluster_lines(sid, labels, rep, chunk_bytes: int = 1 << 24):
    """``cluster_lines`` in which ``rep[i]`` names the cluster of protein i: the same lines in the same order -- clusters by their
    smallest member (``labels``), members by index -- with only the first field changed."""
    return cluster_lines(sid, labels, chunk_bytes, rep=rep)


def _id_lines(sid, rep, member, chunk_bytes: int):
    """``cluster_lines``' text for given lines: line t is ``"{sid[rep[t]]} {sid[member[t]]}\n"``."""
    n = len(member)
    if n == 0:
        return
    wide = _ascii_id_rows(sid)
    yield from _ascii_lines(*wide, rep, member, chunk_bytes) if wide is not None else _field_lines(sid, [rep, member], chunk_bytes)


def _field_lines(table, fields, chunk_bytes: int):
    """Lines made of fields that all draw from one ``table`` of strings: line t is ``' '.join(table[f[t]] for f in fields) + '\n'``,
    ``fields`` = k int64 index arrays of one length.  Yields uint8 arrays of whole lines of about ``chunk_bytes`` each (at least
    one line), gathered from the table's bytes by index arithmetic: no Python loop per line."""
    enc = [f'{s}'.encode('utf8') for s in table]
    lens = np.fromiter((len(e) for e in enc), dtype=np.int64, count=len(enc))
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    raw = np.frombuffer(b''.join(enc) + b' \n', dtype=np.uint8)   # (the two separators sit behind the table)
    del enc
    space, newline = int(off[-1]), int(off[-1]) + 1
    ends = np.cumsum(sum(lens[f] for f in fields) + len(fields))
    t0, n = 0, len(ends)
    while t0 < n:
        t1 = min(n, max(t0 + 1, int(np.searchsorted(ends, (ends[t0 - 1] if t0 else 0) + chunk_bytes, 'right'))))
        one = np.ones(t1 - t0, dtype=np.int64)
        part = [np.asarray(f[t0:t1], dtype=np.int64) for f in fields]
        starts = np.stack([v for f in part for v in (off[f], space * one)], axis=1)
        sizes = np.stack([v for f in part for v in (lens[f], one)], axis=1)
        starts[:, -1] = newline
        yield _ragged_gather(raw, starts.ravel(), sizes.ravel())
        t0 = t1


def _wide_field_lines(wide, lens, fields, chunk_bytes: int):
    """``_field_lines`` for a table of ASCII strings held as fixed-width rows (``_ascii_id_rows`` of the table): a line is a row of
    its fields' table rows -- each field as wide as its longest string in use -- every one followed by a separator slot, a space
    or behind the last a newline, and cut at its length: one gather per field and one masked copy per chunk of lines."""
    fields = [np.asarray(f, dtype=np.int64) for f in fields]
    widths = [int(lens[f].max()) if len(f) else 0 for f in fields]
    per = max(1, chunk_bytes // (sum(widths) + len(fields)))
    for t0 in range(0, len(fields[0]), per):
        blocks, masks = [], []
        for k, (f, w) in enumerate(zip(fields, widths)):
            f = f[t0:t0 + per]
            end = lens[f][:, None]
            block = np.empty((len(f), w + 1), dtype=np.uint8)
            block[:, :w] = wide[:, :w][f]
            np.put_along_axis(block, end, 32 if k + 1 < len(fields) else 10, axis=1)
            blocks.append(block)
            masks.append(np.arange(w + 1)[None, :] <= end)
        yield np.concatenate(blocks, axis=1)[np.concatenate(masks, axis=1)]


class _ProteinClusters(FilteredPairs):
    """What ``Clusters`` and ``Representatives`` share: cut-offs without domain pairs (nothing is printed per pair), the answers
    that need no tile, and the text."""

    def __init__(self, sid, idx, fps, min_domain=None, min_global=None):
        super().__init__(sid, idx, fps, min_domain=min_domain, min_global=min_global)

    def _plain_labels(self):
        """The labels where no pair has to be looked at -- every protein its own for fewer than two proteins or a bound below 0 (a
        cut-off above 1), all 0 where no bound excludes anything -- else None.  A coverage leaves both as they are: a DCTdomain
        bound below 0 matches no row, one of 17000 matches every row of every pair."""
        n = len(self.idx) - 1
        if n < 2 or min(self.bound_domain, self.bound_global) < 0:
            return np.arange(max(n, 0), dtype=np.int32)
        if min(self.bound_domain, self.bound_global) >= L1_FULL_SCALE:
            return np.zeros(n, dtype=np.int32)
        return None

    def write(self, sink, labels=None, rep=None):
        """Calls ``sink(memoryview)`` with the text (of ``labels()``, or of labels it gave before), whole lines at a time, in order.
        ``rep``: the first field of every line (``cluster_lines``)."""
        for text in cluster_lines(self.sid, self.labels() if labels is None else labels, rep=rep):
            sink(memoryview(text))


class Clusters(_ProteinClusters):
    """Single-linkage clusters of one file at cut-offs: the connected components of the graph whose nodes are all proteins and
    whose edges are exactly ``FilteredPairs``' pairs, joined on the device in a union-find forest (``parent``, n int32) instead of
    listed.  ``labels()[i]`` = the index of the representative of protein i = the smallest index in its cluster: a property of the
    graph, whatever the stripes, the column groups or the order in which the device ran.

    - One cut-off excludes anything: per stripe, ``FilteredPairs.tiles``' tile goes straight to ``tri_link``; nothing comes back
      to the host before the end -- no count, no fill, no ``pair_min``, no lines.
    - Both do: ``FilteredPairs.chunks`` -- which applies the second cut-off to the survivors of the first -- and ``link_pairs`` on
      each chunk's pairs.
    - Neither does (cut-offs <= 0, NaN): one cluster.  A bound below 0 (a cut-off above 1): every protein its own.  No tile.

    Then ``cluster_labels`` on the device and one copy of n int32.  The text is composed on the host (``cluster_lines``), O(n).

    ``medoids()`` (``--rep medoid``) names every cluster by its most central member instead of its first: with key(x, y) =
    min(L1(x, y), 17000) of the route's score -- DCTglobal's last-row L1 on the ``'global'`` route (a DCTglobal cut-off, alone or
    beside the other), else DCTdomain's protein minimum; 17000 for a protein without fingerprints -- S(x) = the sum of key(x, y)
    over the other members y of x's cluster, and the medoid of a cluster is its member with the smallest S, ties to the lowest
    index.  A coverage decides membership only: the sums are taken on ``protein_min``'s tile, so a pair the coverage rejected
    inside one cluster still counts with its distance.  A second pass over the triangle, ``label_sums`` on every stripe's tile
    with the final labels on the device (n int64 sums, exact); when the triangle is one stripe that ``tri_link`` read as it is, the
    tile of the first pass is kept and not filled again, else the tiles are computed anew (what ``Tree`` pays per round).  The
    choice per cluster is n-element work on the device (two ``scatter_reduce_`` minima: of S per label, then of the indices that
    attain it -- no (sum, index) word, so no limit on n beyond the class's own); n int32 come back."""

    def labels(self) -> np.ndarray:
        plain = self._plain_labels()
        if plain is not None:
            return plain
        return self._link()[0].cpu().numpy()

    def _link(self, keep: bool = False):
        """(device int32 labels, kept): the linking of the class text.  ``keep``: kept = [(i0, tile, flags)] of the one stripe when
        the triangle is one stripe, under no coverage, and ``tri_link`` read its tile -- else None."""
        import torch
        parent = torch.arange(len(self.idx) - 1, dtype=torch.int32, device=torch.device('cuda', torch.cuda.current_device()))
        held = [] if keep and self.cover is None else None
        if max(self.bound_domain, self.bound_global) < L1_FULL_SCALE:
            for pi, pj, *_ in self.chunks():
                link_pairs(pi, pj, parent)
        else:
            for i0, tile, flags in self.tile_pass(hold=held):
                tri_link(tile, i0, i0 + 1, self.bound, parent, *flags)
                del tile
        return cluster_labels(parent), held or None

    def medoids(self, labels=None) -> np.ndarray:
        """``rep`` (int32, n): ``rep[x]`` = the medoid of the cluster of protein x (class text) -- of ``labels()``, or of ``labels``
        given (one per protein, each the index of a protein, as ``labels()`` gives them).  ``last_labels`` = the labels it went by."""
        import torch
        n = len(self.idx) - 1
        kept = None
        if labels is None:
            labels = self._plain_labels()
            if labels is None:
                lab_dev, kept = self._link(keep=True)
                labels = lab_dev.cpu().numpy()
        labels = np.ascontiguousarray(np.asarray(labels, dtype=np.int32))
        if len(labels) != max(n, 0):
            raise ValueError('one label per protein')
        if n > 0 and (labels.min() < 0 or labels.max() >= n):
            raise IndexError('a label outside the proteins of the file')
        self.last_labels = labels
        if n < 2 or np.array_equal(labels, np.arange(n, dtype=np.int32)):     # (every protein its own: no pair to sum)
            return np.arange(max(n, 0), dtype=np.int32)
        dev = torch.device('cuda', torch.cuda.current_device())
        lab_dev = torch.as_tensor(labels, device=dev)
        sums = torch.zeros(n, dtype=torch.int64, device=dev)
        for i0, tile, flags in kept or self.tile_pass(cover=False):
            label_sums(tile, i0, i0 + 1, lab_dev, sums, *flags, cap=L1_FULL_SCALE)
            del tile
        del kept
        lab = lab_dev.to(torch.int64)
        # per label the smallest sum, then the lowest index that attains it
        least = torch.full((n,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev).scatter_reduce_(0, lab, sums, 'amin')
        index = torch.arange(n, dtype=torch.int64, device=dev)
        index = torch.where(sums == least[lab], index, torch.full_like(index, n))
        medoid = torch.full((n,), n, dtype=torch.int64, device=dev).scatter_reduce_(0, lab, index, 'amin')
        return medoid[lab].to(torch.int32).cpu().numpy()


KIND_NOISE, KIND_BORDER, KIND_CORE = 0, 1, 2


class DensityClusters(Clusters):
    """Density clusters of one file at cut-offs (``--cluster --min-neighbors M``): DBSCAN whose radius is the cut-off.  G is
    ``Clusters``' graph -- the proteins, and exactly ``FilteredPairs``' pairs as edges, coverage included -- and deg(x) the number of
    edges at x (x itself is not counted).

    - x is a **core** when deg(x) >= M.  A cluster's cores are a connected component of the edges whose two ends are both cores.
    - A non-core with a core neighbour is a **border**: it joins the cluster of its LOWEST core neighbour, so the result does not
      depend on the order in which anything ran (textbook DBSCAN gives a border to whichever cluster reaches it first).
    - A non-core without a core neighbour is **noise**: a cluster of its own.  A protein without fingerprints is on no edge.

    ``labels()[x]`` = the smallest index among ALL members of x's cluster, cores and borders alike -- every other mode's convention --
    and the text is ``cluster_lines``' own.  M = 1 gives ``Clusters.labels()`` exactly: every protein on an edge is a core.

    - One cut-off excludes anything: pass 1 over ``tiles()`` counts the degrees (``tri_degree``), ``core = deg >= M`` on the device,
      pass 2 joins the core-core edges in the forest and keeps per non-core protein its lowest core neighbour (``tri_link_core``).
      When the triangle is one stripe the tile of pass 1 is kept for pass 2; else the tiles are filled again -- twice the work of
      ``Clusters``, the trade ``medoids`` makes.
    - Both do: ``chunks()`` twice, as ``Clusters`` goes through it once -- the degrees by ``index_add_`` of the surviving pairs, then
      the core-core pairs to ``link_pairs`` and the one-core pairs into a ``scatter_reduce_`` minimum: n- and m-element work.
    - Neither does: the graph is complete -- one cluster if n - 1 >= M, else every protein its own.  A bound below 0, or fewer than
      two proteins: every protein its own.  No tile.

    Then n-element work on the device: ``cluster_labels``, the borders take the label of their nearest core, the labels become the
    smallest member of each cluster (a ``scatter_reduce_`` minimum of the indices); n int32 come back.  ``kinds()`` (uint8: 0 noise,
    1 border, 2 core) and ``degrees()`` (int32) are those of the last ``labels()`` / ``medoids()`` run, which they start when there was
    none.  ``medoids()`` is ``Clusters``' on these labels."""

    def __init__(self, sid, idx, fps, min_domain=None, min_global=None, min_neighbors: int = 1):
        if int(min_neighbors) != min_neighbors or int(min_neighbors) < 1:
            raise ValueError('min_neighbors is a number of neighbours: an integer, at least 1')
        super().__init__(sid, idx, fps, min_domain=min_domain, min_global=min_global)
        self.min_neighbors = int(min_neighbors)
        self._found = None                                      # (degrees, kinds) of the last run: numpy arrays or device tensors

    def _plain_labels(self):
        plain = super()._plain_labels()
        if plain is None:
            return None
        n = max(len(self.idx) - 1, 0)
        if n < 2 or min(self.bound_domain, self.bound_global) < 0:     # (every protein its own: no edge at all)
            self._found = (np.zeros(n, dtype=np.int32), np.full(n, KIND_NOISE, dtype=np.uint8))
            return plain
        dense = n - 1 >= self.min_neighbors                     # (the complete graph: every degree is n - 1)
        self._found = (np.full(n, n - 1, dtype=np.int32), np.full(n, KIND_CORE if dense else KIND_NOISE, dtype=np.uint8))
        return plain if dense else np.arange(n, dtype=np.int32)

    def _found_array(self, k: int) -> np.ndarray:
        if self._found is None:
            self.labels()
        v = self._found[k]
        return v if isinstance(v, np.ndarray) else v.cpu().numpy()

    def degrees(self) -> np.ndarray:
        """int32 (n): the number of edges at every protein."""
        return self._found_array(0)

    def kinds(self) -> np.ndarray:
        """uint8 (n): ``KIND_NOISE`` (0), ``KIND_BORDER`` (1) or ``KIND_CORE`` (2) per protein."""
        return self._found_array(1)

    def _link(self, keep: bool = False):
        """(device int32 labels, kept) as ``Clusters._link`` gives them: the two passes and the n-element work of the class text."""
        import torch
        n = len(self.idx) - 1
        dev = torch.device('cuda', torch.cuda.current_device())
        deg = torch.zeros(n, dtype=torch.int32, device=dev)
        parent = torch.arange(n, dtype=torch.int32, device=dev)
        kept = None
        if max(self.bound_domain, self.bound_global) < L1_FULL_SCALE:
            for pi, pj, *_ in self.chunks():
                one = torch.ones_like(pi)
                deg.index_add_(0, pi.to(torch.int64), one).index_add_(0, pj.to(torch.int64), one)
            core = deg >= self.min_neighbors
            nearest = torch.full((n,), NEAREST_NONE, dtype=torch.int64, device=dev)
            for pi, pj, *_ in self.chunks():
                pi, pj = pi.to(torch.int64), pj.to(torch.int64)
                ci, cj = core[pi], core[pj]
                both = ci & cj
                link_pairs(pi[both].to(torch.int32), pj[both].to(torch.int32), parent)
                nearest.scatter_reduce_(0, pj[ci & ~cj], pi[ci & ~cj], 'amin')
                nearest.scatter_reduce_(0, pi[cj & ~ci], pj[cj & ~ci], 'amin')
        else:
            held = []
            for i0, tile, flags in self.tile_pass(hold=held):
                tri_degree(tile, i0, i0 + 1, self.bound, deg, *flags)
                del tile
            core = deg >= self.min_neighbors
            flag = core.to(torch.uint8)
            nearest = torch.full((n,), NEAREST_NONE, dtype=torch.int32, device=dev)
            for i0, tile, flags in held or self.tile_pass():
                tri_link_core(tile, i0, i0 + 1, self.bound, flag, parent, nearest, *flags)
                del tile
            kept = (held or None) if keep and self.cover is None else None
            del held
            nearest = nearest.to(torch.int64)
        lab = cluster_labels(parent).to(torch.int64)           # a core: the root of its component; a non-core: itself
        border = ~core & (nearest != NEAREST_NONE)
        lab = torch.where(border, lab[nearest.clamp(max=n - 1)], lab)
        # per cluster its smallest member, borders included
        index = torch.arange(n, dtype=torch.int64, device=dev)
        first = torch.full((n,), n, dtype=torch.int64, device=dev).scatter_reduce_(0, lab, index, 'amin')
        self._found = (deg, (core.to(torch.uint8) * KIND_CORE + border.to(torch.uint8) * KIND_BORDER))
        return first[lab].to(torch.int32), kept


SCORES = ('domain', 'global')


class Tree(FilteredPairs):
    """The single-linkage tree of one file: the minimum spanning forest of the graph whose nodes are all proteins and whose edges
    are the pairs i < j with key = min(L1, 17000) <= bound, under the strict order (key, i, j) -- unique, because no two edges
    compare equal.  L1 is DCTdomain's (``score='domain'``: ``protein_min``) or DCTglobal's (``'global'``: ``l1_matrix`` of the last
    rows, the proteins without fingerprints flagged as on ``FilteredPairs``' global route); bound = 16999, every pair of similarity
    above 0, unless ``min_cut`` gives ``sim_bound(min_cut)``.  Cut at any bound b <= its own, the tree's edges with key <= b have
    the components ``Clusters`` finds at b: one pass answers every cut-off (``labels``).

    Boruvka's algorithm over ``FilteredPairs.tiles``, in rounds of

    1. ``tri_nearest`` on every stripe's tile: per component the lightest edge that leaves it (both ends of every entry count);
    2. ``tree_hook``: every component appends its edge and joins the two ends in the union-find forest;
    3. ``cluster_labels``: the labels of the next round.

    A round at least halves the components that can still grow, so there are at most ceil(log2 n) + 1 of them; the loop stops when
    one appends nothing (one int32 comes back per round) or the tree is complete, and raises beyond that number rather than go
    on.  When the triangle fits one stripe (TILE_INTS) its tile is computed once and kept; else the tiles are computed anew in
    every round: the cost is rounds x one ``Clusters`` pass.  ``rounds`` = the rounds of the last build.

    ``edges()`` = (i, j, key) in (key, i, j) order: the merge order of single linkage, most similar first.  ``write`` prints them
    as the very lines the all-against-all prints for those pairs ((min, last) from ``pair_min_device``, text from ``pair_lines``):
    n - c lines for a forest of c components."""

    def __init__(self, sid, idx, fps, score: str = 'domain', min_cut=None):
        if score not in SCORES:
            raise ValueError(f'score must be one of {SCORES}')
        super().__init__(sid, idx, fps)
        bound = L1_FULL_SCALE - 1 if min_cut is None else sim_bound(min_cut)
        self.score = self.route = score                         # (the tile of that score whatever the bound)
        if score == 'domain':
            self.bound_domain = bound
        else:
            self.bound_global = bound
        self.rounds = 0
        self._edges = None

    def edges(self):
        """(i, j, key): int64 numpy arrays of the tree's edges in (key, i, j) order (built once)."""
        if self._edges is None:
            i, j, key = self._build()
            order = np.lexsort((j, i, key))
            self._edges = i[order], j[order], key[order]
        return self._edges

    def _build(self):
        n = len(self.idx) - 1
        self.rounds = 0
        if n < 2 or self.bound < 0:
            return tuple(np.zeros(0, dtype=np.int64) for _ in range(3))
        if n > TREE_MAX_NODES:
            raise ValueError(f'the tree takes at most {TREE_MAX_NODES} proteins')
        ts = TreeState(n)
        rows = self.device_rows() if self.route == 'domain' else None
        held = []                                               # (the whole triangle in one tile: computed once)
        most = max(1, int(n - 1).bit_length()) + 1              # ceil(log2 n) + 1
        done = 0
        while done < n - 1:
            if self.rounds >= most:
                raise RuntimeError(f'the tree of {n} proteins is not finished after {most} rounds')
            for i0, tile, flags in held or self.tile_pass(rows, hold=held):
                tri_nearest(tile, i0, i0 + 1, self.bound, ts, *flags)
                del tile
            tree_hook(ts)
            self.rounds += 1
            total = int(ts.counter.item())
            if total == done:
                break
            done = total
            ts.comp = cluster_labels(ts.parent)
        return ts.edges()

    def labels(self, cut: float) -> np.ndarray:
        """The single-linkage clusters at the cut-off ``cut`` from the tree as it is built (no further pass over the pairs):
        ``Clusters(min_domain=cut).labels()`` -- ``min_global`` for ``score='global'`` -- for every cut whose bound is not above the
        tree's own.  ``link_pairs`` on the edges with key <= ``sim_bound(cut)``, then ``cluster_labels``."""
        n = len(self.idx) - 1
        bound = sim_bound(cut)
        if bound > self.bound:
            raise ValueError(f'the tree was built with bound {self.bound}: it does not hold the clusters at {cut} (bound {bound})')
        i, j, key = self.edges()
        keep = key <= bound
        if n < 1 or not keep.any():
            return np.arange(max(n, 0), dtype=np.int32)
        import torch
        dev = torch.device('cuda', torch.cuda.current_device())
        parent = torch.arange(n, dtype=torch.int32, device=dev)
        link_pairs(torch.as_tensor(i[keep].astype(np.int32), device=dev), torch.as_tensor(j[keep].astype(np.int32), device=dev), parent)
        return cluster_labels(parent).cpu().numpy()

    def write(self, sink):
        """Calls ``sink(memoryview)`` with the text of the edges, ranges of at most TEXT_BYTES at a time, in order."""
        i, j, _ = self.edges()
        if not len(i):
            return
        import torch
        dev = torch.device('cuda', torch.cuda.current_device())
        rows = self.device_rows()
        out = TextStream(sink, room=lambda nbytes: max(nbytes, 1 << 16))
        lines = _PairText(self, out, dev)
        ends = np.cumsum(lines.ids.lens[i] + lines.ids.lens[j] + 14)
        k0 = 0
        while k0 < len(i):
            k1 = min(len(i), max(k0 + 1, int(np.searchsorted(ends, (ends[k0 - 1] if k0 else 0) + self.TEXT_BYTES, 'right'))))
            pi, pj = (torch.as_tensor(v[k0:k1].astype(np.int32), device=dev) for v in (i, j))
            lines.write(pi, pj, *self._scores_of(pi, pj, rows=rows))
            k0 = k1
        out.close()


HAC_HEADER = '#rep1 rep2 similarity size'
HAC_METHODS = ('average', 'complete')
HAC_MAX_PROTEINS = 46340                   # similarity.LINKAGE_MAX_N: the dense matrix of --hac
_NEWICK_QUOTED = frozenset("(),:;'[]")


def newick_name(name) -> str:
    """An id as a Newick label: single-quoted, with ``'`` doubled, when it holds any of ``(),:;'[]`` or whitespace."""
    name = f'{name}'
    if any(ch in _NEWICK_QUOTED or ch.isspace() for ch in name):
        return "'" + name.replace("'", "''") + "'"
    return name


class Dendrogram:
    """The complete- (``method='complete'``) or average-linkage (``'average'``: UPGMA) tree of one file, built on the GPU.

    Nodes are the n proteins; key(i, j) = min(L1, 17000) with ``Tree``'s L1 -- DCTdomain's (``score='domain'``: ``protein_min``) or
    DCTglobal's (``'global'``: ``l1_matrix`` of the last rows) -- and 17000 against a protein without fingerprints; bound = 16999
    unless ``min_cut`` gives ``sim_bound(min_cut)``.  A cluster is named by its lowest member.  complete: D(A, B) = the largest key
    over the member pairs, int32; average: S(A, B) = their sum, int64, height = S / (cA cB) compared as an exact fraction -- "D <=
    bound" is S <= bound cA cB.  The state is the dense n x n matrix of D or S on the device (n <= ``LINKAGE_MAX_N`` = 46 340; n * n
    * 4 or 8 bytes, which must fit the free device memory), ``size`` and the live ids.  A round:

    1. ``linkage_nearest``: per live cluster a, nn(a) = the live b != a with D(a, b) <= bound that minimises (D(a, b), id b);
    2. every pair with nn(a) = b and nn(b) = a merges, all at once, under the lower id (n-element work in torch; one int32, the
       number of pairs, comes back per round), recorded as (a, b, height, new size, round);
    3. ``linkage_merge``: every distance to a merged cluster becomes the max / the sum over the pre-round clusters.

    The smallest pair under (D, lo, hi) is always mutual, so a round with a pair within the bound merges at least one: the loop
    ends with the round that merges nothing and raises beyond n - 1 merging rounds rather than go on.  ``rounds`` = the merging
    rounds of the last build.  Merge order: (height exact, round, a); both linkages are reducible, so the heights
    of a parent is never below its children's.

    ``merges()`` = (a, b, num, den, size, round) as int64 numpy arrays in merge order, height = num / den (den = 1 for complete).
    ``labels(cut)`` replays them: the clusters at any cut whose bound is not above the object's own -- for complete linkage every
    pair inside a cluster is then within the cut-off."""

    COL_ROWS = FilteredPairs.COL_ROWS
    TILE_INTS = 1 << 26          # int32 entries of one stripe of the matrix while it is built

    def __init__(self, sid, idx, fps, method: str = 'average', score: str = 'domain', min_cut=None):
        if method not in HAC_METHODS:
            raise ValueError(f'method must be one of {HAC_METHODS}')
        if score not in SCORES:
            raise ValueError(f'score must be one of {SCORES}')
        self.sid, self.idx, self.fps = sid, np.asarray(idx, dtype=np.int64), fps
        self.method, self.score = method, score
        self.bound = L1_FULL_SCALE - 1 if min_cut is None else min(sim_bound(min_cut), L1_FULL_SCALE)
        self.rounds = 0
        self.seconds = {}            # matrix / scan / merge of the last build, filled when ``timed`` is set (tools/linkage_bench.py)
        self.timed = False
        self._merges = None

    @property
    def n(self) -> int:
        return len(self.idx) - 1

    def matrix_bytes(self) -> int:
        return self.n * self.n * (4 if self.method == 'complete' else 8)

    def _matrix(self, dev):
        """The dense key matrix on the device, int32 (complete) or int64 (average), the diagonal at the sentinel; rows padded to
        16 bytes, so that every row is read with 16-byte loads alone.  Built in stripes of rows x all n columns."""
        import torch
        from .similarity import LINKAGE_NONE
        n, idx = self.n, self.idx
        dtype = torch.int32 if self.method == 'complete' else torch.int64
        ld = (n + 3) // 4 * 4
        store = torch.empty((n, ld), dtype=dtype, device=dev)
        mat = store[:, :n]
        total = int(idx[-1])
        empty = torch.as_tensor(idx[1:] == idx[:-1], device=dev)
        if self.score == 'global':
            last_rows, _ = _last_rows(self.fps[:total], idx)
            last = to_device_int8(last_rows)
            groups = [(i0, min(n, i0 + max(1, self.TILE_INTS // n))) for i0 in range(0, n, max(1, self.TILE_INTS // n))]
        else:
            rows = _DeviceRows(self.fps, idx, self.COL_ROWS)
            groups = list(_protein_groups(idx, self.COL_ROWS))
            step = max(1, self.TILE_INTS // n)
            groups = [(j0, min(i1, j0 + step)) for i0, i1 in groups for j0 in range(i0, i1, step)]
        for i0, i1 in groups:
            tile = mat[i0:i1] if dtype == torch.int32 else torch.empty((i1 - i0, n), dtype=torch.int32, device=dev)
            if self.score == 'global':
                l1_matrix(last[i0:i1], last, out=tile)
            else:
                a, ia = rows(i0, i1), idx[i0:i1 + 1] - idx[i0]
                for q0, q1 in _protein_groups(idx, self.COL_ROWS):
                    protein_min(a, ia, rows(q0, q1), idx[q0:q1 + 1] - idx[q0], out=tile[:, q0:q1])
            tile.clamp_(max=L1_FULL_SCALE)
            tile[empty[i0:i1]] = L1_FULL_SCALE                 # (the last rows of a protein without fingerprints are zeros: no L1)
            tile[:, empty] = L1_FULL_SCALE
            if dtype != torch.int32:
                mat[i0:i1] = tile
            del tile
        mat.diagonal().fill_(LINKAGE_NONE[dtype])
        return mat

    def _build(self):
        n = self.n
        self.rounds = 0
        self.seconds = {}
        none = tuple(np.zeros(0, dtype=np.int64) for _ in range(6))
        if n < 2 or self.bound < 0:
            return none
        from .similarity import LINKAGE_MAX_N, linkage_merge, linkage_nearest
        if n > LINKAGE_MAX_N:
            raise ValueError(f'--hac keeps the dense matrix of the file on the device: at most {LINKAGE_MAX_N} proteins, not {n}')
        import torch
        dev = torch.device('cuda', torch.cuda.current_device())
        free = torch.cuda.mem_get_info(dev)[0]
        if self.matrix_bytes() > free:
            raise ValueError(f'the {self.method}-linkage matrix of {n} proteins needs {self.matrix_bytes()} bytes on the device: {free} are free')

        def clock(name, t0=None):
            if not self.timed:
                return None
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            if t0 is not None:
                self.seconds[name] = self.seconds.get(name, 0.0) + now - t0
            return now

        t0 = clock(None)
        mat = self._matrix(dev)
        clock('matrix', t0)
        wide = mat.dtype == torch.int64
        size = torch.ones(n, dtype=torch.int32, device=dev)
        live = torch.arange(n, dtype=torch.int32, device=dev)
        made = []
        while True:
            if live.numel() < 2:                                # (one cluster left: nothing to scan for)
                break
            if self.rounds >= n - 1:
                raise RuntimeError(f'the {self.method}-linkage tree of {n} proteins is not finished after {n - 1} merging rounds')
            t0 = clock(None)
            nn = linkage_nearest(mat, size, live, self.bound)
            clock('scan', t0)
            a = live.long()
            b = nn[a].long()
            mutual = (b > a) & (nn[b.clamp(min=0)].long() == a)
            lo, hi = a[mutual], b[mutual]
            if lo.numel() == 0:                                 # (the one number a round sends to the host)
                break
            self.rounds += 1
            num = mat[lo, hi].long()
            den = size[lo].long() * size[hi].long() if wide else torch.ones_like(num)
            partner = torch.full((n,), -1, dtype=torch.int32, device=dev)
            partner[lo] = hi.int()
            partner[hi] = lo.int()
            t0 = clock(None)
            linkage_merge(mat, size, partner, lo.int().contiguous())
            clock('merge', t0)
            size[lo] += size[hi]
            size[hi] = 0
            made.append(torch.stack([lo, hi, num, den, size[lo].long(), torch.full_like(lo, self.rounds)]))
            live = live[size[live.long()] > 0].contiguous()
        del mat
        if not made:
            return none
        out = torch.cat(made, dim=1).cpu().numpy()
        a, b, num, den, sz, rnd = out
        # merge order (height exact, round, a): heights as Python fractions -- S * den' against S' * den in integers, never floats
        from fractions import Fraction
        order = sorted(range(len(a)), key=lambda k: (Fraction(int(num[k]), int(den[k])), rnd[k], a[k]))
        return tuple(v[order] for v in (a, b, num, den, sz, rnd))

    def merges(self):
        """(a, b, num, den, size, round): int64 numpy arrays of the merges in merge order (built once); height = num / den."""
        if self._merges is None:
            self._merges = self._build()
        return self._merges

    def heights(self) -> list:
        """The heights as exact integer pairs (numerator, denominator), in merge order."""
        _, _, num, den, _, _ = self.merges()
        return [(int(p), int(q)) for p, q in zip(num, den)]

    def labels(self, cut: float = None) -> np.ndarray:
        """labels[i] = the lowest member of protein i's cluster at the object's own bound, or at the cut-off ``cut``: the merges of
        height <= ``sim_bound(cut)`` replayed in merge order.  ValueError for a cut whose bound is above the object's own."""
        bound = self.bound if cut is None else sim_bound(cut)
        if bound > self.bound:
            raise ValueError(f'the tree was built with bound {self.bound}: it does not hold the clusters at {cut} (bound {bound})')
        lab = np.arange(max(self.n, 0), dtype=np.int32)
        a, b, num, den, _, _ = self.merges()
        members = {}
        for k in np.flatnonzero(num <= bound * den):           # (int64: at most 17000 * 46340^2 / 4)
            x, y = int(lab[a[k]]), int(lab[b[k]])
            x, y = min(x, y), max(x, y)
            mx, my = members.pop(x, [x]), members.pop(y, [y])
            lab[my] = x
            members[x] = mx + my
        return lab

    def lines(self) -> list:
        """The merge lines ``{id a} {id b} {similarity:.4f} {size}`` in merge order; similarity = 1 - height / 17000 in one correctly
        rounded division of Python ints."""
        a, b, num, den, size, _ = self.merges()
        return [f'{self.sid[a[k]]} {self.sid[b[k]]} {1 - int(num[k]) / (L1_FULL_SCALE * int(den[k])):.4f} {size[k]}' for k in range(len(a))]

    def write(self, sink):
        """Calls ``sink(bytes)`` with the text of the merges (no header)."""
        text = ''.join(line + '\n' for line in self.lines())
        if text:
            sink(text.encode('utf8'))

    def newick(self) -> str:
        """One tree per line in id order, each ending in ``;``: a merge is ``(A:la,B:lb)`` with the lower id first, a branch
        (height - the child's height, 0 for a leaf) / 17000 as ``.6f``, an unmerged protein ``id;``."""
        from fractions import Fraction
        a, b, num, den, _, _ = self.merges()
        node = {i: (newick_name(self.sid[i]), Fraction(0)) for i in range(self.n)}
        for k in range(len(a)):
            h = Fraction(int(num[k]), int(den[k]))
            (ta, ha), (tb, hb) = node[int(a[k])], node.pop(int(b[k]))
            la, lb = (h - ha) / L1_FULL_SCALE, (h - hb) / L1_FULL_SCALE
            node[int(a[k])] = (f'({ta}:{la.numerator / la.denominator:.6f},{tb}:{lb.numerator / lb.denominator:.6f})', h)
        return ''.join(node[i][0] + ';\n' for i in sorted(node))


AUC1_HEADER = '#query family members tp auc1 first_fp fp_score'


def dense_families(families):
    """(int32 code per protein, the family behind every code) for one label per protein, of any hashable kind: codes in the order
    in which the families first appear."""
    codes = {}
    fam = np.fromiter((codes.setdefault(f, len(codes)) for f in families), dtype=np.int32)
    return fam, list(codes)


def auc1_of_counts(tp, fam) -> np.ndarray:
    """float64 (n): tp / (size of the protein's family - 1), 0 for a family of one (the reference's ``ZeroDivisionError`` branch,
    bench/cathdb/plot_results.py)."""
    fam = np.asarray(fam, dtype=np.int64)
    others = (np.bincount(fam, minlength=1)[fam] - 1) if len(fam) else np.zeros(0, dtype=np.int64)
    return np.where(others > 0, np.asarray(tp, dtype=np.float64) / np.maximum(others, 1), 0.0)


def auc1_summary(tp, fam) -> dict:
    """The summary over the queries -- the proteins whose family has at least two members: ``queries``, ``families`` (those with
    queries), ``mean_auc1``, ``top1_raw`` (the share of queries whose best hit is of their own family: tp >= 1, see ``Auc1``) and
    ``top1_norm`` (the mean over those families of each family's share).  Without a query the three rates are 0."""
    fam, tp = np.asarray(fam, dtype=np.int64), np.asarray(tp, dtype=np.int64)
    size = np.bincount(fam, minlength=1) if len(fam) else np.zeros(1, dtype=np.int64)
    query = size[fam] > 1 if len(fam) else np.zeros(0, dtype=bool)
    q = int(query.sum())
    if q == 0:
        return {'queries': 0, 'families': 0, 'mean_auc1': 0.0, 'top1_raw': 0.0, 'top1_norm': 0.0}
    top = (tp >= 1) & query
    share = np.bincount(fam[top], minlength=len(size))[size > 1] / size[size > 1]
    return {'queries': q, 'families': int((size > 1).sum()), 'mean_auc1': float(auc1_of_counts(tp, fam)[query].mean()),
            'top1_raw': float(top.sum() / q), 'top1_norm': float(share.mean())}


def auc1_lines(sid, fam, names, tp, fp_index, fp_key, score: str = 'domain', chunk_bytes: int = 1 << 24):
    """The text of ``--auc1`` as uint8 arrays of whole lines of about ``chunk_bytes`` each: per protein, in file order,
    ``"{query} {family} {members} {tp} {auc1} {first_fp} {fp_score}\\n"`` -- ``members`` the family's size, ``auc1`` as ``%.4f``,
    ``first_fp`` the id of the first false positive and ``fp_score`` that pair's similarity as the pair lines print the score
    (``score_table``), both ``-`` where there is none -- then one line ``# queries=.. families=.. mean_auc1=.. top1_raw=..
    top1_norm=..`` with the rates as ``%.4f``.  One table of strings -- the ids, the families, the integers, the distinct AUC1
    values and score texts -- and index arithmetic over it: fixed-width rows cut at their lengths where every string is ASCII
    (``_wide_field_lines``, ``cluster_lines``' way), else ``_field_lines``.  No Python loop per line."""
    fam, tp = np.asarray(fam, dtype=np.int64), np.asarray(tp, dtype=np.int64)
    fp_index, fp_key = np.asarray(fp_index, dtype=np.int64), np.asarray(fp_key, dtype=np.int64)
    n = len(fam)
    if n:
        members = np.bincount(fam)[fam]
        auc, auc_of = np.unique(auc1_of_counts(tp, fam), return_inverse=True)
        none = fp_index < 0
        keys, key_of = np.unique(np.where(none, 0, fp_key), return_inverse=True)
        which = SCORES.index(score)                             # (score_table's entry, for the distinct keys alone)
        parts = (np.asarray(sid, dtype=np.str_), [f'{f}' for f in names], [str(v) for v in range(int(max(members.max(), tp.max())) + 1)],
                 ['%.4f' % v for v in auc], [f'{_scores(int(k), int(k))[which]:.3f}' for k in keys], [NO_DOMAIN])
        at = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
        table = np.concatenate([np.asarray(p, dtype=np.str_) for p in parts])
        me = np.arange(n, dtype=np.int64)
        fields = [me, at[1] + fam, at[2] + members, at[2] + tp, at[3] + auc_of.reshape(-1), np.where(none, at[5], fp_index),
                  np.where(none, at[5], at[4] + key_of.reshape(-1))]
        wide = _ascii_id_rows(table)
        yield from _wide_field_lines(*wide, fields, chunk_bytes) if wide is not None else _field_lines(table, fields, chunk_bytes)
    s = auc1_summary(tp, fam)
    last = '# queries=%d families=%d mean_auc1=%.4f top1_raw=%.4f top1_norm=%.4f\n' % (
        s['queries'], s['families'], s['mean_auc1'], s['top1_raw'], s['top1_norm'])
    yield np.frombuffer(last.encode('ascii'), dtype=np.uint8)


class Auc1(FilteredPairs):
    """How good the scores of one labelled file are (``--auc1``): the sensitivity benchmark of the reference's
    bench/cathdb/plot_results.py without a line of ranked text.  Every protein x is searched against the whole file; y != x is a
    **hit** of x when key(x, y) = min(L1, 17000) <= bound (17000 where either has no fingerprint), and the hits of x are ranked by
    the word ``key << 32 | y``: by key, ties to the lower index in the file.  L1 is DCTdomain's (``score='domain'``:
    ``protein_min``) or DCTglobal's (``'global'``: ``l1_matrix`` of the last rows, the proteins without fingerprints flagged as on
    ``Tree``'s global route); bound = 16999, every pair of similarity above 0, unless ``min_cut`` gives ``sim_bound(min_cut)``.
    ``families``: one label per protein, of any hashable kind.

    - ``first_fp[x]`` = the smallest word over the hits of another family: the first false positive (all ones: none);
    - ``tp[x]`` = the hits of x's own family whose word is below ``first_fp[x]``;
    - ``auc1[x]`` = ``tp[x]`` / (size of x's family - 1), 0 for a family of one.

    The best hit of x is of its own family exactly when ``tp[x] >= 1``: were the overall best hit of another family it would itself
    be ``first_fp[x]`` and nothing could rank before it; else it is a true positive ranked before ``first_fp[x]``.  So the top-1
    rates (Qraw, Qnorm) need no third pass.

    Two passes over ``FilteredPairs.tiles`` with the dense families on the device: ``tri_first_fp`` on every tile, then
    ``tri_tp_before`` with the finished words.  When the triangle is one stripe the tile of pass 1 is kept for pass 2, else the
    tiles are filled again.  ``first`` and ``tp`` stay on the device between the passes and 12 bytes per protein come back, once.
    Fewer than two proteins or a bound below 0: no hit at all, no tile.  Unlike the reference's script -- which ranks fingerprint
    rows with faiss and keeps 300 hits per query -- this ranks proteins by ``dct-sim``'s own scores and has no hit limit."""

    def __init__(self, sid, idx, fps, families, score: str = 'domain', min_cut=None):
        if score not in SCORES:
            raise ValueError(f'score must be one of {SCORES}')
        super().__init__(sid, idx, fps)
        bound = L1_FULL_SCALE - 1 if min_cut is None else sim_bound(min_cut)
        self.score = self.route = score                         # (the tile of that score whatever the bound)
        if score == 'domain':
            self.bound_domain = bound
        else:
            self.bound_global = bound
        self.fam, self.families = dense_families(families)
        if len(self.fam) != len(self.idx) - 1:
            raise ValueError('families must have one entry per protein')
        self._counts = None

    def counts(self):
        """(tp int32, fp_index int32, fp_key int32) per protein: the true positives before the first false positive, that
        protein's index (-1: none) and the pair's key (17000: none).  Computed once."""
        if self._counts is None:
            self._counts = self._scan()
        return self._counts

    def _scan(self):
        n = len(self.idx) - 1
        if n < 2 or self.bound < 0:
            return np.zeros(max(n, 0), dtype=np.int32), np.full(max(n, 0), -1, dtype=np.int32), np.full(max(n, 0), L1_FULL_SCALE, dtype=np.int32)
        import torch
        dev = torch.device('cuda', torch.cuda.current_device())
        fam = torch.as_tensor(self.fam, device=dev)
        first = torch.full((n,), BEST_NONE, dtype=torch.int64, device=dev)
        tp = torch.zeros(n, dtype=torch.int32, device=dev)
        rows = self.device_rows() if self.route == 'domain' else None
        held = []
        for i0, tile, flags in self.tile_pass(rows, hold=held):
            tri_first_fp(tile, i0, i0 + 1, self.bound, fam, first, *flags)
            del tile
        for i0, tile, flags in held or self.tile_pass(rows):
            tri_tp_before(tile, i0, i0 + 1, self.bound, fam, first, tp, *flags)
            del tile
        del held
        back = torch.cat([first.view(torch.int32), tp]).cpu().numpy()       # one copy of 12 bytes per protein
        word, count = back[:2 * n].view(np.int64), back[2 * n:]
        none = word == BEST_NONE
        return (count.copy(), np.where(none, -1, word & 0xffffffff).astype(np.int32),
                np.where(none, L1_FULL_SCALE, word >> 32).astype(np.int32))

    def auc1(self) -> np.ndarray:
        """float64 (n): AUC1 per protein."""
        return auc1_of_counts(self.counts()[0], self.fam)

    def summary(self) -> dict:
        """``auc1_summary`` of the file."""
        return auc1_summary(self.counts()[0], self.fam)

    def write(self, sink):
        """Calls ``sink(memoryview)`` with the text (``auc1_lines``), whole lines at a time, in order."""
        for text in auc1_lines(self.sid, self.fam, self.families, *self.counts(), score=self.score):
            sink(memoryview(text))


HIST_BINS = 100            # --bins: the cut-offs of a --hist table
HIST_MAX_BINS = 1000


def hist_header(score: str, families: bool) -> str:
    """The header of a ``--hist`` report."""
    return f'#min-{score} same other kept-same kept-other recall precision fpr' if families else f'#min-{score} pairs kept'


def hist_cuts(bins: int):
    """(texts, bounds) of the ``bins`` cut-offs of a ``--hist`` table, highest first: cut-off b is the text
    ``'%.4f' % ((bins - 1 - b) / bins)`` -- what a user types behind ``--min-domain`` -- and its bound is ``sim_bound`` of that text
    read back as a float, not the arithmetic edge (b + 1) x 17000 / bins, which is off by one at a fifth of the edges of 100 bins.
    The last text is ``0.0000``, whose bound is 17000: every pair."""
    texts = ['%.4f' % ((bins - 1 - b) / bins) for b in range(bins)]
    sims = _sim(np.arange(L1_FULL_SCALE + 1))                       # (sim_bound's expression, evaluated once for all texts)
    return texts, [int(np.count_nonzero(~(sims < float(t)))) - 1 for t in texts]


def hist_roc_auc(hist, rest):
    """The ROC AUC of the key as a classifier of (same family, other family) from the two rows of counts: the Mann-Whitney statistic
    with ties counted half, sum_k same[k] (2 (other pairs of a larger key) + other[k]) / (2 same other), the pairs of ``rest`` as one
    more bin behind the last -- they tie at the bottom.  Python integers, divided once; None when either class is empty.  What
    ``sklearn.metrics.roc_curve`` + ``auc`` give on the same scores."""
    same = [int(v) for v in hist[0]] + [int(rest[0])]
    other = [int(v) for v in hist[1]] + [int(rest[1])]
    n_same, n_other = sum(same), sum(other)
    if n_same == 0 or n_other == 0:
        return None
    above, total = n_other, 0
    for s, o in zip(same, other):
        above -= o
        total += s * (2 * above + o)
    return total / (2 * n_same * n_other)


def hist_best_f1(hist, rest):
    """(best F1, its bound) over the integer bounds 0 .. len - 1 of the two rows of counts: F1 of "keep the pairs of key <= b" as a
    call of "same family" = 2 kept_same / (kept_same + kept_other + same).  Compared as fractions of Python integers; ties to the
    lowest bound.  (None, None) without a pair of one family or without a bound."""
    n_same = int(sum(int(v) for v in hist[0])) + int(rest[0])
    if n_same == 0 or len(hist[0]) == 0:
        return None, None
    best_num, best_den, best_b, ks, ko = -1, 1, None, 0, 0
    for b, (s, o) in enumerate(zip(hist[0], hist[1])):
        ks, ko = ks + int(s), ko + int(o)
        num, den = 2 * ks, ks + ko + n_same
        if num * best_den > best_num * den:
            best_num, best_den, best_b = num, den, b
    return best_num / best_den, best_b


def _rate(num: int, den: int) -> str:
    return '%.4f' % (num / den) if den else '-'


class Histogram(FilteredPairs):
    """The distribution of one score over all pairs of a file (``--hist``), and with a family per protein what every cut-off would
    keep of the pairs of one family and of the pairs of two: the number that chooses the cut-off of every clustering mode.  The
    reference draws the one from the printed all-against-all (bench/G6PD/hist.py) and takes the ROC AUC of labelled pairs from it
    (bench/homo/results/AUC.py); here no pair is printed.  L1 is DCTdomain's (``score='domain'``: ``protein_min``) or DCTglobal's
    (``'global'``: ``l1_matrix`` of the last rows, the proteins without fingerprints flagged as on ``Tree``'s global route);
    bound = 16999, every pair of similarity above 0, unless ``min_cut`` gives a lower ``sim_bound(min_cut)``.  ``families``: one
    label per protein, of any hashable kind, or None.

    One pass over ``FilteredPairs.tile_pass``: ``tri_hist`` adds every entry right of the diagonal with key = min(L1, 17000) <= bound
    to ``hist[cls, key]`` on the device, cls = 0 without families, else (family of i != family of j).  No tile is held; ``hist``
    stays on the device and its bins 0 .. bound come back once -- 8 bytes per bin and class, whatever the size of the file.  The
    bin of similarity 0, where nearly all pairs of a large file land, is never counted on the device: the pairs above the bound
    (``rest``) follow from the totals the host knows, n (n - 1) / 2 pairs and sum s (s - 1) / 2 of one family over the family sizes
    s.  Fewer than two proteins or a bound below 0: no tile is filled and no kernel launched."""

    def __init__(self, sid, idx, fps, families=None, score: str = 'domain', min_cut=None):
        if score not in SCORES:
            raise ValueError(f'score must be one of {SCORES}')
        super().__init__(sid, idx, fps)
        bound = L1_FULL_SCALE - 1 if min_cut is None else min(sim_bound(min_cut), L1_FULL_SCALE - 1)
        self.score = self.route = score                         # (the tile of that score whatever the bound)
        self.min_cut = min_cut
        if score == 'domain':
            self.bound_domain = bound
        else:
            self.bound_global = bound
        self.fam = self.families = None
        if families is not None:
            self.fam, self.families = dense_families(families)
            if len(self.fam) != len(self.idx) - 1:
                raise ValueError('families must have one entry per protein')
        self._counts = None

    def totals(self):
        """The pairs of every class as Python integers: (n (n - 1) / 2,) without families, else (same, other)."""
        n = max(len(self.idx) - 1, 0)
        pairs = n * (n - 1) // 2
        if self.fam is None:
            return (pairs,)
        same = sum(int(s) * (int(s) - 1) // 2 for s in np.bincount(self.fam))
        return same, pairs - same

    def counts(self):
        """(hist, rest): ``hist`` uint64 (classes, bound + 1), the pairs of every key 0 .. bound -- one row without families, else the
        pairs of one family and the pairs of two --, and ``rest`` uint64 (classes), the pairs above the bound: similarity 0, no
        fingerprint, or below the cut-off.  Computed once."""
        if self._counts is None:
            hist = self._scan()
            rest = [t - int(hist[c].sum()) for c, t in enumerate(self.totals())]
            self._counts = hist, np.asarray(rest, dtype=np.uint64)
        return self._counts

    def _scan(self):
        n = len(self.idx) - 1
        classes = 1 if self.fam is None else 2
        if n < 2 or self.bound < 0:
            return np.zeros((classes, max(self.bound + 1, 0)), dtype=np.uint64)
        import torch
        dev = torch.device('cuda', torch.cuda.current_device())
        fam = torch.as_tensor(self.fam, device=dev) if self.fam is not None else None
        hist = torch.zeros((classes, L1_FULL_SCALE + 1), dtype=torch.int64, device=dev)
        rows = self.device_rows() if self.route == 'domain' else None
        for i0, tile, flags in self.tile_pass(rows):
            tri_hist(tile, i0, i0 + 1, self.bound, hist, fam, *flags)
            del tile
        return hist[:, :self.bound + 1].cpu().numpy().astype(np.uint64)     # one copy of 8 bytes per bin and class

    def table(self, bins: int = HIST_BINS):
        """(texts, kept): the cut-offs of ``hist_cuts(bins)`` that are not below ``min_cut`` -- the last, ``0.0000``, always -- and
        ``kept`` int64 (lines, classes), the pairs whose score is not below each: exactly the lines ``dct-sim --min-<score> <text>``
        prints.  A cut-off's bound is clipped to the instance's; the last keeps every pair."""
        hist, _rest = self.counts()
        below = np.concatenate([np.zeros((hist.shape[0], 1), dtype=np.int64), np.cumsum(hist.astype(np.int64), axis=1)], axis=1)
        texts, kept = [], []
        for b, (text, edge) in enumerate(zip(*hist_cuts(bins))):
            if b == bins - 1:
                kept.append(list(self.totals()))
            elif self.min_cut is not None and float(text) < self.min_cut:
                continue
            else:
                kept.append([int(v) for v in below[:, min(edge, self.bound) + 1]])
            texts.append(text)
        return texts, np.asarray(kept, dtype=np.int64).reshape(len(texts), hist.shape[0])

    def summary(self) -> dict:
        """From the counts at full resolution: ``pairs``; without families ``scored``, the pairs within the bound; with them
        ``same``, ``other``, ``roc_auc`` (``hist_roc_auc``), ``best_f1`` and ``at`` (``hist_best_f1``): ``at`` is the text
        ``'%.6f' % (1 - (b + 0.5) / 17000)``, halfway between two representable similarities, so ``sim_bound(float(at)) == b``
        whatever the rounding and ``--min-<score> <at>`` reproduces the best-F1 set (None without a bound)."""
        hist, rest = self.counts()
        totals = self.totals()
        if self.fam is None:
            return {'pairs': totals[0], 'scored': int(hist[0].sum())}
        f1, b = hist_best_f1(hist, rest)
        return {'pairs': sum(totals), 'same': totals[0], 'other': totals[1], 'roc_auc': hist_roc_auc(hist, rest), 'best_f1': f1,
                'at': None if b is None else '%.6f' % (1 - (b + 0.5) / L1_FULL_SCALE)}

    def lines(self, bins: int = HIST_BINS) -> list:
        """The text of ``--hist`` without its header: per cut-off of ``table(bins)`` one line -- ``cut-off pairs kept``, or with
        families ``cut-off same other kept-same kept-other recall precision fpr``, ``pairs`` / ``same`` / ``other`` being the
        pairs between this cut-off and the one before, the rates as ``%.4f`` and ``-`` where a denominator is 0 -- then the summary
        line ``# pairs=.. scored=..`` or ``# pairs=.. same=.. other=.. roc_auc=.. best_f1=.. at=..``."""
        texts, kept = self.table(bins)
        totals = self.totals()
        out, before = [], [0] * len(totals)
        for text, row in zip(texts, kept.tolist()):
            step = [k - p for k, p in zip(row, before)]
            if self.fam is None:
                out.append(f'{text} {step[0]} {row[0]}')
            else:
                out.append(f'{text} {step[0]} {step[1]} {row[0]} {row[1]} {_rate(row[0], totals[0])} {_rate(row[0], row[0] + row[1])} '
                           f'{_rate(row[1], totals[1])}')
            before = row
        s = self.summary()
        if self.fam is None:
            out.append(f'# pairs={s["pairs"]} scored={s["scored"]}')
        else:
            auc, f1 = ('%.4f' % s[k] if s[k] is not None else '-' for k in ('roc_auc', 'best_f1'))
            out.append(f'# pairs={s["pairs"]} same={s["same"]} other={s["other"]} roc_auc={auc} best_f1={f1} at={s["at"] or "-"}')
        return out

    def write(self, sink, bins: int = HIST_BINS):
        """Calls ``sink(memoryview)`` with the text (``lines``), once."""
        sink(memoryview(('\n'.join(self.lines(bins)) + '\n').encode('ascii')))


def domain_cluster_lines(sid, idx, labels, row_labels, chunk_bytes: int = 1 << 24):
    """The text of ``--cluster --level domain`` for given labels (``labels[r]`` = the representative row of fingerprint row r, -1
    for a row that is no node and prints nothing), as uint8 arrays of whole lines of about ``chunk_bytes`` each: one line
    ``"{id of the representative's protein} {id of the member's protein} {label of the representative} {label of the member}\n"``
    per node in the order of a stable sort of the nodes by label -- clusters by representative row, members by row, a
    representative's own line first.  ``row_labels`` = one string per row (``fingerprint_labels``).  Composed from the bytes of
    the ids and labels by index arithmetic, as ``cluster_lines``: no Python loop per line."""
    idx = np.asarray(idx, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    total = int(idx[-1]) if len(idx) else 0
    if len(labels) != total or len(row_labels) != total or len(sid) != len(idx) - 1:
        raise ValueError('one label and one name per fingerprint row, one id per protein')
    if total == 0:
        return
    if labels.min() < -1 or labels.max() >= total:
        raise IndexError('a label outside the rows of the file')
    nodes = np.flatnonzero(labels >= 0)
    member = nodes[np.argsort(labels[nodes], kind='stable')]
    rep = labels[member]
    if len(member) == 0:
        return
    if (labels[rep] != rep).any():
        raise IndexError('a representative that is no node of its own cluster')
    owner = np.repeat(np.arange(len(idx) - 1, dtype=np.int64), np.diff(idx))
    n_ids = len(idx) - 1
    yield from _field_lines(list(sid) + list(row_labels), [owner[rep], owner[member], n_ids + rep, n_ids + member], chunk_bytes)


class DomainClusters:
    """Domain families of one file at a DCTdomain cut-off (``--cluster --level domain``): single-linkage clusters whose nodes
    are the fingerprint ROWS.  Rows a < b are joined when they belong to different proteins, both are nodes and
    min(L1(a, b), 17000) <= ``sim_bound(min_domain)`` -- ``FilteredPairs``' survival rule on row pairs instead of protein minima.
    ``whole=False`` (``--no-whole``): the whole-protein row -- the last one -- of every protein of more than one fingerprint is no
    node (``make_db`` appends it only when there are several domains: a single-domain protein's only row stays in).
    ``labels()[r]`` = the smallest row of r's component, -1 for a row that is no node: a property of the graph, whatever the
    stripes, the groups or the order in which the device ran.

    The forest has one entry per row.  Stripes of at most STRIPE_ROWS rows run against the rows from the stripe's start onward,
    those in groups of at most COL_ROWS (``rows_link``: the pairs on or left of the diagonal are left out inside the kernel); the
    file stays on the device when it has at most COL_ROWS rows, else stripes and groups are uploaded as they come.  Nothing of
    size rows x rows exists anywhere: the distances never leave the registers.  Then ``cluster_labels`` and one copy of one int32
    per row.  A bound below 0 (a cut-off above 1): every node its own cluster, no launch.  There is no other shortcut: at a
    bound of 17 000 the rows of a file's only non-empty protein still stay apart.  Joining all rows of each protein on top of
    these components (with ``whole``) gives exactly ``Clusters(min_domain=...)``' proteins.

    ``labels`` (``fingerprint_labels`` of the file; default: the 1-based indices) = what ``write`` prints for each row."""

    COL_ROWS = 1 << 22      # fingerprints of a group on the device at a time (the whole file stays there if it fits)
    STRIPE_ROWS = 1 << 20   # rows of a stripe (dctfp_rows_link takes at most 8M per call)

    def __init__(self, sid, idx, fps, min_domain, whole: bool = True, labels=None):
        self.sid, self.idx, self.fps = sid, np.asarray(idx, dtype=np.int64), fps
        self.total = int(self.idx[-1]) if len(self.idx) else 0
        self.row_labels = labels if labels is not None else fingerprint_labels(sid, self.idx)
        if len(self.row_labels) != self.total:
            raise ValueError('labels must have one entry per fingerprint row')
        self.bound = sim_bound(min_domain)
        self.whole = bool(whole)

    def nodes(self) -> np.ndarray:
        """bool per row: is it a node."""
        keep = np.ones(self.total, dtype=bool)
        if not self.whole:
            counts = np.diff(self.idx)
            keep[self.idx[1:][counts > 1] - 1] = False
        return keep

    def labels(self) -> np.ndarray:
        total, keep = self.total, self.nodes()
        if total == 0 or self.bound < 0:
            return np.where(keep, np.arange(total), -1).astype(np.int32)
        import torch
        dev = torch.device('cuda', torch.cuda.current_device())
        parent = torch.arange(total, dtype=torch.int32, device=dev)
        owner = torch.as_tensor(np.repeat(np.arange(len(self.idx) - 1, dtype=np.int32), np.diff(self.idx)), device=dev)
        skip = None if keep.all() else torch.as_tensor((~keep).astype(np.uint8), device=dev)
        resident = to_device_int8(self.fps[:total]) if total <= self.COL_ROWS else None

        def rows(r0, r1):
            return resident[r0:r1] if resident is not None else to_device_int8(self.fps[r0:r1])

        for s0 in range(0, total, self.STRIPE_ROWS):
            s1 = min(total, s0 + self.STRIPE_ROWS)
            a = rows(s0, s1)
            for g0 in range(s0, total, self.COL_ROWS):
                g1 = min(total, g0 + self.COL_ROWS)
                rows_link(a, s0, a if (g0, g1) == (s0, s1) else rows(g0, g1), g0, owner, parent, self.bound, skip, cap=L1_FULL_SCALE)
        out = cluster_labels(parent).cpu().numpy()
        out[~keep] = -1
        return out

    def write(self, sink):
        """Calls ``sink(memoryview)`` with the text, whole lines at a time, in order."""
        for text in domain_cluster_lines(self.sid, self.idx, self.labels(), self.row_labels):
            sink(memoryview(text))


class Representatives(_ProteinClusters):
    """Greedy incremental clusters of one file at cut-offs, in file order, over the graph ``Clusters`` takes the components of
    (nodes: all proteins; edges: exactly ``FilteredPairs``' pairs):

        for x in 0 .. n - 1:  if no earlier representative has an edge to x, x is a representative;
                              else x belongs to the lowest representative it has an edge to.

    So every member is within the cut-offs of its representative and no two representatives are within them of each other --
    the representatives are the lexicographically first maximal independent set: a property of the graph, whatever the stripes,
    the column groups, the row ranges or the order in which the device ran.  A user who wants CD-HIT's "longest first" sorts the
    FASTA before ``make_db``.

    The nodes are decided on the device, range by range in ascending order (``GreedyState``: assign, state, blocked).  When a
    range [i0, i1) starts, every representative below i0 has marked all its columns; a cover pass makes members of the nodes
    they marked, then rounds of ``greedy_decide`` (a node without a stamp from an earlier undecided node of the range becomes a
    representative) and a mark launch (new representatives mark all their columns, undecided rows stamp their columns inside
    the range) until the range has no undecided node.  Only the count of those comes back, once per round.  A full row is walked
    once; the re-reads stay inside the range's diagonal block.  A path of k nodes inside one range takes about k rounds.

    - One cut-off excludes anything: the ranges are the stripes of ``FilteredPairs.tiles``, marked by ``greedy_tri_mark``.
    - Both do: the ranges are the rows of ``FilteredPairs.chunks``' pair lists, marked by ``greedy_pairs_mark``.
    - Neither does: all labels 0.  A bound below 0: every protein its own.  No tile.

    ``rounds`` = the rounds of the last ``labels()`` over all ranges.  The text is ``Clusters``': ``cluster_lines``."""

    rounds = 0

    def _decide_range(self, gs, i0: int, i1: int, mark):
        """Rounds over the nodes [i0, i1); ``mark(next_round)`` = the mark launch of the range's rows."""
        greedy_decide(gs, i0, i1, 0)
        if gs.left() == 0:                                      # (every node of the range belongs to an earlier representative)
            return
        mark(self._round)                                       # (all rows undecided: the stamps of the first round)
        while True:
            greedy_decide(gs, i0, i1, self._round)
            self._round += 1
            self.rounds += 1
            mark(self._round)                                   # (also after the last decide: its representatives mark)
            if gs.left() == 0:
                break
        self._round += 1

    def labels(self) -> np.ndarray:
        n = len(self.idx) - 1
        self.rounds = 0
        plain = self._plain_labels()
        if plain is not None:
            return plain
        gs = GreedyState(n)
        self._round = 1                                         # the next unused round number (0 = the cover pass, blocked starts as 0)
        done = 0                                                # every node below is decided and has marked
        if max(self.bound_domain, self.bound_global) < L1_FULL_SCALE:
            for pi, pj, *_ in self.chunks():
                i1 = int(pi[-1]) + 1                            # (i ascending: the rows of this list end here, and none of them comes again)
                self._decide_range(gs, done, i1, lambda nxt: greedy_pairs_mark(pi, pj, gs, i1, nxt))
                done = i1
        else:
            for i0, i1, tile, flags in self.tiles():
                self._decide_range(gs, i0, i1, lambda nxt: greedy_tri_mark(tile, i0, i0 + 1, self.bound, gs, i1, nxt, *flags))
                done = i1
                del tile
        greedy_decide(gs, done, n, self._round)                 # no later neighbour, no stamp of this round: whoever is not marked represents itself
        return gs.assign.cpu().numpy()


def _all_ids(rep_sid, sid):
    """The ids of the nodes of an assignment: the representatives' file, then the new one."""
    if isinstance(rep_sid, np.ndarray) and isinstance(sid, np.ndarray) and rep_sid.dtype.kind == sid.dtype.kind == 'U':
        return np.concatenate([rep_sid, sid])
    return [f'{s}' for s in rep_sid] + [f'{s}' for s in sid]


def assign_lines(rep_sid, sid, labels, chunk_bytes: int = 1 << 24):
    """The text of ``--assign`` for given labels (``Assignment.labels()``: one per protein of ``sid``, in the numbering
    0 .. m - 1 for ``rep_sid`` and m .. m + n - 1 for ``sid``): one line ``"{id of representative} {id of member}\n"`` per protein
    of ``sid`` and none for those of ``rep_sid``, in the order of a stable sort by label -- the clusters of the old representatives
    first, in their order, then the new representatives' clusters, each representative's own line first.  Composed as
    ``cluster_lines`` composes its text: no Python loop per line."""
    labels = np.asarray(labels, dtype=np.int64)
    m, n = len(rep_sid), len(sid)
    if len(labels) != n:
        raise ValueError('one label per new protein')
    if n == 0:
        return
    if labels.min() < 0 or labels.max() >= m + n:
        raise IndexError('a label outside the proteins of the two files')
    order = np.argsort(labels, kind='stable')
    yield from _id_lines(_all_ids(rep_sid, sid), labels[order], m + order, chunk_bytes)


class Assignment:
    """New proteins placed on an existing set of representatives (``--assign``): greedy incremental clustering that starts from
    a file ``R`` of m fixed representatives and goes through a file ``N`` of n new proteins.  Nodes are numbered 0 .. m - 1 for
    ``R`` and m .. m + n - 1 for ``N``, each file in its own order.  An edge joins a node of R u N to a LATER node of N exactly
    when ``FilteredPairs`` would keep that protein pair -- min(L1, 17000) <= ``sim_bound(cut-off)`` on the protein minimum for
    DCTdomain, on the last-row pair for DCTglobal, on both when both cut-offs are given.  There are no edges inside R: every
    protein of R is a representative, whatever its distance to the others.  Then ``Representatives``' rule over N in file order:

        a protein of N with an edge from a representative (of R, or an earlier new one) belongs to the lowest such node;
        otherwise it becomes a representative itself.

    So for any file F and split point k, with R = the greedy representatives among the first k proteins and N = the rest, the
    proteins of N get exactly the labels ``Representatives(F)`` gives them.  ``labels()`` = n int32 in the numbering above.

    The cover pass fills ``assign`` (m + n int32 on the device, ``GREEDY_NONE`` at the start) with the lowest node of R within the
    cut-offs of every new protein:
    - one cut-off excludes anything: ``rows_assign`` per (group of at most COL_ROWS representative rows, stripe of at most
      STRIPE_ROWS new rows) -- DCTdomain on all fingerprint rows with their proteins' nodes, DCTglobal on the last rows of the
      proteins that have fingerprints.  No distance is stored;
    - both do: per stripe of representatives the DCTglobal tile of the last rows (``l1_matrix``, at most TILE_INTS entries),
      ``tri_filter_count`` / ``tri_filter_fill`` with col0 = m (the whole rectangle lies right of the diagonal), ``pair_min_device``
      on the survivors, the DCTdomain bound, and an ``amin`` scatter of what is left.
    Nothing of size m x n exists anywhere.  The proteins of N still uncovered are then clustered among themselves by
    ``Representatives``, unchanged: covered proteins are members and influence nobody, so leaving them out is exact.

    A protein without fingerprints has no L1 against anything: in N it becomes its own representative, in R it covers nobody.
    A bound below 0 (a cut-off above 1): every new protein its own representative, no launch.  Bounds that exclude nothing (every
    given cut-off <= 0 or NaN): ``FilteredPairs`` keeps every pair, so every new protein belongs to node 0, as in ``Clusters`` and
    ``Representatives``."""

    COL_ROWS = 1 << 22      # representative rows on the device at a time (they all stay there if they fit)
    STRIPE_ROWS = 1 << 20   # new rows per call of rows_assign
    TILE_INTS = 1 << 28     # int32 entries of one DCTglobal tile (both cut-offs)

    def __init__(self, rep_sid, rep_idx, rep_fps, sid, idx, fps, min_domain=None, min_global=None):
        self.rep_sid, self.rep_idx, self.rep_fps = rep_sid, np.asarray(rep_idx, dtype=np.int64), rep_fps
        self.sid, self.idx, self.fps = sid, np.asarray(idx, dtype=np.int64), fps
        if min_domain is None and min_global is None:
            raise ValueError('an assignment needs a cut-off: min_domain, min_global or both')
        self.min_domain, self.min_global = min_domain, min_global
        self.bound_domain = L1_FULL_SCALE if min_domain is None else sim_bound(min_domain)
        self.bound_global = L1_FULL_SCALE if min_global is None else sim_bound(min_global)
        self.m, self.n = max(len(self.rep_idx) - 1, 0), max(len(self.idx) - 1, 0)
        if self.m and self.n and int(self.rep_idx[-1]) and int(self.idx[-1]) and rep_fps.shape[1] != fps.shape[1]:
            raise ValueError('the fingerprints of the two files differ in width')
        self.calls = 0          # rows_assign calls / tiles of the last labels()

    def _route_rows(self, fps, idx, node0: int):
        """(rows, node of every row) one file hands to ``rows_assign``: all rows on the DCTdomain route, the last rows of the
        proteins that have fingerprints on the DCTglobal route."""
        counts = np.diff(idx)
        if self.bound_global < L1_FULL_SCALE:
            has = np.flatnonzero(counts > 0)
            return fps[idx[1:][has] - 1], (node0 + has).astype(np.int32)
        return fps[:int(idx[-1])], (node0 + np.repeat(np.arange(len(counts), dtype=np.int64), counts)).astype(np.int32)

    def _cover_rows(self, assign):
        """One cut-off excludes anything: ``rows_assign`` per (group, stripe)."""
        import torch
        a, va = self._route_rows(self.rep_fps, self.rep_idx, 0)
        b, sb = self._route_rows(self.fps, self.idx, self.m)
        if len(a) == 0 or len(b) == 0:
            return
        bound = min(self.bound_domain, self.bound_global)
        dev = assign.device
        resident = to_device_int8(a) if len(a) <= self.COL_ROWS else None
        va_dev = torch.as_tensor(va, device=dev)
        for s0 in range(0, len(b), self.STRIPE_ROWS):
            s1 = min(len(b), s0 + self.STRIPE_ROWS)
            stripe, slots = to_device_int8(b[s0:s1]), torch.as_tensor(sb[s0:s1], device=dev)
            for g0 in range(0, len(a), self.COL_ROWS):
                g1 = min(len(a), g0 + self.COL_ROWS)
                group = resident[g0:g1] if resident is not None else to_device_int8(a[g0:g1])
                rows_assign(group, stripe, assign, bound, va_dev[g0:g1], slots, cap=L1_FULL_SCALE)
                self.calls += 1

    def _cover_pairs(self, assign):
        """Both cut-offs exclude something: DCTglobal tiles, the survivors' DCTdomain, an ``amin`` scatter."""
        import torch
        m, n, dev = self.m, self.n, assign.device
        if int(self.rep_idx[-1]) == 0 or int(self.idx[-1]) == 0:
            return
        last_a, empty_a = _last_rows(self.rep_fps[:int(self.rep_idx[-1])], self.rep_idx)
        last_b, empty_b = _last_rows(self.fps[:int(self.idx[-1])], self.idx)
        rows_a = _DeviceRows(self.rep_fps, self.rep_idx, self.COL_ROWS)
        rows_b = _DeviceRows(self.fps, self.idx, self.COL_ROWS)
        for q0, q1 in _protein_groups(self.idx, self.COL_ROWS):            # new proteins: their fingerprints fit on the device
            if self.idx[q1] == self.idx[q0]:
                continue
            b, idx_b = rows_b(q0, q1), torch.as_tensor(self.idx[q0:q1 + 1] - self.idx[q0], device=dev)
            lb, eb = to_device_int8(last_b[q0:q1]), torch.as_tensor(empty_b[q0:q1], device=dev)
            per = max(1, self.TILE_INTS // (q1 - q0))
            p0 = 0
            while p0 < m:                                                   # stripes of representatives: the tile and their rows fit
                by_rows = int(np.searchsorted(self.rep_idx, self.rep_idx[p0] + self.COL_ROWS, 'right')) - 1
                p1 = min(m, max(p0 + 1, min(p0 + per, by_rows)))
                if self.rep_idx[p1] > self.rep_idx[p0]:
                    tile = l1_matrix(to_device_int8(last_a[p0:p1]), lb)
                    ea = torch.as_tensor(empty_a[p0:p1], device=dev)
                    count = tri_filter_count(tile, p0, m + q0, self.bound_global, ea, eb)
                    total = int(count.sum())
                    self.calls += 1
                    if total:
                        pi, pj = tri_filter_fill(tile, p0, m + q0, self.bound_global, count, total, ea, eb)
                        idx_a = torch.as_tensor(self.rep_idx[p0:p1 + 1] - self.rep_idx[p0], device=dev)
                        pairs = torch.stack([pi - p0, pj - (m + q0)], dim=1).contiguous()
                        mn, _ = pair_min_device(rows_a(p0, p1), idx_a, b, idx_b, pairs)
                        keep = mn.clamp(max=L1_FULL_SCALE) <= self.bound_domain
                        assign.scatter_reduce_(0, pj[keep].long(), pi[keep], 'amin')
                    del tile
                p0 = p1

    def labels(self) -> np.ndarray:
        m, n = self.m, self.n
        self.calls = 0
        lo, hi = min(self.bound_domain, self.bound_global), max(self.bound_domain, self.bound_global)
        if n <= 0 or lo < 0:
            return (m + np.arange(max(n, 0))).astype(np.int32)
        if lo >= L1_FULL_SCALE:                                             # (every pair is kept: node 0 has an edge to every new protein)
            return np.zeros(n, dtype=np.int32)
        out = np.full(n, GREEDY_NONE, dtype=np.int32)
        if m:
            import torch
            assign = torch.full((m + n,), GREEDY_NONE, dtype=torch.int32, device=torch.device('cuda', torch.cuda.current_device()))
            if hi < L1_FULL_SCALE:
                self._cover_pairs(assign)
            else:
                self._cover_rows(assign)
            out = assign[m:].cpu().numpy()
        rest = np.flatnonzero(out == GREEDY_NONE)                           # the uncovered: clustered among themselves, in file order
        bare = np.diff(self.idx)[rest] == 0                                 # (no fingerprints, no edges: their own representatives)
        out[rest[bare]] = m + rest[bare]
        rest = rest[~bare]
        if len(rest):
            rows, sub_idx = _compact(self.fps, self.idx, rest)
            sub_sid = np.asarray(self.sid)[rest] if isinstance(self.sid, np.ndarray) else [self.sid[k] for k in rest.tolist()]
            sub = Representatives(sub_sid, sub_idx, rows, min_domain=self.min_domain, min_global=self.min_global).labels()
            out[rest] = m + rest[sub]
        return out.astype(np.int32)

    def write(self, sink, labels=None):
        """Calls ``sink(memoryview)`` with the text, whole lines at a time, in order."""
        for text in assign_lines(self.rep_sid, self.sid, self.labels() if labels is None else labels):
            sink(memoryview(text))


def _npz_dom(filename: str, rows: int):
    """The ``dom`` array of a ``-dct.npz`` (one name per fingerprint row), or None for a file that carries none."""
    with np.load(filename) as data:
        if 'dom' not in data.files:
            return None
        dom = np.asarray(data['dom'])
    if dom.ndim != 1 or len(dom) != rows:
        raise ValueError(f'{filename}: dom holds {dom.shape} names for {rows} fingerprint rows')
    return dom


def write_reps(path: str, parts):
    """``--reps-out``: a ``-dct.npz`` (``sid``, ``idx``, ``dct``; ``dom`` too when every part has one) of the chosen proteins of
    each part in turn, with their fingerprint rows.  ``parts`` = [(sid, idx, fps, dom or None, protein indices or None for all)].
    ``_load_npz`` reads it back; written to ``path`` exactly (no suffix is added)."""
    sids, counts, rows, doms = [], [], [], []
    width = 0
    for sid, idx, fps, dom, proteins in parts:
        idx = np.asarray(idx, dtype=np.int64)
        proteins = np.arange(len(idx) - 1) if proteins is None else np.asarray(proteins, dtype=np.int64)
        lens = idx[proteins + 1] - idx[proteins]
        take = np.repeat(idx[proteins] - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()), dtype=np.int64)
        sids.append(np.asarray(sid, dtype=str)[proteins] if len(proteins) else np.zeros(0, dtype='<U1'))
        counts.append(lens)
        rows.append(np.asarray(fps)[take] if len(take) else None)
        doms.append(None if dom is None else np.asarray(dom, dtype=str)[take])
        width = max(width, np.asarray(fps).shape[1] if np.asarray(fps).ndim == 2 else 0)
    rows = [r for r in rows if r is not None]
    out = {'sid': np.concatenate(sids) if sids else np.zeros(0, dtype='<U1'),
           'idx': np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64) if counts else np.zeros(1, dtype=np.int64)}
    if all(d is not None for d in doms) and doms:
        out['dom'] = np.concatenate(doms) if sum(len(d) for d in doms) else np.zeros(0, dtype='<U1')
    out['dct'] = np.concatenate(rows).astype(np.int8) if rows else np.zeros((0, width), dtype=np.int8)
    with open(path, 'wb') as fh:
        np.savez(fh, **out)
    print(f'representatives saved to {path} ({len(out["sid"])} proteins)')


def _add_hits(parts, t0: int, p0: int, off, key, col):
    """``threshold_select``'s hits of a tile -- query proteins from ``t0``, database proteins from ``p0`` -- each row's to the list
    of its query in ``parts``, the columns as database protein indices."""
    for r in range(len(off) - 1):
        s = slice(off[r], off[r + 1])
        parts[t0 + r].append((key[s], col[s] + p0))


class ProteinSearch:
    """A fingerprint database (the ``dct`` / ``idx`` arrays of a ``-dct.npz``) searched protein by protein the way db_search
    does (src/dct-sim.py:126-156), without the n_query x n_db block matrix:

    1. rank on the whole-protein fingerprints only: an int32 tile of L1 distances, query last rows x database last rows;
    2. select each query's printed hits on the GPU (``threshold_select``): key min(L1, 17000) ascending, ties to the lower
       database index, the first max(top, #(DCTglobal >= threshold));
    3. DCTdomain (``pair_min``) for the printed pairs only.

    ``rank='domain'`` ranks on DCTdomain instead: the tile of step 1 holds each (query, database protein) pair's minimum L1
    over all their fingerprints (``protein_min``, the group's fingerprints resident on the device), and steps 2 and 3 are
    the same -- the first max(top, #(DCTdomain >= threshold)), best DCTdomain first.

    The database goes to the device in protein groups of at most COL_ROWS fingerprints (a single group stays there between
    searches); the query side is tiled so that a distance tile holds at most TILE_INTS entries.  The groups' hit lists are
    merged per query (``merge_candidates``).  ``search`` returns, per query, (database protein indices, min L1, last L1); with
    ``domains=True`` also (row of the minimum within the query, within the database protein), -1 = none (step 3 through
    ``pair_argmin``)."""

    COL_ROWS = 1 << 22      # fingerprints of the database on the device at a time (2 GB of int8 at 480 columns)
    TILE_INTS = 1 << 28     # int32 entries of one distance tile (1 GiB)
    MAX_TILE_ROWS = 1 << 20  # (dctfp_l1_matrix takes at most 8M rows per call)

    def __init__(self, db_fps, db_idx):
        self.fps = db_fps
        self.idx = np.asarray(db_idx, dtype=np.int64)
        self.groups = list(_protein_groups(self.idx, self.COL_ROWS))
        self._resident = {}

    def _group(self, g: int, need_rows: bool):
        """(device fingerprints or None, prefix array, device last rows, empty flags) of database group g."""
        hit = self._resident.get(g)
        if hit is not None and (hit[0] is not None or not need_rows):
            return hit
        p0, p1 = self.groups[g]
        r0, r1 = self.idx[p0], self.idx[p1]
        sub_idx = self.idx[p0:p1 + 1] - r0
        last, empty = _last_rows(self.fps[r0:r1], sub_idx)
        rows = to_device_int8(self.fps[r0:r1]) if need_rows and r1 > r0 else None
        entry = (rows, sub_idx, to_device_int8(last), empty)
        if len(self.groups) == 1:
            self._resident[g] = entry
        return entry

    def tiles(self, a_fps, a_idx, route: str, bare: bool = True):
        """The walk over the rectangle A x database, A = the proteins of ``a_fps`` / ``a_idx``: yields, per database group and per
        tile of A, (t0, p0, tile, (row flags, column flags)) -- ``tile`` = device int32, proteins [t0, t1) of A x [p0, p1) of the
        database; the flags = ``_last_rows``' of the two sides (uint8, 1 = a protein without fingerprints).
        - ``route='global'``: the L1 of the two last rows (``l1_matrix``; a zero row where a protein has none: the flags say so), A
          in tiles of at most TILE_INTS entries and MAX_TILE_ROWS rows; A's last rows stay on the device when A has at most
          COL_ROWS proteins.
        - ``route='domain'``: the minimum over all fingerprint pairs (``protein_min``; 0x7fffffff where a protein has none), the
          fingerprints of A going up in chunks of at most COL_ROWS (a single chunk once), each in tiles of at most TILE_INTS
          entries.  ``bare=False`` leaves out the tiles whose database group or chunk of A has no fingerprint at all, which hold
          nothing else; ``search`` takes them, because a query's first ``top`` hits are printed whatever they score."""
        import torch
        aidx = np.asarray(a_idx, dtype=np.int64)
        na = len(aidx) - 1
        if route == 'global':
            a_last, a_empty = _last_rows(a_fps, aidx)
            a_dev = to_device_int8(a_last) if na <= self.COL_ROWS else None
            for g, (p0, p1) in enumerate(self.groups):
                _, _, last, empty = self._group(g, need_rows=False)
                per = int(min(self.MAX_TILE_ROWS, max(1, self.TILE_INTS // (p1 - p0))))
                for t0 in range(0, na, per):
                    t1 = min(na, t0 + per)
                    yield t0, p0, l1_matrix(a_dev[t0:t1] if a_dev is not None else a_last[t0:t1], last), (a_empty[t0:t1], empty)
            return
        if route != 'domain':
            raise ValueError(f'route must be one of {RANKS}')
        a_empty = (aidx[1:] == aidx[:-1]).astype(np.uint8)
        chunks = list(_protein_groups(aidx, self.COL_ROWS))
        resident = None
        for g, (p0, p1) in enumerate(self.groups):
            rows, sub_idx, _, empty = self._group(g, need_rows=True)
            if rows is None:                                    # (a group without fingerprints: every pair is empty)
                if not bare:
                    continue
                rows = torch.empty((0, self.fps.shape[1]), dtype=torch.int8, device=torch.cuda.current_device())
            per = int(max(1, self.TILE_INTS // (p1 - p0)))
            for c0, c1 in chunks:
                if not bare and aidx[c1] == aidx[c0]:
                    continue
                if resident is not None and resident[0] == c0:
                    a = resident[1]
                else:
                    a = to_device_int8(a_fps[aidx[c0]:aidx[c1]])
                    if len(chunks) == 1:
                        resident = (c0, a)
                for t0 in range(c0, c1, per):
                    t1 = min(c1, t0 + per)
                    yield t0, p0, protein_min(a, aidx[t0:t1 + 1] - aidx[c0], rows, sub_idx), (a_empty[t0:t1], empty)

    def moment_limit(self) -> int:
        """``rect_moments``' limit for tiles of this database: one above the largest L1 of two int8 fingerprints of its width."""
        return 255 * int(self.fps.shape[1]) + 1

    def search(self, query_fps, query_idx, top: int, threshold: float, rank: str = 'global', domains: bool = False, zscore: bool = False):
        """``zscore``: every tile also goes to ``rect_moments`` (the rows' side alone) before the selection, and each query's tuple
        ends with one more array -- the z-score of every printed hit (``zscore_of``; float64, NaN where undefined) in the query's
        background under the score of ``rank``."""
        if rank not in RANKS:
            raise ValueError(f'rank must be one of {RANKS}')
        top = int(top)
        qidx = np.asarray(query_idx, dtype=np.int64)
        nq, n_db = len(qidx) - 1, len(self.idx) - 1
        if nq == 0 or n_db == 0:
            return [(np.zeros(0, dtype=np.int64),) * (5 if domains else 3) + ((np.zeros(0, dtype=np.float64),) if zscore else ())
                    for _ in range(nq)]
        bound = sim_bound(threshold)
        top1 = max(top, 1)      # (top <= 0: the reference prints the threshold hits only -- trimmed after the merge)
        parts = [[] for _ in range(nq)]
        state = MomentState(nq, 0, cols=False) if zscore else None
        for t0, p0, tile, flags in self.tiles(query_fps, qidx, rank):
            if state is not None:
                rect_moments(tile, t0, p0, state, *flags, limit=self.moment_limit())
            _add_hits(parts, t0, p0, *threshold_select(tile, top1, bound, *flags))
            del tile
        merged = (merge_candidates(pq, top1, bound) for pq in parts)
        hits = [c if top >= 1 else c[k <= bound] for k, c in merged]
        del parts
        counts = np.array([len(h) for h in hits], dtype=np.int64)
        q_of = np.repeat(np.arange(nq, dtype=np.int64), counts)
        db_of = np.concatenate(hits).astype(np.int64) if nq else np.zeros(0, dtype=np.int64)
        scores = self._pair_scores(query_fps, qidx, q_of, db_of, domains)
        bounds = np.concatenate([[0], np.cumsum(counts)])
        if state is not None:
            # (a pair has an L1 when both proteins have a fingerprint; the hit's L1 under the ranking score is min / last)
            has_l1 = (self.idx[db_of + 1] > self.idx[db_of]) & (qidx[q_of + 1] > qidx[q_of])
            scores += (zscores_of(state.moments()[0], q_of, scores[0 if rank == 'domain' else 1], has_l1),)
        return [(db_of[a:b],) + tuple(v[a:b] for v in scores) for a, b in zip(bounds[:-1], bounds[1:])]

    def _pair_scores(self, query_fps, qidx, q_of, db_of, domains: bool = False):
        """(min, last) L1 of the pairs (query q_of[k], database protein db_of[k]): per database group, per chunk of queries.
        ``domains``: (min, last, arg_q, arg_db) through ``pair_argmin``."""
        out, score = _score_arrays(len(q_of), domains)
        for g, (p0, p1) in enumerate(self.groups):
            in_g = np.flatnonzero((db_of >= p0) & (db_of < p1))
            if len(in_g) == 0:
                continue
            rows, sub_idx, _, _ = self._group(g, need_rows=True)
            if rows is None:
                continue
            for c0, c1 in _protein_groups(qidx, self.COL_ROWS):
                sel = in_g[(q_of[in_g] >= c0) & (q_of[in_g] < c1)]
                if len(sel) == 0 or qidx[c1] == qidx[c0]:
                    continue
                qrows = to_device_int8(query_fps[qidx[c0]:qidx[c1]])
                pairs = np.stack([q_of[sel] - c0, db_of[sel] - p0], axis=1)
                for o, v in zip(out, score(qrows, qidx[c0:c1 + 1] - qidx[c0], rows, sub_idx, pairs)):
                    o[sel] = v
        return tuple(out)

    def _pair_row_best(self, query_fps, qidx, q_of, db_of):
        """(row_off, l1, arg) of ``pair_row_best`` for the pairs (query q_of[k], database protein db_of[k]), in ``_pair_scores``'
        chunks: per database group, per chunk of queries."""
        q_of, db_of = np.asarray(q_of, dtype=np.int64), np.asarray(db_of, dtype=np.int64)
        off = pair_row_offsets(qidx, self.idx, np.stack([q_of, db_of], axis=1))
        out = np.full(off[-1], 0x7fffffff, dtype=np.int64), np.full(off[-1], -1, dtype=np.int64)
        for g, (p0, p1) in enumerate(self.groups):
            in_g = np.flatnonzero((db_of >= p0) & (db_of < p1))
            if len(in_g) == 0:
                continue
            rows, sub_idx, _, _ = self._group(g, need_rows=True)
            if rows is None:
                continue
            for c0, c1 in _protein_groups(qidx, self.COL_ROWS):
                sel = in_g[(q_of[in_g] >= c0) & (q_of[in_g] < c1)]
                if len(sel) == 0 or qidx[c1] == qidx[c0]:
                    continue
                qrows = to_device_int8(query_fps[qidx[c0]:qidx[c1]])
                pairs = np.stack([q_of[sel] - c0, db_of[sel] - p0], axis=1)
                part_off, *parts = pair_row_best(qrows, qidx[c0:c1 + 1] - qidx[c0], rows, sub_idx, pairs)
                _scatter_rows(out, off, sel, part_off, parts)
        return (off,) + out

    def map_fields(self, query_fps, qidx, q_of, db_of, bound: int, labels, db_labels) -> list:
        """``map_field`` of the pairs (query q_of[k], database protein db_of[k]): rows matched within ``bound``, named by the two
        files' ``fingerprint_labels``."""
        qidx = np.asarray(qidx, dtype=np.int64)
        off, l1, arg = self._pair_row_best(query_fps, qidx, q_of, db_of)
        return _map_fields(off, l1, arg, bound, list(zip(np.asarray(q_of).tolist(), np.asarray(db_of).tolist())), labels, qidx, db_labels, self.idx)


class ReciprocalBest(ProteinSearch):
    """The reciprocal best hits of two files, A (``--dct``) and B (``--db``): the first-pass ortholog call.  key(a, b) =
    min(L1, 17000), L1 = the smallest L1 over all fingerprint pairs of the two proteins (``score='domain'``: ``protein_min``) or
    the L1 of their two last fingerprints (``'global'``: ``l1_matrix`` of the last rows, the proteins without fingerprints flagged:
    key 17000 against everything).  A pair is a hit when key <= bound; bound = 16999, every pair of similarity above 0, unless
    ``min_cut`` gives min(``sim_bound(min_cut)``, 16999) -- so a protein without fingerprints never has or is a hit.  best_b(a) = the
    hit of a that is smallest under the strict order (key, b), best_a(b) the same under (key, a): ties go to the lower index in
    the file, as ``db_search`` ranks.  (a, b) is a reciprocal best hit iff best_b(a) == b and best_a(b) == a: a property of the
    two files, whatever the tiles, the groups or the order in which the device ran.

    ``ProteinSearch``'s walk with B as the database: B in protein groups of at most COL_ROWS fingerprints, A in tiles of at most
    TILE_INTS entries (for ``'domain'`` the fingerprints of A go up in chunks of at most COL_ROWS).  Every tile goes straight to
    ``rect_best``, which keeps the best column of every row and the best row of every column in the same pass (``BestState``);
    merging across tiles and groups is the atomic minimum itself.  Nothing returns to the host before the end except the two
    arrays, 8 bytes per protein.  An empty side or a bound below 0 (a cut-off above 1): no hits, no device.

    ``best()`` = ``BestState.hits()``; ``pairs()`` = (a, b, key) of the reciprocal best hits, a ascending; ``lines`` / ``write`` =
    ``db_search``'s lines for them (both scores from ``_pair_scores``)."""

    def __init__(self, sid_a, idx_a, fps_a, sid_b, idx_b, fps_b, score: str = 'domain', min_cut=None):
        if score not in SCORES:
            raise ValueError(f'score must be one of {SCORES}')
        super().__init__(fps_b, idx_b)
        self.sid_a, self.idx_a, self.fps_a, self.sid_b = sid_a, np.asarray(idx_a, dtype=np.int64), fps_a, sid_b
        self.n_a, self.n_b = max(len(self.idx_a) - 1, 0), max(len(self.idx) - 1, 0)
        if max(self.n_a, self.n_b) >= 1 << 31:
            raise ValueError('reciprocal best hits take fewer than 2^31 proteins on a side')
        self.score = score
        self.bound = L1_FULL_SCALE - 1 if min_cut is None else min(sim_bound(min_cut), L1_FULL_SCALE - 1)
        self._best = None
        self.zscore, self._moments = False, None

    def with_zscore(self):
        """This job with z-scores: every tile of the pass also goes to ``rect_moments``, both sides -- the rows are the backgrounds of
        the proteins of A over file B, the columns those of B over A -- and ``lines`` / ``write`` append `` z_a z_b``.  To be called
        before the pass (``best``); returns the job."""
        if self._best is not None:
            raise ValueError('the pass has been made: ask for z-scores before best()')
        self.zscore = True
        return self

    def best(self):
        """((best_b, its key) per protein of A, (best_a, its key) per protein of B): int64 numpy arrays, -1 in both where a protein
        has no hit (built once)."""
        if self._best is None:
            if self.n_a == 0 or self.n_b == 0 or self.bound < 0:
                self._best = tuple((np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)) for n in (self.n_a, self.n_b))
            else:
                state = BestState(self.n_a, self.n_b)
                background = MomentState(self.n_a, self.n_b) if self.zscore else None
                for t0, p0, tile, flags in self.tiles(self.fps_a, self.idx_a, self.score, bare=False):
                    if background is not None:                      # (both sides of the same tile: rows = A over B, columns = B over A)
                        rect_moments(tile, t0, p0, background, *flags, limit=self.moment_limit())
                    # (the domain tile holds 0x7fffffff, key 17000, for a protein without fingerprints: no flags needed)
                    rect_best(tile, t0, p0, self.bound, state, *(flags if self.score == 'global' else ()), cap=L1_FULL_SCALE)
                    del tile
                self._best = state.hits()
                if background is not None:
                    self._moments = background.moments()
        return self._best

    def zscores(self, a, b, d):
        """(z_a, z_b) of the pairs (a[k], b[k]) with L1 ``d[k]`` under the score: its place in a's background over file B (the rows'
        side of the tiles) and in b's background over file A (the columns' side).  float64 arrays (``zscores_of``), NaN where undefined."""
        self.best()
        if self._moments is None:
            raise ValueError('no z-scores were asked for: with_zscore()')
        rows, cols = self._moments
        return zscores_of(rows, a, d), zscores_of(cols, b, d)

    def pairs(self):
        """(a, b, key): int64 numpy arrays of the reciprocal best hits, a ascending."""
        (best_b, key), (best_a, _) = self.best()
        a = np.flatnonzero(best_b >= 0)
        a = a[best_a[best_b[a]] == a]
        return a, best_b[a], key[a]

    def lines(self, domains: bool = False, labels=None, db_labels=None, min_z: float = None, map_l1: int = None) -> list:
        """``db_search``'s lines of the reciprocal best hits, in ascending order of a.  ``domains``: with the domain pair behind
        DCTdomain, named by ``labels`` / ``db_labels`` (``fingerprint_labels`` of the two files; default: the 1-based indices).
        ``map_l1`` (``map_bound``; implies ``domains``): then the domain map of the pair (``map_field``).  After
        ``with_zscore``: every line ends with `` z_a z_b`` (``zscores``), and ``min_z`` keeps the lines whose two z are defined and
        not below it."""
        a, b, _ = self.pairs()
        if len(a) == 0:
            return []
        domains = domains or map_l1 is not None
        mn, last, *args = self._pair_scores(self.fps_a, self.idx_a, a, b, domains)
        if domains:
            labels = labels if labels is not None else fingerprint_labels(self.sid_a, self.idx_a)
            db_labels = db_labels if db_labels is not None else fingerprint_labels(self.sid_b, self.idx)
        maps = self.map_fields(self.fps_a, self.idx_a, a, b, map_l1, labels, db_labels) if map_l1 is not None else None
        out = []
        z_a, z_b = self.zscores(a, b, mn if self.score == 'domain' else last) if self.zscore else (None, None)
        for k, (i, j, m, l) in enumerate(zip(a.tolist(), b.tolist(), mn, last)):
            maxs, s = _scores(m, l)
            tail = f' {_label(labels, self.idx_a[i], args[0][k])} {_label(db_labels, self.idx[j], args[1][k])}' if domains else ''
            if maps is not None:
                tail += f' {maps[k]}'
            if self.zscore:
                if min_z is not None and not _z_passes(min_z, z_a[k], z_b[k]):
                    continue
                tail += f' {zscore_text(z_a[k])} {zscore_text(z_b[k])}'
            out.append(f'{self.sid_a[i]} {self.sid_b[j]} {maxs} {s}{tail}')
        return out

    def write(self, report, domains: bool = False, labels=None, db_labels=None, min_z: float = None, map_l1: int = None):
        """One ``report.line`` per reciprocal best hit."""
        for text in self.lines(domains, labels, db_labels, min_z, **({'map_l1': map_l1} if map_l1 is not None else {})):
            report.line(text)


class Report:
    """Result lines to a file (header first) or to stdout."""

    def __init__(self, path: str = None, header: str = HEADER):
        self.path = path
        self.out = open(path, 'w', encoding='utf8') if path else sys.stdout
        self.line(header)

    def line(self, text: str):
        self.out.write(text + '\n')

    def raw(self, data):
        """UTF-8 bytes straight to the binary layer under the text one (flushed first, so that the order of everything written
        stays as it is); text for a stream without one (a ``StringIO``) or with another encoding."""
        buf = _utf8_binary(self.out)
        if buf is None:
            self.out.write(bytes(data).decode('utf8'))
            return
        self.out.flush()
        buf.write(data)

    def close(self):
        if self.path:
            self.out.close()
            print('results saved to', self.path)
        else:
            self.out.flush()


def _header(base: str, level: str = None, domains=False, domain_map=None) -> str:
    """The header of a report: ``base`` (HEADER, or CLUSTER_HEADER for the modes that print clusters) with the two columns of the
    domain pair where the lines carry them, and behind those the column of the domain map (``domain_map`` not None)."""
    if base == CLUSTER_HEADER:
        return DOMAIN_CLUSTER_HEADER if level == 'domain' else base
    if base == HEADER and domain_map is not None:
        return DOMAIN_HEADER + MAP_COLUMN
    return DOMAIN_HEADER if base == HEADER and domains else base


def _z_header(zscore, rbh: bool = False, rank: str = None) -> str:
    """What ``--zscore`` adds to the header, behind every other column: the z of the ranking score, or the two z of ``--rbh``."""
    return '' if not zscore else ' z-query z-db' if rbh else f' z-{rank or "global"}'


def _lines_header(kw: dict, rbh: bool = False) -> str:
    """The header of the modes that print pair lines, from the keyword arguments of the mode function: a call that asks for the domain
    pair carries the two extra column names, one that asks for the map its column, one that asks for z its (``rbh``: the two of ``--rbh``)."""
    return (_header(HEADER, None, any(kw.get(k) for k in ('domains', 'dom', 'db_dom')), kw.get('domain_map'))
            + _z_header(kw.get('zscore') or kw.get('min_z') is not None, rbh, kw.get('rank')))


def mode_header(name: str, kw: dict) -> str:
    """The header under which the mode function ``name`` prints when it is called with the keyword arguments ``kw``: the one place that
    knows it (the entry of ``_MODES``), for ``main`` and for a mode function that opens its own report."""
    return next(mode for mode in _MODES if mode.fn == name).header(kw)


@contextlib.contextmanager
def _opened(report, header: str):
    """The report argument of a mode function as an open ``Report``: itself if it is one (the caller closes it), else one opened here on
    that path (``None``: stdout) under ``header`` and closed on the way out."""
    if isinstance(report, Report):
        yield report
        return
    report = Report(report, header)
    try:
        yield report
    finally:
        report.close()


def _reporting(fn):
    """The mode functions keep the reference's signature -- the last positional argument may be an output path or ``None`` (stdout) --
    and also take an open ``Report``.  Keyword arguments (options beyond the reference's) pass through, and say under which header a
    report opened here prints (``mode_header`` of the function's name)."""
    def run(*args, **kw):
        *head, output = args
        with _opened(output, mode_header(fn.__name__, kw)) as report:
            return fn(*head, report, **kw)
    run.__doc__, run.__name__ = fn.__doc__, fn.__name__
    return run


@_reporting
def pair_sim(npzfile: str, pairfile: str, pairfound: str, report: Report, domains: bool = False, dom: str = None, domain_map=None):
    """Similarity of every listed protein pair (src/dct-sim.py:86-124).  Lines starting with ``#``
    are comments (copied to ``pairfound``); pairs with an unknown protein are counted, not printed.  ``domains`` / ``dom`` (the
    ``.dom`` of the npz): the best domain pair behind the scores.  ``domain_map`` (True, or the similarity X from which a row is
    matched: ``map_bound``; implies ``domains``): then the domain map of the pair (``map_field``)."""
    sid, idx, fps = _load_npz(npzfile)
    domains = domains or dom is not None or domain_map is not None
    labels = _labels_of(sid, idx, dom) if domains else None
    where = {name: i for i, name in enumerate(sid)}           # a repeated id: the later one, like a dict of arrays
    listed = 0
    kept, found = [], []
    with open(pairfile, encoding='utf8') as pairs:
        for text in pairs:
            if text.startswith('#'):
                kept.append(text)
                continue
            first, second = text.split()[:2]
            listed += 1
            if first not in where or second not in where:
                continue
            found.append((first, second, where[first], where[second]))
            kept.append(text)
    listed_pairs = [(i, j) for _, _, i, j in found]
    mn, last, *args = pair_scores(fps, idx, listed_pairs, domains=domains)
    maps = None
    if domain_map is not None:
        maps = _map_fields(*pair_row_bests(fps, idx, listed_pairs), map_bound(domain_map), listed_pairs, labels, idx, labels, idx)
    for k, ((first, second, i, j), m, l) in enumerate(zip(found, mn, last)):
        maxs, s = _scores(m, l)
        tail = f' {_label(labels, idx[i], args[0][k])} {_label(labels, idx[j], args[1][k])}' if domains else ''
        if maps is not None:
            tail += f' {maps[k]}'
        report.line(f'{first} {second} {maxs} {s}{tail}')
    print(f'total pair {pairfile} found {len(found)} (not found: {listed - len(found)})')
    if pairfound:
        with open(pairfound, 'w', encoding='utf8') as out:
            out.writelines(kept)
        print(f'pairs saved to file {pairfound}')


@_reporting
def db_search(npzfile: str, dbfile: str, top: int, threshold: float, report: Report, rank: str = 'global', domains: bool = False,
              dom: str = None, db_dom: str = None, zscore: bool = False, min_z: float = None, domain_map=None):
    """Hits of every query protein in a fingerprint database, best DCTglobal first (stable); the first
    ``top`` always, further ones while they reach ``threshold`` (src/dct-sim.py:126-156).  ``rank='domain'``: best
    DCTdomain first, and the threshold applies to DCTdomain (the same loop with the domain score as the key).  ``domains`` /
    ``dom`` / ``db_dom`` (the ``.dom`` files of the two npz): the best domain pair behind the scores of every printed hit.
    ``zscore``: one more field at the end of every line, the hit's z-score in the query's background over the database under the
    ranking score (``zscore_of``); ``min_z`` (implies ``zscore``) prints a selected line only if its z is defined and not below it.
    ``domain_map`` (as in ``pair_sim``; implies ``domains``): the domain map of every selected hit, before the z."""
    sid, idx, fps = _load_npz(npzfile)
    db_sid, db_idx, db_fps = _load_npz(dbfile)
    domains = domains or dom is not None or db_dom is not None or domain_map is not None
    zscore = zscore or min_z is not None
    if domains:
        labels, db_labels = _labels_of(sid, idx, dom), _labels_of(db_sid, db_idx, db_dom)
    search = ProteinSearch(db_fps, db_idx)
    hits = search.search(fps, idx, top, threshold, rank=rank, domains=domains, **({'zscore': True} if zscore else {}))
    maps = None
    if domain_map is not None:                                  # (the selected hits only, in the order of the lines)
        q_of = np.repeat(np.arange(len(hits), dtype=np.int64), [len(h[0]) for h in hits])
        db_of = np.concatenate([h[0] for h in hits]).astype(np.int64) if hits else np.zeros(0, dtype=np.int64)
        maps = iter(search.map_fields(fps, idx, q_of, db_of, map_bound(domain_map), labels, db_labels))
    for i, (query, (cols, mn, last, *args)) in enumerate(zip(sid, hits)):
        for k, (q, m, l) in enumerate(zip(cols, mn, last)):
            maxs, s = _scores(m, l)
            tail = f' {_label(labels, idx[i], args[0][k])} {_label(db_labels, db_idx[q], args[1][k])}' if domains else ''
            if maps is not None:
                tail += f' {next(maps)}'
            if zscore:
                if min_z is not None and not _z_passes(min_z, args[-1][k]):
                    continue
                tail += f' {zscore_text(args[-1][k])}'
            report.line(f'{query} {db_sid[q]} {maxs} {s}{tail}')


def _file_weights(npzfile: str, sid, idx, unit: str, dom: str = None) -> np.ndarray:
    """``coverage_weights`` of a file: residues from its ``.dom`` file (``dom``) if given, else from the ``dom`` array of the npz."""
    names = None
    if unit == 'residues':
        names = fingerprint_labels(sid, idx, read_dom_file(dom)) if dom else _npz_dom(npzfile, int(idx[-1]))
    return coverage_weights(sid, idx, names, unit)


@_reporting
def all_sim(npzfile: str, report: Report, min_domain: float = None, min_global: float = None, domains: bool = False, dom: str = None,
            min_coverage: float = None, cov_unit: str = 'residues', domain_map=None):
    """All-against-all, upper triangle (src/dct-sim.py:158-176), streamed from the device (``AllPairs``).  With ``min_domain`` /
    ``min_global``: only the pairs whose DCTdomain / DCTglobal is not below them (``FilteredPairs``).  ``domains`` / ``dom`` (the
    ``.dom`` of the npz): the best domain pair behind the scores -- ``FilteredPairs`` with or without cut-offs.  ``min_coverage``
    (with ``min_domain``): only the pairs that also cover that share of both proteins, in ``cov_unit`` -- residues (from ``dom``, else
    from the npz) or domains (``FilteredPairs``).  ``domain_map`` (True, or the similarity X from which a row is matched; implies
    ``domains``): then the domain map of every printed pair, composed on the device (``FilteredPairs.with_map``); without X the rows
    within ``min_domain`` are matched, where that is given (``map_bound``)."""
    sid, idx, fps = _load_npz(npzfile)
    domains = domains or dom is not None or domain_map is not None
    if min_domain is None and min_global is None and not domains and min_coverage is None:
        AllPairs(sid, idx, fps).write(report.raw)
    else:
        labels = _labels_of(sid, idx, dom) if domains else None
        weights = _file_weights(npzfile, sid, idx, cov_unit, dom) if min_coverage is not None else None
        job = FilteredPairs(sid, idx, fps, min_domain=min_domain, min_global=min_global, labels=labels, min_coverage=min_coverage,
                            weights=weights)
        if domain_map is not None:
            job.with_map(map_bound(domain_map, min_domain))
        job.write(report.raw)


@_reporting
def cluster_sim(npzfile: str, report: Report, min_domain: float = None, min_global: float = None, linkage: str = 'single',
                level: str = 'protein', whole: bool = True, dom: str = None, reps_out: str = None, min_coverage: float = None,
                cov_unit: str = 'residues', rep: str = 'first', min_neighbors: int = None):
    """Clusters at the cut-offs, one line ``representative member`` per protein: single linkage (``Clusters``) or, with
    ``linkage='greedy'``, greedy incremental clusters in file order (``Representatives``).  ``level='domain'``: the domain
    families instead (``DomainClusters``: single linkage at ``min_domain`` alone), one line ``representative member dom1 dom2``
    per fingerprint row -- ``whole=False`` without the whole-protein rows of multi-domain proteins, ``dom`` (the ``.dom`` of the
    npz) names the rows by their residue ranges.  ``reps_out`` (greedy linkage at protein level only): the representatives as a
    ``-dct.npz`` of their own (``write_reps``), which ``assign_sim`` takes as its fixed set.  ``min_coverage`` (protein level, with
    ``min_domain``): two proteins are joined only if the pair also covers that share of both, in ``cov_unit`` (``all_sim``); ``dom``
    then gives the residues.  ``rep='medoid'`` (single linkage at protein level): the first field of a line is the medoid of the
    member's cluster -- the member with the smallest summed distance to the others (``Clusters.medoids``) -- instead of the cluster's
    first member; the lines and their order stay.  ``reps_out`` then writes the medoids, in the order of the clusters' first members.
    ``min_neighbors`` (single linkage at protein level): density clusters instead (``DensityClusters``) -- only a protein with that
    many pairs within the cut-offs passes a link on; 1 changes nothing."""
    if min_domain is None and min_global is None:
        raise ValueError('clustering needs a cut-off: min_domain, min_global or both')
    if min_neighbors is not None and (linkage != 'single' or level != 'protein' or int(min_neighbors) != min_neighbors or min_neighbors < 1):
        raise ValueError('min_neighbors is an integer of at least 1 and thins the graph of single linkage at protein level: the greedy '
                         'rule names representatives another way, and the domain level has no protein tile')
    if rep not in REPS:
        raise ValueError(f'rep must be one of {REPS}')
    if rep == 'medoid' and (linkage != 'single' or level != 'protein'):
        raise ValueError('medoids name single-linkage clusters at protein level: every member of a greedy cluster is within the '
                         'cut-offs of its representative, which a medoid would not keep, and the domain level has no protein tile')
    if reps_out is not None and (level != 'protein' or (linkage != 'greedy' and rep != 'medoid')):
        raise ValueError('reps_out writes the representatives of greedy clusters at protein level')
    if linkage not in LINKAGES:
        raise ValueError(f'linkage must be one of {LINKAGES}')
    if level not in LEVELS:
        raise ValueError(f'level must be one of {LEVELS}')
    if level == 'domain':
        if min_domain is None or min_global is not None or linkage != 'single' or min_coverage is not None:
            raise ValueError('domain-level clusters are single-linkage clusters at min_domain alone')
        sid, idx, fps = _load_npz(npzfile)
        DomainClusters(sid, idx, fps, min_domain, whole=whole, labels=_labels_of(sid, idx, dom)).write(report.raw)
        return
    if not whole or (dom is not None and min_coverage is None):
        raise ValueError('whole applies to level="domain" only, and so does dom without min_coverage')
    sid, idx, fps = _load_npz(npzfile)
    if min_neighbors is not None:
        job = DensityClusters(sid, idx, fps, min_domain=min_domain, min_global=min_global, min_neighbors=min_neighbors)
    else:
        job = (Representatives if linkage == 'greedy' else Clusters)(sid, idx, fps, min_domain=min_domain, min_global=min_global)
    if min_coverage is not None:
        if min_domain is None:
            raise ValueError('min_coverage needs min_domain: it counts the fingerprints within that cut-off')
        job.with_coverage(min_coverage, _file_weights(npzfile, sid, idx, cov_unit, dom))
    if rep == 'medoid':
        medoid = job.medoids()
        labels = job.last_labels
    else:
        medoid, labels = None, job.labels()
    job.write(report.raw, labels, rep=medoid)
    if reps_out is not None:
        first = np.flatnonzero(labels == np.arange(len(labels)))      # one per cluster, in the order of the clusters' first members
        write_reps(reps_out, [(sid, idx, fps, _npz_dom(npzfile, int(idx[-1])), first if medoid is None else medoid[first])])


@_reporting
def assign_sim(npzfile: str, repfile: str, report: Report, min_domain: float = None, min_global: float = None, reps_out: str = None):
    """Places the proteins of ``npzfile`` on the representatives of ``repfile`` at the cut-offs (``Assignment``): one line
    ``representative member`` per protein of ``npzfile``.  ``reps_out``: all proteins of ``repfile`` followed by the new
    representatives, as a ``-dct.npz`` (``write_reps``) -- the fixed set of the next assignment."""
    if min_domain is None and min_global is None:
        raise ValueError('an assignment needs a cut-off: min_domain, min_global or both')
    rep_sid, rep_idx, rep_fps = _load_npz(repfile)
    sid, idx, fps = _load_npz(npzfile)
    job = Assignment(rep_sid, rep_idx, rep_fps, sid, idx, fps, min_domain=min_domain, min_global=min_global)
    labels = job.labels()
    job.write(report.raw, labels)
    if reps_out is not None:
        m = len(rep_idx) - 1
        write_reps(reps_out, [(rep_sid, rep_idx, rep_fps, _npz_dom(repfile, int(rep_idx[-1])), None),
                              (sid, idx, fps, _npz_dom(npzfile, int(idx[-1])), np.flatnonzero(labels == m + np.arange(len(labels))))])


def _cut_of(score: str, min_domain, min_global, what: str):
    """The cut-off of ``score`` for a mode that goes by one score; ValueError for another score or the other score's cut-off."""
    if score not in SCORES:
        raise ValueError(f'score must be one of {SCORES}')
    if (min_global if score == 'domain' else min_domain) is not None:
        raise ValueError(f'{what} by one score: only that score\'s cut-off applies')
    return min_domain if score == 'domain' else min_global


@_reporting
def tree_sim(npzfile: str, report: Report, score: str = 'domain', min_domain: float = None, min_global: float = None):
    """The single-linkage tree of the file (``Tree``) on DCTdomain (``score='domain'``) or DCTglobal (``'global'``): one all-against-all
    line per edge, most similar first.  ``min_domain`` / ``min_global``: the cut-off of that score below which no edge is taken
    (the forest then has a tree per cluster at that cut-off); the other score's cut-off is an error."""
    min_cut = _cut_of(score, min_domain, min_global, 'the tree orders the pairs')
    sid, idx, fps = _load_npz(npzfile)
    Tree(sid, idx, fps, score=score, min_cut=min_cut).write(report.raw)


@_reporting
def rbh_sim(npzfile: str, dbfile: str, report: Report, score: str = 'domain', min_domain: float = None, min_global: float = None,
            domains: bool = False, dom: str = None, db_dom: str = None, zscore: bool = False, min_z: float = None, domain_map=None):
    """The reciprocal best hits of the proteins of ``npzfile`` and ``dbfile`` (``ReciprocalBest``) on DCTdomain (``score='domain'``) or
    DCTglobal (``'global'``): one ``db_search`` line per pair, in the order of ``npzfile``.  ``min_domain`` / ``min_global``: the cut-off
    of that score below which a pair is no hit; the other score's cut-off is an error.  ``domains`` / ``dom`` / ``db_dom``: as in
    ``db_search``.  ``zscore``: two more fields at the end of every line, the pair's z-score in the background of the ``npzfile``
    protein over ``dbfile`` and in that of the ``dbfile`` protein over ``npzfile``, both under ``score``; ``min_z`` (implies
    ``zscore``) prints a pair only if both are defined and not below it.  ``domain_map``: as in ``all_sim``, before the two z."""
    min_cut = _cut_of(score, min_domain, min_global, 'reciprocal best hits are ranked')
    sid, idx, fps = _load_npz(npzfile)
    db_sid, db_idx, db_fps = _load_npz(dbfile)
    domains = domains or dom is not None or db_dom is not None or domain_map is not None
    labels, db_labels = (_labels_of(sid, idx, dom), _labels_of(db_sid, db_idx, db_dom)) if domains else (None, None)
    zscore = zscore or min_z is not None
    job = ReciprocalBest(sid, idx, fps, db_sid, db_idx, db_fps, score=score, min_cut=min_cut)
    if zscore:
        job.with_zscore()
    job.write(report, domains=domains, labels=labels, db_labels=db_labels, **({'min_z': min_z} if min_z is not None else {}),
              **({'map_l1': map_bound(domain_map, min_domain)} if domain_map is not None else {}))


def read_families(path: str, sid) -> list:
    """The family of every protein of ``sid`` from a file of ``id family`` lines, separated by whitespace (``--families``).  Blank
    lines and lines that start with ``#`` are skipped, ids that are not in ``sid`` ignored.  ValueError for a line that is not two
    fields, an id given twice with different families and an id of ``sid`` the file does not have (the first such id is named)."""
    wanted = {f'{s}' for s in sid}
    family = {}
    with open(path, encoding='utf8') as fh:
        for number, line in enumerate(fh, 1):
            fields = line.split()
            if not fields or fields[0].startswith('#'):
                continue
            if len(fields) != 2:
                raise ValueError(f'{path}, line {number}: a line is "id family", two fields separated by whitespace')
            name, fam = fields
            if name not in wanted:
                continue
            if family.setdefault(name, fam) != fam:
                raise ValueError(f'{path}, line {number}: {name} is given two families, {family[name]} and {fam}')
    for s in sid:
        if f'{s}' not in family:
            raise ValueError(f'{path} gives no family for {s}')
    return [family[f'{s}'] for s in sid]


def families_from_ids(sid, sep: str) -> list:
    """The family of every protein from its own id: the text after the first ``sep`` (``--family-sep``; the reference's CATH20
    ids, ``16vpA00|3.30.930.10`` with ``|``).  ValueError for an empty ``sep`` and for an id without it (the first is named)."""
    if not sep:
        raise ValueError('the separator between id and family is at least one character')
    out = []
    for s in sid:
        head, found, fam = f'{s}'.partition(sep)
        if not found:
            raise ValueError(f'the id {s} has no {sep!r}: no family can be read from it')
        out.append(fam)
    return out


@_reporting
def auc1_sim(npzfile: str, report: Report, score: str = 'domain', families: str = None, family_sep: str = None, min_domain: float = None,
             min_global: float = None):
    """AUC1 and the top-1 rates of a labelled file (``Auc1``) on DCTdomain (``score='domain'``) or DCTglobal (``'global'``): one line
    ``query family members tp auc1 first_fp fp_score`` per protein and a last line with the summary.  The families come from
    ``families`` (a file of ``id family`` lines: ``read_families``) or from the ids themselves (``family_sep``:
    ``families_from_ids``) -- exactly one of the two.  ``min_domain`` / ``min_global``: the cut-off of that score below which a
    pair is no hit; the other score's cut-off is an error."""
    min_cut = _cut_of(score, min_domain, min_global, 'the hits of a query are ranked')
    if (families is None) == (family_sep is None):
        raise ValueError('the families come from one place: families (a file) or family_sep (the ids themselves)')
    sid, idx, fps = _load_npz(npzfile)
    labels = read_families(families, sid) if families is not None else families_from_ids(sid, family_sep)
    Auc1(sid, idx, fps, labels, score=score, min_cut=min_cut).write(report.raw)


def hist_sim(npzfile: str, report: Report, score: str = 'domain', bins: int = HIST_BINS, families: str = None, family_sep: str = None,
             min_domain: float = None, min_global: float = None):
    """The distribution of DCTdomain (``score='domain'``) or DCTglobal (``'global'``) over all pairs of the file (``Histogram``): a
    header, one line per cut-off of the ``bins`` (1 .. 1000) and a summary line (``Histogram.lines``).  The families, if any, come
    from ``families`` (a file of ``id family`` lines: ``read_families``) or from the ids themselves (``family_sep``:
    ``families_from_ids``) -- at most one of the two; with them the pairs of one family and of two are counted apart.
    ``min_domain`` / ``min_global``: the cut-off of that score below which no pair is counted and no line printed but the last; the
    other score's cut-off is an error.  ``report``: an open ``Report``, or a path / None as for the other modes."""
    min_cut = _cut_of(score, min_domain, min_global, 'the histogram bins the pairs')
    if families is not None and family_sep is not None:
        raise ValueError('the families come from one place: families (a file) or family_sep (the ids themselves)')
    if not isinstance(bins, (int, np.integer)) or not 1 <= bins <= HIST_MAX_BINS:
        raise ValueError(f'bins is a number of cut-offs: 1 .. {HIST_MAX_BINS}')
    with _opened(report, mode_header('hist_sim', {'score': score, 'families': families, 'family_sep': family_sep})) as report:
        sid, idx, fps = _load_npz(npzfile)
        labels = read_families(families, sid) if families is not None else families_from_ids(sid, family_sep) if family_sep is not None else None
        Histogram(sid, idx, fps, labels, score=score, min_cut=min_cut).write(report.raw, bins)


def hac_sim(npzfile: str, report: Report, score: str = 'domain', method: str = 'average', min_domain: float = None, min_global: float = None,
            flat: bool = False, newick: str = None):
    """The average- (``method='average'``: UPGMA) or complete-linkage (``'complete'``) tree of the file (``Dendrogram``) on DCTdomain
    (``score='domain'``) or DCTglobal (``'global'``): a header and one line ``rep1 rep2 similarity size`` per merge, most similar
    first.  ``min_domain`` / ``min_global``: the cut-off of that score above which nothing merges; the other score's cut-off is an
    error.  ``flat`` (needs the cut-off): the clusters at the cut-off instead, as ``cluster_sim``'s ``representative member`` lines
    -- with complete linkage every pair inside a cluster is within the cut-off.  ``newick``: a file that gets the trees beside
    either output (``Dendrogram.newick``).  ``report``: an open ``Report``, or a path / None as for the other modes."""
    min_cut = _cut_of(score, min_domain, min_global, 'the linkage tree orders the pairs')
    if method not in HAC_METHODS:
        raise ValueError(f'method must be one of {HAC_METHODS}')
    if flat and min_cut is None:
        raise ValueError('flat clusters are the clusters at a cut-off: min_domain, or min_global with score="global"')
    with _opened(report, mode_header('hac_sim', {'flat': flat})) as report:
        sid, idx, fps = _load_npz(npzfile)
        tree = Dendrogram(sid, idx, fps, method=method, score=score, min_cut=min_cut)
        if flat:
            for part in cluster_lines(sid, tree.labels()):
                report.raw(memoryview(part))
        else:
            tree.write(report.raw)
        if newick is not None:
            with open(newick, 'w', encoding='utf8') as fh:
                fh.write(tree.newick())


RANKS = ('global', 'domain')
LINKAGES = ('single', 'greedy')
LEVELS = ('protein', 'domain')
REPS = ('first', 'medoid')


def _value(ns, flag: str):
    """The value of ``flag`` in the namespace; None where the namespace has no such key (the options added with ``argparse.SUPPRESS``)."""
    return getattr(ns, flag[2:].replace('-', '_'), None)


# the flags that are given when their value is true; every other one when it is not None
_SWITCHES = frozenset(('--pair', '--db', '--cluster', '--domains', '--no-whole', '--zscore', '--flat'))


def _given(ns, flag: str) -> bool:
    """Is ``flag`` on the command line, by its value in the namespace."""
    return bool(_value(ns, flag)) if flag in _SWITCHES else _value(ns, flag) is not None


# The conditions of a rule, each a function of the namespace: one of the flags is given, none of them is, the value of a flag is
# ``test`` or passes it, all of several conditions hold.
def _with(*flags):
    return lambda ns: any(_given(ns, flag) for flag in flags)


def _without(*flags):
    return lambda ns: not any(_given(ns, flag) for flag in flags)


def _when(flag: str, test):
    return lambda ns: test(_value(ns, flag)) if callable(test) else _value(ns, flag) == test


def _and(*conditions):
    return lambda ns: all(holds(ns) for holds in conditions)


_DOMAIN_LEVEL = _when('--level', 'domain')


def _needs_hac(does: str) -> tuple:
    return ((_without('--hac'), f'{{0}} {does}: it needs --hac'),)


def _of_db_hits(does: str) -> tuple:
    return ((_with('--pair'), f'{{0}} {does}: not with --pair'), (_with('--cluster'), f'{{0}} {does}: not with --cluster'),
            (_without('--db'), f'{{0}} {does}: it needs --db'))


def _reps_out_has_no_set(ns) -> bool:
    """--reps-out has three contexts: --assign, and --cluster at protein level with --linkage greedy or with --rep medoid."""
    clusters = _given(ns, '--cluster') and (_value(ns, '--linkage') == 'greedy' or _value(ns, '--rep') == 'medoid')
    return not _given(ns, '--assign') and not (clusters and not _DOMAIN_LEVEL(ns))


def _explains(ns) -> bool:
    """Do the result lines carry the domain pair: --domains, or what implies it -- --domain-map, --db-dom and --dom, except that beside
    --cluster with --min-coverage --dom gives the coverage its residues (no result lines to explain)."""
    weighs = _given(ns, '--min-coverage') and _given(ns, '--cluster')
    return _with('--domains', '--domain-map', '--db-dom')(ns) or (_given(ns, '--dom') and not weighs)


# The family options of --auc1 and --hist: none without either, and each the same text for both.
_FAMILY = ((_without('--auc1', '--hist'), '{0} says which family a protein belongs to, for --auc1 to judge the hits by: it needs --auc1'),)
_FAMILIES = ((_and(_with('--families'), _with('--family-sep')), '{0} takes the families from one place: --families or --family-sep, not both'),
             (_when('--family-sep', ''), '--family-sep is the text between id and family: at least one character'))
# (--rbh takes its own score's cut-off)
_ALL_ONLY = ((_and(_with('--pair', '--db'), _without('--rbh')), '{0} applies to all-against-all only, not to --pair or --db'),)

# flag -> its rules as rows (condition on the namespace, message), checked in this order when the flag is given; the message is formatted
# with the flag ({0}) and the namespace.  The options are checked in the order of the table, after the modes.
_OPTIONS = {
    '--method': _needs_hac('says which linkage the tree of --hac is built by'),
    '--flat': _needs_hac('prints the clusters of --hac at its cut-off') + (
        (lambda ns: getattr(ns, f'min_{ns.hac}') is None, '--flat prints the clusters at a cut-off: with --hac {hac} it needs --min-{hac}'),),
    '--newick': _needs_hac('writes the tree of --hac in Newick format'),
    '--bins': ((_without('--hist'), '--bins says how many cut-offs the table of --hist has: it needs --hist'),
               (_when('--bins', lambda bins: not 1 <= bins <= HIST_MAX_BINS), f'--bins is a number of cut-offs: 1 .. {HIST_MAX_BINS}')),
    '--families': _FAMILY,
    '--family-sep': _FAMILY,
    '--zscore': _of_db_hits('places every hit of a database search in the background of its query'),
    '--min-z': _of_db_hits('cuts the hits of a database search by their z-score'),
    '--reps-out': ((_reps_out_has_no_set, '--reps-out writes representatives: it needs --assign, or --cluster --linkage greedy at protein level'),),
    '--rank': ((lambda ns: _given(ns, '--pair') or not _given(ns, '--db'),
                '--rank applies to database search (--db) only, not to --pair or all-against-all'),),
    '--db-dom': ((_without('--db'), '--db-dom names the .dom file of --db: it needs --db'),),
    '--min-coverage': (
        (_with('--pair', '--db'), '--min-coverage applies to all-against-all only, not to --pair or --db'),
        (_DOMAIN_LEVEL, '--min-coverage is a share of a protein: not with --level domain, which joins single fingerprints'),
        (_without('--min-domain'), '--min-coverage counts the fingerprints within the DCTdomain cut-off: it needs --min-domain'),
        (_when('--min-coverage', lambda c: not 0 < c <= 1), '--min-coverage is a share of a protein: above 0 and at most 1')),
    '--cov-unit': ((_without('--min-coverage'), '--cov-unit says what --min-coverage counts: it needs --min-coverage'),),
    '--domain-map': (      # (True for the bare flag, else its X)
        (_with('--cluster'), '--domain-map lists the matched domain pairs behind a result line: not with --cluster'),
        (_when('--domain-map', lambda x: x is not True and not 0 < x <= 1),
         '--domain-map X is the similarity from which a domain is matched: above 0 and at most 1')),
    '--linkage': ((_without('--cluster'), '--linkage says how --cluster forms its clusters: it needs --cluster'),),
    '--level': ((_without('--cluster'), '--level says what --cluster clusters: it needs --cluster'),),
    '--no-whole': ((lambda ns: not _DOMAIN_LEVEL(ns),
                    '--no-whole leaves the whole-protein rows out of the domain families: it needs --level domain'),),
    '--rep': (
        (_without('--cluster'), '--rep says which member names a cluster: it needs --cluster'),
        (_DOMAIN_LEVEL, '--rep names clusters of proteins: not with --level domain, whose nodes are fingerprints with no protein tile to sum'),
        (_and(_when('--rep', 'medoid'), _when('--linkage', 'greedy')),
         '--rep medoid names single-linkage clusters: not with --linkage greedy, where every member is within the '
         'cut-offs of its representative -- a medoid would break that guarantee')),
    '--min-neighbors': (
        (_without('--cluster'), '--min-neighbors says how many neighbours a protein needs to pass a link of --cluster on: it needs --cluster'),
        (_when('--min-neighbors', lambda m: m < 1), '--min-neighbors is a number of neighbours: at least 1 (1 is plain single linkage)'),
        (_when('--linkage', 'greedy'), '--min-neighbors thins the graph of single linkage: not with --linkage greedy, which names its '
                                       'representatives by a rule of its own'),
        (_DOMAIN_LEVEL, '--min-neighbors counts the neighbours of a protein: not with --level domain, whose nodes are fingerprints')),
    '--cluster': (
        (lambda ns: _explains(ns) and not _DOMAIN_LEVEL(ns), '--domains (--dom, --db-dom) explains the scores of result lines: not with --cluster'),
        (_with('--pair', '--db'), '--cluster applies to all-against-all only, not to --pair or --db'),
        (_without('--min-domain', '--min-global'), '--cluster needs a cut-off: --min-domain, --min-global or both'),
        (_and(_DOMAIN_LEVEL, _without('--min-domain')), '--level domain joins fingerprints by their own L1: it needs --min-domain'),
        (_and(_DOMAIN_LEVEL, _with('--min-global')), '--level domain has no whole-protein score to cut: not with --min-global'),
        (_and(_DOMAIN_LEVEL, _when('--linkage', 'greedy')), '--level domain forms single-linkage clusters: not with --linkage greedy')),
    '--min-domain': _ALL_ONLY,
    '--min-global': _ALL_ONLY}


class _Mode(typing.NamedTuple):
    """A mode of dct-sim.  ``fn``: the name of its function, a module attribute looked up when it is called.  ``args``: the options
    that are its positional arguments before the report.  ``kw``: its keyword arguments -- name -> the default where the command line
    has no such option, or ``_IF_GIVEN`` for an argument that is passed only where it has; a mode that goes by a score gets ``score``.
    ``header``: the keyword arguments of a call -> the first line of its report.  ``flag``: what selects the mode (None: what is
    left, the all-against-all).  A mode with ``does`` (what it does, for the message) refuses every flag of ``names`` beside it but
    its own, those it ``takes`` and the flags of the modes before it in ``_MODES``, which have refused it by then; ``orders``: what
    its score does -- the other score's cut-off is then an error; ``needs``: rules as those of ``_OPTIONS``, checked between the two.
    ``adjust``: what the keyword arguments need beyond the table, done to them in place."""
    fn: str
    args: tuple
    kw: dict
    header: typing.Callable
    flag: str = None
    does: str = None
    orders: str = None
    takes: tuple = ()
    needs: tuple = ()
    names: tuple = None
    adjust: typing.Callable = None


# The order in which a mode names the flags it refuses: the first of them that is given is the one in the message.  --families,
# --family-sep and --bins are in no mode's "not with": their own "it needs" rule catches them later.
_NAMES = ('--pair', '--db', '--cluster', '--assign', '--tree', '--rank', '--linkage', '--level', '--no-whole', '--reps-out', '--domains', '--dom',
          '--db-dom', '--domain-map', '--min-coverage', '--cov-unit', '--rep', '--min-neighbors', '--zscore', '--min-z', '--auc1', '--hist',
          '--hac', '--method', '--flat', '--newick')
# --assign alone names the four flags of the domain pair before --linkage, --level and --no-whole (its messages are older than the order)
_PAIR_FLAGS = ('--domains', '--dom', '--db-dom', '--domain-map')
_ASSIGN_NAMES = tuple(flag for name in _NAMES if name not in _PAIR_FLAGS for flag in (_PAIR_FLAGS + (name,) if name == '--linkage' else (name,)))


def _cluster_kw(kw: dict):
    """``cluster_sim`` takes ``whole``, the opposite of --no-whole, and ``dom`` only where it names the rows of the domain level or gives
    --min-coverage its residues."""
    kw['whole'] = not kw.pop('no_whole')
    if kw['level'] != 'domain' and 'min_coverage' not in kw:
        kw['dom'] = None


_IF_GIVEN = object()
_CUTS = {'min_domain': None, 'min_global': None}
_PAIR_KW = {'domains': False, 'dom': None, 'domain_map': _IF_GIVEN}
_DB_KW = {**_PAIR_KW, 'db_dom': None, 'zscore': _IF_GIVEN, 'min_z': _IF_GIVEN}
_FAMILY_KW = {'families': None, 'family_sep': None}
_COVER_KW = {'min_coverage': _IF_GIVEN, 'cov_unit': _IF_GIVEN}
# an option that brings another argument with it: --min-z implies --zscore, --min-coverage counts residues unless --cov-unit says otherwise
_BRINGS = {'min_z': ('zscore', True), 'min_coverage': ('cov_unit', 'residues')}

# The modes, in the order in which the parser checks them and main looks for the one to run: the first that is given.
_MODES = (
    _Mode('rbh_sim', ('dct', 'db'), {**_CUTS, **_DB_KW}, lambda kw: _lines_header(kw, rbh=True),
          '--rbh', 'prints the reciprocal best hits of --dct and --db', 'ranks the hits', takes=('--db',) + _PAIR_FLAGS + ('--zscore', '--min-z'),
          needs=((_without('--db'), '--rbh compares the proteins of --dct with those of another file: it needs --db'),)),
    _Mode('tree_sim', ('dct',), _CUTS, lambda kw: HEADER, '--tree', 'prints the single-linkage tree of --dct', 'orders the pairs'),
    _Mode('assign_sim', ('dct', 'assign'), {**_CUTS, 'reps_out': None}, lambda kw: CLUSTER_HEADER,
          '--assign', 'places the proteins of --dct on a fixed set of representatives', takes=('--reps-out',), names=_ASSIGN_NAMES,
          needs=((_without('--min-domain', '--min-global'), '--assign needs a cut-off: --min-domain, --min-global or both'),)),
    _Mode('auc1_sim', ('dct',), {**_CUTS, **_FAMILY_KW}, lambda kw: AUC1_HEADER,
          '--auc1', 'measures the AUC1 and the top-1 rates of --dct', 'ranks the hits',
          needs=((_without('--families', '--family-sep'), '--auc1 needs the family of every protein: --families FILE or --family-sep C'),)
          + _FAMILIES),
    _Mode('hist_sim', ('dct',), {**_CUTS, **_FAMILY_KW, 'bins': HIST_BINS},
          lambda kw: hist_header(kw.get('score', 'domain'), kw.get('families') is not None or kw.get('family_sep') is not None),
          '--hist', 'bins the scores of all pairs of --dct', 'bins the pairs', needs=_FAMILIES),
    _Mode('hac_sim', ('dct',), {**_CUTS, 'method': 'average', 'flat': False, 'newick': None},
          lambda kw: CLUSTER_HEADER if kw.get('flat') else HAC_HEADER,
          '--hac', 'prints the average- or complete-linkage tree of --dct', 'orders the pairs', takes=('--method', '--flat', '--newick')),
    # (no "not with" of their own: the rules of the options refuse what does not go with them)
    _Mode('pair_sim', ('dct', 'pair', 'pairfound'), _PAIR_KW, _lines_header, '--pair'),
    _Mode('db_search', ('dct', 'db', 'top', 'threshold'), {'rank': 'global', **_DB_KW}, _lines_header, '--db'),
    _Mode('cluster_sim', ('dct',), {**_CUTS, 'linkage': 'single', 'level': 'protein', 'no_whole': False, 'dom': None, 'reps_out': _IF_GIVEN,
                                    **_COVER_KW, 'rep': _IF_GIVEN, 'min_neighbors': _IF_GIVEN},
          lambda kw: _header(CLUSTER_HEADER, kw.get('level')), '--cluster', adjust=_cluster_kw),
    _Mode('all_sim', ('dct',), {**_CUTS, **_PAIR_KW, **_COVER_KW}, _lines_header))
# mode flag -> the flags it refuses, in the order they are named
_REFUSED = {mode.flag: tuple(flag for flag in mode.names or _NAMES if flag != mode.flag and flag not in mode.takes
                             and flag not in [earlier.flag for earlier in _MODES[:at]])
            for at, mode in enumerate(_MODES) if mode.does}


def _call_of(mode: _Mode, ns) -> tuple:
    """(the positional arguments before the report, the keyword arguments) with which ``main`` calls the function of ``mode``."""
    kw = {}
    for name, default in mode.kw.items():
        value = getattr(ns, name, None)
        if value is not None or default is not _IF_GIVEN:
            kw[name] = default if value is None else value
    for name, (brought, default) in _BRINGS.items():
        if name in kw:
            kw.setdefault(brought, default)
    if mode.orders:
        kw['score'] = _value(ns, mode.flag)
    if mode.adjust:
        mode.adjust(kw)
    return tuple(getattr(ns, name) for name in mode.args), kw


class _Parser(argparse.ArgumentParser):
    """argparse's parser with the rules of dct-sim's command line, which are data: ``_MODES`` and ``_OPTIONS``.  After argparse's own
    checks, in this order:

    1. every mode of ``_MODES`` that is given and has a refusal list (``_REFUSED``, derived from what it takes), in the order of
       the table: the first refused flag that is given, in the mode's naming order; then the mode's own requirements; then, for a
       mode that goes by one score, the cut-off of the other score;
    2. every option of ``_OPTIONS`` that is given, in the order of the table: its rules, in their order;
    3. what the namespace of an accepted command line says beyond its own words: ``domains`` is True where the lines carry the
       domain pair (``_explains``), and ``--rep first``, the default, leaves the namespace of a command line without it.

    The first rule that fails ends the parse with its message.  What an option is for is in its help text (``build_parser``), why a
    rule holds in its message."""

    def _check(self, ns, flag, rules):
        for fails, message in rules:
            if fails(ns):
                self.error(message.format(flag, **vars(ns)))

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        for mode in _MODES:
            if not mode.does or not _given(ns, mode.flag):
                continue
            beside = [flag for flag in _REFUSED[mode.flag] if _given(ns, flag)]
            if beside:
                self.error(f'{mode.flag} {mode.does}: not with {beside[0]}')
            self._check(ns, mode.flag, mode.needs)
            score = _value(ns, mode.flag)
            other = {'domain': 'global', 'global': 'domain'}.get(score)
            if mode.orders and _given(ns, f'--min-{other}'):
                self.error(f'{mode.flag} {score} {mode.orders} by DCT{score}: its cut-off is --min-{score}, not --min-{other}')
        for flag, rules in _OPTIONS.items():
            if _given(ns, flag):
                self._check(ns, flag, rules)
        if _explains(ns):
            ns.domains = True
        if _value(ns, '--rep') == 'first':
            del ns.rep
        return ns, rest


def build_parser() -> argparse.ArgumentParser:
    ap = _Parser(description='protein similarity from DCT fingerprints (GPU L1)')
    ap.add_argument('--dct', required=True, help='fingerprints of the proteins to compare (-dct.npz)')
    ap.add_argument('--output', help='write the result lines here instead of stdout')
    ap.add_argument('--pair', help='file of protein pairs to score (two ids per line)')
    ap.add_argument('--pairfound', help='copy of --pair restricted to the pairs that were scored')
    ap.add_argument('--db', help='search every protein of --dct in this -dct.npz')
    ap.add_argument('--top', type=int, default=5, help='database search: hits always reported per query')
    ap.add_argument('--threshold', type=float, default=0.25,
                    help='database search: further hits down to this score (DCTglobal, or DCTdomain with --rank domain)')
    ap.add_argument('--rank', choices=RANKS, default=None,
                    help='database search: order hits by the whole-protein score (global, the default) or by the best '
                         'domain pair (domain)')
    ap.add_argument('--min-domain', type=float, default=None, metavar='X',
                    help='all-against-all: print a pair only if its DCTdomain is not below X')
    ap.add_argument('--min-global', type=float, default=None, metavar='Y',
                    help='all-against-all: print a pair only if its DCTglobal is not below Y (with --min-domain: both must hold)')
    ap.add_argument('--min-coverage', type=float, default=argparse.SUPPRESS, metavar='C',
                    help='with --min-domain, all-against-all or --cluster: keep a pair only if the fingerprints of each protein that '
                         'are within the cut-off of a fingerprint of the other cover at least the share C (above 0, at most 1) of '
                         'that protein -- of both proteins')
    ap.add_argument('--cov-unit', choices=COV_UNITS, default=argparse.SUPPRESS,
                    help='--min-coverage: count a protein\'s covered residues (the default: from the dom array of the npz, or from '
                         '--dom) or its covered domains')
    ap.add_argument('--cluster', action='store_true',
                    help='all-against-all with a cut-off: print single-linkage clusters (one "representative member" line per '
                         'protein) instead of the pairs')
    # (absent from the namespace unless given: a command line without them parses to what it always did)
    ap.add_argument('--domains', action='store_true', default=argparse.SUPPRESS,
                    help='add two fields to every result line: the fingerprint of each protein that DCTdomain came from (its '
                         '1-based index within the protein; "-" when no pair scores above 0)')
    ap.add_argument('--dom', metavar='FILE', default=argparse.SUPPRESS, help='the .dom file of --dct: print residue ranges instead of indices (implies --domains)')
    ap.add_argument('--db-dom', metavar='FILE', default=argparse.SUPPRESS, help='the .dom file of --db, likewise (implies --domains)')
    ap.add_argument('--domain-map', nargs='?', type=float, const=True, metavar='X', default=argparse.SUPPRESS,
                    help='add one more field behind dom1 dom2 (implies --domains): every fingerprint of prot1 that has a counterpart '
                         'in prot2, then after "/" every fingerprint of prot2 that has one in prot1, each as '
                         '"label=label of its nearest fingerprint in the other protein:similarity", joined by ";" ("-" when there is '
                         'none).  A fingerprint has a counterpart when that similarity is at least X (above 0, at most 1; default: '
                         f'--min-domain where given, else {MAP_SIMILARITY}) and above 0.  Not with --cluster')
    ap.add_argument('--linkage', choices=LINKAGES, default=argparse.SUPPRESS,
                    help='--cluster: single linkage (the default: connected components, the representative is the first protein of '
                         'the component) or greedy (in file order, a protein joins the first representative it is within the cut-off '
                         'of, else it becomes one: every member is within the cut-off of its representative)')
    ap.add_argument('--rep', choices=REPS, default=argparse.SUPPRESS,
                    help='--cluster (single linkage, protein level): what names a cluster in the first field -- its first protein in '
                         'the file (first, the default) or its medoid, the member with the smallest summed distance to the others, '
                         'ties to the first (medoid); the lines and their order stay.  With medoid, --reps-out FILE writes the '
                         'medoids as a -dct.npz (the REPS of a later --assign)')
    ap.add_argument('--min-neighbors', type=int, metavar='M', default=argparse.SUPPRESS,
                    help='--cluster (single linkage, protein level): density clusters -- only a protein with at least M pairs within '
                         'the cut-offs (a core) passes a link on, so a sparse bridge no longer chains two families; a protein with '
                         'fewer joins the cluster of its first core neighbour in the file, or stays alone if it has none.  1 is '
                         'plain single linkage')
    ap.add_argument('--level', choices=LEVELS, default=argparse.SUPPRESS,
                    help='--cluster: what is clustered -- the proteins (the default) or, with --min-domain, the fingerprints of '
                         'the file (domain: the domain families; one "representative member dom1 dom2" line per fingerprint, --dom '
                         'names them by residue ranges)')
    ap.add_argument('--no-whole', action='store_true', default=argparse.SUPPRESS,
                    help='--level domain: leave the whole-protein fingerprint of every multi-domain protein out')
    ap.add_argument('--assign', metavar='REPS', default=argparse.SUPPRESS,
                    help='with a cut-off: place the proteins of --dct on the representatives in this -dct.npz (all of its proteins are '
                         'representatives) -- one "representative member" line per protein of --dct; a protein within the cut-off of no '
                         'representative becomes a new one, in file order')
    ap.add_argument('--reps-out', metavar='FILE', default=argparse.SUPPRESS,
                    help='--assign: write the proteins of REPS followed by the new representatives as a -dct.npz; --cluster --linkage '
                         'greedy: write that run\'s representatives (the REPS of a later --assign)')
    ap.add_argument('--tree', nargs='?', choices=SCORES, const='domain', default=argparse.SUPPRESS,
                    help='print the single-linkage tree of the file instead of all pairs: the n - 1 all-against-all lines that join the '
                         'proteins most similar first, by DCTdomain (domain, the default) or DCTglobal (global) -- cut at any score they '
                         'give the clusters --cluster finds there; --min-domain X (--min-global Y with global) takes no pair below it')
    ap.add_argument('--hac', nargs='?', choices=SCORES, const='domain', default=argparse.SUPPRESS,
                    help='print the average- or complete-linkage tree of the file (--method) instead of all pairs: one "rep1 rep2 similarity '
                         'size" line per merge, most similar first, by DCTdomain (domain, the default) or DCTglobal (global); a cluster is '
                         'named by its first protein in the file.  --min-domain X (--min-global Y with global) merges nothing below it.  At '
                         f'most {HAC_MAX_PROTEINS} proteins: the dense matrix of the file stays on the GPU')
    ap.add_argument('--method', choices=HAC_METHODS, default=argparse.SUPPRESS,
                    help='--hac: average linkage (the default: UPGMA, the mean distance of the member pairs) or complete linkage (the '
                         'largest: every pair inside a cluster is then within the height at which it formed)')
    ap.add_argument('--flat', action='store_true', default=argparse.SUPPRESS,
                    help='--hac with a cut-off: print the clusters at the cut-off, one "representative member" line per protein as --cluster '
                         'does, instead of the merges')
    ap.add_argument('--newick', metavar='FILE', default=argparse.SUPPRESS,
                    help='--hac: also write the tree to FILE in Newick format, one tree per line for a forest, branch lengths in units of '
                         'distance (1 - similarity)')
    ap.add_argument('--rbh', nargs='?', choices=SCORES, const='domain', default=argparse.SUPPRESS,
                    help='with --db: print the reciprocal best hits of the two files instead of every query\'s hits -- the pairs in which '
                         'each protein is the other\'s best hit among the proteins of the other file, by DCTdomain (domain, the default) or '
                         'DCTglobal (global), ties to the lower index in the file; one database-search line per pair, in the order of '
                         '--dct.  A hit is a pair of similarity above 0, or with --min-domain X (--min-global Y with global) one not '
                         'below it; --top and --threshold do not apply.  If --db names the same file as --dct, every protein with a '
                         'fingerprint is its own best hit')
    ap.add_argument('--auc1', nargs='?', choices=SCORES, const='domain', default=argparse.SUPPRESS,
                    help='with --families or --family-sep: measure how well a score ranks the proteins of a labelled file instead of '
                         'printing pairs -- every protein is searched against the file by DCTdomain (domain, the default) or DCTglobal '
                         '(global), ties to the lower index in the file, and its AUC1 is the share of the other members of its family '
                         'ranked before the first hit of another family; one "query family members tp auc1 first_fp fp_score" line per '
                         'protein, then a line with the mean AUC1 and the top-1 rates.  A hit is a pair of similarity above 0, or with '
                         '--min-domain X (--min-global Y with global) one not below it')
    ap.add_argument('--families', metavar='FILE', default=argparse.SUPPRESS,
                    help='--auc1: the family of every protein of --dct, one "id family" line each (blank lines and # lines are '
                         'skipped, other ids ignored)')
    ap.add_argument('--family-sep', metavar='C', default=argparse.SUPPRESS,
                    help='--auc1: the family of a protein is the text after the first C in its own id (CATH20 ids: '
                         '16vpA00|3.30.930.10 with C = "|")')
    ap.add_argument('--hist', nargs='?', choices=SCORES, const='domain', default=argparse.SUPPRESS,
                    help='print the distribution of DCTdomain (domain, the default) or DCTglobal (global) over all pairs of the file '
                         'instead of the pairs: per cut-off of --bins the pairs that --min-domain X (--min-global Y with global) would '
                         'keep; with --families or --family-sep, the pairs of one family and of two apart, recall, precision and '
                         'false-positive rate per cut-off, and a last line with the ROC AUC and the cut-off of the best F1.  '
                         '--min-domain X (--min-global Y with global) leaves the cut-offs below it out')
    ap.add_argument('--bins', type=int, metavar='B', default=argparse.SUPPRESS,
                    help=f'--hist: the number of cut-offs of the table, (B - 1) / B down to 0 (default {HIST_BINS}, at most {HIST_MAX_BINS})')
    ap.add_argument('--zscore', action='store_true', default=argparse.SUPPRESS,
                    help='--db, with or without --rbh: add the z-score of every hit as the last field of its line -- (mean - L1) / sigma '
                         'of the hit\'s L1 among the L1s of the query against EVERY protein of --db under the ranking score (--rank; with '
                         '--rbh its score, and two fields: the pair among the hits of the --dct protein over --db, then among those of '
                         'the --db protein over --dct); positive = closer than the background, "-" where undefined (fewer than two '
                         'proteins to compare with, or all at one distance).  z is relative to the database searched; a query that is '
                         'itself in --db counts in its own background like any other protein')
    ap.add_argument('--min-z', type=float, metavar='Z', default=argparse.SUPPRESS,
                    help='--db: of the lines --top / --threshold (or --rbh) selected, print only those whose z-score is defined and not '
                         'below Z -- with --rbh both of them (implies --zscore)')
    return ap


def main(argv=None):
    t_start = time.time()
    args = build_parser().parse_args(argv)
    mode = next(mode for mode in _MODES if mode.flag is None or _given(args, mode.flag))
    head, kw = _call_of(mode, args)
    report = Report(args.output, mode.header(kw))
    t_work = time.time()
    globals()[mode.fn](*head, report, **kw)
    report.close()
    t_end = time.time()
    print(f'total time used {t_end - t_start:.1f}s')
    print(f'distance calculation used {t_end - t_work:.1f}s')


if __name__ == '__main__':
    main()
