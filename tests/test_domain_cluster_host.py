"""CPU-side checks of dct-sim --cluster --level domain: the numpy oracle (domain_cluster_rule.py, the GPU tests' reference) pinned
on the committed reference fixtures, the line composer, the command line, and the entry point in the libraries and the header."""

import ctypes
import os
import re

import numpy as np
import pytest

import cluster_rule as crule
import domain_cluster_rule as drule
import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {'G6PD': os.path.join(gu.GOLD, 'ref_fixtures', 'G6PD-dct.npz'), 'example': os.path.join(gu.GOLD, 'ref_fixtures', 'example-dct.npz'),
            'all': os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')}


def _load(path):
    with np.load(path) as data:
        return [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']


@pytest.fixture(scope='module')
def files():
    return {name: _load(path) for name, path in FIXTURES.items()}


# ---- the rule on the committed fixtures

@pytest.mark.parametrize('name', sorted(FIXTURES))
@pytest.mark.parametrize('cut', [0.3, 0.5, 0.8])
def test_row_components_project_to_the_protein_clusters(files, name, cut):
    """The invariant the rule gives for free: the row components with all rows of each protein joined, projected to proteins, are
    the single-linkage protein clusters at the same cut-off."""
    sid, idx, dct = files[name]
    label = drule.labels(dct, idx, cut)
    total = int(idx[-1])
    assert label.dtype == np.int32 and len(label) == total and (label >= 0).all()
    assert (label <= np.arange(total)).all() and (label[label] == label).all()
    assert np.array_equal(drule.project(label, idx), crule.labels(dct, idx, min_domain=cut)[0])


def test_pinned_counts_on_g6pd(files):
    sid, idx, dct = files['G6PD']
    assert (len(sid), int(idx[-1])) == (27, 221)
    assert drule.summary(drule.labels(dct, idx, 0.5)) == (67, 27)
    assert drule.summary(drule.labels(dct, idx, 0.8))[0] == 130
    kept = drule.labels(dct, idx, 0.5, whole=False)
    assert (kept < 0).sum() == 27 and np.array_equal(kept < 0, ~drule.nodes(idx, whole=False))
    assert drule.summary(kept)[0] == 63
    # ... where the protein level sees one cluster
    assert len(np.unique(crule.labels(dct, idx, min_domain=0.5)[0])) == 1


def test_the_rule_is_the_bound_of_sim_bound_on_row_pairs(files):
    from dctdomain_amd import dct_sim
    sid, idx, dct = files['example']
    l1 = drule.row_l1(dct)
    own = drule.owners(idx)
    for cut in (0.3, 0.5, 0.8, 1.0, 1.5, 0.0):
        a, b = drule.edges(dct, idx, cut)
        want = (np.minimum(l1, 17000) <= dct_sim.sim_bound(cut)) & (own[:, None] != own[None, :]) & np.triu(np.ones_like(l1, dtype=bool), 1)
        assert np.array_equal(np.stack(np.nonzero(want)), np.stack([a, b]))


def test_nodes_with_and_without_the_whole_protein_rows():
    from dctdomain_amd import dct_sim
    idx = np.array([0, 0, 1, 3, 10, 10, 11], dtype=np.int64)             # proteins of 0, 1, 2, 7, 0 and 1 rows
    sid = list('abcdef')
    fps = np.zeros((11, 480), dtype=np.int8)
    want = np.ones(11, dtype=bool)
    want[[2, 9]] = False
    assert np.array_equal(drule.nodes(idx, whole=False), want) and drule.nodes(idx).all()
    assert np.array_equal(dct_sim.DomainClusters(sid, idx, fps, 0.5, whole=False).nodes(), want)
    assert dct_sim.DomainClusters(sid, idx, fps, 0.5).nodes().all()
    # a cut-off above 1: every node its own cluster, without a device
    assert dct_sim.DomainClusters(sid, idx, fps, 1.5).labels().tolist() == list(range(11))
    got = dct_sim.DomainClusters(sid, idx, fps, 1.5, whole=False).labels()
    assert got.dtype == np.int32 and got.tolist() == [0, 1, -1, 3, 4, 5, 6, 7, 8, -1, 10]
    empty = dct_sim.DomainClusters(['a', 'b'], [0, 0, 0], fps[:0], 0.5)
    assert empty.labels().tolist() == [] and list(dct_sim.domain_cluster_lines(['a', 'b'], [0, 0, 0], [], [])) == []
    with pytest.raises(ValueError):
        dct_sim.DomainClusters(sid, idx, fps, 0.5, labels=['x'] * 10)


# ---- the text from given labels

def _loop_text(sid, idx, label, row_labels) -> bytes:
    """The lines, by a literal loop."""
    owner = []
    for p in range(len(idx) - 1):
        owner += [p] * int(idx[p + 1] - idx[p])
    out = []
    for rep in sorted(set(int(v) for v in label if v >= 0)):
        for r in range(len(label)):
            if label[r] == rep:
                out.append(f'{sid[owner[rep]]} {sid[owner[r]]} {row_labels[rep]} {row_labels[r]}\n'.encode('utf8'))
    return b''.join(out)


def _text(sid, idx, label, row_labels, **kw) -> bytes:
    from dctdomain_amd import dct_sim
    return b''.join(bytes(part) for part in dct_sim.domain_cluster_lines(sid, idx, label, row_labels, **kw))


def test_text_order_and_rows_that_are_no_nodes():
    sid = ['p0', 'p1', 'p2']
    idx = [0, 2, 2, 5]
    names = ['1', '2', '1', '2', '3']
    assert _text(sid, idx, [0, 1, 0, 1, 4], names) == b'p0 p0 1 1\np0 p2 1 1\np0 p0 2 2\np0 p2 2 2\np2 p2 3 3\n' == _loop_text(sid, idx, [0, 1, 0, 1, 4], names)
    assert _text(sid, idx, [0, -1, 0, 3, -1], names) == b'p0 p0 1 1\np0 p2 1 1\np2 p2 2 2\n'
    assert _text(sid, idx, [-1] * 5, names) == b''
    assert _text(sid, idx, [0, 1, 0, 1, 4], names) == drule.text(sid, idx, [0, 1, 0, 1, 4], names)


def test_text_with_non_ascii_long_ids_and_dom_labels():
    from dctdomain_amd import dct_sim
    sid = ['a', 'é', 'ß蛋', '😀' * 75, 'L' * 300, 'α' * 150, 'x|y.z', '']
    assert len(sid[0].encode()) == 1 and len(sid[3].encode('utf8')) == len(sid[4]) == len(sid[5].encode('utf8')) == 300
    rng = np.random.default_rng(5)
    counts = np.array([3, 1, 0, 4, 2, 7, 1, 2])
    idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(idx[-1])
    doms = {f'{s}': [f'{10 * k + 1}-{10 * k + 10}' for k in range(c - 1)] if c > 1 else ['1-9,20-α'] for s, c in zip(sid, counts)}
    by_dom = dct_sim.fingerprint_labels(sid, idx, doms)
    assert by_dom.count('whole') == int((counts > 1).sum()) and by_dom[0] == '1-10' and by_dom[3] == '1-9,20-α'
    by_index = dct_sim.fingerprint_labels(sid, idx)
    for trial in range(6):
        label = np.arange(total)
        for _ in range(trial * 5):                              # random merges, the smaller row on top
            a, b = rng.integers(0, total, size=2)
            la, lb = label[a], label[b]
            label[(label == la) | (label == lb)] = min(la, lb)
        if trial % 2:                                           # rows that are no nodes: members only (a representative stays)
            out = rng.random(total) < 0.3
            label[out & (label != np.arange(total))] = -1
        for names in (by_index, by_dom):
            want = _loop_text(sid, idx, label, names)
            assert want.count(b'\n') == int((label >= 0).sum())
            assert _text(sid, idx, label, names) == want == drule.text(sid, idx, label, names)
            for chunk in (1, 7, 300, 2000):                     # (whole lines however small the pieces)
                parts = [bytes(p) for p in dct_sim.domain_cluster_lines(sid, idx, label, names, chunk_bytes=chunk)]
                assert b''.join(parts) == want and all(p.endswith(b'\n') for p in parts) and len(parts) > 1


def test_text_rejects_labels_that_name_no_row():
    with pytest.raises(IndexError):
        _text(['a', 'b'], [0, 1, 2], [0, 2], ['1', '1'])
    with pytest.raises(IndexError):
        _text(['a', 'b'], [0, 1, 2], [-1, 0], ['1', '1'])      # the representative is no node
    with pytest.raises(ValueError):
        _text(['a', 'b'], [0, 1, 2], [0], ['1', '1'])


# ---- the command line

@pytest.mark.parametrize('argv,want', [
    (['--cluster', '--level', 'domain', '--min-domain', '0.5'], dict(level='domain', min_domain=0.5)),
    (['--cluster', '--level', 'domain', '--min-domain', '0.5', '--no-whole'], dict(level='domain', no_whole=True)),
    (['--cluster', '--level', 'domain', '--min-domain', '0.5', '--dom', 'x.dom'], dict(level='domain', dom='x.dom')),
    (['--cluster', '--level', 'domain', '--min-domain', '0.5', '--linkage', 'single'], dict(level='domain', linkage='single')),
    (['--cluster', '--level', 'protein', '--min-global', '0.5'], dict(level='protein', min_global=0.5)),
    (['--cluster', '--level', 'protein', '--min-domain', '0.5', '--linkage', 'greedy'], dict(level='protein', linkage='greedy')),
])
def test_parser_accepts(argv, want):
    from dctdomain_amd import dct_sim
    args = vars(dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv))
    assert args['cluster'] is True and all(args[k] == v for k, v in want.items())
    assert ('no_whole' in args) == ('--no-whole' in argv)


@pytest.mark.parametrize('argv,said', [
    (['--level', 'domain', '--min-domain', '0.5'], '--level says what --cluster clusters: it needs --cluster'),
    (['--level', 'protein'], '--level says what --cluster clusters: it needs --cluster'),
    (['--cluster', '--level', 'domain'], '--cluster needs a cut-off'),
    (['--cluster', '--level', 'domain', '--min-global', '0.5'], '--level domain joins fingerprints by their own L1: it needs --min-domain'),
    (['--cluster', '--level', 'domain', '--min-domain', '0.5', '--min-global', '0.5'], 'not with --min-global'),
    (['--cluster', '--level', 'domain', '--min-domain', '0.5', '--linkage', 'greedy'], 'not with --linkage greedy'),
    (['--cluster', '--min-domain', '0.5', '--no-whole'], '--no-whole'),
    (['--cluster', '--level', 'protein', '--min-domain', '0.5', '--no-whole'], 'it needs --level domain'),
    (['--min-domain', '0.5', '--no-whole'], 'it needs --level domain'),
    (['--cluster', '--min-domain', '0.5', '--dom', 'x.dom'], 'not with --cluster'),
    (['--cluster', '--min-domain', '0.5', '--domains'], 'not with --cluster'),
    (['--cluster', '--level', 'protein', '--min-domain', '0.5', '--dom', 'x.dom'], 'not with --cluster'),
    (['--cluster', '--level', 'domain', '--min-domain', '0.5', '--db', 'd.npz'], '--cluster applies to all-against-all only'),
    (['--cluster', '--level', 'rows', '--min-domain', '0.5'], 'invalid choice'),
])
def test_parser_rejects(argv, said, capsys):
    from dctdomain_amd import dct_sim
    with pytest.raises(SystemExit) as e:
        dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv)
    assert e.value.code == 2
    assert said in capsys.readouterr().err


@pytest.mark.parametrize('argv', [[], ['--min-domain', '0.5', '--output', 'o'], ['--pair', 'p', '--pairfound', 'f'],
                                  ['--db', 'd', '--rank', 'domain', '--top', '3', '--threshold', '0.4']])
def test_the_other_modes_parse_as_before(argv):
    from dctdomain_amd import dct_sim
    args = vars(dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv))
    assert set(args) == {'dct', 'output', 'pair', 'pairfound', 'db', 'top', 'threshold', 'rank', 'min_domain', 'min_global', 'cluster'}
    assert args['cluster'] is False


def test_cluster_sim_checks_its_keywords(tmp_path):
    import inspect
    from dctdomain_amd import dct_sim
    out = str(tmp_path / 'out.txt')
    npz = FIXTURES['example']
    for kw in (dict(level='domain'), dict(level='domain', min_global=0.5), dict(level='domain', min_domain=0.5, min_global=0.5),
               dict(level='domain', min_domain=0.5, linkage='greedy'), dict(level='rows', min_domain=0.5),
               dict(min_domain=0.5, whole=False), dict(min_domain=0.5, dom='x.dom')):
        with pytest.raises(ValueError):
            dct_sim.cluster_sim(npz, out, **kw)
    # a cut-off above 1 needs no device: the header, then every row its own cluster
    dct_sim.cluster_sim(npz, out, min_domain=1.5, level='domain')
    sid, idx, _ = _load(npz)
    names = dct_sim.fingerprint_labels(sid, idx)
    assert open(out, 'rb').read() == drule.HEADER + drule.text(sid, idx, np.arange(int(idx[-1])), names)
    assert dct_sim.DOMAIN_CLUSTER_HEADER.encode() + b'\n' == drule.HEADER
    assert list(inspect.signature(dct_sim.DomainClusters.__init__).parameters)[1:] == ['sid', 'idx', 'fps', 'min_domain', 'whole', 'labels']
    assert dct_sim.DomainClusters.STRIPE_ROWS > 0 and dct_sim.DomainClusters.COL_ROWS == dct_sim.FilteredPairs.COL_ROWS


# ---- the library

PARAMS = ('dctfp_ctx* ctx, const int8_t* a, int64_t na, int64_t lda, int64_t a0, const int8_t* b, int64_t nb, int64_t ldb, int64_t b0, '
          'int32_t d, const int32_t* owner, const uint8_t* skip, int32_t cap, int32_t bound, int32_t* parent, int64_t n_nodes, void* stream')


def test_library_exports_the_entry_point_and_header_documents_it():
    from dctdomain_amd import _lib
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    decl = re.search(r'int dctfp_rows_link\(([^;]*)\);', header)
    assert decl and ' '.join(decl.group(1).split()) == PARAMS
    # the comment right above the declaration says what the call extends and names its error codes
    doc = header[:decl.start()].rsplit('/*', 1)[1]
    flat = ' '.join(doc.split())
    assert '*/' in doc and 'DCTFP_ERR_LIMIT' in doc and 'DCTFP_ERR_INVALID' in doc
    assert 'dctfp_tri_link' in doc and 'dctfp_tri_filter_count' in doc and 'survival rule' in flat
    assert re.fullmatch(r'\s*', doc.split('*/', 1)[1]), 'the comment must sit right above the declaration'
    version = int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1))
    assert version >= 107                                       # (the parent commit's: 106)
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, 'dctfp_rows_link') and lib.dctfp_version() == version
    assert 'dctfp_rows_link' in _lib.EXPORTS
    fn = _lib._configure(ctypes.CDLL(_lib.LIB_PATH)).dctfp_rows_link
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 17 == len(PARAMS.split(','))
    launch = open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'launch.h')).read()
    assert 'void launch_rows_link(' in launch


def test_the_wrapper_is_public_and_carries_the_stated_signature():
    import inspect
    from dctdomain_amd import similarity
    assert list(inspect.signature(similarity.rows_link).parameters) == ['a', 'a0', 'b', 'b0', 'owner', 'parent', 'bound', 'skip', 'cap']
    assert inspect.signature(similarity.rows_link).parameters['cap'].default == 17000
