"""CPU-side checks of dct-sim --cluster: the numpy oracle (cluster_rule.py, the GPU tests' reference) pinned on the committed
reference golden, the host parts that need no GPU (the text from given labels, the trivial cases), the command line, and the
three entry points in the libraries and the header."""

import ctypes
import io
import os
import re

import numpy as np
import pytest

import cluster_rule as crule
import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NPZ = os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')


@pytest.fixture(scope='module')
def golden():
    with np.load(NPZ) as data:
        return [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64), data['dct']


# ---- the oracle on the reference's 139 proteins: (cut-offs) -> (clusters, largest, clusters with > 1 member, edges)

PINNED = [
    ({'min_domain': 0.1}, (9, 131, 1, 7237)),
    ({'min_global': 0.1}, (13, 127, 1, 7131)),
    ({'min_domain': 0.5}, (22, 20, 7, 973)),
    ({'min_global': 0.5}, (22, 20, 7, 962)),
    ({'min_domain': 0.9}, (120, 8, 7, 52)),
    ({'min_global': 0.9}, (121, 7, 7, 45)),
    ({'min_domain': 1.0}, (132, 4, 5, 10)),
    ({'min_global': 1.0}, (135, 2, 4, 4)),
]


@pytest.mark.parametrize('kw,want', PINNED)
def test_oracle_on_the_reference_golden(golden, kw, want):
    sid, idx, dct = golden
    label, edges = crule.labels(dct, idx, **kw)
    assert crule.summary(label) + (edges,) == want
    assert label.dtype == np.int32 and (label <= np.arange(139)).all() and (label[label] == label).all()
    # the same components from scipy's own routine
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    import all_sim_filter_rule as rule
    i, j, mn, last = rule.triangle_l1(dct, idx)
    keep = rule.kept(mn, last, **kw)
    k, comp = connected_components(coo_matrix((np.ones(keep.sum()), (i[keep], j[keep])), shape=(139, 139)), directed=False)
    assert k == want[0]
    first = np.full(k, 139)
    np.minimum.at(first, comp, np.arange(139))
    assert np.array_equal(first[comp], label)


# ---- the text from given labels

def _text(sid, labels, **kw) -> bytes:
    from dctdomain_amd import dct_sim
    return b''.join(bytes(part) for part in dct_sim.cluster_lines(sid, labels, **kw))


def test_text_order_singletons_and_the_stable_sort():
    sid = ['p0', 'p1', 'p2', 'p3', 'p4', 'p5']
    labels = [0, 1, 0, 3, 1, 0]
    assert _text(sid, labels) == b'p0 p0\np0 p2\np0 p5\np1 p1\np1 p4\np3 p3\n' == crule.text(sid, labels)
    assert _text(sid, np.arange(6)) == b''.join(f'p{k} p{k}\n'.encode() for k in range(6))
    assert _text(sid, np.zeros(6, dtype=np.int32)) == b''.join(f'p0 p{k}\n'.encode() for k in range(6))


def test_text_with_the_golden_ids_non_ascii_and_long_ones(golden):
    sid = list(golden[0][:40]) + ['é', 'ß蛋', '😀' * 75, 'L' * 300, 'α' * 150, '']
    assert len('😀'.encode('utf8')) * 75 == 300 and len(('α' * 150).encode('utf8')) == 300
    rng = np.random.default_rng(3)
    n = len(sid)
    for trial in range(6):
        labels = np.arange(n)
        for _ in range(trial * 12):                         # random merges, the smaller index on top
            a, b = rng.integers(0, n, size=2)
            la, lb = labels[a], labels[b]
            labels[(labels == la) | (labels == lb)] = min(la, lb)
        want = crule.text(sid, labels)
        assert _text(sid, labels) == want
        for chunk in (1, 7, 300, 1000):                      # (whole lines however small the pieces)
            from dctdomain_amd import dct_sim
            parts = [bytes(p) for p in dct_sim.cluster_lines(sid, labels, chunk_bytes=chunk)]
            assert b''.join(parts) == want and all(p.endswith(b'\n') for p in parts)
            assert len(parts) > 1 and (chunk < 300 or len(parts) < n)


def test_text_of_a_numpy_id_array_is_the_f_string_of_each(golden):
    with np.load(NPZ) as data:
        sid = data['sid']
    labels = np.arange(len(sid)) // 3 * 3
    assert _text(sid, labels) == crule.text([f'{s}' for s in sid], labels)


def _merged_labels(rng, n, merges):
    labels = np.arange(n)
    for _ in range(merges):                                  # random merges, the smaller index on top
        a, b = rng.integers(0, n, size=2)
        la, lb = labels[a], labels[b]
        labels[(labels == la) | (labels == lb)] = min(la, lb)
    return labels


@pytest.mark.parametrize('layout', ['plain', 'strided', 'swapped'])
def test_ascii_id_arrays_take_the_fixed_width_path_and_give_the_same_text(monkeypatch, layout):
    """What every ``-dct.npz`` of ASCII ids takes: a numpy unicode array, ids of differing lengths padded to one width.  An empty
    id, one at the full width, one with a NUL inside; whole lines at any chunk size; the same bytes as the general path (the ids
    as a list) and as the oracle -- and the fixed-width branch is the one that ran (or, for another byte order, did not)."""
    from dctdomain_amd import dct_sim
    rng = np.random.default_rng(21)
    alphabet = list('abcXYZ019_|.- ')
    ids = [''.join(rng.choice(alphabet, size=int(m))) for m in rng.integers(0, 24, size=500)]
    ids[3], ids[7], ids[11], ids[12] = '', 'W' * 40, 'in\0side', ' '
    sid = np.array(ids)
    assert sid.dtype == np.dtype('<U40') and [f'{s}' for s in sid] == ids
    if layout == 'strided':
        sid = np.repeat(sid, 2)[::2]
        assert not sid.flags['C_CONTIGUOUS'] and list(sid) == ids
    elif layout == 'swapped':
        sid = sid.astype(sid.dtype.newbyteorder())
        assert list(sid) == ids
    calls = []
    real = dct_sim._ascii_lines
    monkeypatch.setattr(dct_sim, '_ascii_lines', lambda *a: (calls.append(1), real(*a))[1])
    for merges in (0, 40, 300, 5000):
        labels = _merged_labels(rng, len(ids), merges)
        want = crule.text(ids, labels)
        for chunk in (1, 50, 83, 4096, 1 << 24):
            calls.clear()
            parts = [bytes(p) for p in dct_sim.cluster_lines(sid, labels, chunk_bytes=chunk)]
            assert (len(calls) == 1) == (layout != 'swapped')
            assert b''.join(parts) == want and all(p.endswith(b'\n') for p in parts)
            assert chunk > 4096 or len(parts) > 1
            calls.clear()
            assert b''.join(bytes(p) for p in dct_sim.cluster_lines(ids, labels, chunk_bytes=chunk)) == want and not calls
    # ids that are not all ASCII, or no unicode array, leave the branch alone
    for other in (np.array(ids[:20] + ['é']), np.array(ids[:20], dtype=object), np.array([s.encode() for s in ids[:20]])):
        calls.clear()
        labels = np.zeros(len(other), dtype=np.int64)
        got = b''.join(bytes(p) for p in dct_sim.cluster_lines(other, labels))
        assert got == crule.text([f'{s}' for s in other], labels) and not calls


def test_text_rejects_labels_that_name_no_protein():
    with pytest.raises(IndexError):
        _text(['a', 'b'], [0, 2])
    with pytest.raises(ValueError):
        _text(['a', 'b'], [0])


@pytest.mark.parametrize('n', [0, 1])
def test_no_protein_and_one_protein_need_no_device(tmp_path, n):
    from dctdomain_amd import dct_sim
    sid = ['only'][:n]
    idx = np.arange(n + 1, dtype=np.int64)
    fps = np.zeros((n, 480), dtype=np.int8)
    c = dct_sim.Clusters(sid, idx, fps, min_domain=0.5)
    labels = c.labels()
    assert labels.dtype == np.int32 and labels.tolist() == list(range(n))
    got = []
    c.write(lambda mv: got.append(bytes(mv)))
    assert b''.join(got) == b'only only\n' * n
    # ... and through the mode function: the header, then the lines
    path, out = str(tmp_path / 'x-dct.npz'), str(tmp_path / 'out.txt')
    np.savez(path, sid=np.array(sid, dtype='<U4'), idx=idx, dom=np.array(['1-9'] * n, dtype='<U3'), dct=fps)
    dct_sim.cluster_sim(path, out, min_global=0.9)
    assert open(out, 'rb').read() == crule.HEADER + b'only only\n' * n


def test_a_cut_off_above_one_gives_singletons_and_one_nothing_fails_one_cluster_without_a_tile(golden):
    from dctdomain_amd import dct_sim
    sid, idx, dct = golden
    for kw in ({'min_domain': 1.0001}, {'min_global': 1.5}, {'min_domain': 0.5, 'min_global': 1.0001}):
        assert np.array_equal(dct_sim.Clusters(sid, idx, dct, **kw).labels(), np.arange(139))
        assert np.array_equal(crule.labels(dct, idx, **kw)[0], np.arange(139))
    for kw in ({'min_domain': 0.0}, {'min_global': -1.0}, {'min_domain': float('nan'), 'min_global': 0.0}):
        assert not dct_sim.Clusters(sid, idx, dct, **kw).labels().any()
        assert not crule.labels(dct, idx, **kw)[0].any()


def test_clusters_shares_the_stripes_routes_and_bounds_of_the_filtered_pairs():
    import inspect
    from dctdomain_amd import dct_sim
    assert list(inspect.signature(dct_sim.Clusters.__init__).parameters)[1:] == ['sid', 'idx', 'fps', 'min_domain', 'min_global']
    c = dct_sim.Clusters(['a', 'b'], [0, 1, 2], np.zeros((2, 480), np.int8), min_domain=0.5, min_global=0.25)
    f = dct_sim.FilteredPairs(['a', 'b'], [0, 1, 2], np.zeros((2, 480), np.int8), min_domain=0.5, min_global=0.25)
    assert (c.bound_domain, c.bound_global, c.route) == (f.bound_domain, f.bound_global, f.route) == (8500, 12750, 'global')
    assert dct_sim.Clusters.stripes is dct_sim.FilteredPairs.stripes and dct_sim.Clusters.tiles is dct_sim.FilteredPairs.tiles
    assert dct_sim.Clusters.chunks is dct_sim.FilteredPairs.chunks


def test_report_header_is_an_argument_that_defaults_to_the_pair_header(monkeypatch):
    from dctdomain_amd import dct_sim
    for args, want in (((), dct_sim.HEADER), ((dct_sim.CLUSTER_HEADER,), '#representative member')):
        out = io.StringIO()
        monkeypatch.setattr(dct_sim.sys, 'stdout', out)
        dct_sim.Report(None, *args).close()
        assert out.getvalue() == want + '\n'
    assert dct_sim.HEADER == '#prot1 prot2 sim-domain sim-global'


# ---- the command line

@pytest.mark.parametrize('argv,want', [
    (['--cluster', '--min-domain', '0.5'], (0.5, None)),
    (['--min-global', '0.25', '--cluster'], (None, 0.25)),
    (['--cluster', '--min-domain', '0.1', '--min-global', '1', '--output', 'f.txt'], (0.1, 1.0)),
    (['--cluster', '--min-domain', 'nan'], None),
])
def test_parser_accepts_cluster_with_a_cut_off(argv, want):
    from dctdomain_amd import dct_sim
    args = dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv)
    assert args.cluster is True and not args.pair and not args.db
    if want is not None:
        assert (args.min_domain, args.min_global) == want


@pytest.mark.parametrize('argv,said', [
    (['--cluster'], '--cluster needs a cut-off'),
    (['--cluster', '--threshold', '0.5'], '--cluster needs a cut-off'),
    (['--cluster', '--pair', 'p.txt'], '--cluster applies to all-against-all only'),
    (['--cluster', '--db', 'd.npz'], '--cluster applies to all-against-all only'),
    (['--cluster', '--min-domain', '0.5', '--pair', 'p.txt'], '--cluster applies to all-against-all only'),
    (['--cluster', '--min-global', '0.5', '--db', 'd.npz'], '--cluster applies to all-against-all only'),
    (['--cluster', '--min-global', '0.5', '--db', 'd.npz', '--rank', 'domain'], '--cluster applies to all-against-all only'),
    (['--cluster', 'yes', '--min-domain', '0.5'], 'unrecognized arguments: yes'),
])
def test_parser_rejects(argv, said, capsys):
    from dctdomain_amd import dct_sim
    with pytest.raises(SystemExit) as e:
        dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv)
    assert e.value.code == 2
    assert said in capsys.readouterr().err


@pytest.mark.parametrize('argv,want', [
    ([], dict(pair=None, db=None, rank=None, min_domain=None, min_global=None, top=5, threshold=0.25, output=None, pairfound=None)),
    (['--min-domain', '0.5', '--output', 'o'], dict(pair=None, db=None, rank=None, min_domain=0.5, min_global=None, output='o')),
    (['--pair', 'p', '--pairfound', 'f'], dict(pair='p', pairfound='f', db=None, min_domain=None, min_global=None)),
    (['--db', 'd', '--rank', 'domain', '--top', '3', '--threshold', '0.4'], dict(db='d', rank='domain', top=3, threshold=0.4, pair=None)),
])
def test_the_other_modes_parse_as_before(argv, want):
    from dctdomain_amd import dct_sim
    args = vars(dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv))
    assert args.pop('cluster') is False
    assert args['dct'] == 'x.npz' and all(args[k] == v for k, v in want.items())
    assert set(args) == {'dct', 'output', 'pair', 'pairfound', 'db', 'top', 'threshold', 'rank', 'min_domain', 'min_global'}


def test_cluster_sim_needs_a_cut_off(tmp_path):
    from dctdomain_amd import dct_sim
    with pytest.raises(ValueError):
        dct_sim.cluster_sim(NPZ, str(tmp_path / 'out.txt'))


# ---- the library

@pytest.mark.parametrize('name,params', [
    ('dctfp_tri_link', 'dctfp_ctx* ctx, const int32_t* tile, int64_t n_rows, int64_t n_cols, int64_t ld, int64_t row0, int64_t col0, '
                       'const uint8_t* row_empty, const uint8_t* col_empty, int32_t cap, int32_t bound, int32_t* parent, int64_t n_nodes, '
                       'void* stream'),
    ('dctfp_link_pairs', 'dctfp_ctx* ctx, const int32_t* pi, const int32_t* pj, int64_t n_pairs, int32_t* parent, int64_t n_nodes, void* stream'),
    ('dctfp_cluster_labels', 'dctfp_ctx* ctx, int32_t* parent, int64_t n_nodes, int32_t* labels, void* stream'),
])
def test_library_exports_the_entry_points_and_header_documents_them(name, params):
    from dctdomain_amd import _lib
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    decl = re.search(r'int %s\(([^;]*)\);' % name, header)
    assert decl and ' '.join(decl.group(1).split()) == params
    # the comment right above the declaration says what the call extends and names its error code
    doc = header[:decl.start()].rsplit('/*', 1)[1]
    assert '*/' in doc and 'DCTFP_ERR_LIMIT' in doc and 'dctfp_tri_filter_count' in doc and 'survival rule' in ' '.join(doc.split())
    assert re.fullmatch(r'\s*', doc.split('*/', 1)[1]), 'the comment must sit right above the declaration'
    version = int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1))
    assert version >= 104
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, name)
        assert lib.dctfp_version() == version
    assert name in _lib.EXPORTS


def test_exports_match_the_header_and_carry_signatures():
    from dctdomain_amd import _lib
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        declared = sorted(set(re.findall(r'\b(dctfp_[a-z0-9_]+)\s*\(', fh.read())))
    assert sorted(_lib.EXPORTS) == declared
    lib = _lib._configure(ctypes.CDLL(_lib.LIB_PATH))
    sizes = {'dctfp_tri_link': 14, 'dctfp_link_pairs': 7, 'dctfp_cluster_labels': 5}
    for name, n_args in sizes.items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args


def test_new_unit_and_shared_header_are_part_of_the_build():
    import build_ext
    assert 'k_cluster.hip' in build_ext.UNITS and 'k_filter.hip' in build_ext.UNITS
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    shared = [h for h in build_ext.HEADERS if os.path.dirname(h) == csrc]
    # filter_quad is defined once, in a header both units include
    holders = [p for p in shared + [os.path.join(csrc, u) for u in build_ext.UNITS] if re.search(r'\bQuad filter_quad\(', open(p).read())]
    assert len(holders) == 1 and holders[0] in shared
    inc = '#include "%s"' % os.path.basename(holders[0])
    for unit in ('k_filter.hip', 'k_cluster.hip'):
        text = open(os.path.join(csrc, unit)).read()
        assert inc in text and 'filter_quad(' in text


def test_the_tile_description_is_defined_once_and_checked_in_one_place():
    """The ten values that describe an L1 tile are struct TriTile, in one header; the five kernels that scan a tile take the struct, not
    the list; the five exports check it with one function.  The forest's routines live in a header of their own, part of the build."""
    import build_ext
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    code = {}
    for name in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, name)) as fh:
            code[name] = '\n'.join(line.split('//', 1)[0] for line in fh.read().splitlines())
    holders = [name for name, text in code.items() if re.search(r'\bstruct TriTile\s*\{', text)]
    assert holders == ['tri_tile.hip.h'] and os.path.join(csrc, holders[0]) in build_ext.HEADERS
    # ... a header that holds nothing else, and no unit restates it under another name
    assert not re.search(r'__device__|__global__|\binline\b', code['tri_tile.hip.h'])
    assert set(re.findall(r'\bstruct (\w+Tile)\s*\{', '\n'.join(code.values()))) == {'TriTile'}
    for header in ('tri_walk.hip.h', 'band_walk.hip.h'):
        assert '#include "tri_tile.hip.h"' in code[header] and os.path.join(csrc, header) in build_ext.HEADERS
    assert 'struct TriTile;' in code['launch.h']
    kernels = {'k_filter.hip': ('tri_filter_count_kernel', 'tri_filter_fill_kernel'), 'k_cluster.hip': ('tri_link_kernel',),
               'k_greedy.hip': ('greedy_tri_mark_kernel',), 'k_tree.hip': ('tri_nearest_kernel',)}
    # (every unit that includes the header: sim_lines_kernel of k_search.hip has a row0 / col0 of its own and scans no such tile)
    assert sorted(kernels) == sorted(u for u in build_ext.UNITS if u.startswith('k_') and '#include "tri_walk.hip.h"' in code[u])
    for unit, names in kernels.items():
        heads = re.sub(r'\s+', ' ', ' '.join(re.findall(r'__global__[^{]*\{', code[unit])))
        assert not re.search(r'int64_t row0, int64_t col0', heads), unit
        for kernel in names:
            assert ' %s(const TriTile t, ' % kernel in heads, kernel
    host = code['dctfp_sim.hip']
    exports = ('dctfp_tri_filter_count', 'dctfp_tri_filter_fill', 'dctfp_tri_link', 'dctfp_greedy_tri_mark', 'dctfp_tri_nearest')
    assert host.count('check_tri_tile(') == 1 + len(exports) and 'static int check_tri_tile(const char* name, const TriTile& t)' in host
    for name in exports:
        body = host[host.index('\nint %s(' % name):host.index('DCTFP_GUARD("%s")' % name)]
        assert body.count('check_tri_tile("%s", t)' % name) == 1 and 'ld < n_cols' not in body, name
    assert sum('check_tri_tile(' in text for text in code.values()) == 1
    # the union-find is a header both users include, the last of build_ext.HEADERS (kernel_sources() covers it)
    assert build_ext.HEADERS[-1] == os.path.join(csrc, 'union_find.hip.h') and build_ext.HEADERS[-1] in build_ext.kernel_sources()
    assert sum(bool(re.search(r'\bint32_t uf_find\(', text)) for text in code.values()) == 1 and 'uf_find(' in code['union_find.hip.h']
    for unit in ('k_cluster.hip', 'k_tree.hip'):
        assert '#include "union_find.hip.h"' in code[unit] and 'DCTFP_UNION_FIND_ONLY' not in code[unit]


def test_the_band_walk_is_defined_once_and_five_kernels_are_passes_of_it():
    """The five kernels that reduce a band of rows of a tile of a triangle onto per-protein arrays (label_sums, tri_degree,
    tri_link_core, tri_first_fp, tri_tp_before) are passes of ONE function template, band_walk, in a header of its own.  rect_best_kernel
    is exempt by name -- it keeps a loop of its own over the same TriTile, constants and grid, because it measured slower as a pass
    (the reason is written at the kernel and in profiles/band_walk/README.md).  What makes the walk right is asserted here, once; what a
    pass does with its arrays is asserted beside its unit (test_rbh_host.py, test_medoid_host.py, test_density_host.py,
    test_auc1_host.py).  The five exports over a triangle check the tile with one function."""
    import build_ext
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    code = {}
    for name in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, name)) as fh:
            code[name] = '\n'.join(line.split('//', 1)[0] for line in fh.read().splitlines())
    walk = code['band_walk.hip.h']
    assert os.path.join(csrc, 'band_walk.hip.h') in build_ext.HEADERS and os.path.join(csrc, 'band_walk.hip.h') in build_ext.kernel_sources()
    kernels = {'k_best.hip': ('rect_best_kernel',), 'k_medoid.hip': ('label_sums_kernel',), 'k_density.hip': ('tri_degree_kernel', 'tri_link_core_kernel'),
               'k_auc.hip': ('tri_first_fp_kernel', 'tri_tp_before_kernel')}
    exempt = {'k_best.hip': 'rect_best_kernel'}     # (keeps a loop of its own: the reason is at the kernel and in profiles/band_walk/README.md)
    assert sorted(kernels) == sorted(u for u in build_ext.UNITS if '#include "band_walk.hip.h"' in code[u])
    for unit, names in kernels.items():
        heads = re.sub(r'\s+', ' ', ' '.join(re.findall(r'__global__[^{]*\{', code[unit])))
        assert not re.search(r'int64_t row0, int64_t col0', code[unit]), unit
        on_walk = [k for k in names if k != exempt.get(unit)]
        assert len(re.findall(r'__global__', code[unit])) == len(names) and code[unit].count('band_walk(t, n_bands, n_steps, ') == len(on_walk)
        for kernel in names:
            assert ' %s(const TriTile t, ' % kernel in heads and '__launch_bounds__(kBandThreads)' in heads, kernel
        # a unit has no loop, no LDS and no constants of the walk of its own
        assert unit in exempt or not re.search(r'\bfor\b|\bwhile\b|__shared__|__syncthreads|__ballot|__shfl|= 256|= 64\b', code[unit]), unit
        assert code[unit].count('band_grid(t)') == len(names) and 'n_cols +' not in code[unit], unit
    # the skeleton -- rows of a band, a word of s_row per (row, wave) -- occurs in one file
    assert [name for name, text in code.items() if 's_row[tid >> 2][tid & 3]' in text] == ['band_walk.hip.h']
    assert [name for name, text in code.items() if 'rows = (int)min((int64_t)kBandRows, t.n_rows - r_lo)' in text] == ['band_walk.hip.h'] + sorted(exempt)
    for unit, kernel in exempt.items():
        assert 'EXEMPT from band_walk by name' in open(os.path.join(csrc, unit)).read() and kernel in open(os.path.join(ROOT, 'profiles', 'band_walk', 'README.md')).read()
    assert len(re.findall(r'template <class Pass>', walk)) == 1 and 'void band_walk(const TriTile& t, int64_t n_bands, int64_t n_steps, const Pass& pass)' in walk
    for constant in ('kBandThreads = 256;', 'kBandWaves = kBandThreads / 64;', 'kBandPer = 4;', 'kBandStep = kBandThreads * kBandPer;', 'kBandRows = 64;'):
        assert walk.count('constexpr int ' + constant) == 1, constant
    assert walk.count('static_assert(') == 2 and 'kBandRows * kBandWaves == kBandThreads' in walk and 'kBandStep == 1 << 10 && kBandRows == 1 << 6' in walk
    assert '(int64_t)1 << 20' in walk and "flagged || x >= cap ? cap : x" in walk
    for name in ('lower_hit', 'hit_word', 'key_of', 'band_grid'):
        assert sum(bool(re.search(r'\b%s\([^)]*\)\s*\{' % name, text)) for text in code.values()) == 1 and re.search(r'\b%s\([^)]*\)\s*\{' % name, walk), name
    body = walk[walk.index('void band_walk('):]
    # the tile's pointers are __restrict__ locals of the walk, not struct members read per access
    for pointer in ('const int32_t* __restrict__ tile = t.tile;', 'const uint8_t* __restrict__ row_empty = t.row_empty;', 'const uint8_t* __restrict__ col_empty = t.col_empty;'):
        assert pointer in body
    assert not re.search(r't\.(tile|row_empty|col_empty)\b', body.split('const int32_t bound = t.bound;', 1)[1])
    # a job of a triangle on or left of the diagonal is left before anything is loaded
    assert body.index('if (j_lo + min((int64_t)kBandStep, t.n_cols - v0) - 1 <= i_lo) continue;') < body.index('col_empty[') < body.index('pass.side(')
    # one job loop, gridDim.x apart, and no loop that waits; s_row is cleared between two barriers, the flush behind a third
    assert 'for (int64_t job = blockIdx.x; job < n_bands * n_steps; job += gridDim.x) {' in body and not re.search(r'\bwhile\b|for \(;;\)', walk)
    clear = body.index('s_row[tid >> 2][tid & 3] = Pass::kIdle;')
    sync = [m.start() for m in re.finditer(r'__syncthreads\(\);', body)]
    rows = body.index('for (int rl = 0; rl < rows; ++rl) {')
    entries = body.index('for (int e = 0; e < kBandPer; ++e) {', rows)
    flush = body.index('if (tid < rows) {')
    assert len(sync) == 3 and sync[0] < clear < sync[1] < rows < entries < sync[2] < flush
    # the side value: fetched in exactly two places -- per column before the row loop, per row inside it and outside the entry loop
    side = [m.start() for m in re.finditer(r'pass\.side\(', body)]
    assert len(side) == 2 and side[0] < sync[0] and rows < side[1] < entries
    # the entry is loaded only after inside, the diagonal and the pass's predicate; the bound follows the key
    wants, load, bound, entry = (body.index(x, entries) for x in ('!Pass::wants(row_side, col_side[e])) continue;', '(uint32_t)row[kBandThreads * e]',
                                                                   'if (Pass::kBounded && (int32_t)key > bound) continue;', 'pass.entry('))
    assert body.index('if (!inside[e] || j <= i || ', entries) < wants < load < bound < entry and len(re.findall(r'\brow\[', body)) == 1
    # the early-out, the reduction in the wave, one LDS slot per wave
    ballot, shuffle, slot = body.index('if (__ballot(mine != Pass::kIdle) == 0) continue;'), body.index('__shfl_xor('), body.index('if (lane == 0) s_row[rl][wave] = mine;')
    assert entry < ballot < shuffle < slot < sync[2] and 'atomic' not in body
    # the flush: an idle part is not sent, and the output arrays are touched through row_out / col_out alone -- the walk knows no array
    assert body.index('if (part != Pass::kIdle) pass.row_out(i_lo + tid, j_lo, part);') > flush
    assert body.index('if (col[e] != Pass::kIdle) pass.col_out(j_lo + tid + kBandThreads * e, i_lo, col[e]);') > flush
    assert re.findall(r'pass\.(\w+)\(', body) == ['side', 'side', 'entry', 'row_out', 'col_out'] and set(re.findall(r'Pass::(\w+)', body)) == {
        'Word', 'Side', 'kBounded', 'kIdle', 'wants', 'join'}
    # the exports: one check for the five over a triangle, the rectangle keeps its own conditions; check_tri_tile's users are as they were
    host = code['dctfp_sim.hip']
    exports = ('dctfp_label_sums', 'dctfp_tri_degree', 'dctfp_tri_link_core', 'dctfp_tri_first_fp', 'dctfp_tri_tp_before')
    assert host.count('check_band_tile(') == 1 + len(exports) and 'static int check_band_tile(const char* name, const TriTile& t, int64_t n_nodes)' in host
    assert 'density_tile_ok' not in host and sum('check_band_tile(' in text for text in code.values()) == 1
    for name in exports + ('dctfp_rect_best',):
        body = host[host.index('\nint %s(' % name):host.index('DCTFP_GUARD("%s")' % name)]
        assert body.count('check_band_tile("%s", t, n_nodes)' % name) == (name != 'dctfp_rect_best') and 'check_tri_tile(' not in body, name
        assert ('ld < n_cols' in body) == (name == 'dctfp_rect_best') and 'TriTile' in body, name
        launch = re.search(r'void launch_%s\(([^)]*)\);' % name[len('dctfp_'):], code['launch.h']).group(1)
        assert launch.startswith('const TriTile& t, ') and 'n_rows' not in launch, name


def test_the_sad_tile_is_defined_once_in_a_header_every_user_includes():
    """The 128 x 128 v_sad_u8 contraction of l1_matrix16_kernel, protein_min_kernel and rows_link_kernel is one function template in
    one shared header.  Exempt by name, each for a reason written at the place: l1_knn_kernel (k_query.hip) and rows_assign_kernel
    (k_assign.hip) keep a copy of the tile because the shared one measured slower there (profiles/sad_tile/README.md);
    k_search.hip's per-pair kernel (pair_min_kernel) and l1_matrix_kernel in kernels.hip.h are contractions of their own."""
    import build_ext
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    shared = [h for h in build_ext.HEADERS if os.path.dirname(h) == csrc]
    code = {p: '\n'.join(line.split('//', 1)[0] for line in open(p).read().splitlines())
            for p in shared + [os.path.join(csrc, u) for u in build_ext.UNITS]}
    holders = [p for p, text in code.items() if re.search(r'\bvoid sad_tile\(', text)]
    assert len(holders) == 1 and holders[0] in shared and holders[0] in build_ext.kernel_sources()
    tile = holders[0]
    exempt = {'k_search.hip': 'pair_min_kernel', 'kernels.hip.h': 'l1_matrix_kernel', 'k_query.hip': 'l1_knn_kernel',
              'k_assign.hip': 'rows_assign_kernel'}
    assert sorted(p for p, text in code.items() if '__builtin_amdgcn_sad_u8' in text) == sorted([tile] + [os.path.join(csrc, f) for f in exempt])
    for name, kernel in exempt.items():
        text = code[os.path.join(csrc, name)]
        assert ' void %s(' % kernel in text
        if name != 'kernels.hip.h':
            assert 'sad_tile<' not in text
            # the intrinsic lies inside the named kernel's body and nowhere else in the file
            body = text[text.index(' void %s(' % kernel):]
            assert body[:body.index('\n}\n')].count('__builtin_amdgcn_sad_u8') == text.count('__builtin_amdgcn_sad_u8')
    for name in ('k_query.hip', 'k_assign.hip'):               # the copies say that they are copies, and of what
        assert 'copy of its own of sad_tile<' in open(os.path.join(csrc, name)).read()
        # ... with the header's layout numbers, not numbers of their own
        assert 'using dctfp::kSadLD;' in code[os.path.join(csrc, name)] and 'sad_b_slot(r)' in code[os.path.join(csrc, name)]
        assert not re.search(r'constexpr int k\w*(Tile|KC|LD) = \d', code[os.path.join(csrc, name)])
    # l1_matrix_kernel's use lies inside its own body: the intrinsic is gone from kernels.hip.h behind the next kernel's head
    text = code[os.path.join(csrc, 'kernels.hip.h')]
    assert text.index(' void l1_matrix_kernel(') < text.index('__builtin_amdgcn_sad_u8') <= text.rindex('__builtin_amdgcn_sad_u8') \
        < text.index(' void l1_matrix16_kernel(')
    inc = '#include "%s"' % os.path.basename(tile)
    for unit, call in (('kernels.hip.h', 'sad_tile<16>('), ('k_protein.hip', 'sad_tile<16>('), ('k_cluster.hip', 'sad_tile<ALIGN>(')):
        assert inc in code[os.path.join(csrc, unit)] and code[os.path.join(csrc, unit)].count(call) == 1
    # the constants and the choice of a fill are the header's too
    for name in ('kSadTile = 128', 'kSadKC = 32', 'kSadLD = kSadKC + 4', 'int sad_tile_align(', 'uint64_t sad_keep_mask('):
        assert sum(name in text for text in code.values()) == 1 and name in code[tile]
    for unit in ('k_cluster.hip', 'k_assign.hip', 'dctfp_sim.hip'):
        text = code[os.path.join(csrc, unit)]
        assert 'sad_tile_align(a, lda, b, ldb)' in text and '& 15u) == 0 &&' not in text


def test_link_kernels_touch_the_forest_through_agent_scope_atomics_only():
    """The access rule of the kernels that link, read off the source: no plain load or store of `parent` in the forest's routines
    (union_find.hip.h) and in k_cluster.hip outside the launch that only reads it (labels_kernel)."""
    csrc = os.path.join(ROOT, 'dctdomain_amd', 'csrc')
    text = open(os.path.join(csrc, 'union_find.hip.h')).read() + open(os.path.join(csrc, 'k_cluster.hip')).read()
    code = '\n'.join(line.split('//')[0] for line in text.splitlines())
    body = code[:code.index('void labels_kernel')] + code[code.index('unsigned link_grid'):]
    assert not re.search(r'parent\s*\[', body) and not re.search(r'(?<!_t)\*\(?\s*parent\b', body)    # (`int32_t* parent` declares)
    assert body.count('__HIP_MEMORY_SCOPE_AGENT') >= 4 and '__ATOMIC_RELAXED' in body
    assert 'asm' not in code
