"""CPU-side checks of dct-sim --domains: the numpy rule (domain_pair_rule.py, the GPU tests' oracle) against a literal restatement
of the reference's double loop, the .dom parser and the labels, the command line, and the two entry points in the header and the
libraries."""

import ctypes
import os
import re

import numpy as np
import pytest

import domain_pair_rule as rule
import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(gu.GOLD, 'ref_fixtures')


# ---- the rule

def _reference_loop(dct_i, dct_j):
    """src/dct-sim.py:12-50, word for word where it matters: the running maximum starts at 0 and is replaced on ``s > maxs``; the
    position of the last replacement is what --domains reports."""
    best = None
    maxs = 0
    s = None
    for pi in range(dct_i.shape[0]):
        for pj in range(dct_j.shape[0]):
            d = abs(dct_i[pi].astype(np.int64) - dct_j[pj].astype(np.int64)).sum()
            d = d / 17000
            d = min(d, 1)
            s = 1 - d
            if s > maxs:
                maxs = s
                best = (pi, pj)
    return maxs, s, best


def _row_with_l1(v, width=480):
    row = np.zeros(width, dtype=np.int8)
    q, r = divmod(int(v), 127)
    row[:q] = 127
    row[q] = r
    return row


def _cases():
    rng = np.random.default_rng(5)
    zero = np.zeros((1, 480), dtype=np.int8)
    for v in (0, 1, 16999, 17000, 17001, 40000):                # one pair on either side of "similarity 0"
        yield zero, _row_with_l1(v)[None]
    for _ in range(40):                                         # random sets around a few families: near and far pairs
        fam = rng.integers(-60, 61, size=(3, 480))
        sets = []
        for _ in range(2):
            k = int(rng.integers(1, 6))
            sets.append(np.clip(fam[rng.integers(0, 3, size=k)] + rng.integers(-15, 16, size=(k, 480)), -127, 127).astype(np.int8))
        yield tuple(sets)
    for _ in range(20):                                         # planted exact duplicates: ties at several positions
        a = rng.integers(-40, 41, size=(4, 480)).astype(np.int8)
        b = rng.integers(-40, 41, size=(5, 480)).astype(np.int8)
        x, y = rng.choice(4, size=2, replace=False)             # rows x and y of a and one or two rows of b are one fingerprint
        a[y] = a[x]
        for z in rng.choice(5, size=int(rng.integers(1, 3)), replace=False):
            b[z] = a[x]
        yield a, b
    far = np.full((3, 480), 127, dtype=np.int8)                 # every pair at 17000 or more, several of them equal
    yield far, -far
    yield np.stack([_row_with_l1(17000)] * 2), np.zeros((3, 480), dtype=np.int8)


def test_rule_is_the_reference_loop():
    seen = {'none': 0, 'tie': 0, 'pair': 0}
    for a, b in _cases():
        maxs, s, best = _reference_loop(a, b)
        mn, last, arg_a, arg_b = rule.best_pair(a, b)
        assert (arg_a, arg_b) == (best if best is not None else (-1, -1))
        assert 1 - min(last / 17000, 1) == s
        assert (1 - min(mn / 17000, 1) if best is not None else 0) == maxs
        d = np.abs(a.astype(np.int64)[:, None] - b.astype(np.int64)[None]).sum(2)
        seen['none' if best is None else 'pair'] += 1
        seen['tie'] += int(best is not None and np.count_nonzero(d == d.min()) > 1)
    assert seen['none'] >= 5 and seen['tie'] >= 15 and seen['pair'] >= 50


def test_rule_without_fingerprints_has_no_pair():
    some, none = np.zeros((2, 480), dtype=np.int8), np.zeros((0, 480), dtype=np.int8)
    for a, b in ((some, none), (none, some), (none, none)):
        assert rule.best_pair(a, b) == (0x7fffffff, 0x7fffffff, -1, -1)
        assert _reference_loop(a, b)[2] is None


def test_rule_counts_on_the_all_sim_golden():
    with np.load(os.path.join(gu.GOLD, 'all_sim', 'all-dct.npz')) as data:
        idx, dct = np.asarray(data['idx'], dtype=np.int64), data['dct']
    i, j, mn, last, arg_i, arg_j = rule.triangle_args(dct, idx)
    tied, whole = rule.pair_facts(dct, idx, dct, idx, i, j)
    assert (len(i), int((arg_i < 0).sum()), int(tied.sum()), int(whole.sum())) == (9591, 1110, 271, 2460)
    assert np.array_equal(arg_i < 0, mn >= 17000) and np.array_equal(arg_i < 0, arg_j < 0)


# ---- the .dom file and the labels

def _example():
    with np.load(os.path.join(FIX, 'example-dct.npz')) as data:
        return [str(s) for s in data['sid']], np.asarray(data['idx'], dtype=np.int64)


def test_dom_parser_on_the_reference_example():
    from dctdomain_amd import dct_sim
    sid, idx = _example()
    doms = dct_sim.read_dom_file(os.path.join(FIX, 'example.dom'))
    assert doms == rule.read_dom(os.path.join(FIX, 'example.dom')) and len(doms) == 8
    assert doms['Q9XZJ4'] == ['1-34', '35-169', '170-244']
    counts = np.diff(idx)
    assert [len(doms[s]) + 1 for s in sid] == counts.tolist()   # every protein: its domains and the whole-protein row
    labels = dct_sim.fingerprint_labels(sid, idx, doms)
    assert labels == rule.labels(idx, doms, sid) and len(labels) == idx[-1] == 43
    for p, s in enumerate(sid):
        assert labels[idx[p]:idx[p + 1]] == doms[s] + ['whole']
    assert dct_sim.fingerprint_labels(sid, idx) == rule.labels(idx) == [str(r + 1) for k in counts for r in range(k)]


def test_dom_parser_line_format(tmp_path):
    from dctdomain_amd import dct_sim
    path = tmp_path / 'x.dom'
    path.write_text('a 1 1-50\nsp|P1|X two words 2 1-20,50-80;21-49\n\nb 1 1-9\nb 2 1-4;5-9\né 1 1-7\n', encoding='utf8')
    doms = dct_sim.read_dom_file(str(path))
    assert doms == {'a': ['1-50'], 'sp|P1|X two words': ['1-20,50-80', '21-49'], 'b': ['1-4', '5-9'], 'é': ['1-7']}   # (the later b)
    # k names for k fingerprints (no unnamed row), k - 1 names (the last row is the whole protein), a protein without fingerprints
    sid, idx = ['a', 'none', 'sp|P1|X two words', 'b'], [0, 1, 1, 4, 6]
    assert dct_sim.fingerprint_labels(sid, idx, doms) == ['1-50', '1-20,50-80', '21-49', 'whole', '1-4', '5-9']
    for bad_idx, named in (([0, 3, 3, 6, 8], 'a'), ([0, 1, 1, 2, 4], 'sp|P1|X two words'), ([0, 1, 1, 4, 10], 'b')):
        with pytest.raises(ValueError, match=re.escape(named)):
            dct_sim.fingerprint_labels(sid, bad_idx, doms)
    with pytest.raises(ValueError, match='missing'):
        dct_sim.fingerprint_labels(['a', 'missing'], [0, 1, 2], doms)
    assert dct_sim.fingerprint_labels(['a', 'missing'], [0, 1, 1], doms) == ['1-50']
    for text in ('a 1\n', 'a x 1-5\n', 'a 2 1-5\n', 'lonely\n'):
        path.write_text(text, encoding='utf8')
        with pytest.raises(ValueError, match='x.dom:1'):
            dct_sim.read_dom_file(str(path))


def test_label_table_has_one_entry_per_row_and_the_sentinel():
    """What FilteredPairs hands to the line kernel: the labels' UTF-8 bytes with prefix offsets, '-' last."""
    from dctdomain_amd import dct_sim
    sid, idx = _example()
    labels = dct_sim.fingerprint_labels(sid, idx, dct_sim.read_dom_file(os.path.join(FIX, 'example.dom')))
    table = labels + [dct_sim.NO_DOMAIN]
    assert len(table) == idx[-1] + 1 and table[-1] == '-' and dct_sim.WHOLE == 'whole'
    f = dct_sim.FilteredPairs(sid, idx, np.zeros((43, 480), np.int8), labels=labels)
    assert f.row_labels == labels and (f.bound_domain, f.bound_global, f.route) == (17000, 17000, 'domain')   # (bounds that keep everything)
    with pytest.raises(ValueError, match='one entry per fingerprint row'):
        dct_sim.FilteredPairs(sid, idx, np.zeros((43, 480), np.int8), labels=labels[:-1])


# ---- the command line

def test_flagless_parser_and_headers_are_unchanged():
    from dctdomain_amd import dct_sim
    assert dct_sim.HEADER == '#prot1 prot2 sim-domain sim-global' and dct_sim.CLUSTER_HEADER == '#representative member'
    assert dct_sim.DOMAIN_HEADER == '#prot1 prot2 sim-domain sim-global dom1 dom2'
    args = dct_sim.build_parser().parse_args(['--dct', 'x.npz'])
    assert vars(args) == {'dct': 'x.npz', 'output': None, 'pair': None, 'pairfound': None, 'db': None, 'top': 5, 'threshold': 0.25,
                          'rank': None, 'min_domain': None, 'min_global': None, 'cluster': False}   # (no attribute unless asked for)


@pytest.mark.parametrize('argv,want', [
    (['--domains'], (True, None, None)),
    (['--dom', 'x.dom'], (True, 'x.dom', None)),
    (['--db', 'y.npz', '--db-dom', 'y.dom'], (True, None, 'y.dom')),
    (['--db', 'y.npz', '--rank', 'domain', '--dom', 'x.dom', '--db-dom', 'y.dom'], (True, 'x.dom', 'y.dom')),
    (['--pair', 'p.txt', '--domains', '--dom', 'x.dom'], (True, 'x.dom', None)),
    (['--min-domain', '0.5', '--min-global', '0.1', '--domains'], (True, None, None)),
])
def test_parser_accepts_the_domain_flags(argv, want):
    from dctdomain_amd import dct_sim
    args = dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv)
    assert (args.domains, getattr(args, 'dom', None), getattr(args, 'db_dom', None)) == want


@pytest.mark.parametrize('argv,named', [
    (['--db-dom', 'y.dom'], '--db-dom'),
    (['--pair', 'p.txt', '--db-dom', 'y.dom'], '--db-dom'),
    (['--min-domain', '0.5', '--cluster', '--domains'], '--domains'),
    (['--min-domain', '0.5', '--cluster', '--dom', 'x.dom'], '--domains'),
    (['--dom'], '--dom'),
])
def test_parser_rejects(argv, named, capsys):
    from dctdomain_amd import dct_sim
    with pytest.raises(SystemExit) as e:
        dct_sim.build_parser().parse_args(['--dct', 'x.npz'] + argv)
    assert e.value.code == 2
    assert named in capsys.readouterr().err


# ---- the entry points

@pytest.mark.parametrize('name,params,sibling', [
    ('dctfp_pair_argmin', 'dctfp_ctx* ctx, const int32_t* pairs, int64_t n_pairs, const int8_t* a, int64_t lda, const int64_t* idx_a, '
                          'int64_t npa, const int8_t* b, int64_t ldb, const int64_t* idx_b, int64_t npb, int32_t d, int32_t* out_min, '
                          'int32_t* out_last, int32_t* out_arg_a, int32_t* out_arg_b, void* stream', 'dctfp_pair_min'),
    ('dctfp_pair_domain_lines', 'dctfp_ctx* ctx, int64_t n_lines, const int32_t* pi, const int32_t* pj, const int32_t* mn, '
                                'const int32_t* last, const int32_t* la, const int32_t* lb, const uint8_t* ids, const int64_t* id_off, '
                                'int64_t n_ids, const uint8_t* labels, const int64_t* label_off, int64_t n_labels, const char* table, '
                                'const int64_t* line_off, uint8_t* out, int64_t out_bytes, void* stream', 'dctfp_pair_lines'),
])
def test_library_exports_the_entry_points_and_header_documents_them(name, params, sibling):
    from dctdomain_amd import _lib
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        header = fh.read()
    decl = re.search(r'int %s\(([^;]*)\);' % name, header)
    assert decl and ' '.join(decl.group(1).split()) == params
    doc = header[:decl.start()].rsplit('/*', 1)[1]
    assert '*/' in doc and 'DCTFP_ERR_LIMIT' in doc and sibling in doc
    assert re.fullmatch(r'\s*', doc.split('*/', 1)[1]), 'the comment must sit right above the declaration'
    # the sibling's own arguments, in its order, are a prefix of / contained in the new call's
    sib = ' '.join(re.search(r'int %s\(([^;]*)\);' % sibling, header).group(1).split())
    if name == 'dctfp_pair_argmin':
        assert params == sib.replace(', void* stream', ', int32_t* out_arg_a, int32_t* out_arg_b, void* stream')
    version = int(re.search(r'#define DCTFP_VERSION (\d+)', header).group(1))
    assert version >= 105
    for path in (_lib.LIB_PATH, _lib.EXPERIMENTS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, name)
        assert lib.dctfp_version() == version
    assert name in _lib.EXPORTS
    with open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'launch.h')) as fh:
        assert 'launch_' + name[len('dctfp_'):] + '(' in fh.read()
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as fh:
        assert '`%s`' % name in fh.read()


def test_binding_declares_one_argument_type_per_parameter():
    import ctypes as C
    from dctdomain_amd import _lib
    lib = _lib._configure(C.CDLL(_lib.LIB_PATH))
    assert len(lib.dctfp_pair_argmin.argtypes) == 17 and lib.dctfp_pair_argmin.argtypes[:14] == lib.dctfp_pair_min.argtypes[:14]
    assert len(lib.dctfp_pair_domain_lines.argtypes) == 19
    assert lib.dctfp_pair_domain_lines.argtypes[1] == C.c_int64 and lib.dctfp_pair_domain_lines.argtypes[10] == C.c_int64
    assert lib.dctfp_pair_domain_lines.argtypes[13] == C.c_int64 and lib.dctfp_pair_domain_lines.argtypes[17] == C.c_int64
    assert lib.dctfp_pair_argmin.restype == C.c_int and lib.dctfp_pair_domain_lines.restype == C.c_int


def test_null_and_bad_arguments_are_refused_without_a_device():
    """The argument checks stand in front of every HIP call: a NULL context is DCTFP_ERR_INVALID on any machine."""
    import ctypes as C
    from dctdomain_amd import _lib
    lib = _lib._configure(C.CDLL(_lib.LIB_PATH))
    assert lib.dctfp_pair_argmin(None, *([None, 0, None, 0, None, 0, None, 0, None, 0, 0] + [None] * 5)) == _lib.DCTFP_ERR_INVALID
    assert lib.dctfp_pair_domain_lines(None, 0, *([None] * 8), 0, None, None, 0, None, None, None, 0, None) == _lib.DCTFP_ERR_INVALID
