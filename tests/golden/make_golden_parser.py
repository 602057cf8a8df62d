"""Writes the goldens of dct-sim's command line: what ``dct_sim.build_parser().parse_args(['--dct', 'x'] + argv)`` does, and what
``dct_sim.main`` then runs, for two sets of command lines.

    python tests/golden/make_golden_parser.py

expected.json.gz: every combination of at most four of the twenty option tokens of OPTIONS, never the same option twice, in the
order listed -- 5 514 command lines.  It is written only where it is missing: an existing file is compared with what the parser
does now and left byte for byte as it is (it names the commit it was recorded on).
expected_all.json.gz: every combination of at most three of all 46 tokens (OPTIONS + MORE_OPTIONS) -- 15 589 command lines.
Per command line one of two outcomes: the exit code and the last line of stderr with the program name removed, or, for an accepted
line, the sorted items of the namespace.  Distinct outcomes are stored once and referenced by index.  The recipe counts the
``self.error(`` call sites of dct_sim.py that the two sets reach, by the line of the caller, prints the count and fails where the
union is below the number of such calls in the file.
dispatch.json.gz: for every accepted command line of both sets, what ``dct_sim.main(['--dct', 'x'] + argv)`` does when the ten mode
functions are recorders (``dispatch``): the one function called, its positional arguments without the ``Report``, its keyword
arguments as they are, and the first line on stdout -- the header.  No file is opened and no GPU touched.
help.txt: ``format_help()`` of the parser, named dct-sim, at 100 columns (``help_text``).
All four are replayed by tests/test_parser_rules_host.py.  Run it on the commit whose command line is the reference -- the files
record that commit -- never on a parser under change."""

from __future__ import annotations

import contextlib
import gzip
import io
import itertools
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'dct_sim_parser')

OPTIONS = [['--pair', 'p'], ['--db', 'd'], ['--rank', 'domain'], ['--min-domain', '0.5'], ['--min-global', '0.5'], ['--cluster'],
           ['--domains'], ['--dom', 'x'], ['--db-dom', 'y'], ['--linkage', 'single'], ['--linkage', 'greedy'], ['--level', 'protein'],
           ['--level', 'domain'], ['--no-whole'], ['--assign', 'r'], ['--reps-out', 'o'], ['--tree'], ['--tree', 'global'], ['--rbh'],
           ['--rbh', 'global']]
MOST = 4
MORE_OPTIONS = [['--min-coverage', '0.5'], ['--min-coverage', '0'], ['--cov-unit', 'domains'], ['--rep', 'first'], ['--rep', 'medoid'],
                ['--min-neighbors', '3'], ['--min-neighbors', '0'], ['--auc1'], ['--auc1', 'global'], ['--families', 'f'],
                ['--family-sep', '|'], ['--family-sep', ''], ['--hist'], ['--hist', 'global'], ['--bins', '10'], ['--bins', '0'],
                ['--zscore'], ['--min-z', '2'], ['--domain-map'], ['--domain-map', '0.5'], ['--domain-map', '0'], ['--hac'],
                ['--hac', 'global'], ['--method', 'complete'], ['--flat'], ['--newick', 'n']]
ALL_OPTIONS = OPTIONS + MORE_OPTIONS
ALL_MOST = 3
MODE_FUNCTIONS = ('pair_sim', 'db_search', 'all_sim', 'cluster_sim', 'assign_sim', 'tree_sim', 'rbh_sim', 'auc1_sim', 'hist_sim', 'hac_sim')


def command_lines(options=OPTIONS, most=MOST):
    """The index tuples of the golden's command lines: ascending, no option name twice."""
    for k in range(most + 1):
        for combo in itertools.combinations(range(len(options)), k):
            names = [options[c][0] for c in combo]
            if len(set(names)) == len(names):
                yield combo


def outcome(parser, argv):
    """{'exit': code, 'error': last line of stderr without the program name} or {'namespace': sorted items}."""
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            ns = parser.parse_args(['--dct', 'x'] + argv)
    except SystemExit as stop:
        last = err.getvalue().rstrip('\n').rsplit('\n', 1)[-1]
        prefix = f'{parser.prog}: '
        return {'exit': stop.code, 'error': last[len(prefix):] if last.startswith(prefix) else last}
    return {'namespace': sorted([k, v] for k, v in vars(ns).items())}


def dispatch(dct_sim, argv):
    """What ``dct_sim.main(['--dct', 'x'] + argv)`` runs: {'function', 'args' (without the Report), 'kwargs', 'header'}.  The mode
    functions are replaced for the call and put back; ``open`` is refused meanwhile, and exactly one of the ten must be called."""
    calls = []

    def recorder(name):
        def record(*args, **kw):
            calls.append({'function': name, 'args': [a for a in args if not isinstance(a, dct_sim.Report)], 'kwargs': kw})
        return record

    def refuse(*args, **kw):
        raise AssertionError(f'dct_sim.main opens a file: {args}')

    kept = {name: getattr(dct_sim, name) for name in MODE_FUNCTIONS}
    out = io.StringIO()
    try:
        for name in MODE_FUNCTIONS:
            setattr(dct_sim, name, recorder(name))
        dct_sim.open = refuse
        with contextlib.redirect_stdout(out):
            dct_sim.main(['--dct', 'x'] + argv)
    finally:
        del dct_sim.open
        for name, fn in kept.items():
            setattr(dct_sim, name, fn)
    if len(calls) != 1:
        raise AssertionError(f'{argv}: {len(calls)} mode functions called')
    return dict(calls[0], header=out.getvalue().split('\n', 1)[0])


def help_text(dct_sim):
    """``--help`` of a parser named dct-sim on a terminal of 100 columns."""
    columns = os.environ.get('COLUMNS')
    os.environ['COLUMNS'] = '100'
    try:
        parser = dct_sim.build_parser()
        parser.prog = 'dct-sim'
        return parser.format_help()
    finally:
        if columns is None:
            del os.environ['COLUMNS']
        else:
            os.environ['COLUMNS'] = columns


def _distinct(got, outcomes, where):
    key = json.dumps(got, sort_keys=True)
    if key not in where:
        where[key] = len(outcomes)
        outcomes.append(got)
    return where[key]


def record(dct_sim, options, most):
    """(outcomes, cases, the argv of the accepted command lines) of one set."""
    outcomes, where, cases, accepted = [], {}, [], []
    for combo in command_lines(options, most):
        argv = [token for c in combo for token in options[c]]
        got = outcome(dct_sim.build_parser(), argv)
        cases.append([list(combo), _distinct(got, outcomes, where)])
        if 'namespace' in got:
            accepted.append(argv)
    return outcomes, cases, accepted


def _write(name, data):
    os.makedirs(OUT, exist_ok=True)
    with gzip.GzipFile(os.path.join(OUT, name), 'wb', mtime=0) as fh:
        fh.write(json.dumps(data, separators=(',', ':')).encode('utf8'))


def main():
    sys.path.insert(0, ROOT)
    from dctdomain_amd import dct_sim
    commit = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(['git', 'status', '--porcelain', '--', 'dctdomain_amd/dct_sim.py'], cwd=ROOT, capture_output=True, text=True,
                           check=True).stdout.strip()
    if dirty:
        raise SystemExit('dctdomain_amd/dct_sim.py differs from the commit: the golden records a committed parser')
    # the ``self.error(`` call sites the command lines reach, by the caller's line in dct_sim.py
    source = dct_sim.__file__
    with open(source, encoding='utf8') as fh:
        sites = fh.read().count('self.error(')
    reached = set()
    error = dct_sim._Parser.error

    def noting(self, message):
        caller = sys._getframe(1)
        if os.path.samefile(caller.f_code.co_filename, source):
            reached.add(caller.f_lineno)
        error(self, message)
    dct_sim._Parser.error = noting
    try:
        first = record(dct_sim, OPTIONS, MOST)
        reached_first = set(reached)
        reached.clear()
        second = record(dct_sim, ALL_OPTIONS, ALL_MOST)
    finally:
        dct_sim._Parser.error = error
    for name, options, (outcomes, cases, accepted) in (('expected.json.gz', OPTIONS, first), ('expected_all.json.gz', ALL_OPTIONS, second)):
        path = os.path.join(OUT, name)
        if name == 'expected.json.gz' and os.path.exists(path):
            with gzip.open(path, 'rt', encoding='utf8') as fh:
                old = json.load(fh)
            same = old['options'] == options and [[c, old['outcomes'][k]] for c, k in old['cases']] == json.loads(json.dumps(
                [[c, outcomes[k]] for c, k in cases]))
            if not same:
                raise SystemExit(f'{name} of commit {old["commit"]} records another parser than this commit\'s: it is left as it is')
        else:
            _write(name, {'commit': commit, 'options': options, 'outcomes': outcomes, 'cases': cases})
        errors = {o['error'] for o in outcomes if 'error' in o}
        print(f'{name}: {len(cases)} command lines, {len(accepted)} accepted, {len(errors)} distinct messages, '
              f'{sum("namespace" in o for o in outcomes)} distinct namespaces')
    records, where, cases = [], {}, []
    for argv in first[2] + [argv for argv in second[2] if argv not in first[2]]:
        cases.append([argv, _distinct(dispatch(dct_sim, argv), records, where)])
    _write('dispatch.json.gz', {'commit': commit, 'functions': list(MODE_FUNCTIONS), 'records': records, 'cases': cases})
    print(f'dispatch.json.gz: {len(cases)} accepted command lines, {len(records)} distinct records; of the new token set '
          f'{len({json.dumps(dispatch(dct_sim, argv), sort_keys=True) for argv in second[2]})} distinct')
    with open(os.path.join(OUT, 'help.txt'), 'w', encoding='utf8') as fh:
        fh.write(help_text(dct_sim))
    both = reached_first | reached
    print(f'self.error call sites reached: {len(reached_first)} by the first set, {len(reached)} by the second, {len(both)} of {sites} by both')
    if len(both) < sites:
        raise SystemExit(f'the command lines reach {len(both)} of the {sites} self.error calls of dct_sim.py')


if __name__ == '__main__':
    main()
