"""Writes the golden of dct-sim's command-line rules: what ``dct_sim.build_parser().parse_args(['--dct', 'x'] + argv)`` does for every
combination of at most four of the twenty option tokens below, never the same option twice, in the order listed -- 5 514 command
lines, which reach every ``error`` call of ``dct_sim._Parser``.

    python tests/golden/make_golden_parser.py

Per command line one of two outcomes: the exit code and the last line of stderr with the program name removed, or, for an accepted
line, the sorted items of the namespace.  Distinct outcomes are stored once and referenced by index.  Output:
tests/golden/dct_sim_parser/expected.json.gz, replayed by tests/test_parser_rules_host.py.  Run it on the commit whose parser is the
reference -- the file records that commit -- never on a parser under change."""

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


def main():
    sys.path.insert(0, ROOT)
    from dctdomain_amd import dct_sim
    commit = subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(['git', 'status', '--porcelain', '--', 'dctdomain_amd/dct_sim.py'], cwd=ROOT, capture_output=True, text=True,
                           check=True).stdout.strip()
    if dirty:
        raise SystemExit('dctdomain_amd/dct_sim.py differs from the commit: the golden records a committed parser')
    outcomes, where, cases = [], {}, []
    for combo in command_lines():
        got = outcome(dct_sim.build_parser(), [token for c in combo for token in OPTIONS[c]])
        key = json.dumps(got, sort_keys=True)
        if key not in where:
            where[key] = len(outcomes)
            outcomes.append(got)
        cases.append([list(combo), where[key]])
    os.makedirs(OUT, exist_ok=True)
    with gzip.GzipFile(os.path.join(OUT, 'expected.json.gz'), 'wb', mtime=0) as fh:
        fh.write(json.dumps({'commit': commit, 'options': OPTIONS, 'outcomes': outcomes, 'cases': cases}, separators=(',', ':')).encode('utf8'))
    errors = {o['error'] for o in outcomes if 'error' in o}
    print(f'{len(cases)} command lines, {len(errors)} distinct messages, {sum("namespace" in o for o in outcomes)} distinct namespaces')


if __name__ == '__main__':
    main()
