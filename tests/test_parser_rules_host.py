"""dct-sim's command-line rules against the golden of tests/golden/make_golden_parser.py: every combination of at most four of
twenty option tokens -- 5 514 command lines that reach every ``error`` call of ``dct_sim._Parser`` -- must be refused with the
recorded message or accepted with the recorded namespace.  The golden was recorded on the commit it names, before the rules became
a table."""

import contextlib
import gzip
import io
import json
import os

import golden_util as gu


def _golden():
    with gzip.open(os.path.join(gu.GOLD, 'dct_sim_parser', 'expected.json.gz'), 'rt', encoding='utf8') as fh:
        return json.load(fh)


def _outcome(parser, argv):
    """What make_golden_parser.outcome records, after a round trip through JSON."""
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            ns = parser.parse_args(['--dct', 'x'] + argv)
    except SystemExit as stop:
        last = err.getvalue().rstrip('\n').rsplit('\n', 1)[-1]
        prefix = f'{parser.prog}: '
        return {'exit': stop.code, 'error': last[len(prefix):] if last.startswith(prefix) else last}
    return {'namespace': sorted([k, v] for k, v in vars(ns).items())}


def test_every_recorded_command_line_parses_as_recorded():
    from dctdomain_amd import dct_sim
    gold = _golden()
    options, outcomes, cases = gold['options'], gold['outcomes'], gold['cases']
    assert len(gold['commit']) == 40 and len(options) == 20 and len(cases) == 5514
    messages = {o['error'] for o in outcomes if 'error' in o}
    assert len(messages) == 51 and all(o['exit'] == 2 for o in outcomes if 'error' in o)
    assert all(m.startswith('error: --') for m in messages)     # (the rules' own messages: each opens with the flag it is about)
    parser = dct_sim.build_parser()
    wrong = []
    for combo, k in cases:
        argv = [token for c in combo for token in options[c]]
        got = json.loads(json.dumps(_outcome(parser, argv)))
        if got != outcomes[k]:
            wrong.append((argv, got, outcomes[k]))
    assert not wrong, f'{len(wrong)} command lines differ, the first: {wrong[0]}'
