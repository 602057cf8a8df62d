"""dct-sim's command line against the goldens of tests/golden/make_golden_parser.py.  Every combination of at most four of twenty
option tokens (5 514 command lines) and of at most three of all 46 (15 589) must be refused with the recorded message or accepted
with the recorded namespace; every accepted one must run the recorded mode function with the recorded arguments under the
recorded header; and ``--help`` prints the recorded text.  Each golden was recorded on the commit it names, before the rules, the
modes and ``main`` became one table."""

import contextlib
import gzip
import importlib.util
import io
import json
import os

import golden_util as gu


def _golden(name='expected.json.gz'):
    with gzip.open(os.path.join(gu.GOLD, 'dct_sim_parser', name), 'rt', encoding='utf8') as fh:
        return json.load(fh)


def _recipe():
    """tests/golden/make_golden_parser.py as a module: ``dispatch`` and ``help_text`` record here as they did there."""
    spec = importlib.util.spec_from_file_location('make_golden_parser', os.path.join(gu.GOLD, 'make_golden_parser.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


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
    _replay(dct_sim.build_parser(), options, outcomes, cases)


def _replay(parser, options, outcomes, cases):
    wrong = []
    for combo, k in cases:
        argv = [token for c in combo for token in options[c]]
        got = json.loads(json.dumps(_outcome(parser, argv)))
        if got != outcomes[k]:
            wrong.append((argv, got, outcomes[k]))
    assert not wrong, f'{len(wrong)} command lines differ, the first: {wrong[0]}'


def test_every_recorded_command_line_of_all_option_tokens_parses_as_recorded():
    from dctdomain_amd import dct_sim
    gold = _golden('expected_all.json.gz')
    options, outcomes, cases = gold['options'], gold['outcomes'], gold['cases']
    assert gold['commit'].startswith('011bbd6') and len(options) == 46 and options[:20] == _golden()['options'] and len(cases) == 15589
    assert max(len(combo) for combo, k in cases) == 3
    assert sum('namespace' in outcomes[k] for combo, k in cases) == 184
    assert all(o['exit'] == 2 and o['error'].startswith('error: --') for o in outcomes if 'error' in o)
    _replay(dct_sim.build_parser(), options, outcomes, cases)


def test_every_accepted_command_line_runs_the_recorded_mode_function_under_the_recorded_header():
    from dctdomain_amd import dct_sim
    gold, recipe = _golden('dispatch.json.gz'), _recipe()
    records, cases = gold['records'], gold['cases']
    assert gold['commit'].startswith('011bbd6') and len(gold['functions']) == 10 and {r['function'] for r in records} == set(gold['functions'])
    # (every accepted line of the two goldens above, and no other)
    accepted = set()
    for name in ('expected.json.gz', 'expected_all.json.gz'):
        g = _golden(name)
        accepted |= {json.dumps([t for c in combo for t in g['options'][c]]) for combo, k in g['cases'] if 'namespace' in g['outcomes'][k]}
    assert {json.dumps(argv) for argv, k in cases} == accepted and len(cases) == len(accepted) == 218
    kept = {name: getattr(dct_sim, name) for name in gold['functions']}
    wrong = []
    for argv, k in cases:
        got = json.loads(json.dumps(recipe.dispatch(dct_sim, argv)))
        if got != records[k]:
            wrong.append((argv, got, records[k]))
    assert not wrong, f'{len(wrong)} command lines differ, the first: {wrong[0]}'
    assert all(getattr(dct_sim, name) is fn for name, fn in kept.items()) and 'open' not in vars(dct_sim)


def test_help_prints_the_recorded_text():
    from dctdomain_amd import dct_sim
    with open(os.path.join(gu.GOLD, 'dct_sim_parser', 'help.txt'), encoding='utf8') as fh:
        assert _recipe().help_text(dct_sim) == fh.read()
