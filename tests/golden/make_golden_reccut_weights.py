#!/usr/bin/env python3
"""The reference's own RecCut.cpp (compiled into oracle/_ref/RecCut by oracle/Makefile) on the seeded graphs of
recipes_contacts.weight_class_graphs: weights below 0 and above 255.  Build container only.  Outputs
reccut_weights_golden.json (data only): per graph the sha256 of the .ce text it was given, its exit status and the domain
strings it printed."""

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
from oracle import contacts_oracle as co  # noqa: E402
from recipes_contacts import weight_class_graphs  # noqa: E402

assert os.path.exists(co.REF_BIN), 'oracle/_ref/RecCut not built (make -C oracle ref)'
cases = []
for L, ii, jj, pv in weight_class_graphs():
    text = co.ce_text('x', 'A' * L, ii, jj, pv)
    rc, out = co.run_ref_binary(text)
    cases.append({'L': L, 'ce_sha256': hashlib.sha256(text.encode()).hexdigest(), 'reccut_rc': rc,
                  'domains': out.strip().split()[2].split(';')[:-1] if rc == 0 else None})
with open(os.path.join(HERE, 'reccut_weights_golden.json'), 'w') as fh:
    json.dump({'generator': 'tests/golden/make_golden_reccut_weights.py', 'seed': 4711, 'cases': cases}, fh, indent=1)
print(len(cases), 'graphs;', sum(1 for c in cases if c['reccut_rc'] != 0), 'refused;',
      sum(1 for c in cases if c['domains'] and len(c['domains']) > 1), 'multi-domain;',
      sum(1 for c in cases if c['domains'] and any(',' in d for d in c['domains'])), 'with discontinuous domains')
