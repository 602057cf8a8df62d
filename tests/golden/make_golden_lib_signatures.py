"""Writes tests/golden/lib_signatures.json: what ``_lib._configure`` declares for every export of libdctfp.so.

    python tests/golden/make_golden_lib_signatures.py

{export name: [restype, [argument kinds]]} with the kinds ``ptr`` (``c_void_p``, ``c_char_p`` and every ``POINTER(...)``), ``i32``,
``int``, ``i64``, ``f64``, ``f32``; a result is ``int``, ``i64`` or ``str`` (``c_char_p``).  ``_configure`` runs on a stand-in library
object, so neither the built library nor a GPU is needed.  The file was recorded on the commit whose ``_configure`` was the
hand-written table (one ``argtypes`` line per export); tests/test_binding_host.py holds every later ``_configure`` to it.  An
existing file is compared and left byte for byte as it is."""

from __future__ import annotations

import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'lib_signatures.json')

#: ctypes makes c_int32 an alias of c_int where int has 32 bits; both are ``i32`` there, and ``int`` is a kind of its own elsewhere
KINDS = {C.c_int: 'int', C.c_int64: 'i64', C.c_double: 'f64', C.c_float: 'f32', C.c_int32: 'i32'}


def kind(ctype):
    """The kind of one ctypes argument type; a type of no kind is an error, never a guess."""
    if ctype in (C.c_void_p, C.c_char_p) or isinstance(ctype, type) and issubclass(ctype, C._Pointer):
        return 'ptr'
    return KINDS[ctype]


def result(ctype):
    return 'str' if ctype is C.c_char_p else kind(ctype)


class _Export:
    """What ctypes gives a foreign function before anyone declares it: ``argtypes`` None, ``restype`` c_int."""
    argtypes = None
    restype = C.c_int


class StandIn:
    """A library that has every symbol it is asked for."""
    _name = 'stand-in'

    def __getattr__(self, name):
        if not name.startswith('dctfp_'):
            raise AttributeError(name)
        fn = _Export()
        setattr(self, name, fn)
        return fn


def signatures(lib, names):
    return {name: [result(getattr(lib, name).restype), [kind(t) for t in getattr(lib, name).argtypes or ()]] for name in names}


def main():
    sys.path.insert(0, ROOT)
    from dctdomain_amd import _lib
    table = signatures(_lib._configure(StandIn()), list(_lib.EXPORTS) + list(_lib.LINKAGE_EXPORTS))
    text = json.dumps(table, indent=0, sort_keys=True, separators=(',', ':')).replace('\n', '').replace('],"', '],\n"') + '\n'
    if os.path.exists(OUT):
        with open(OUT, encoding='utf8') as fh:
            if json.load(fh) != table:
                raise SystemExit(f'{OUT} records another table than this commit\'s _configure: it is left as it is')
        print(f'{OUT}: {len(table)} exports, unchanged')
        return
    with open(OUT, 'w', encoding='utf8') as fh:
        fh.write(text)
    print(f'{OUT}: {len(table)} exports')


if __name__ == '__main__':
    main()
