"""The ctypes binding of libdctfp.so (dctdomain_amd/_lib.py): the signatures it reads from the two public headers are the ones the
hand-written table declared (tests/golden/lib_signatures.json, recorded from that table), the header parser refuses what it
does not know, and ``Context.call`` is context first, stream last, the code checked against the library it went to."""

import ctypes
import json
import os

import pytest

import make_golden_lib_signatures as golden
from dctdomain_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_configure_declares_the_recorded_signatures_on_the_built_library():
    with open(golden.OUT, encoding='utf8') as fh:
        recorded = json.load(fh)
    names = list(_lib.EXPORTS) + list(_lib.LINKAGE_EXPORTS)
    assert sorted(recorded) == sorted(names) and len(set(names)) == len(names) == 68
    lib = _lib._configure(ctypes.CDLL(_lib.LIB_PATH))
    assert lib is not None and golden.signatures(lib, names) == recorded
    assert golden.signatures(_lib._configure(golden.StandIn()), names) == recorded
    # every kind the headers use is one the golden tells apart, and a pointer is a plain address whatever it points to
    assert {k for _res, args in recorded.values() for k in args} == {'ptr', 'i32', 'i64', 'f64'}
    assert all(t is ctypes.c_void_p for name in names for t in getattr(lib, name).argtypes if golden.kind(t) == 'ptr')
    assert lib.dctfp_last_error.restype is ctypes.c_char_p and lib.dctfp_contact_count.restype is ctypes.c_int64


def test_constants_are_the_headers():
    assert (_lib.DCTFP_OK, _lib.DCTFP_ERR_INVALID, _lib.DCTFP_ERR_SHAPE, _lib.DCTFP_ERR_HIP, _lib.DCTFP_ERR_NOMEM, _lib.DCTFP_ERR_LIMIT,
            _lib.DCTFP_ERR_UNSUPPORTED) == (0, -1, -2, -3, -4, -5, -6)
    assert (_lib.DCTFP_MAX_N, _lib.DCTFP_MAX_M) == (8, 128)
    assert (_lib.DCTFP_F32, _lib.DCTFP_F64, _lib.DCTFP_F16, _lib.DCTFP_BF16) == (0, 1, 2, 3)
    assert _lib.DCTFP_LINKAGE_VERSION == 1 and _lib.LINKAGE_MAX_N == 46340 == _lib.DCTFP_LINKAGE_MAX_N
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.dctfp_version() == _lib.DCTFP_VERSION and lib.dctfp_linkage_version() == _lib.DCTFP_LINKAGE_VERSION


def test_the_parser_maps_what_it_knows_and_refuses_the_rest(tmp_path):
    path = tmp_path / 'some.h'
    path.write_text('/* int dctfp_in_a_comment(int x); */\n#define DCTFP_SOME (-7) /* why */\n#define DCTFP_GUARD\n'
                    'typedef struct { int32_t n; } dctfp_thing;\n'
                    'int dctfp_one(dctfp_ctx* ctx, const dctfp_thing* things, int32_t n, const int64_t* offs, float f,\n'
                    '              double t, int device, const char* text, int8_t out[], void* const* many, void* stream);\n'
                    'int64_t dctfp_two(int32_t n_res);\nconst char* dctfp_three(void);\n')
    exports, defines = _lib.parse_header(str(path))
    p, C = ctypes.c_void_p, ctypes
    assert exports == {'dctfp_one': (C.c_int, [p, p, C.c_int32, p, C.c_float, C.c_double, C.c_int, p, p, p, p]),
                       'dctfp_two': (C.c_int64, [C.c_int32]), 'dctfp_three': (C.c_char_p, [])}
    assert list(exports) == ['dctfp_one', 'dctfp_two', 'dctfp_three'] and defines == {'DCTFP_SOME': -7}
    for declaration in ('int dctfp_bad(dctfp_ctx* ctx, size_t n, void* stream);', 'int dctfp_bad(unsigned int n);', 'int dctfp_bad(uint8_t flag);',
                        'float dctfp_bad(int32_t n);', 'void* dctfp_bad(void);'):
        path.write_text('int dctfp_fine(int32_t n);\n' + declaration + '\n')
        with pytest.raises(ImportError) as err:
            _lib.parse_header(str(path))
        assert 'dctfp_bad' in str(err.value) and declaration[:-1].split('(')[1].split(')')[0] in str(err.value)       # the declaration itself
    missing = str(tmp_path / 'not_there.h')
    with pytest.raises(ImportError) as err:
        _lib.parse_header(missing)
    assert missing in str(err.value)
    assert os.path.samefile(_lib.INCLUDE_DIR, os.path.join(ROOT, 'include'))


class _Recorder:
    """A library whose exports record their arguments and return ``code``; ``dctfp_last_error`` is this library's own."""

    def __init__(self, code=0, message=b'the message of this library'):
        self.calls, self.code, self.message = [], code, message

    def dctfp_create(self, device, out):
        ctypes.cast(out, ctypes.POINTER(ctypes.c_void_p))[0] = 0xabc0
        return 0

    def dctfp_destroy(self, handle):
        return 0

    def dctfp_last_error(self):
        return self.message

    def __getattr__(self, name):
        if not name.startswith('dctfp_'):
            raise AttributeError(name)
        return lambda *args: (self.calls.append((name,) + args), self.code)[1]


class _Stream:
    cuda_stream = 0x5117


def test_context_call_is_handle_first_stream_last_and_checks_with_its_own_library():
    lib = _Recorder()
    ctx = _lib.Context(3, lib)
    assert ctx.device == 3 and ctx.handle.value == 0xabc0
    assert ctx.call('dctfp_anything', 1, None, 2.5, b'text', stream=_Stream()) is None
    (name, handle, *args, stream), = lib.calls
    assert name == 'dctfp_anything' and handle is ctx.handle and args == [1, None, 2.5, b'text']
    assert isinstance(stream, ctypes.c_void_p) and stream.value == 0x5117
    ctx.call('dctfp_no_arguments', stream=_Stream())
    assert [type(a) for a in lib.calls[1][1:]] == [ctypes.c_void_p, ctypes.c_void_p]
    for code, raised in ((_lib.DCTFP_ERR_INVALID, _lib.DctfpError), (_lib.DCTFP_ERR_LIMIT, _lib.DctfpError), (_lib.DCTFP_ERR_SHAPE, ValueError),
                         (_lib.DCTFP_ERR_NOMEM, MemoryError)):
        lib.code = code
        with pytest.raises(raised) as err:
            ctx.call('dctfp_anything', 1, stream=_Stream())
        assert 'the message of this library' in str(err.value)      # (not the product library's: dctfp_last_error is per library)
        if raised is _lib.DctfpError:
            assert err.value.code == code and err.value.msg == 'the message of this library'
    ctx.close()
    with pytest.raises(RuntimeError):
        ctx.call('dctfp_anything', stream=_Stream())
    assert len(lib.calls) == 6
