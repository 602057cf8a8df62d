"""AddressSanitizer over the HOST side of libdctfp.so, on this machine, without a GPU.

GPU AddressSanitizer is not available on the pool, and a wrong index in a job table shows up on the GPU box as a fault
(or as an abort without a message).  So the host code of dctdomain_amd/csrc (dctfp.hip, dctfp_sim.hip and the launchers' units) is compiled on its own
(`hipcc --cuda-host-only -fsanitize=address`), linked against a stand-in for the HIP runtime (tests/asan/hip_stub.cpp:
device memory = host memory; a kernel launch walks the job tables the way the kernel's waves do and touches every address
they would) and driven over a few hundred seeded random batches (tests/asan/driver.cpp): every shape class, option,
fused-group layout, the split at giant domains, failure injection (also std::bad_alloc from any allocation of the table
build: the C ABI must answer DCTFP_ERR_NOMEM, not std::terminate) and arena restarts of the cosine-table cache.  Round 4: the
entry points either side of dctfp_quantize too -- the domain-string parser, the top-k job / stripe tables and sorting-network
groups, the window jobs of the stitcher in both forms, the L1 matrix / block minima / row select with its candidate scratch
-- over random and malformed arguments, again with allocation failures injected.  Every call runs on one of three caller's
streams in turn, the stub keeps the stream order (a vector clock per stream and event), and no call may return with work on
another stream that its caller's stream is not ordered after -- on its error paths either, where kernel launches are made to
fail now and then.  A second section (tests/asan/driver_sim.cpp) does the same for every export of dct-sim and query_db, and holds
each of them to the limits include/dctfp.h states: the stub refuses what the HIP runtime refuses (a grid of 2^32 threads or more
in a dimension, more than 1024 threads in a workgroup, ...), so the largest accepted value of every limit must launch and the
smallest refused one must come back as the library's own error code.  UndefinedBehaviorSanitizer runs beside AddressSanitizer: an
argument check that overflows is a report, not a wrapped comparison that passes."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CLANG = '/opt/rocm/lib/llvm/bin/clang++'


def _records(text, names):
    """{struct name: [field names in order]} for the job-table records."""
    out = {}
    for name in names:
        body = re.search(r'struct %s \{(.*?)\n\};' % name, text, re.S).group(1)
        body = re.sub(r'//[^\n]*', '', body)
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if decl:
                first, *rest = [d.strip() for d in decl.split(',')]
                fields.append(re.split(r'[\s\*]+', first)[-1])
                fields.extend(re.split(r'[\s\*]+', r)[-1] for r in rest)
        out[name] = fields
    return out


def test_stub_records_match_the_kernel_header():
    names = ['JobA', 'PieceA', 'JobB', 'Walk', 'Run', 'BasisJob']
    with open(os.path.join(ROOT, 'dctdomain_amd', 'csrc', 'kernels.hip.h')) as fh:
        a = _records(fh.read(), names)
    with open(os.path.join(ROOT, 'tests', 'asan', 'hip_stub.cpp')) as fh:
        b = _records(fh.read(), names)
    assert a == b


# Exports the driver does not have to call, each with its reason.  Every other `int dctfp_*(` of include/dctfp.h must be in the
# driver's report: an export added without a driver section fails the test.  (dctfp_last_error, dctfp_contact_count and
# dctfp_reccut_room do not return int and are not parsed; the driver calls all three.)
NOT_DRIVEN = {
    'dctfp_version': 'a constant',
    'dctfp_runtime_info': 'reads the process map for the HIP runtime: there is none under the stub',
    'dctfp_crash_handler': 'installs signal handlers: the sanitizer has its own',
    'dctfp_host_device_pointer': 'one runtime call, no argument to check beyond NULL',
    'dctfp_stream_synchronize': 'one runtime call',
    'dctfp_profile': 'hipEvent timing: the stub has no clock',
}
# Exports with nothing to refuse: a successful call is all that is asked of them.
NO_REFUSAL = {
    'dctfp_destroy': 'dctfp_destroy(NULL) is a no-op, like free(NULL)',
}


def _exports():
    with open(os.path.join(ROOT, 'include', 'dctfp.h')) as fh:
        return sorted(set(re.findall(r'^int (dctfp_\w+)\(', fh.read(), re.M)))


def test_the_header_parse_finds_the_exports():
    names = _exports()
    assert len(names) >= 60 and 'dctfp_quantize' in names and 'dctfp_query_lines' in names and set(NOT_DRIVEN) <= set(names)


@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(CLANG)), reason='needs the ROCm compilers')
def test_host_calls_under_address_sanitizer(tmp_path):
    sanitize = ['-fsanitize=address', '-fsanitize=undefined', '-fno-sanitize-recover=undefined']
    flags = ['-O1', '-g', '-std=c++17', '-fno-omit-frame-pointer', *sanitize]
    # (the host side only: -Xarch_host keeps the flags the device target does not take away from it)
    hip_flags = ['-O1', '-g', '-std=c++17', '-fno-omit-frame-pointer', *(x for f in sanitize for x in ('-Xarch_host', f))]
    inc = ['-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'dctdomain_amd', 'csrc')]
    import build_ext
    stub_o, syms, exe = (str(tmp_path / n) for n in ('hip_stub.o', 'fatbin_syms.cpp', 'driver'))
    inc += ['-I', os.path.join(ROOT, 'dctdomain_amd', 'csrc')]
    host_objs, procs = [], []
    for unit in build_ext.UNITS:          # every unit of the library, host side only (the launchers live in their own units)
        obj = str(tmp_path / (unit[:-4] + '.host.o'))
        host_objs.append(obj)
        procs.append(subprocess.Popen([HIPCC, '--offload-arch=gfx950', '--cuda-host-only', '-fPIC', '-DDCTFP_EXPERIMENTS', *hip_flags, *inc, '-c',
                                       os.path.join(ROOT, 'dctdomain_amd', 'csrc', unit), '-o', obj]))
    assert all(p.wait() == 0 for p in procs)
    subprocess.run([CLANG, '-D__HIP_PLATFORM_AMD__', '-fPIC', *flags, '-I', '/opt/rocm/include', '-c',
                    os.path.join(ROOT, 'tests', 'asan', 'hip_stub.cpp'), '-o', stub_o], check=True)
    # the host objects refer to the device code they would carry: empty ones will do (no kernel ever runs here)
    undefined = subprocess.run(['nm', '-u', *host_objs], check=True, capture_output=True, text=True).stdout
    with open(syms, 'w') as fh:
        for sym in sorted(set(re.findall(r'__hip_fatbin_[0-9a-f]+', undefined))):
            fh.write(f'extern "C" {{ extern const unsigned long long {sym}[4]; const unsigned long long {sym}[4] = {{0, 0, 0, 0}}; }}\n')
    subprocess.run([CLANG, *flags, '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'asan', 'driver.cpp'),
                    os.path.join(ROOT, 'tests', 'asan', 'driver_sim.cpp'), syms,
                    *host_objs, stub_o, '-o', exe, '-lpthread'], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    for seed in (1, 2, 3):
        r = subprocess.run([exe, '250', str(seed)], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        assert 'no memory error' in r.stdout
        # std::bad_alloc inside the table build comes back as DCTFP_ERR_NOMEM through the exception barrier of the C ABI
        assert int(re.search(r'reported as DCTFP_ERR_NOMEM: (\d+)', r.stdout).group(1)) >= 10, r.stdout
        # a kernel launch that fails (hip_stub.cpp) comes back as DCTFP_ERR_HIP -- with the context's own streams joined back into the
        # caller's, as on every path (the driver fails on any call that leaves work on another stream its caller's is not ordered after)
        assert int(re.search(r'reported as DCTFP_ERR_HIP: (\d+)', r.stdout).group(1)) >= 40, r.stdout
        walked = int(re.search(r'(\d+) walk-kernel launches', r.stdout).group(1))
        assert walked >= 12, r.stdout          # the production path is among what was exercised (a seed's share: 15-40 of 500 calls)
        # the entry points either side of dctfp_quantize (round 4): domain-string parser, top-k tables, stitch jobs, row select
        other = re.search(r'the other entry points: (\d+) calls \((\d+) ended in an expected error\)', r.stdout)
        assert int(other.group(1)) >= 500 and int(other.group(2)) < int(other.group(1)) // 3, r.stdout
        # ---- the exports of dct-sim and query_db (driver_sim.cpp), reported apart: the thresholds above count the old section only
        rows = re.search(r'limit table: (\d+) of (\d+) rows passed', r.stdout)
        assert int(rows.group(1)) == int(rows.group(2)) >= 70, r.stdout
        probes = re.search(r'overflow probes: (\d+) of (\d+) refused', r.stdout)
        assert int(probes.group(1)) == int(probes.group(2)) >= 20, r.stdout
        # no launch anywhere in the run had a shape the runtime refuses
        assert int(re.search(r'launches the stub refused for their shape: (\d+)', r.stdout).group(1)) == 0, r.stdout
        # the scratch users ran on a scratch of exactly the bytes they asked for, with the emulators touching every region's ends
        tight = re.search(r'(\d+) calls on a scratch of exactly the bytes asked for, (\d+) scratch regions touched', r.stdout)
        assert int(tight.group(1)) >= 20 and int(tight.group(2)) >= 200, r.stdout
        # completeness: every export of the header, but for the two literal lists above
        report = {}
        for m in re.finditer(r'^export (dctfp_\w+): (\d+) calls, (\d+) ok, (\d+) ok with a launch, refused invalid (\d+) shape (\d+) limit (\d+) '
                             r'unsupported (\d+), nomem \d+ hip \d+, limit rows (\d+) of (\d+)$', r.stdout, re.M):
            report[m.group(1)] = [int(x) for x in m.groups()[1:]]
        host_only = {'dctfp_build_pieces', 'dctfp_reccut_pieces', 'dctfp_stitch_sizes', 'dctfp_create', 'dctfp_destroy', 'dctfp_set_option',
                     'dctfp_get_option'}       # (no kernel of their own: a successful call, not a launching one)
        for name in _exports():
            if name in NOT_DRIVEN:
                continue
            assert name in report, f'{name} is exported by include/dctfp.h and never called by tests/asan/driver*.cpp'
            calls, ok, launching, invalid, shape, limit, unsupported, rows_ok, rows_all = report[name]
            assert (ok if name in host_only else launching) >= 1, (name, report[name])
            assert name in NO_REFUSAL or invalid + shape + limit + unsupported >= 1, (name, report[name])
            assert rows_ok == rows_all, (name, report[name])
        print(r.stdout.strip().splitlines()[-3:])
