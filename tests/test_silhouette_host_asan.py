"""AddressSanitizer and UndefinedBehaviorSanitizer over the host side of the export of include/dctfp_silhouette.h, without a GPU.

Built and run exactly as test_linkage_host_asan.py builds its driver -- the host objects of every unit of the library
(`hipcc --cuda-host-only`, the sanitizers on the host side), tests/asan/hip_stub.cpp unchanged as the HIP runtime -- but linked
into a program of its own, tests/asan/driver_silhouette.cpp: the export lives in a header of its own, which the completeness
checks of the other two sanitizer tests do not read.  This test holds it to the same report rules: every `int dctfp_*(` of the
header is in the report, launched, refused for every stated limit, every limit row (the largest accepted and the smallest refused
value) passed, and every injected launch failure reported as DCTFP_ERR_HIP."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CLANG = '/opt/rocm/lib/llvm/bin/clang++'
NOT_DRIVEN = {'dctfp_silhouette_version': 'a constant'}


def _exports():
    with open(os.path.join(ROOT, 'include', 'dctfp_silhouette.h')) as fh:
        return sorted(set(re.findall(r'^int (dctfp_\w+)\(', fh.read(), re.M)))


def test_the_header_parse_finds_the_exports():
    assert _exports() == ['dctfp_silhouette_rows', 'dctfp_silhouette_version']


@pytest.mark.skipif(not (os.path.exists(HIPCC) and os.path.exists(CLANG)), reason='needs the ROCm compilers')
def test_silhouette_host_calls_under_address_sanitizer(tmp_path):
    sanitize = ['-fsanitize=address', '-fsanitize=undefined', '-fno-sanitize-recover=undefined']
    flags = ['-O1', '-g', '-std=c++17', '-fno-omit-frame-pointer', *sanitize]
    hip_flags = ['-O1', '-g', '-std=c++17', '-fno-omit-frame-pointer', *(x for f in sanitize for x in ('-Xarch_host', f))]
    inc = ['-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'dctdomain_amd', 'csrc')]
    import build_ext
    stub_o, syms, exe = (str(tmp_path / n) for n in ('hip_stub.o', 'fatbin_syms.cpp', 'driver_silhouette'))
    host_objs, procs = [], []
    for unit in build_ext.UNITS:          # every unit of the library, host side only
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
    subprocess.run([CLANG, *flags, '-I', os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'asan', 'driver_silhouette.cpp'), syms,
                    *host_objs, stub_o, '-o', exe, '-lpthread'], check=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    for seed in (1, 2, 3):
        r = subprocess.run([exe, '100', str(seed)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        assert 'no memory error' in r.stdout and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
        assert int(re.search(r'reported as DCTFP_ERR_HIP: (\d+)', r.stdout).group(1)) == 100, r.stdout
        assert int(re.search(r'launches the stub refused for their shape: (\d+)', r.stdout).group(1)) == 0, r.stdout
        report = {}
        for m in re.finditer(r'^export (dctfp_\w+): (\d+) calls, (\d+) ok, (\d+) ok with a launch, refused invalid (\d+) shape (\d+) limit (\d+) '
                             r'unsupported (\d+), nomem (\d+) hip (\d+), limit rows (\d+) of (\d+)$', r.stdout, re.M):
            report[m.group(1)] = [int(x) for x in m.groups()[1:]]
        for name in _exports():
            if name in NOT_DRIVEN:
                continue
            assert name in report, f'{name} is exported by include/dctfp_silhouette.h and never called by tests/asan/driver_silhouette.cpp'
            calls, ok, launching, invalid, shape, limit, unsupported, nomem, hip, rows_ok, rows_all = report[name]
            assert launching >= 100 and invalid >= 1000 and limit >= 3 and hip == 100 and shape == unsupported == nomem == 0, (name, report[name])
            # cap, pass_clusters and n_nodes at both ends, n_clusters, rows, columns and ld at their largest
            assert rows_ok == rows_all == 9, (name, report[name])
