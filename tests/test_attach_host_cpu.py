"""What functionals and quadratics of the resident IMEX loop do on the host
alone (`csrc/attach_host.hpp`): the stacked sparse rows against a dense
statement, the sum of the workgroups' shares in index order, and every argument
check of the two setters that needs no device -- one input per condition, the
message compared with the literal text -- compiled WITHOUT HIP under
AddressSanitizer + UndefinedBehaviorSanitizer into a program of its own
(`tests/attach_host_sanitize.cpp`).  No device."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, 'dolfin_navier_scipy_amd', 'csrc')


def test_header_is_a_dependency_and_free_of_hip():
    from dolfin_navier_scipy_amd import build
    assert os.path.join(CSRC, 'attach_host.hpp') in build.dependencies()
    text = open(os.path.join(CSRC, 'attach_host.hpp')).read()
    assert '#include "status.hpp"' in text
    assert 'hip/' not in text and 'common.hpp' not in text


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_host_parts_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / 'attach_host_sanitize')
    build = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror',
         '-I' + os.path.join(ROOT, 'include'),
         os.path.join(HERE, 'attach_host_sanitize.cpp'), '-o', exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert build.returncode == 0, build.stdout.decode()[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0',
               UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=600)
    out = run.stdout.decode()
    assert run.returncode == 0, out[-4000:]
    assert 'all checks passed' in out
    assert 'runtime error' not in out and 'AddressSanitizer' not in out, out
