"""csrc/dispatch.h on the CPU: with_bool / with_int, the runtime-value -> template-argument
dispatchers every launcher goes through.  dispatch_check.cpp (its own main, no HIP) is built with
the host compiler and run; it checks that each listed value reaches its own constant, that the
functor runs exactly once, that an unlisted value calls nothing and returns false, and that two
levels nest."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), 'nesie_amd', 'csrc')


def test_dispatch_header(tmp_path):
    cxx = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if not cxx:
        pytest.fail('no host C++ compiler (CXX, g++, c++, clang++)')
    exe = str(tmp_path / 'dispatch_check')
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC,
                            os.path.join(HERE, 'dispatch_check.cpp'), '-o', exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == 'dispatch.h: ok'
