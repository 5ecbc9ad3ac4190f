"""csrc/lte_dispatch.h, the launchers' run-time value -> template argument
helpers, checked on the host: dispatch_check.cpp (plain C++17, no HIP) is built
with the host compiler and run.  It asserts that every listed value reaches the
callable as that exact constant, usable as an array bound and a template
argument, that an unlisted value calls nothing and reports no match, and that
the fallback forms take their fallback."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'ofdm-lte_amd', 'csrc')


def _host_cxx():
    for c in (os.environ.get('CXX'), 'g++', 'c++', 'clang++'):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_dispatch_helpers(tmp_path):
    cxx = _host_cxx()
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = tmp_path / 'dispatch_check'
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I', CSRC,
                    os.path.join(HERE, 'dispatch_check.cpp'), '-o', str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stdout + r.stderr
