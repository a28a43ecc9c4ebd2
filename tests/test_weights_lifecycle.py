"""csrc/weights.hip.h on the CPU: tools/weights_lifecycle.cpp (a program of its own, the header's two HIP calls stubbed) built with
AddressSanitizer + UBSan and run.  Its asserts keep `users` exact through share / leave / re-finalize / either destroy order."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_weights_lifecycle_program_runs_clean_under_sanitizers(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'weights_lifecycle')
    subprocess.run([cxx, '-std=c++17', '-g', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    os.path.join(ROOT, 'tools', 'weights_lifecycle.cpp'), '-o', exe], check=True, timeout=120)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'ok' in run.stdout
