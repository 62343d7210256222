"""The host bookkeeping of models with several clusters (csrc/cluster_partition.h: row partition, gather and the scatter
of per-cluster predictions) in a stand-alone program: tests/host/cluster_partition_check.cpp, plain C++, no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.path.join(rocm, "llvm", "bin", "clang++"), shutil.which("c++"), shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    return None


def test_partition_and_scatter_program(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.fail("no C++ compiler found (the library's build needs one too)")
    exe = str(tmp_path / "cluster_partition_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", f"-I{os.path.join(ROOT, 'gpboost_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "host", "cluster_partition_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "cluster_partition_check ok" in r.stdout
