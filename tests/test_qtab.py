"""The query tables (csrc/swbank_qtab.h, header-inline, host-only: the code prepare*() of
libswbank.so run) compiled into a CPU harness (tests/c/qtab_check.cc) with the ROCm host clang
(the header needs _Float16).  Per case of tests/c/qtab_cases.h the harness decodes every table by
its documented layout and compares each entry with the matrix, and compares a digest of the
tables in upload order, the stored scalars and every refusal with tests/golden/qtab_digests.tsv,
which was recorded from the library as it was before the builders moved into the header."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "smith-waterman-fpga-module_amd")
CSRC = os.path.join(PKG, "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "qtab_digests.tsv")


def _clang():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("amdclang++")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("the ROCm host clang++ was not found")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("qtab")
    exe, host = str(d / "qtab_check"), str(d / "swbank_host.o")
    inc = ["-I", CSRC, "-I", os.path.join(REPO, "include")]
    cxx = _clang()
    # sw_fill_matrix (the case list's matrices) comes from the library's own C unit
    subprocess.run([cxx, "-x", "c", "-std=c11", "-O2", *inc, "-c",
                    os.path.join(CSRC, "swbank_host.c"), "-o", host], check=True)
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", *inc,
                    os.path.join(REPO, "tests", "c", "qtab_check.cc"), host, "-lm", "-o", exe],
                   check=True)
    return exe


def test_tables_vs_matrix_and_parent_digests(harness):
    r = subprocess.run([harness, GOLDEN], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("qtab ok ("), r.stdout
