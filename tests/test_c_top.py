"""The top-hits calls from a plain C99 client (tests/c/top_client.c) compiled against
include/swbank.h and linked to libswbank.so: the macros and NULL-bank errors on the host,
sw_score_batch + sw_top_hits on the GPU for the 12 best of query100 x data500."""
import os
import subprocess

import pytest

import swbank as S
from oracle import oracle as O

import top_cases as TC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "c", "top_client.c")


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("top") / "top_client")
    libdir = os.path.dirname(S.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "include"), SRC, "-o", exe, "-L", libdir,
                    "-lswbank", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_c_client_host_checks(client):
    r = subprocess.run([client, "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "host ok"


@pytest.mark.gpu
def test_c_client_top12(client):
    r = subprocess.run([client, "gpu", O.golden_fasta("query100.fa"),
                        O.golden_fasta("data500.fa"), "12"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    n = len(O.read_fasta(O.golden_fasta("data500.fa")))
    assert lines[0] == f"kernel top k=12 nq=1 n={n}" and lines[-1] == "top ok"
    assert [tuple(ln.split()) for ln in lines[1:-1]] == [(a, str(b)) for a, b in TC.GOLDEN_TOP12]
