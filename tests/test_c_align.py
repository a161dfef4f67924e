"""The alignment calls from a plain C99 client (tests/c/align_client.c) compiled against
include/swbank.h and linked to libswbank.so: sw_cigar_string on the host, sw_align_hits on the
GPU for the db211 row of tests/golden/alignments500.tsv."""
import os
import subprocess

import pytest

import swbank as S
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "c", "align_client.c")


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("align") / "align_client")
    libdir = os.path.dirname(S.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "include"), SRC, "-o", exe, "-L", libdir,
                    "-lswbank", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_c_client_cigar_string(client):
    r = subprocess.run([client, "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "host ok"


@pytest.mark.gpu
def test_c_client_aligns_db211(client):
    rows = [ln.rstrip("\n").split("\t")
            for ln in open(os.path.join(O.GOLDEN, "alignments500.tsv"))][1:]
    row = next(r for r in rows if r[0] == "db211")
    r = subprocess.run([client, "align", O.golden_fasta("query100.fa"),
                        O.golden_fasta("data500.fa"), "db211"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "kernel align i32 hits=2 chunks=1" and lines[-1] == "align ok"
    assert lines[1].split() == row[1:]
