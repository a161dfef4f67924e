"""The alignments of global-local hits from a plain C99 client (tests/c/glalign_client.c) compiled
against include/swbank.h and linked to libswbank.so: what the header promises on the host; on
the GPU sw_align_glocal_hits over DNA targets on either strand in all three modes, every record
and CIGAR against the C model of tests/glalign_cases.py, each record against the score call's
outputs, and the refusals the client checks on its way."""
import os
import subprocess

import numpy as np
import pytest

import swbank as S

import glalign_cases as A
import glocal_cases as G
import strand_cases as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "c", "glalign_client.c")
LETTERS = "TCAGN"  # sw_encode_ascii: A=2 G=3 T=0 C=1 N=4


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("glalign") / "glalign_client")
    libdir = os.path.dirname(S.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "include"), SRC, "-o", exe, "-L", libdir,
                    "-lswbank", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_c_client_header(client):
    r = subprocess.run([client, "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "host ok"


@pytest.mark.gpu
@pytest.mark.parametrize("ends", G.MODES)
def test_c_client_aligns_global_local_hits(client, ends):
    rng = np.random.default_rng(383)
    q = rng.integers(0, 4, 60).astype(np.uint8)
    flank = lambda n: rng.integers(0, 4, n).astype(np.uint8)  # noqa: E731
    seqs = [np.concatenate([flank(7), q, flank(5)]), SC.revcomp(np.concatenate([flank(3), q[4:]])),
            np.delete(q, [30, 31]), np.insert(q[10:50], 20, [1, 2]), SC.revcomp(q[:-5]),
            np.zeros(0, np.uint8), np.array([4], np.uint8), flank(90)]
    seqs = [np.asarray(s, np.uint8) for s in seqs]
    n = len(seqs)
    want = [A.c_align(q, t, G.dna(), *G.DNA_PEN, ends, True) for t in seqs]
    assert want[5][0][1] == S.ALIGN_EMPTY and any(w[0][1] & S.ALIGN_REVERSE for w in want)
    if ends == A.QUERY:
        assert A.cigar(want[3][1]) == "10I20M2D20M10I"  # (it begins and ends with a gap)
    r = subprocess.run([client, "align", str(ends), "".join(LETTERS[c] for c in q)] +
                       ["".join(LETTERS[int(c)] for c in s) for s in seqs],
                       capture_output=True, text=True, env=dict(os.environ, SWBANK_POISON="1"))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"kernel align-glocal i32 ends={ends} nq=1 hits={n} chunks=1"
    assert lines[-1] == "align ok" and len(lines) == n + 2
    for k, (rec, ops) in enumerate(want):
        assert lines[1 + k].split() == ["A", str(k)] + [str(x) for x in rec] + \
            [A.cigar(ops) if ops else "*"], (k, lines[1 + k])
