"""The non-intersecting alignments over reading frames from a plain C99 client
(tests/c/disjoint_frames_client.c) compiled against include/swbank.h and linked to libswbank.so:
what the header promises on the host without a device; on the GPU every record and CIGAR of the
client against the C composition of tests/disjoint_frames_cases.py."""
import os
import subprocess

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import disjoint_cases as D
import disjoint_frames_cases as DF

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "c", "disjoint_frames_client.c")
LETTERS = "TCAGN"  # sw_encode_ascii: A=2 G=3 T=0 C=1 N=4


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("disjoint_frames") / "disjoint_frames_client")
    libdir = os.path.dirname(S.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "include"), SRC, "-o", exe, "-L", libdir,
                    "-lswbank", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def _dna(codes):
    return "".join(LETTERS[int(c)] for c in codes)


def _protein(codes):
    return "".join(O.PROT_LETTERS[int(c)] for c in codes)


def _case():
    q, t = DF.exon_case(60, seed=13)
    rng = np.random.default_rng(577)
    seqs = [t, DF.tie_case()[1], np.zeros(0, np.uint8), np.array([4, 4], np.uint8),
            rng.integers(0, 4, 90).astype(np.uint8), t[:100]]
    return q, seqs


def test_c_client_header(client):
    r = subprocess.run([client, "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "host ok"


@pytest.mark.gpu
@pytest.mark.parametrize("rounds, min_score", [(4, 20), (3, 100)])
def test_c_client_aligns_over_the_frames(client, rounds, min_score):
    q, seqs = _case()
    n = len(seqs)
    want = [DF.c_merged(q, t, O.BLOSUM62, *DF.PEN, rounds, min_score) for t in seqs]
    assert want[2] == [D.EMPTY_REC] * rounds and len(set(DF.frames(want[0])[:3])) == 3
    r = subprocess.run([client, "align", str(rounds), str(min_score), _protein(q)] +
                       [_dna(s) for s in seqs], capture_output=True, text=True,
                       env=dict(os.environ, SWBANK_POISON="1"))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"kernel align-disjoint-frames i32 rounds={rounds} nq=1 hits={n} chunks=1"
    assert lines[-1] == "align ok" and len(lines) == n * rounds + 2
    for k, w in enumerate(want):
        for x, (rec, ops) in enumerate(w):
            assert lines[1 + k * rounds + x].split() == ["A", str(k), str(x)] + \
                [str(v) for v in rec] + [D.cigar(ops) if ops else "*"], (k, x)
