"""The global-local search from a plain C99 client (tests/c/glocal_client.c) compiled against
include/swbank.h and linked to libswbank.so: the new constants and the NULL-bank refusal on the
host; on the GPU sw_score_glocal over DNA targets on both strands, every score, end position and
strand against the C model of tests/glocal_cases.py, and the refusals the client checks on its
way."""
import os
import subprocess

import numpy as np
import pytest

import swbank as S

import glocal_cases as G
import strand_cases as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "c", "glocal_client.c")
LETTERS = "TCAGN"  # sw_encode_ascii: A=2 G=3 T=0 C=1 N=4


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("glocal") / "glocal_client")
    libdir = os.path.dirname(S.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "include"), SRC, "-o", exe, "-L", libdir,
                    "-lswbank", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_c_client_constants(client):
    r = subprocess.run([client, "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "host ok"


@pytest.mark.gpu
@pytest.mark.parametrize("ends", G.MODES)
def test_c_client_scores_end_to_end(client, ends):
    rng = np.random.default_rng(331)
    q = rng.integers(0, 4, 80).astype(np.uint8)
    whole = np.concatenate([rng.integers(0, 4, 12), q, rng.integers(0, 4, 7)]).astype(np.uint8)
    seqs = [whole, SC.revcomp(whole), q[40:].copy(), q[:40].copy(), np.delete(q, [20, 21, 22]),
            SC.revcomp(np.insert(q, 33, [1, 2])), rng.integers(0, 5, 90).astype(np.uint8),
            np.array([0, 4], np.uint8), q.copy()]
    n = len(seqs)
    sc, ep, sd = G.c_search(q, seqs, G.dna(), *G.DNA_PEN, ends, True)
    assert sd.tolist()[:2] == [0, 1] and (sc < 0).any()
    if ends == G.QUERY:
        assert sc.tolist()[:2] == [400, 400] and ep.tolist()[:2] == [91, len(whole) - 1 - 91]
    # (an empty string cannot be an argument's target here: every target has a residue)
    r = subprocess.run([client, "search", str(ends), "".join(LETTERS[c] for c in q)] +
                       ["".join(LETTERS[int(c)] for c in s) for s in seqs],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"kernel glocal ends={ends} nq=1 n={n}"
    assert lines[-1] == "search ok" and len(lines) == n + 2
    for k in range(n):
        end = "none" if int(ep[k]) == G.END_NONE else str(int(ep[k]))
        assert lines[1 + k].split() == ["S", str(k), str(int(sc[k])), end, str(int(sd[k]))]
