"""The frameshift-tolerant translated search from a plain C99 client (tests/c/fshift_client.c)
compiled against include/swbank.h and linked to libswbank.so: the new constants on the host; on
the GPU sw_score_fshift over DNA targets holding the query with a base inserted or removed, on
either strand, every score and strand against the C model of tests/fshift_cases.py, and the
refusals the client checks on its way."""
import os
import subprocess

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import frame_cases as F
import fshift_cases as FS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "c", "fshift_client.c")
LETTERS = "TCAGN"  # sw_encode_ascii: A=2 G=3 T=0 C=1 N=4


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fshift") / "fshift_client")
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
def test_c_client_follows_frameshifts(client):
    rng = np.random.default_rng(157)
    made = [FS.shift_case(rng, kind, rev) for kind in ("ins", "del") for rev in (False, True)]
    q = made[0][0]
    core = F.back_translate(rng, q)
    seqs = [made[0][1], F.SC.revcomp(made[0][1]), np.insert(core, 61, 3), np.delete(core, 30),
            F.SC.revcomp(np.delete(core, 30)), core, np.zeros(0, np.uint8),
            np.array([0, 4], np.uint8), rng.integers(0, 5, 90).astype(np.uint8)]
    n = len(seqs)
    want_sc, want_sd = FS.c_search(q, seqs, O.BLOSUM62, *F.PEN, -15)
    six, _ = FS.six_frames(q, seqs)
    assert want_sd.tolist()[:6] == [0, 1, 0, 0, 1, 0] and want_sc[5] == F.self_score(q)
    assert (want_sc[:5] > six[:5]).all() and want_sc[6] == want_sc[7] == 0
    r = subprocess.run([client, "search", "-15", "".join(O.PROT_LETTERS[c] for c in q)] +
                       ["".join(LETTERS[int(c)] for c in s) for s in seqs],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"kernel fshift nq=1 n={n}"
    assert lines[-1] == "search ok" and len(lines) == n + 2
    for k in range(n):
        assert lines[1 + k].split() == ["S", str(k), str(int(want_sc[k])), str(int(want_sd[k]))]
