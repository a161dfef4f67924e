"""The alignments of frameshift hits from a plain C99 client (tests/c/fsalign_client.c) compiled
against include/swbank.h and linked to libswbank.so: the new op codes and their text on the host;
on the GPU sw_align_fshift_hits over DNA targets holding the query with a base inserted or
removed, on either strand, every record and CIGAR against the C model of tests/fsalign_cases.py,
and the refusals the client checks on its way."""
import os
import subprocess

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import frame_cases as F
import fsalign_cases as A
import fshift_cases as FS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "c", "fsalign_client.c")
LETTERS = "TCAGN"  # sw_encode_ascii: A=2 G=3 T=0 C=1 N=4


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fsalign") / "fsalign_client")
    libdir = os.path.dirname(S.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "include"), SRC, "-o", exe, "-L", libdir,
                    "-lswbank", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_c_client_op_codes(client):
    r = subprocess.run([client, "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "host ok"


@pytest.mark.gpu
@pytest.mark.parametrize("poison", ["plain", "poison"])
def test_c_client_aligns_frameshift_hits(client, poison):
    rng = np.random.default_rng(157)
    made = [FS.shift_case(rng, kind, rev) for kind in ("ins", "del") for rev in (False, True)]
    q = made[0][0]
    core = F.back_translate(rng, q)
    seqs = [made[0][1], F.SC.revcomp(made[0][1]), np.insert(core, 61, 3), np.delete(core, 30),
            F.SC.revcomp(np.delete(core, 30)), core, np.zeros(0, np.uint8),
            np.array([0, 4], np.uint8), rng.integers(0, 5, 90).astype(np.uint8)]
    n = len(seqs)
    want = [A.c_align(q, t, O.BLOSUM62, *F.PEN, -15) for t in seqs]
    assert [S.cigar_string(w[1]) for w in want[:3]] == ["20M1/20M"] * 3
    assert "\\" in S.cigar_string(want[3][1]) and want[5][1] == (40 << 4,)
    assert want[6] == want[7] == A.EMPTY and want[1][0][1] & S.ALIGN_REVERSE
    r = subprocess.run([client, "align", "-15", "".join(O.PROT_LETTERS[c] for c in q)] +
                       ["".join(LETTERS[int(c)] for c in s) for s in seqs],
                       capture_output=True, text=True,
                       env=dict(os.environ, SWBANK_POISON="1" if poison == "poison" else "0"))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"kernel align-fshift i32 nq=1 hits={n} chunks=1"
    assert lines[-1] == "align ok" and len(lines) == n + 2
    for k, (rec, ops) in enumerate(want):
        assert lines[1 + k].split() == ["A", str(k)] + [str(x) for x in rec] + \
            [S.cigar_string(ops) if ops else "*"], (k, lines[1 + k])
