"""The both-strand calls from a plain C99 client (tests/c/strand_client.c) compiled against
include/swbank.h and linked to libswbank.so: the new constant and sw_revcomp_codes on the host;
on the GPU sw_score_strands and sw_align_strand_hits over targets of both strands, every score
against the oracle and every record against the brute-force coordinates and the reference
traceback on the strand's own target."""
import os
import subprocess

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_cases as AL
import align_check as AC
import strand_cases as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "c", "strand_client.c")
LETTERS = "TCAG"  # sw_encode_ascii: A=2 G=3 T=0 C=1


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("strand") / "strand_client")
    libdir = os.path.dirname(S.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "include"), SRC, "-o", exe, "-L", libdir,
                    "-lswbank", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_c_client_constants(client):
    r = subprocess.run([client, "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "host ok"


def _text(codes):
    return "".join(LETTERS[int(c)] for c in codes)


@pytest.mark.gpu
def test_c_client_searches_both_strands(client):
    rng = np.random.default_rng(23)
    q = rng.integers(0, 4, 120).astype(np.uint8)
    seqs = [AL.planted(rng, q, 90), SC.revcomp(AL.planted(rng, q, 64)),
            SC.revcomp(AL.planted(rng, q, 130)), np.tile(S.encode("ACGT"), 8),
            AL.planted(rng, q, 200), SC.revcomp(q)]
    n = len(seqs)
    sub = O.dna_matrix()
    fwd, rev = SC.oracle_strands(q, seqs)
    best, strand = SC.merge(fwd, rev)
    assert strand.tolist() == [0, 1, 1, 0, 0, 1] and fwd[3] == rev[3]  # (the palindrome ties)
    own = [SC.revcomp(s) if strand[k] else s for k, s in enumerate(seqs)]
    brute = AC.brute_ends_batch(O, q, own, sub, -12, -4, S.GAP_MERGED)
    paths = AL.ref_paths(q, own, brute, sub, -12, -4, S.GAP_MERGED)

    def want(k):
        flag = S.ALIGN_REVERSE if strand[k] else 0
        if brute[k][0] == 0:
            return [k, 0, S.ALIGN_EMPTY | flag, 0, 0, 0, 0, 0, 0, "-"]
        s, qs, qe, ts, te = SC.flip_ends(brute[k], len(seqs[k])) if strand[k] else brute[k]
        p = paths[k]
        return [k, s, flag, qs, qe, ts, te, p.n_columns, p.n_identities, S.cigar_string(p.ops)]

    r = subprocess.run([client, "search", _text(q)] + [_text(s) for s in seqs],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"kernel strands nq=1 n={n} slices=1"
    assert lines[-1] == "search ok" and len(lines) == 2 * n + 3
    for k in range(n):
        assert lines[1 + k].split() == ["S", str(k), str(int(best[k])), str(int(strand[k]))]
    assert lines[1 + n].startswith(f"kernel align-strand i32 nq=1 hits={n} chunks=")
    for k in range(n):
        f = lines[2 + n + k].split()
        assert f[:2] == ["A", str(k)]
        assert [int(x) for x in f[2:11]] + [f[11]] == want(k), (f, want(k))
    assert want(n - 1)[1] == 5 * len(q) and want(n - 1)[-1] == f"{len(q)}M"
