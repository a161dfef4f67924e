"""The query-set calls from a plain C99 client (tests/c/align_set_client.c) compiled against
include/swbank.h and linked to libswbank.so: the new constants on the host; on the GPU a
two-query set through sw_align_set_hits in both hit-query forms and sw_best_queries between
them, every record against the brute-force coordinates and the reference traceback."""
import os
import subprocess

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_cases as AL
import align_check as AC
import set_cases as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "c", "align_set_client.c")
LETTERS = "TCAG"  # sw_encode_ascii: A=2 G=3 T=0 C=1


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("align_set") / "align_set_client")
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


def _record(fields):
    """index score flags q_start q_end t_start t_end columns identities cigar"""
    return [int(x) for x in fields[:9]] + [fields[9]]


@pytest.mark.gpu
def test_c_client_aligns_a_set(client):
    rng = np.random.default_rng(21)
    queries = [rng.integers(0, 4, 120).astype(np.uint8), rng.integers(0, 4, 70).astype(np.uint8)]
    queries[0][queries[0] == 2] = 3  # no A in the queries: the all-A target scores 0 against both
    queries[1][queries[1] == 2] = 1
    seqs = [AL.planted(rng, queries[0], 90), AL.planted(rng, queries[1], 64),
            AL.planted(rng, queries[1], 130), np.full(12, 2, np.uint8),
            AL.planted(rng, queries[0], 200)]
    assert [_text(O.encode_dna(_text(s))) for s in seqs] == [_text(s) for s in seqs]
    n = len(seqs)
    sub = O.dna_matrix()
    brute = [AC.brute_ends_batch(O, q, seqs, sub, -12, -4, S.GAP_MERGED) for q in queries]
    paths = [AL.ref_paths(q, seqs, b, sub, -12, -4, S.GAP_MERGED) for q, b in zip(queries, brute)]

    def want(qi, t):
        s, qs, qe, ts, te = brute[qi][t]
        if s == 0:
            return [t, 0, S.ALIGN_EMPTY, 0, 0, 0, 0, 0, 0, "-"]
        p = paths[qi][t]
        return [t, s, 0, qs, qe, ts, te, p.n_columns, p.n_identities, S.cigar_string(p.ops)]

    r = subprocess.run([client, "align"] + [_text(q) for q in queries] + [_text(s) for s in seqs],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith(f"kernel align-set i32 nq=2 hits={2 * n} chunks=")
    assert lines[-1] == "align ok" and len(lines) == 3 * n + 3
    for h in range(2 * n):
        f = lines[1 + h].split()
        assert f[:2] == ["A", str(h)] and _record(f[2:]) == want(h // n, h % n), f
    assert lines[1 + 2 * n] == f"kernel best-query nq=2 n={n}"
    scores = np.array([[b[0] for b in brute[0]], [b[0] for b in brute[1]]], np.int32)
    bq, bs = SC.ref_best(scores, 1)
    assert int((bq == SC.QUERY_NONE).sum()) == 1 and len(set(bq.tolist())) == 3
    for k in range(n):
        f = lines[2 + 2 * n + k].split()
        assert f[:2] == ["B", str(k)]
        if bq[k] == SC.QUERY_NONE:
            assert [int(f[2]), int(f[3])] == [-1, SC.INT32_MIN]
            assert _record(f[4:]) == [-1, 0, S.ALIGN_EMPTY | S.ALIGN_NO_HIT, 0, 0, 0, 0, 0, 0, "-"]
        else:
            assert [int(f[2]), int(f[3])] == [int(bq[k]), int(bs[k])]
            assert _record(f[4:]) == want(int(bq[k]), k), f
