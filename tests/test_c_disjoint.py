"""The non-intersecting local alignments from a plain C99 client (tests/c/disjoint_client.c)
compiled against include/swbank.h and linked to libswbank.so, and from the swbank CLI's -N: what
the header promises on the host and the CLI's refusals without a device; on the GPU every record
and CIGAR of the client against the C model of tests/disjoint_cases.py, and the CLI's -A 2 -N 3
against the Python call."""
import os
import subprocess

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import disjoint_cases as D
import glocal_cases as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "c", "disjoint_client.c")
LETTERS = "TCAGN"  # sw_encode_ascii: A=2 G=3 T=0 C=1 N=4


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("disjoint") / "disjoint_client")
    libdir = os.path.dirname(S.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "include"), SRC, "-o", exe, "-L", libdir,
                    "-lswbank", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def _text(codes):
    return "".join(LETTERS[int(c)] for c in codes)


def _case():
    q, t, _ = D.copies_case()
    q2, t2 = D.repeat_case()
    rng = np.random.default_rng(457)
    seqs = [t, np.concatenate([q[10:50], rng.integers(0, 4, 7), q[10:50]]).astype(np.uint8),
            np.zeros(0, np.uint8), np.array([4], np.uint8), rng.integers(0, 4, 90).astype(np.uint8),
            t2]
    return q, seqs


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("disjoint_cli")
    q, seqs = _case()
    qf, lf = str(d / "q.fa"), str(d / "lib.fa")
    with open(qf, "w") as f:
        f.write(f">query\n{_text(q)}\n")
    with open(lf, "w") as f:
        for k, s in enumerate(seqs):
            f.write(f">rec{k}\n{_text(s)}\n")
    return qf, lf


def test_c_client_header(client):
    r = subprocess.run([client, "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "host ok"


@pytest.mark.parametrize("extra, words", [
    (["-N", "3"], ["-N", "-A"]),                          # without -A
    (["-A", "2", "-N", "3", "-B"], ["-N", "-B"]),
    (["-A", "2", "-N", "3", "-X"], ["-N", "-X"]),
    (["-A", "2", "-N", "3", "-G", "q"], ["-G"]),          # (-G refuses -A first)
    (["-A", "2", "-N", "0"], ["-N", "rounds"]),
    (["-A", "2", "-N", "65"], ["-N", "rounds"]),
    (["-A", "2", "-N", "3,0"], ["-N", "min"]),
    (["-A", "2", "-N", "x"], ["-N", "rounds"]),
])
def test_cli_refuses(files, extra, words):
    qf, lf = files
    r = subprocess.run([S.CLI_PATH, "-q", qf, "-l", lf] + extra, capture_output=True, text=True)
    assert r.returncode == 1 and "usage" in r.stderr and r.stdout == ""
    first = r.stderr.splitlines()[0]
    assert all(w in first for w in words), first


@pytest.mark.gpu
@pytest.mark.parametrize("rounds, min_score", [(3, 1), (4, 200)])
def test_c_client_aligns_disjoint_hits(client, rounds, min_score):
    q, seqs = _case()
    n = len(seqs)
    want = [D.c_rounds(q, t, G.dna(), *G.DNA_PEN, rounds, min_score) for t in seqs]
    assert want[2] == [D.EMPTY_REC] * rounds and sum(s > 0 for s in D.scores(want[0])) >= 3
    r = subprocess.run([client, "align", str(rounds), str(min_score), _text(q)] +
                       [_text(s) for s in seqs], capture_output=True, text=True,
                       env=dict(os.environ, SWBANK_POISON="1"))
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"kernel align-disjoint i32 rounds={rounds} nq=1 hits={n} chunks=1"
    assert lines[-1] == "align ok" and len(lines) == n * rounds + 2
    for k, w in enumerate(want):
        for x, (rec, ops) in enumerate(w):
            assert lines[1 + k * rounds + x].split() == ["A", str(k), str(x)] + \
                [str(v) for v in rec] + [D.cigar(ops) if ops else "*"], (k, x)


@pytest.mark.gpu
def test_cli_lists_the_next_best_alignments(files):
    """swbank -A 2 -N 3: under each of the two best records, round 0 as -A prints a hit and the
    further rounds numbered from 2, all as the Python call returns them."""
    qf, lf = files
    q, seqs = _case()
    r = subprocess.run([S.CLI_PATH, "-q", qf, "-l", lf, "-A", "2", "-N", "3"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    res, offs, lens = S.pack_targets(seqs)
    with S.ScoreBank(gap_model=O.GAP_GOTOH) as bank:
        bank.set_penalties(5, -4, -12, -4)
        bank.load_query(q)
        scores = bank.score_batch(res, offs, lens)
        order = sorted(range(len(seqs)), key=lambda k: (-int(scores[k]), k))[:2]
        got = bank.align_disjoint_hits(res, offs, lens, 3, hits=order, hits_per_query=2)
    assert lines[:len(seqs)] == [f">rec{k} score: {int(s)}" for k, s in enumerate(scores)]
    want = []
    for k, hit in zip(order, got):
        want += [f">>rec{k} ({len(seqs[k])} nt)", f" s-w opt: {hit[0].score}"]
        for x, a in enumerate(hit):
            if a.empty:
                break
            pct = 100.0 * a.n_identities / a.n_columns
            want += [("" if x == 0 else f"#{x + 1} ") +
                     f"Smith-Waterman score: {a.score}; {pct:.1f}% identity ({pct:.1f}% similar) in "
                     f"{a.n_columns} nt overlap ({a.q_start + 1}-{a.q_end + 1}:"
                     f"{a.t_start + 1}-{a.t_end + 1})", f"cigar: {a.cigar}"]
    assert lines[len(seqs):] == want
    assert sum(ln.startswith("#") for ln in lines) == 4 and order[0] == 0
