"""The hit-statistics calls from a plain C99 client (tests/c/stats_client.c) compiled against
include/swbank.h and linked to libswbank.so: the macros, the struct, the fit, the reference's
bits and E and the NULL-bank errors on the host; sw_estimate_statistics on the GPU for
query100 x data500, equal to the Python call and within the fit's tolerances of the CPU
reference (tests/stat_cases.py)."""
import os
import subprocess

import pytest

import swbank as S
from oracle import oracle as O

import stat_cases as SC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "c", "stats_client.c")


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stats") / "stats_client")
    libdir = os.path.dirname(S.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "include"), SRC, "-o", exe, "-L", libdir,
                    "-lswbank", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_c_client_host_checks(client):
    r = subprocess.run([client, "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    hits = SC.golden_stats()[4]
    assert r.stdout.splitlines() == [f"{h[3]} {h[4]}" for h in hits] + ["host ok"]


@pytest.mark.gpu
def test_c_client_estimate(client):
    r = subprocess.run([client, "gpu", O.golden_fasta("query100.fa"),
                        O.golden_fasta("data500.fa"), "8", "100"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    q, res, offs, lens = SC.golden()
    assert lines[0] == f"kernel stats rounds=8 nq=1 n={len(lens)} slices=1" and lines[-1] == "stats ok"
    lam, K, ns = lines[1].split()
    want_lam, want_K, _ = SC.fit(*SC.golden_hist(100, 8), len(q))
    assert abs(float(lam) - want_lam) <= 1e-9 * want_lam
    assert abs(float(K) - want_K) <= 1e-6 * want_K
    assert int(ns) == 8 * len(lens)
    with S.ScoreBank() as bank:
        bank.set_penalties(*SC.REF)
        bank.load_query(q)
        (st,) = bank.estimate_statistics(res, offs, lens, seed=100, rounds=8)
    assert (float(lam), float(K)) == (st.lambda_, st.K)
