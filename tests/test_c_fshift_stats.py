"""The frameshift search's statistics from a plain C99 client (tests/c/fshift_stats_client.c)
compiled against include/swbank.h and linked to libswbank.so: the macro and the NULL-bank errors
on the host; on the GPU sw_estimate_fshift_statistics over the shared batch of
tests/fshift_stats_cases.py, its counters equal to the reference pipeline's and lambda and K
within the fit's tolerances (tests/test_gpu_stats.py), the refusals the client checks on its way,
and the bits and E of the search's best hit."""
import os
import subprocess

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import frame_cases as F
import fshift_cases as FS
import fshift_stats_cases as FSS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "c", "fshift_stats_client.c")
LETTERS = "TCAGN"  # sw_encode_ascii: A=2 G=3 T=0 C=1 N=4
LAMBDA_RTOL, K_RTOL, SIG_RTOL = 1e-9, 1e-6, 1e-10


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fshift_stats") / "fshift_stats_client")
    libdir = os.path.dirname(S.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "include"), SRC, "-o", exe, "-L", libdir,
                    "-lswbank", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_c_client_host_checks(client):
    r = subprocess.run([client, "host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "host ok"


@pytest.mark.gpu
def test_c_client_estimate(client):
    res, offs, lens = FSS.batch()
    (q,) = FSS.queries("one")
    seqs = FSS.targets_of(res, offs, lens)
    fs, seed = -15, 2
    (want,) = FSS.fitted("one", seed, fs)
    r = subprocess.run([client, "gpu", str(fs), str(FSS.ROUNDS), str(seed),
                        "".join(O.PROT_LETTERS[c] for c in q)] +
                       ["".join(LETTERS[int(c)] for c in s) for s in seqs],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"kernel fshift-stats rounds={FSS.ROUNDS} nq=1 n={len(lens)} slices=1"
    assert lines[-1] == "stats ok" and len(lines) == 4
    lam, K, ns, lo, hi, clamped = lines[1].split()
    assert (int(ns), int(lo), int(hi), int(clamped)) == want[2:]
    assert abs(float(lam) - want[0]) <= LAMBDA_RTOL * want[0]
    assert abs(float(K) - want[1]) <= K_RTOL * want[1]
    sc, _ = FS.c_search(q, seqs, O.BLOSUM62, *F.PEN, fs)
    best = int(np.argmax(sc))
    tag, k, s, bits, ev = lines[2].split()
    assert (tag, int(k), int(s)) == ("H", best, int(sc[best]))
    lam, K, top = float(lam), float(K), float(sc[best])
    assert top > 0
    assert np.isclose(float(bits), (lam * top - np.log(K)) / np.log(2.0), rtol=SIG_RTOL, atol=0)
    assert np.isclose(float(ev), len(lens) * K * len(q) * float(lens[best]) * np.exp(-lam * top),
                      rtol=SIG_RTOL, atol=0)
