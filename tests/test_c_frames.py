"""The translated-search calls from a plain C99 client (tests/c/frame_client.c) compiled against
include/swbank.h and linked to libswbank.so: the new constants and sw_translate_codes on the host;
on the GPU sw_score_frames and sw_align_frame_hits over DNA targets holding the query in every
frame, every score against the oracle on the model's translations and every record against the
brute-force coordinates and the reference traceback on the translation of the hit's frame."""
import os
import subprocess

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_cases as AL
import align_check as AC
import frame_cases as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "c", "frame_client.c")
LETTERS = "TCAGN"  # sw_encode_ascii: A=2 G=3 T=0 C=1 N=4


@pytest.fixture(scope="module")
def client(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame") / "frame_client")
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
def test_c_client_searches_six_frames(client):
    rng = np.random.default_rng(29)
    q = rng.integers(0, 20, 40).astype(np.uint8)
    made = [F.plant(rng, q, 200, o, rev) for rev in (False, True) for o in range(3)]
    core = np.delete(F.back_translate(rng, q), slice(60, 66))  # two codons gone: a gapped path
    gapped = np.concatenate([rng.integers(0, 4, 10), core, rng.integers(0, 4, 7)]).astype(np.uint8)
    seqs = [t for t, _ in made] + [gapped, np.zeros(0, np.uint8), np.array([0, 4], np.uint8),
                                   rng.integers(0, 5, 90).astype(np.uint8)]
    n = len(seqs)
    sub, (go, ge) = O.BLOSUM62, F.PEN
    best, frame = F.merge6(F.oracle_frames(q, seqs))
    assert frame.tolist()[:7] == [0, 1, 2, 3, 4, 5, 1] and best[7] == best[8] == 0
    assert best.tolist()[:6] == [F.self_score(q)] * 6
    own = [F.translate(s, int(frame[k])) for k, s in enumerate(seqs)]
    brute = AC.brute_ends_batch(O, q, own, sub, go, ge, S.GAP_GOTOH)
    paths = AL.ref_paths(q, own, brute, sub, go, ge, S.GAP_GOTOH)

    def want(k):
        flag = F.frame_flags(int(frame[k]))
        if brute[k][0] == 0:
            return [k, 0, S.ALIGN_EMPTY | flag, 0, 0, 0, 0, 0, 0, "-"]
        s, qs, qe, a_start, a_end = brute[k]
        ts, te = F.nt_coords(a_start, a_end, int(frame[k]), len(seqs[k]))
        p = paths[k]
        return [k, s, flag, qs, qe, ts, te, p.n_columns, p.n_identities, S.cigar_string(p.ops)]

    r = subprocess.run([client, "search", "".join(O.PROT_LETTERS[c] for c in q)] +
                       [_text(s) for s in seqs], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"kernel frames nq=1 n={n} slices=1"
    assert lines[-1] == "search ok" and len(lines) == 2 * n + 3
    for k in range(n):
        assert lines[1 + k].split() == ["S", str(k), str(int(best[k])), str(int(frame[k]))]
    assert lines[1 + n].startswith(f"kernel align-frame i32 nq=1 hits={n} chunks=")
    for k in range(n):
        f = lines[2 + n + k].split()
        assert f[:2] == ["A", str(k)]
        assert [int(x) for x in f[2:11]] + [f[11]] == want(k), (f, want(k))
    assert want(0)[-1] == "40M" and "I" in want(6)[-1]
