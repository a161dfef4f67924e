"""swbank -G q|t|b: the CLI scores the query, every record or both end to end (sw_score_glocal),
prints negative scores as they are, with -B searches both strands and prints " [f]" or " [r]"
after every score (the C model of tests/glocal_cases.py says which), and refuses -G with -A, -E,
-S, -X or -F, or with anything but q, t or b, with a message naming the reason."""
import subprocess

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import glocal_cases as G
import strand_cases as SC

DNA = "TCAGN"
PROT = "".join(O.PROT_LETTERS)


def _fasta(path, recs):
    path.write_text("".join(f">{n}\n{s}\n" for n, s in recs))
    return str(path)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("glocalcli")
    rng = np.random.default_rng(317)
    q = rng.integers(0, 4, 60).astype(np.uint8)
    seqs = [np.concatenate([rng.integers(0, 4, 20), q, rng.integers(0, 4, 15)]).astype(np.uint8),
            rng.integers(0, 5, 150).astype(np.uint8), q[10:50].copy(),
            np.array([2, 0], np.uint8),
            SC.revcomp(np.concatenate([rng.integers(0, 4, 9), np.delete(q, [30, 31])])), q.copy()]
    names = [f"nt{k}" for k in range(len(seqs))]
    qf = _fasta(d / "q.fa", [("read", "".join(DNA[c] for c in q))])
    lf = _fasta(d / "lib.fa", [(n, "".join(DNA[c] for c in s)) for n, s in zip(names, seqs)])
    pq = rng.integers(0, 20, 30).astype(np.uint8)
    pseqs = [np.concatenate([rng.integers(0, 20, 7), pq, rng.integers(0, 20, 5)]).astype(np.uint8),
             rng.integers(0, 20, 40).astype(np.uint8), pq[5:25].copy()]
    pqf = _fasta(d / "pq.fa", [("prot", "".join(PROT[c] for c in pq))])
    plf = _fasta(d / "plib.fa", [(f"aa{k}", "".join(PROT[c] for c in s))
                                 for k, s in enumerate(pseqs)])
    return qf, lf, q, names, seqs, pqf, plf, pq, pseqs


@pytest.mark.parametrize("extra, words", [
    (["-G", "q", "-A", "2"], ["-G", "-A", "alignments"]),
    (["-G", "t", "-E", "20"], ["-G", "-E", "statistics"]),
    (["-G", "b", "-S", "0.267,0.041"], ["-G", "-S", "statistics"]),
    (["-G", "q", "-X"], ["-G", "-X", "local"]),
    (["-G", "q", "-X", "-F", "-15"], ["-G", "-F", "local"]),
    (["-G", "x"], ["-G", "q", "t", "b"]),
    (["-G", "qt"], ["-G", "q", "t", "b"]),
])
def test_cli_refuses(files, extra, words):
    qf, lf = files[:2]
    r = subprocess.run([S.CLI_PATH, "-q", qf, "-l", lf] + extra, capture_output=True, text=True)
    assert r.returncode == 1 and "usage" in r.stderr and r.stdout == ""
    first = r.stderr.splitlines()[0]
    assert all(w in first for w in words), first


@pytest.mark.gpu
@pytest.mark.parametrize("mode, ends", [("q", G.QUERY), ("t", G.TARGET), ("b", G.BOTH)])
def test_cli_global_local_search(files, mode, ends):
    qf, lf, q, names, seqs = files[:5]
    n = len(seqs)
    for both in (True, False):
        want_sc, _, want_sd = G.c_search(q, seqs, G.dna(), *G.DNA_PEN, ends, both)
        assert (want_sc < 0).any()  # no floor
        if ends == G.QUERY and both:
            assert want_sc.tolist()[0::5] == [300, 300] and want_sd.tolist()[4] == 1
        # -G implies -g: no -g given
        r = subprocess.run([S.CLI_PATH, "-q", qf, "-l", lf, "-G", mode, "-b"] +
                           (["-B"] if both else []), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        tag = [f" [{'r' if want_sd[k] else 'f'}]" if both else "" for k in range(n)]
        assert r.stdout.splitlines() == [
            f">{names[k]} score: {int(want_sc[k])}{tag[k]}" for k in range(n)]
        b = int(np.argmax(want_sc))  # (the lowest index with the best score)
        assert r.stderr.strip() == f"best: >{names[b]} score: {int(want_sc[b])}{tag[b]}"


@pytest.mark.gpu
def test_cli_global_local_search_of_proteins(files):
    pqf, plf, pq, pseqs = files[5:]
    want_sc = G.c_search(pq, pseqs, O.BLOSUM62, *G.PROT_PEN, G.QUERY)[0]
    r = subprocess.run([S.CLI_PATH, "-q", pqf, "-l", plf, "-P", "-G", "q"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == [f">aa{k} score: {int(s)}" for k, s in enumerate(want_sc)]
    r = subprocess.run([S.CLI_PATH, "-q", pqf, "-l", plf, "-P", "-G", "q", "-B"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "-B" in r.stderr.splitlines()[0]  # -B searches DNA strands
