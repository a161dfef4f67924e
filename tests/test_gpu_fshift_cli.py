"""swbank -X -F: the CLI follows hits across frameshifts (sw_score_fshift), prints " [f]" or
" [r]" after every score as -B does (the C model of tests/fshift_cases.py says which), and refuses
-F without -X or with -A, -E, -S or -B with a message naming the reason."""
import subprocess

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import frame_cases as F
import fshift_cases as FS

DNA = "TCAGN"


def _fasta(path, recs):
    path.write_text("".join(f">{n}\n{s}\n" for n, s in recs))
    return str(path)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("fshiftcli")
    rng = np.random.default_rng(163)
    made = [FS.shift_case(rng, "ins", True), FS.shift_case(rng, "del", False)]
    q = made[0][0]
    core = F.back_translate(rng, q)
    seqs = [made[0][1], rng.integers(0, 5, 150).astype(np.uint8), np.delete(core, 45),
            np.array([2, 0], np.uint8), F.SC.revcomp(np.insert(core, 31, 1)), core]
    names = [f"nt{k}" for k in range(len(seqs))]
    qf = _fasta(d / "q.fa", [("prot", "".join(O.PROT_LETTERS[c] for c in q))])
    lf = _fasta(d / "lib.fa", [(n, "".join(DNA[c] for c in s)) for n, s in zip(names, seqs)])
    return qf, lf, q, names, seqs


@pytest.mark.parametrize("extra, words", [
    (["-F", "-15"], ["-F", "-X"]),                       # without -X
    (["-X", "-F", "-15", "-A", "2"], ["-F", "-A", "alignments"]),
    (["-X", "-F", "-15", "-E", "20"], ["-F", "-E", "statistics"]),
    (["-X", "-F", "-15", "-S", "0.267,0.041"], ["-F", "-S", "statistics"]),
    (["-X", "-F", "-15", "-B"], ["-F", "-B", "strands"]),
    (["-X", "-F", "1"], ["-F", "-32767"]),               # outside 0 .. -32767
    (["-X", "-F", "-32768"], ["-F", "-32767"]),
    (["-X", "-F", "x"], ["-F", "-32767"]),
])
def test_cli_refuses(files, extra, words):
    qf, lf = files[:2]
    r = subprocess.run([S.CLI_PATH, "-q", qf, "-l", lf] + extra, capture_output=True, text=True)
    assert r.returncode == 1 and "usage" in r.stderr and r.stdout == ""
    first = r.stderr.splitlines()[0]
    assert all(w in first for w in words), first


@pytest.mark.gpu
@pytest.mark.parametrize("fs", [-15, 0])
def test_cli_frameshift_search(files, fs):
    qf, lf, q, names, seqs = files
    want_sc, want_sd = FS.c_search(q, seqs, O.BLOSUM62, *F.PEN, fs)
    six, _ = FS.six_frames(q, seqs)
    assert want_sd.tolist()[0::2] == [1, 0, 1] and want_sc[3] == 0
    assert all(want_sc[k] > six[k] for k in (0, 2, 4)) and want_sc[5] >= F.self_score(q)
    r = subprocess.run([S.CLI_PATH, "-q", qf, "-l", lf, "-X", "-F", str(fs), "-b"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    n = len(seqs)
    assert r.stdout.splitlines() == [
        f">{names[k]} score: {int(want_sc[k])} [{'r' if want_sd[k] else 'f'}]" for k in range(n)]
    b = int(np.argmax(want_sc))  # (the lowest index with the best score)
    assert r.stderr.strip() == \
        f"best: >{names[b]} score: {int(want_sc[b])} [{'r' if want_sd[b] else 'f'}]"
    # -X alone still prints the six-frame search's frame tags
    r6 = subprocess.run([S.CLI_PATH, "-q", qf, "-l", lf, "-X", "-g"], capture_output=True, text=True)
    assert r6.returncode == 0, r6.stderr
    assert [ln.split()[2] for ln in r6.stdout.splitlines()] == [str(int(s)) for s in six]
    assert all(ln.split()[-1][1] in "+-" for ln in r6.stdout.splitlines())
