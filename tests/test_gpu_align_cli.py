"""swbank -A k: the CLI prints, after the score lines, the alignments of the k best library
records as ssearch36 reports them; for query100.fa x data500.fa the two summary lines of the
reference's data/alignments500.txt (tests/golden/alignments500_lines.txt), byte for byte."""
import os
import subprocess

import pytest

import swbank as S
from oracle import oracle as O


def test_cli_rejects_a_bad_count():
    q, lib = O.golden_fasta("query100.fa"), O.golden_fasta("data500.fa")
    for arg in ("x", "-1", "2k"):
        r = subprocess.run([S.CLI_PATH, "-q", q, "-l", lib, "-A", arg], capture_output=True,
                           text=True)
        assert r.returncode == 1 and "usage" in r.stderr, (arg, r.returncode, r.stderr)


@pytest.mark.gpu
def test_cli_prints_the_ssearch36_summary_lines():
    q, lib = O.golden_fasta("query100.fa"), O.golden_fasta("data500.fa")
    want = open(os.path.join(O.GOLDEN, "alignments500_lines.txt")).read().splitlines()
    r = subprocess.run([S.CLI_PATH, "-q", q, "-l", lib, "-A", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    plain = subprocess.run([S.CLI_PATH, "-q", q, "-l", lib], capture_output=True, text=True,
                           check=True)
    assert r.stdout.startswith(plain.stdout)        # the score lines are unchanged
    block = r.stdout[len(plain.stdout):].splitlines()
    assert block == [">>db211 (128 nt)", " s-w opt: 78", want[0], "cigar: 15M2I17M4D13M",
                     ">>db428 (128 nt)", " s-w opt: 72", want[1], "cigar: 27M"]
    assert [ln for ln in block if ln.startswith("Smith-Waterman score:")] == want
