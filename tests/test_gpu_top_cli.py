"""swbank -A k picks its k hits with sw_top_hits (k <= SW_TOP_MAX_K) or, past that, with the
host sort it always had: both print the 12 best records of query100.fa x data500.fa in the
order of ssearch36's best-scores list."""
import subprocess

import pytest

import swbank as S
from oracle import oracle as O

import top_cases as TC

pytestmark = pytest.mark.gpu


def _blocks(arg):
    q, lib = O.golden_fasta("query100.fa"), O.golden_fasta("data500.fa")
    r = subprocess.run([S.CLI_PATH, "-q", q, "-l", lib, "-A", arg], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    n = len(O.read_fasta(lib))
    lines = r.stdout.splitlines()[n:]  # after the score lines
    heads = [i for i, ln in enumerate(lines) if ln.startswith(">>")]
    return [lines[a:b] for a, b in zip(heads, heads[1:] + [len(lines)])]


def test_cli_prints_the_golden_order_on_both_paths():
    device = _blocks("12")
    assert len(device) == 12
    for block, (name, score) in zip(device, TC.GOLDEN_TOP12):
        assert block[0] == f">>{name} (128 nt)" and block[1] == f" s-w opt: {score}"
        assert block[2].startswith(f"Smith-Waterman score: {score}; ")
        assert block[3].startswith("cigar: ")
    host = _blocks(str(S.TOP_MAX_K + 1))  # the qsort path (k is clamped to the library)
    assert len(host) == len(O.read_fasta(O.golden_fasta("data500.fa")))
    assert host[:12] == device
