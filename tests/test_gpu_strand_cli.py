"""swbank -B: the CLI searches both strands of the golden query100.fa x data500.fa, prints [f] or
[r] after every score (tests/golden/strands500.tsv) and in the -A report, the reverse hits as
tests/golden/strand_alignments500.tsv records them with the target range high to low, and with
-S the E-values of a library twice the size."""
import subprocess

import pytest

import swbank as S
from oracle import oracle as O

import strand_cases as SC


def test_cli_refuses_both_strands_of_a_protein():
    q, lib = O.golden_fasta("query100.fa"), O.golden_fasta("data500.fa")
    r = subprocess.run([S.CLI_PATH, "-q", q, "-l", lib, "-B", "-P"], capture_output=True, text=True)
    assert r.returncode == 1 and "usage" in r.stderr and "-B" in r.stderr


def _run(*args):
    q, lib = O.golden_fasta("query100.fa"), O.golden_fasta("data500.fa")
    r = subprocess.run([S.CLI_PATH, "-q", q, "-l", lib] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("gotoh", [False, True])
def test_cli_both_strands_on_the_golden_files(gotoh):
    rows = SC.load_strands500()
    gold = {r["name"]: r for r in SC.load_strand_alignments500()}
    g = ["-g"] if gotoh else []
    plain = _run(*g).stdout.splitlines()
    assert plain == [f">{n} score: {f}" for n, f, _, _ in rows]  # without -B nothing changes
    r = _run("-B", "-b", "-A", "6", "-S", "0.1840,0.1293", *g)
    lines = r.stdout.splitlines()
    assert lines[:len(rows)] == [f">{n} score: {max(f, v)} [{'fr'[s]}]" for n, f, v, s in rows]
    assert r.stderr.strip() == "best: >db35 score: 83 [r]"
    assert lines[len(rows)].startswith("Statistics: Lambda= 0.1840;  K=0.1293")
    block = lines[len(rows) + 1:]
    heads = [ln for ln in block if ln.startswith(">>")]
    assert heads == [">>db35 (128 nt) [r]", ">>db198 (128 nt) [r]", ">>db211 (128 nt) [f]",
                     ">>db428 (128 nt) [f]", ">>db41 (128 nt) [r]", ">>db454 (128 nt) [f]"]
    assert len(block) == 4 * 6
    qlen = len(O.read_fasta(O.golden_fasta("query100.fa"))[0][1])  # (128 bases)
    st = S.make_statistics(0.1840, 0.1293, qlen)
    for i, head in enumerate(heads):
        name = head[2:].split()[0]
        opt, summary, cigar = block[4 * i + 1:4 * i + 4]
        score = int(opt.split()[2])
        bits, ev = S.hit_significance(st, [score], [128], 2 * len(rows))
        assert opt == f" s-w opt: {score}  bits: {bits[0]:.1f} E({2 * len(rows)}): {ev[0]:.2g}"
        if name in gold:  # a reverse hit: the target range runs high to low
            w = gold[name]
            pct = 100.0 * w["n_identities"] / w["n_columns"]
            assert summary == (f"Smith-Waterman score: {w['score']}; {pct:.1f}% identity "
                               f"({pct:.1f}% similar) in {w['n_columns']} nt overlap "
                               f"({w['q_start'] + 1}-{w['q_end'] + 1}:{w['t_end'] + 1}-"
                               f"{w['t_start'] + 1})")
            assert cigar == f"cigar: {w['cigar']}" and w["t_end"] > w["t_start"]
    # the forward hits are the lines of the forward report
    fwd = _run("-A", "2", *g).stdout.splitlines()[len(rows):]
    at = block.index(">>db211 (128 nt) [f]")
    assert block[at + 2:at + 4] == fwd[2:4] and fwd[0] == ">>db211 (128 nt)"
