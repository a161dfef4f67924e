"""swbank -X: the CLI searches a protein query against a DNA library in six reading frames,
prints the frame tag after every score and in the -A report with each hit's nucleotide range (the
model of tests/frame_cases.py and the oracle say which), takes -S and -E (fitted on shuffles of
the six translations), and refuses -B."""
import subprocess

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_check as AC
import frame_cases as F

DNA = "TCAGN"


def _fasta(path, recs):
    path.write_text("".join(f">{n}\n{s}\n" for n, s in recs))
    return str(path)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("framecli")
    rng = np.random.default_rng(97)
    q = rng.integers(0, 20, 40).astype(np.uint8)
    seqs = [F.plant(rng, q, 180, 1, True)[0], rng.integers(0, 5, 150).astype(np.uint8),
            F.plant(rng, q[5:35], 140, 2, False)[0], np.array([2, 0], np.uint8),
            F.plant(rng, q, 200, 0, False)[0]]
    names = [f"nt{k}" for k in range(len(seqs))]
    qf = _fasta(d / "q.fa", [("prot", "".join(O.PROT_LETTERS[c] for c in q))])
    lf = _fasta(d / "lib.fa", [(n, "".join(DNA[c] for c in s)) for n, s in zip(names, seqs)])
    return qf, lf, q, names, seqs


def test_cli_refuses_x_with_b(files):
    qf, lf = files[:2]
    r = subprocess.run([S.CLI_PATH, "-q", qf, "-l", lf, "-X", "-B"], capture_output=True, text=True)
    assert r.returncode == 1 and "usage" in r.stderr and "-X" in r.stderr and "-B" in r.stderr


@pytest.mark.gpu
def test_cli_translated_search(files):
    qf, lf, q, names, seqs = files
    best, frame = F.merge6(F.oracle_frames(q, seqs, model=O.GAP_MERGED))
    assert frame.tolist() == [4, int(frame[1]), 2, 0, 0] and best[3] == 0
    assert best[0] == best[4] == F.self_score(q)  # a tie: the library order decides
    r = subprocess.run([S.CLI_PATH, "-q", qf, "-l", lf, "-X", "-b", "-A", "2", "-S", "0.267,0.041"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    n = len(seqs)
    assert lines[:n] == [f">{names[k]} score: {int(best[k])} [{F.TAGS[int(frame[k])]}]"
                         for k in range(n)]
    assert r.stderr.strip() == f"best: >nt0 score: {int(best[0])} [-2]"
    assert lines[n].startswith("Statistics: Lambda= 0.2670;  K=0.0410")
    block = lines[n + 1:]
    assert len(block) == 8
    st = S.make_statistics(0.267, 0.041, len(q))
    for i, k in enumerate((0, 4)):
        f, L = int(frame[k]), len(seqs[k])
        head, opt, summary, cigar = block[4 * i:4 * i + 4]
        assert head == f">>{names[k]} ({L} nt) [{F.TAGS[f]}]"
        bits, ev = S.hit_significance(st, [int(best[k])], [(L - f % 3) // 3], 6 * n)
        assert opt == f" s-w opt: {int(best[k])}  bits: {bits[0]:.1f} E({6 * n}): {ev[0]:.2g}"
        s, qs, qe, a_start, a_end = AC.brute_ends(O, q, F.translate(seqs[k], f), O.BLOSUM62,
                                                  *F.PEN, O.GAP_MERGED)
        ts, te = F.nt_coords(a_start, a_end, f, L)
        t_from, t_to = (te + 1, ts + 1) if f >= 3 else (ts + 1, te + 1)  # reverse: high to low
        assert (s, qs, qe) == (int(best[k]), 0, len(q) - 1) and te - ts + 1 == 3 * len(q)
        assert summary == (f"Smith-Waterman score: {s}; 100.0% identity (100.0% similar) in "
                           f"{len(q)} aa overlap (1-{len(q)}:{t_from}-{t_to})")
        assert cigar == f"cigar: {len(q)}M"


@pytest.mark.gpu
def test_cli_estimates_statistics_on_the_translations(files):
    """-X -E: lambda and K are those of sw_estimate_statistics over the six translations of the
    library, frame-major, as a protein batch; the hits' E-values use them with db_size 6 n."""
    qf, lf, q, names, seqs = files
    n = len(seqs)
    trans = [F.translate(s, f) for f in range(6) for s in seqs]
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=S.GAP_MERGED) as bank:
        bank.set_matrix(O.BLOSUM62, *F.PEN)
        bank.load_query(q)
        st = bank.estimate_statistics(*S.pack_targets(trans), seed=5, rounds=40)[0]
    assert not st.degenerate
    r = subprocess.run([S.CLI_PATH, "-q", qf, "-l", lf, "-X", "-A", "1", "-E", "40,5"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[n] == (f"Statistics: Lambda= {st.lambda_:.4f};  K={st.K:.4f} "
                        f"({st.n_samples} samples)")
    best = F.self_score(q)
    bits, ev = S.hit_significance(st, [best], [(len(seqs[0]) - 1) // 3], 6 * n)
    assert lines[n + 1] == f">>{names[0]} ({len(seqs[0])} nt) [-2]"
    assert lines[n + 2] == f" s-w opt: {best}  bits: {bits[0]:.1f} E({6 * n}): {ev[0]:.2g}"
