"""The alignment passes at their own seams, and the CIGAR tie rules (sw_align_hits /
sw_align_hits_device against tests/align_cases.py).

Passes A, B and C of csrc/swbank_kalign.hip run one walk in three coordinate systems, so each
has its own strip seams, lanes and column blocks; the inputs put a live gap over every one
(tests/test_align_cases.py proves that on the CPU); the matrix family runs the same passes under
asymmetric matrices.  Every record is compared with the
brute-force coordinates and, op for op, with the reference traceback of the documented path
preference, which the preference-free check_alignment cannot see.  Every test runs with plain
and with poisoned device buffers, through the host call (windows packed by a plan) and the
device call (slots); the CPU references are computed once per process and shared."""
import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_cases as C
import align_check as AC
import matrix_cases as MC

pytestmark = pytest.mark.gpu

ABC = [(tag, model) for tag in C.DNA_SETS for model in C.MODELS]
MODES = ["plan", "slot"]


@pytest.fixture(params=["plain", "poisoned"], autouse=True)
def buffers(request):
    if request.param == "poisoned":
        request.getfixturevalue("poisoned_buffers")


def _bank(P):
    if P.sub.shape[0] > 5:
        bank = S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=P.model)
        bank.set_matrix(P.sub, P.go, P.ge)
    elif P.tag in MC.MATRIX_SETS:
        bank = S.ScoreBank(gap_model=P.model)
        bank.set_matrix(P.sub, P.go, P.ge)
    else:
        bank = S.ScoreBank(gap_model=P.model)
        bank.set_penalties(int(P.sub[0][0]), int(P.sub[0][1]), P.go, P.ge)
    return bank


def _align(bank, mode, seqs, hits):
    """The records of `hits` through the host call or the device call; the kernel name says
    that the alignment unit ran over that many hits."""
    if mode == "plan":
        alns = bank.align_targets(seqs, hits)
    else:
        alns = C.device_align(bank, seqs, hits, 2 * max(len(s) for s in seqs) + 1)
    assert bank.last_kernel().startswith(f"align i32 hits={len(hits)} chunks="), bank.last_kernel()
    return alns


def _chunks(bank):
    return int(bank.last_kernel().split("chunks=")[1])


def _compare(P, q, seqs, hits, brute, refs, alns, full=True):
    """Coordinates against brute force, ops / columns / identities against the reference
    traceback, and the preference-free validation (`full`; once per target is enough)."""
    assert len(alns) == len(hits)
    seen = set()
    for h, a in zip(hits, alns):
        assert a.index == h and a.id == h
        assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end) == brute[h], (h, a, brute[h])
        r = refs[h]
        if r is None:
            assert a.flags == S.ALIGN_EMPTY and not a.ops
        else:
            assert a.flags == 0, (h, a)
            assert tuple(a.ops) == r.ops, (h, a.cigar, S.cigar_string(r.ops))
            assert (a.n_columns, a.n_identities) == (r.n_columns, r.n_identities), (h, a)
        if full and h not in seen:
            AC.check_alignment(O, q, seqs[h], P.sub, P.go, P.ge, P.model, a)
            seen.add(h)


def _run_group(P, g, mode):
    with _bank(P) as bank:
        bank.load_query(g.q)
        alns = _align(bank, mode, g.seqs, g.hits)
        chunks = _chunks(bank)
    _compare(P, g.q, g.seqs, g.hits, g.brute, g.refs, alns)
    return chunks


# ---- 1. the families, by plan and by slot ---------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag,model", ABC)
def test_pass_seams(tag, model, mode):
    """A live I run over strip seam 256 and 512 of pass B, of pass C and of pass A in one batch
    (2-6, 9 and 13 rows: within a lane, over two and over three whole lanes)."""
    P = C.dna_param(tag, model)
    assert _run_group(P, C.seam_family(P), mode) == 1


@pytest.mark.parametrize("mode", MODES)
def test_pass_seams_protein(mode):
    P = C.protein_param()
    assert _run_group(P, C.seam_family(P), mode) == 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag,model", ABC)
def test_pass_seams_chunked(tag, model, mode, monkeypatch):
    """The same with a direction store of 1 MiB: the three-strip windows spread over several
    chunks (two windows fit one), by plan and by slot."""
    monkeypatch.setenv("SWBANK_ALIGN_MB", "1")
    P = C.dna_param(tag, model)
    assert _run_group(P, C.seam_family(P), mode) > 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag,model", ABC)
def test_window_edges(tag, model, mode):
    """Windows of exactly 255 .. 513 rows and 63 .. 129 columns, an indel 7 cells from the
    last row or column, the window's first row off a lane boundary."""
    P = C.dna_param(tag, model)
    _run_group(P, C.edge_family(P), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag,model", ABC)
def test_ties_across_lanes_and_strips(tag, model, mode):
    """Equal maximal cells in different lanes, strips and column blocks (the end rule: the
    smallest t_end, then the smallest q_end) and equal starts in different lanes and strips of
    the reversed walk (the largest t_start)."""
    P = C.dna_param(tag, model)
    for g in C.tie_family(P):
        _run_group(P, g, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("model", C.MODELS)
def test_tie_rich_paths(model, mode):
    """Low-complexity pairs at penalties where co-optimal moves are common: the CIGAR is the
    one the documented preference picks (diagonal, then D, then I; open rather than extend)."""
    for g, tag in zip(C.tie_rich_family(model), C.TIE_SETS):
        _run_group(C.dna_param(tag, model, C.TIE_SETS), g, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,model", MC.PARAMS)
def test_asymmetric_matrices(name, model, mode):
    """The matrix family of tests/matrix_cases.py (banks made with set_matrix): a kernel that
    read the matrix transposed would change 94-98 % of these scores (tests/test_align_cases.py).
    Coordinates against brute force, the CIGAR op for op against the reference traceback."""
    P = MC.matrix_param(name, model)
    assert _run_group(P, MC.matrix_family(P), mode) == 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,model", MC.PARAMS)
def test_asymmetric_matrices_chunked(name, model, mode, monkeypatch):
    """The same with a direction store of 1 MiB: more than one chunk."""
    monkeypatch.setenv("SWBANK_ALIGN_MB", "1")
    P = MC.matrix_param(name, model)
    assert _run_group(P, MC.matrix_family(P), mode) > 1


# ---- 2. exact CIGARs on the lane, chunk and strip edges of test_gpu_align.py ---------------
@pytest.mark.parametrize("model", C.MODELS)
@pytest.mark.parametrize("tag", list(C.DNA_SETS))
@pytest.mark.parametrize("qlen", C.QLENS)
def test_boundaries_exact_cigar(qlen, tag, model):
    P = C.dna_param(tag, model)
    q, seqs, hits = C.boundary_case(qlen, 1000 + qlen)
    brute, refs = C._cached(("bound", qlen, tag, model), lambda: C.prepare(q, seqs, P))
    with _bank(P) as bank:
        bank.load_query(q)
        alns = _align(bank, "plan", seqs, hits)
    _compare(P, q, seqs, hits, brute, refs, alns)


def test_protein_exact_cigar():
    P = C.protein_param()
    q, seqs, hits = C.protein_case()
    brute, refs = C._cached("protein", lambda: C.prepare(q, seqs, P))
    with _bank(P) as bank:
        bank.load_query(q)
        alns = _align(bank, "plan", seqs, hits)
    _compare(P, q, seqs, hits, brute, refs, alns)


# ---- 3. scratch reuse ------------------------------------------------------------------------
@pytest.mark.parametrize("model", C.MODELS)
def test_scratch_reuse(model, monkeypatch):
    """More hits than waves: with a scratch budget of 1 MiB (SWBANK_EDGE_MB) a wave aligns
    several hits in turn and reuses its two scratch rows, a three-strip target after a short or
    empty one and the other way round.  The records are those of the default budget and of the
    references, in both hit orders, by plan and by slot."""
    P = C.dna_param("ref", model)
    g, order2 = C.reuse_case(P)
    waves = C.i32_waves(len(g.hits), max(len(s) for s in g.seqs), 1 << 20)
    assert len(g.hits) >= 300 and len(g.hits) > 2 * waves
    assert C.i32_waves(len(g.hits), max(len(s) for s in g.seqs), 2048 << 20) >= len(g.hits)
    with _bank(P) as bank:
        bank.load_query(g.q)
        for hits in (g.hits, order2):
            want = _align(bank, "plan", g.seqs, hits)  # the default budget: a wave per hit
            _compare(P, g.q, g.seqs, hits, g.brute, g.refs, want, full=hits is g.hits)
            monkeypatch.setenv("SWBANK_EDGE_MB", "1")
            assert _align(bank, "plan", g.seqs, hits) == want
            assert _align(bank, "slot", g.seqs, hits) == want
            monkeypatch.delenv("SWBANK_EDGE_MB")
