"""Alignments of chosen hits on the GPU (sw_align_hits / sw_align_hits_device): coordinates,
CIGAR and identity against the ssearch36 fixture, the brute-force tie rules and the
path-preference-free validation of tests/align_check.py.  Every test runs with plain and with
poisoned device buffers; the CPU references are computed once and shared."""
import os

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_check as AC
from align_cases import QLENS, boundary_case as _boundary_case, device_align as _device_align, \
    protein_case

pytestmark = pytest.mark.gpu

REF = (5, -4, -12, -4)
ALT = (5, -4, -10, -1)   # merged differs from Gotoh: gaps that turn the corner occur
MODELS = [S.GAP_MERGED, S.GAP_GOTOH]
_CACHE = {}


@pytest.fixture(params=["plain", "poisoned"], autouse=True)
def buffers(request):
    if request.param == "poisoned":
        request.getfixturevalue("poisoned_buffers")


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _dna_bank(model, pen, **kw):
    bank = S.ScoreBank(gap_model=model, **kw)
    bank.set_penalties(*pen)
    return bank


def _check_all(q, seqs, hits, alns, sub, go, ge, model, brute, want_path=True):
    assert len(alns) == len(hits)
    for h, a in zip(hits, alns):
        assert a.index == h and a.id == h
        AC.check_alignment(O, q, seqs[h], sub, go, ge, model, a, want_path)
        s, qs, qe, ts, te = brute[h]
        assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end) == (s, qs, qe, ts, te), (h, a)


# ---- 1. golden: the two ssearch36 hits of data/alignments500.txt -------------------------------
def _golden():
    recs = O.read_fasta(O.golden_fasta("data500.fa"))
    q = O.encode_dna(O.read_fasta(O.golden_fasta("query100.fa"))[0][1])
    names = [n for n, _ in recs]
    seqs = [O.encode_dna(s) for _, s in recs]
    rows = [ln.rstrip("\n").split("\t")
            for ln in open(os.path.join(O.GOLDEN, "alignments500.tsv"))][1:]
    return q, names, seqs, rows


@pytest.mark.parametrize("model", MODELS)
def test_golden_hits(model):
    q, names, seqs, rows = _golden()
    assert [r[0] for r in rows] == ["db211", "db428"]
    fixed = [names.index(r[0]) for r in rows]
    others = [k for k in range(0, len(seqs), 16) if k not in fixed][:30]
    hits = fixed + others
    assert len(others) == 30
    sub = O.dna_matrix()
    brute = _cached(("golden", model), lambda: dict(zip(hits, AC.brute_ends_batch(
        O, q, [seqs[h] for h in hits], sub, -12, -4, model))))
    with _dna_bank(model, REF) as bank:
        bank.load_query(q)
        alns = bank.align_targets(seqs, hits)
        assert bank.last_kernel() == f"align i32 hits={len(hits)} chunks=1"
    for a, r in zip(alns, rows):
        want = tuple(int(x) for x in r[1:8])
        assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end, a.n_columns,
                a.n_identities) == want, (r[0], a)
        assert a.cigar == r[8] and a.flags == 0
    _check_all(q, seqs, hits, alns, sub, -12, -4, model, brute)


# ---- 2. boundaries: lane, chunk and strip edges (the inputs: tests/align_cases.py) ---------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("pen", [REF, ALT])
@pytest.mark.parametrize("qlen", QLENS)
def test_boundaries_dna(qlen, pen, model):
    q, seqs, hits = _boundary_case(qlen, 1000 + qlen)
    sub = O.dna_matrix(pen[0], pen[1])
    brute = _cached(("bound", qlen, pen, model),
                    lambda: AC.brute_ends_batch(O, q, seqs, sub, pen[2], pen[3], model))
    with _dna_bank(model, pen) as bank:
        bank.load_query(q)
        alns = bank.align_targets(seqs, hits)
        scores = bank.score_targets(seqs)
    _check_all(q, seqs, hits, alns, sub, pen[2], pen[3], model, brute)
    assert [a.score for a in alns] == [int(scores[h]) for h in hits]


# ---- 3. protein ---------------------------------------------------------------------------------
def test_protein_gotoh():
    q, seqs, hits = protein_case()
    brute = _cached("protein",
                    lambda: AC.brute_ends_batch(O, q, seqs, O.BLOSUM62, -11, -1, S.GAP_GOTOH))
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=S.GAP_GOTOH) as bank:
        bank.set_matrix(O.BLOSUM62, -11, -1)
        bank.load_query(q)
        alns = bank.align_targets(seqs, hits)
    _check_all(q, seqs, hits, alns, O.BLOSUM62, -11, -1, S.GAP_GOTOH, brute)


# ---- 4. tie rules ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_tie_rules(model):
    enc = O.encode_dna
    with _dna_bank(model, REF) as bank:
        bank.load_query(enc("ACGT"))
        a = bank.align_targets([enc("ACGTTTTTACGT")], [0])[0]
        assert (a.score, a.t_start, a.t_end, a.q_start, a.q_end, a.cigar) == (20, 0, 3, 0, 3, "4M")
        bank.load_query(enc("ACGTNNACGT"))
        a = bank.align_targets([enc("ACGT")], [0])[0]
        assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end, a.cigar) == (20, 0, 3, 0, 3, "4M")
    # two co-optimal starts: GGGG scores 16, and so does its extension to the left over a
    # mismatch (-4) and a match (+4); the larger t_start (and q_start) is the start
    pen = (4, -4, -12, -4)
    q, t = enc("ACGGGG"), enc("ATGGGG")
    sub = O.dna_matrix(4, -4)
    assert AC.brute_ends(O, q, t, sub, -12, -4, model) == (16, 2, 5, 2, 5)
    assert O.score_pair(q, t, sub, -12, -4, model) == 16
    with _dna_bank(model, pen) as bank:
        bank.load_query(q)
        a = bank.align_targets([t], [0])[0]
    assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end, a.cigar) == (16, 2, 5, 2, 5, "4M")


def test_corner_turning_gap():
    """CCC against GG between two 20-base matches: under merged gaps one run of 3 I and 2 D
    (10 + 5 x 1) beats two mismatches and a gap (19) and two Gotoh gaps (25); walking back the
    gap from the left comes first, so the I ops precede the D ops.  Gotoh pays per direction."""
    enc = O.encode_dna
    a, b = "ACGTTGCAAGCTTAGCATCA", "TTAGGCATCGATCCGATTAC"
    q, t = enc(a + "CCC" + b), enc(a + "GG" + b)
    sub = O.dna_matrix()
    got = {}
    for model in MODELS:
        with _dna_bank(model, ALT) as bank:
            bank.load_query(q)
            got[model] = bank.align_targets([t], [0])[0]
        AC.check_alignment(O, q, t, sub, -10, -1, model, got[model])
    m = got[S.GAP_MERGED]
    assert (m.score, m.cigar, m.n_columns, m.n_identities) == (185, "20M3I2D20M", 45, 40)
    assert (m.q_start, m.q_end, m.t_start, m.t_end) == (0, 42, 0, 41)
    g = got[S.GAP_GOTOH]
    assert g.score == 181 and sorted(op & 15 for op in g.ops) == [0, 0, 1]


# ---- 5. empty and degenerate ------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_empty_and_degenerate(model):
    enc = O.encode_dna
    q, seqs, _ = _boundary_case(65, 77)
    sub = O.dna_matrix()
    with _dna_bank(model, REF) as bank:
        bank.load_query(enc("AAAA"))
        for a in bank.align_targets([enc("CCCC"), np.zeros(0, np.uint8)], [0, 1, 0]):
            assert a.flags == S.ALIGN_EMPTY and a.score == 0 and not a.ops and a.cigar == ""
            assert (a.q_start, a.q_end, a.t_start, a.t_end, a.n_columns, a.n_identities) == (0,) * 6
        # coordinates only: no path, the coordinates still exact
        bank.load_query(q)
        brute = _cached(("degenerate", model),
                        lambda: AC.brute_ends_batch(O, q, seqs, sub, -12, -4, model))
        hits = list(range(len(seqs)))
        res, offs, lens = S.pack_targets(seqs)
        _check_all(q, seqs, hits, bank.align_hits(res, offs, lens, hits, cigar_cap=0), sub, -12,
                   -4, model, brute, want_path=False)
        _check_all(q, seqs, hits, _device_align(bank, seqs, hits, 0), sub, -12, -4, model, brute,
                   want_path=False)
        # a CIGAR slot of one op: the gapped hits get no path, the ungapped ones keep theirs
        full = bank.align_hits(res, offs, lens, hits)
        one = _device_align(bank, seqs, hits, 1)
        assert any(len(a.ops) > 1 for a in full)
        for a, b in zip(full, one):
            if len(a.ops) > 1:
                AC.check_alignment(O, q, seqs[a.index], sub, -12, -4, model, b, want_path=False)
                assert (b.q_start, b.q_end, b.t_start, b.t_end) == \
                    (a.q_start, a.q_end, a.t_start, a.t_end)
            else:
                assert b == a
        # the host call's CIGAR space running out: the hits that no longer fit get no path
        need = [len(a.ops) for a in full]
        cap = sum(need[:10]) + max(need[10] - 1, 0)
        part = bank.align_hits(res, offs, lens, hits, cigar_cap=cap)
        at = 0
        for a, b in zip(full, part):
            if len(a.ops) <= cap - at:
                assert b == a
                at += len(a.ops)
            else:
                assert b.flags == S.ALIGN_NO_PATH and not b.ops and b.score == a.score
        assert any(b.flags == S.ALIGN_NO_PATH for b in part)


# ---- 6. the direction-store budget -------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_budget(model, monkeypatch):
    rng = np.random.default_rng(6)
    q = rng.integers(0, 4, 2048).astype(np.uint8)
    t = q.copy()
    for pos in rng.integers(8, 2040, 40):
        t[pos] = (t[pos] + 1) & 3
    t = np.concatenate([t[:700], rng.integers(0, 4, 3).astype(np.uint8), t[700:1500],
                        t[1504:]])[:2048]
    sub = O.dna_matrix()
    brute = _cached(("budget", model), lambda: AC.brute_ends_batch(O, q, [t], sub, -12, -4, model))
    assert brute[0][2] - brute[0][1] > 1900  # a window of about 2048 x 2048 cells
    with _dna_bank(model, REF) as bank:
        bank.load_query(q)
        monkeypatch.setenv("SWBANK_ALIGN_MB", "1")
        _check_all(q, [t], [0], bank.align_targets([t], [0]), sub, -12, -4, model, brute,
                   want_path=False)
        assert bank.last_kernel() == "align i32 hits=1 chunks=0"
        _check_all(q, [t], [0], _device_align(bank, [t], [0], 4097), sub, -12, -4, model, brute,
                   want_path=False)
        monkeypatch.delenv("SWBANK_ALIGN_MB")
        alns = bank.align_targets([t], [0])
        _check_all(q, [t], [0], alns, sub, -12, -4, model, brute)
        assert _device_align(bank, [t], [0], 4097) == alns


# ---- 7. past 16 bits ----------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_past_16_bits(model):
    q = np.random.default_rng(7).integers(0, 4, 14000).astype(np.uint8)
    want = _cached("past16", lambda: O.score_pair(q, q, O.dna_matrix(), -12, -4, S.GAP_MERGED))
    assert want == 70000
    with _dna_bank(model, REF) as bank:
        bank.load_query(q)
        a = bank.align_targets([q], [0])[0]
    assert (a.score, a.flags, a.q_start, a.q_end, a.t_start, a.t_end) == (70000, 0, 0, 13999, 0,
                                                                         13999)
    assert a.cigar == "14000M" and (a.n_columns, a.n_identities) == (14000, 14000)


# ---- 8. entry points agree ----------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_entry_points_agree(model, monkeypatch):
    q, seqs, hits = _boundary_case(300, 88)
    ids = np.arange(len(seqs), dtype=np.uint64) * 31 + (1 << 33)
    res, offs, lens = S.pack_targets(seqs)
    stride = 2 * max(len(s) for s in seqs) + 1
    got = []
    for kw in ({}, {"devices": [0, 0]}):
        with _dna_bank(model, ALT, **kw) as bank:
            bank.load_query(q)
            got.append(bank.align_hits(res, offs, lens, hits, ids=ids))
            got.append(_device_align(bank, seqs, hits, stride, ids=ids))
            assert bank.last_kernel().startswith(f"align i32 hits={len(hits)} chunks=")
    # a direction store of 1 MiB: the same records from several chunks (the host call packs the
    # hits' actual windows, the device call slots of 2 strips x (200 + 63) steps x 256 bytes)
    monkeypatch.setenv("SWBANK_ALIGN_MB", "1")
    with _dna_bank(model, ALT) as bank:
        bank.load_query(q)
        got.append(_device_align(bank, seqs, hits, stride, ids=ids))
        assert bank.last_kernel() == f"align i32 hits={len(hits)} chunks=4"
        many = [h for h in hits for _ in range(3)]
        tripled = bank.align_hits(res, offs, lens, many, ids=ids)
        assert int(bank.last_kernel().split("chunks=")[1]) > 1
        assert tripled[::3] == got[0] and tripled[1::3] == got[0] and tripled[2::3] == got[0]
    assert all(a.id == int(ids[a.index]) and a.index == h for a, h in zip(got[0], hits))
    assert any(len(a.ops) > 1 for a in got[0])
    for other in got[1:]:
        assert other == got[0]


# ---- 9. errors ------------------------------------------------------------------------------------
def test_errors():
    enc = O.encode_dna
    seqs = [enc("ACGTACGT"), enc("TTTT")]
    with _dna_bank(S.GAP_MERGED, REF) as bank:
        with pytest.raises(S.SwbankError) as e:  # no query yet
            bank.align_targets(seqs, [0])
        assert e.value.status == S.ERR_STATE
        bank.load_query(enc("ACGT"))
        with pytest.raises(S.SwbankError) as e:
            bank.align_targets(seqs, [0, 2])
        assert e.value.status == S.ERR_ARG
        assert bank.align_targets(seqs, []) == []
        bank.load_queries([enc("ACGT"), enc("GGGTTT")])
        with pytest.raises(S.SwbankError) as e:
            bank.align_targets(seqs, [0])
        assert e.value.status == S.ERR_STATE
        bank.load_query(enc("ACGT"))
        assert bank.align_targets(seqs, [0])[0].cigar == "4M"
    with S.ScoreBank() as bank:  # merged gaps with max(s) > open + extend: documented refusal
        bank.set_penalties(5, -4, -2, -1)
        bank.load_query(enc("ACGT"))
        with pytest.raises(S.SwbankError) as e:
            bank.align_targets(seqs, [0])
        assert e.value.status == S.ERR_UNSUPPORTED
