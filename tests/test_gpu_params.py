"""GPU: the scoring-parameter envelope (tests/seam_cases.py CASES), bit-exact against the oracle.

Asymmetric matrices (every host table builder indexes m[query * A + target]; a transposed table
changes >= 50 % of these scores, tests/test_param_envelope.py), matrices without a positive
entry, the widest substitution range, zero gap penalties, extend larger than open, penalties in
the hundreds and thousands that are still paid, the negative side of the f16 / u16 switch
(o + 2e + S - smin = 2047, 2048, 2049) and the 16-bit limits with their two refusals.  Every
case runs through each score kernel and the int32 re-score kernel at two query lengths and both
gap models: 260 targets (two tiles and a tail), one in four a straddle target, empty and
1-letter targets included."""
import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_check as AC
import seam_cases as SC

pytestmark = pytest.mark.gpu

MODELS = [S.GAP_MERGED, S.GAP_GOTOH]
_WANT = {}


@pytest.fixture(params=["tile", "tile-lut", "tile-u16", "wave", "wave-u16", "i32"])
def kernel_choice(request, monkeypatch):
    """The env hooks of tests/test_gpu_parity.py, and SWBANK_I32=1 (the library's own kernel
    choice, then every pair again through the int32 kernel)."""
    if request.param == "i32":
        monkeypatch.setenv("SWBANK_I32", "1")
        monkeypatch.delenv("SWBANK_KERNEL", raising=False)
    else:
        monkeypatch.setenv("SWBANK_KERNEL", request.param.split("-")[0])
        monkeypatch.setenv("SWBANK_F16", "0" if request.param.endswith("-u16") else "1")
        monkeypatch.setenv("SWBANK_PAIR", "0" if request.param.endswith("-lut") else "1")
    return request.param


def _bank(case, model):
    bank = S.ScoreBank(alphabet=S.ALPHABET_PROTEIN if case.alphabet == SC.PROTEIN
                       else S.ALPHABET_DNA, gap_model=model)
    bank.set_matrix(SC.MATRICES[case.matrix](), case.go, case.ge)
    return bank


def _want(case, qlen, model):
    key = (case.name, qlen, model)
    if key not in _WANT:
        q, seqs, _ = SC.case_inputs(case, qlen)
        _WANT[key] = SC.oracle_scores(O, q, seqs, SC.MATRICES[case.matrix](), case.go, case.ge,
                                      O.GAP_GOTOH if model == S.GAP_GOTOH else O.GAP_MERGED)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def _arith(kern):
    """The arithmetic token of a kernel name: "f16", "f16+u16-rescore" or "u16"."""
    return kern.split()[1].replace("-profile", "")


def _check_kernel(case, qlen, model, choice, kern, max_len):
    base = choice.split("-")[0]
    if choice == "i32":
        assert kern.endswith("+i32-rescore"), kern
        return
    assert kern.startswith(base + " "), kern
    if choice.endswith("-u16"):
        assert _arith(kern) == "u16", kern
    if case.name == "asym-pair" and qlen == 33:
        if choice == "tile":
            assert " pair R=" in kern, kern
        if choice == "tile-lut":
            assert " pair" not in kern and _arith(kern) == "f16", kern
    if case.name == "asym-odd":  # odd entries past 8: no one-byte f16 table
        assert "-profile" in kern, kern
    if "f16neg" in case.tags and choice in ("tile", "wave"):
        if "neg2049" in case.tags:
            assert _arith(kern) == "u16", kern
        else:
            smax = int(SC.MATRICES[case.matrix]().max())
            exact = min(qlen, max_len) * smax + smax <= 2048
            assert _arith(kern) == ("f16" if exact else "f16+u16-rescore"), kern
            assert exact == (qlen == 33)


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c.name)
def test_case_exact(case, kernel_choice, poisoned_buffers):
    for qlen in case.qlens:
        q, seqs, mt = SC.case_inputs(case, qlen)
        assert len(seqs) == 260 and sum(m is not None for m in mt) == 65
        assert min(len(t) for t in seqs) == 0 and 1 in {len(t) for t in seqs}
        for model in MODELS:
            omodel = O.GAP_GOTOH if model == S.GAP_GOTOH else O.GAP_MERGED
            with _bank(case, model) as bank:
                bank.load_query(q)
                if SC.expect_range_error(case, omodel):
                    with pytest.raises(S.SwbankError) as e:
                        bank.score_targets(seqs)
                    assert e.value.status == S.ERR_RANGE
                    continue
                got = bank.score_targets(seqs)
                kern = bank.last_kernel()
            want = _want(case, qlen, model)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (case.name, qlen, model, kern, int(bad.size),
                                   [(int(i), len(seqs[i]), int(got[i]), int(want[i]))
                                    for i in bad[:8]])
            _check_kernel(case, qlen, model, kernel_choice, kern, max(len(t) for t in seqs))
            if "nopos" in case.tags:
                assert not got.any()
            if case.name == "merged-32767":  # gaps that nobody can pay: the gap-free score
                free = SC.oracle_scores(O, q, seqs, SC.MATRICES[case.matrix](), -32767, -32767,
                                        O.GAP_MERGED)
                assert np.array_equal(got, free)


def test_refusals(kernel_choice):
    """SW_ERR_RANGE is raised for a substitution range past 254 and for Gotoh gaps with
    o + e + S > 65535, by every kernel choice, and for nothing else in the table (the other
    cases return scores in test_case_exact)."""
    q, seqs, _ = SC.case_inputs(SC.GOTOH_REFUSED, 33)
    with _bank(SC.GOTOH_REFUSED, S.GAP_GOTOH) as bank:
        bank.load_query(q)
        with pytest.raises(S.SwbankError) as e:
            bank.score_targets(seqs)
        assert e.value.status == S.ERR_RANGE
    with _bank(SC.GOTOH_REFUSED, S.GAP_MERGED) as bank:  # the merged model has no such limit
        bank.load_query(q)
        want = SC.oracle_scores(O, q, seqs, SC.MATRICES["dna"](), SC.GOTOH_REFUSED.go,
                                SC.GOTOH_REFUSED.ge, O.GAP_MERGED)
        assert np.array_equal(bank.score_targets(seqs), want)
    m = SC.MATRICES["wide"]()
    m[0, 1] = -128  # S - smin = 255
    for model in MODELS:
        with S.ScoreBank(gap_model=model) as bank:
            bank.set_matrix(m, -12, -4)
            bank.load_query(q)
            with pytest.raises(S.SwbankError) as e:
                bank.score_targets(seqs)
            assert e.value.status == S.ERR_RANGE
    assert [c.name for c in SC.CASES for mdl in (O.GAP_MERGED, O.GAP_GOTOH)
            if SC.expect_range_error(c, mdl)] == ["merged-32767"]


# ---- the other entry points ----------------------------------------------------------------------
ENTRY = [c for c in SC.CASES if "entry" in c.tags]


def _device(seqs):
    import torch
    dev = torch.device("cuda", 0)
    res, offs, lens = S.pack_targets(seqs)
    return (torch.from_numpy(res).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev),
            torch.from_numpy(lens.view(np.int32)).to(dev), int(lens.max()))


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", ENTRY, ids=lambda c: c.name)
def test_entry_host_and_device(case, model, poisoned_buffers):
    """score_targets (the host feeder, the library's own kernel choice) and score_batch_device."""
    import torch
    for qlen in case.qlens:
        q, seqs, _ = SC.case_inputs(case, qlen)
        want = _want(case, qlen, model)
        with _bank(case, model) as bank:
            bank.load_query(q)
            got = bank.score_targets(seqs)
            assert np.array_equal(got, want), (case.name, qlen, bank.last_kernel())
            d_res, d_offs, d_lens, maxlen = _device(seqs)
            d_sc = torch.full((len(seqs),), -7, dtype=torch.int32, device=d_res.device)
            st = torch.cuda.Stream()
            bank.score_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(),
                                    len(seqs), maxlen, d_sc.data_ptr(), st.cuda_stream)
            st.synchronize()
            assert np.array_equal(d_sc.cpu().numpy(), want), (case.name, qlen, bank.last_kernel())


@pytest.mark.parametrize("model", MODELS)
def test_entry_records(model, poisoned_buffers):
    """score_records: CAPI records (2-bit codes, at most 232 bases, no N) under the asymmetric
    DNA matrix with free extension; the query from a record too."""
    case = next(c for c in ENTRY if c.alphabet == SC.DNA)
    q, seqs, _ = SC.case_inputs(case, 300)
    q = (q % 4)[:230]
    seqs = [(t % 4)[:232] for t in seqs]
    want = SC.oracle_scores(O, q, seqs, SC.MATRICES[case.matrix](), case.go, case.ge,
                            O.GAP_GOTOH if model == S.GAP_GOTOH else O.GAP_MERGED)
    assert (want > 300).sum() >= 40  # the straddle targets still align across their indel
    with _bank(case, model) as bank:
        bank.load_query_record(S.make_records([q])[0])
        got = bank.score_records(S.make_records(seqs))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", ENTRY, ids=lambda c: c.name)
def test_entry_query_set(case, model, poisoned_buffers):
    """load_queries with lengths 17, 200 and 129: one launch for the DNA row-LUT kernels
    ("queries=3"), one query at a time for the protein profile ("x3 queries")."""
    import torch
    q, seqs, _ = SC.case_inputs(case, 300)
    queries = [q[:17].copy(), q[40:240].copy(), q[150:279].copy()]
    d_res, d_offs, d_lens, maxlen = _device(seqs)
    d_sc = torch.full((3, len(seqs)), -7, dtype=torch.int32, device=d_res.device)
    with _bank(case, model) as bank:
        bank.load_queries(queries)
        st = torch.cuda.Stream()
        bank.score_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), len(seqs),
                                maxlen, d_sc.data_ptr(), st.cuda_stream)
        st.synchronize()
        kern = bank.last_kernel()
    assert ("queries=3" in kern) if case.alphabet == SC.DNA else ("x3 queries" in kern), kern
    got = d_sc.cpu().numpy()
    for k, qq in enumerate(queries):
        want = SC.oracle_scores(O, qq, seqs, SC.MATRICES[case.matrix](), case.go, case.ge,
                                O.GAP_GOTOH if model == S.GAP_GOTOH else O.GAP_MERGED)
        assert np.array_equal(got[k], want), (case.name, k, kern)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("case", ENTRY, ids=lambda c: c.name)
def test_entry_alignments(case, model, poisoned_buffers):
    """align_targets on 16 hits, straddle targets among them: the record validated without a
    path preference (align_check.check_alignment) and the coordinates against the brute-force
    tie rules.  Both cases lie outside the merged model's unsupported region (max(s) <= o + e)."""
    q, seqs, mt = SC.case_inputs(case, 300)
    sub = SC.MATRICES[case.matrix]()
    omodel = O.GAP_GOTOH if model == S.GAP_GOTOH else O.GAP_MERGED
    assert int(sub.max()) <= -case.go - case.ge
    hits = [k for k, m in enumerate(mt) if m is not None][:12] + [1, 2, 5, 7]
    assert len(hits) == 16
    brute = AC.brute_ends_batch(O, q, [seqs[h] for h in hits], sub, case.go, case.ge, omodel)
    with _bank(case, model) as bank:
        bank.load_query(q)
        alns = bank.align_targets(seqs, hits)
        assert bank.last_kernel().startswith("align i32 hits=16"), bank.last_kernel()
    for h, a, b in zip(hits, alns, brute):
        assert a.index == h
        AC.check_alignment(O, q, seqs[h], sub, case.go, case.ge, omodel, a)
        assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end) == b, (h, a, b)


def test_alignments_merged_first_column_rule_refused():
    """Merged gaps with max(s) > open + extend (the first-column rule alive): alignments are
    refused as include/swbank.h documents, scores are not."""
    case = next(c for c in SC.CASES if c.name == "blosum62-8/0")
    q, seqs, _ = SC.case_inputs(case, 33)
    with _bank(case, S.GAP_MERGED) as bank:
        bank.load_query(q)
        with pytest.raises(S.SwbankError) as e:
            bank.align_targets(seqs, [0, 4])
        assert e.value.status == S.ERR_UNSUPPORTED
        assert np.array_equal(bank.score_targets(seqs), _want(case, 33, S.GAP_MERGED))
