"""The k best hits on the GPU (sw_top_hits / sw_top_hits_device): every input family of
tests/top_cases.py against the stable descending sort, element for element; the optional
outputs; two streams without synchronisation; the score -> top hits -> align chain on one
stream against the ssearch36 fixtures; query sets; the multi-device bank; the argument errors.
Every test runs with plain and with poisoned device buffers; the CPU references are computed
once (top_cases.group) and shared."""
import os

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import top_cases as TC

pytestmark = pytest.mark.gpu

REF = (5, -4, -12, -4)
FILL = 0x3C
_DEV = {}


@pytest.fixture(params=["plain", "poisoned"], autouse=True)
def buffers(request):
    if request.param == "poisoned":
        request.getfixturevalue("poisoned_buffers")


def _torch():
    import torch
    return torch


def _to_dev(a):
    torch = _torch()
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(torch.device("cuda", 0))


def _dev_scores(name):
    """The group's scores on the device, after 0..3 scores of padding (a row that starts at any
    multiple of 4 bytes): (the tensor, the pointer of row 0)."""
    if name not in _DEV:
        scores = TC.group(name)[0]
        pad = len(name) % 4
        t = _to_dev(np.concatenate([np.full(pad, 0x3C3C3C3C, np.int32), scores.reshape(-1)]))
        _DEV[name] = (t, t.data_ptr() + 4 * pad)
    return _DEV[name]


def _perm_ids(n):
    return np.random.default_rng([9, n]).permutation(n).astype(np.uint64) + np.uint64(1 << 33)


class Call:
    """One sw_top_hits_device call on torch buffers pre-filled with 0x3C bytes.  The constructor
    allocates and fills the buffers and waits for that; issue() only makes the call, so several
    prepared calls go out back to back with nothing between them."""

    def __init__(self, bank, d_scores, nq, n, k, min_score=None, ids=None, stream=0,
                 outs=("scores", "ids", "counts"), issue=True):
        torch = _torch()
        dev = torch.device("cuda", 0)
        self.bank, self.d_scores, self.nq, self.n, self.k = bank, d_scores, nq, n, k
        self.min_score, self.stream = min_score, stream
        self.d_ids = _to_dev(ids) if ids is not None else None
        self.buf = {"hits": torch.full((nq * k * 8,), FILL, dtype=torch.uint8, device=dev)}
        for name, size in (("scores", nq * k * 4), ("ids", nq * k * 8), ("counts", nq * 4)):
            if name in outs:
                self.buf[name] = torch.full((size,), FILL, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        if issue:
            self.issue()

    def issue(self):
        ptr = lambda name: self.buf[name].data_ptr() if name in self.buf else 0
        self.bank.top_hits_device(self.d_scores, self.n, self.k, ptr("hits"), nq=self.nq,
                                  d_ids=self.d_ids.data_ptr() if self.d_ids is not None else 0,
                                  min_score=self.min_score, d_hit_scores=ptr("scores"),
                                  d_hit_ids=ptr("ids"), d_counts=ptr("counts"),
                                  stream=self.stream)
        return self

    def result(self):
        """(hits, hit_scores | None, hit_ids | None, counts | None) once the work is done."""
        types = {"hits": np.uint64, "scores": np.int32, "ids": np.uint64, "counts": np.uint32}
        get = lambda name: self.buf[name].cpu().numpy().view(types[name]) \
            if name in self.buf else None
        shape = lambda a: a.reshape(self.nq, self.k) if a is not None else None
        return shape(get("hits")), shape(get("scores")), shape(get("ids")), get("counts")


def _want_ids(hits, ids):
    none = hits == TC.HIT_NONE
    safe = np.where(none, 0, hits).astype(np.int64)
    return np.where(none, TC.HIT_NONE, ids[safe] if ids is not None else hits)


def _check(got, want, ids, what):
    hits, hsc, hid, cnt = got
    assert np.array_equal(hits, want[0]), what
    if hsc is not None:
        assert np.array_equal(hsc, want[1]), what
    if hid is not None:
        assert np.array_equal(hid, _want_ids(want[0], ids)), what
    if cnt is not None:
        assert np.array_equal(cnt, want[2]), what


# ---- 1. every family, device and host call -------------------------------------------------------
@pytest.mark.parametrize("name", list(TC.GROUPS))
def test_families(name):
    scores, runs, orders = TC.group(name)
    nq, n = scores.shape
    _, d_scores = _dev_scores(name)
    ids = _perm_ids(n)
    with S.ScoreBank() as bank:  # neither penalties nor a query: the call needs none
        for k, ms in runs:
            want = TC.ref_top(scores, k, ms, orders)
            for idv in (None, ids):
                call = Call(bank, d_scores, nq, n, k, ms, idv)
                assert bank.last_kernel() == f"top k={k} nq={nq} n={n}"
                bank.sync()
                _check(call.result(), want, idv, (name, k, ms, idv is not None))
            host = bank.top_hits(scores, k, ids=ids, min_score=ms)
            _check(host, want, ids, (name, k, ms, "host"))
            assert bank.last_kernel() == f"top k={k} nq={nq} n={n}"


def test_host_call_takes_one_row_or_a_matrix():
    scores, runs, orders = TC.group("rows-3x2049")
    k = runs[0][0]
    want = TC.ref_top(scores, k, None, orders)
    with S.ScoreBank() as bank:
        hits, hsc, hid, cnt = bank.top_hits(scores, k)
        assert hits.shape == (3, k) and cnt.shape == (3,)
        _check((hits, hsc, hid, cnt), want, None, "2-D")
        hits, hsc, hid, cnt = bank.top_hits(scores[1], k)
        assert hits.shape == (k,) and int(cnt) == want[2][1]
        assert np.array_equal(hits, want[0][1]) and np.array_equal(hsc, want[1][1])
        assert np.array_equal(hid, want[0][1])
        with pytest.raises(ValueError):
            bank.top_hits(scores, k, ids=np.arange(5))


# ---- 2. optional outputs ---------------------------------------------------------------------------
def test_optional_outputs():
    name = "threshold"
    scores, runs, orders = TC.group(name)
    nq, n = scores.shape
    _, d_scores = _dev_scores(name)
    ids = _perm_ids(n)
    with S.ScoreBank() as bank:
        for k, ms in runs[1:3]:  # a full row, and a count inside k (sentinels follow)
            want = TC.ref_top(scores, k, ms, orders)
            for outs in (("ids", "counts"), ("scores", "counts"), ("scores", "ids"), ()):
                call = Call(bank, d_scores, nq, n, k, ms, ids, outs=outs)
                bank.sync()
                got = call.result()
                assert [x is not None for x in got[1:]] == \
                    [o in outs for o in ("scores", "ids", "counts")]
                _check(got, want, ids, (k, ms, outs))


# ---- 3. two streams, no synchronisation between the calls ------------------------------------
def test_two_streams():
    """Both calls are prepared first; then they are issued back to back on two streams with
    nothing between them, and one synchronisation follows.  The first is the long one (a million
    scores, k = 4096), the second has 16 rows, so the second would overwrite the first's state
    and key slots in flight if the bank did not order it after the first."""
    torch = _torch()
    jobs = []
    for name, k in (("sizes-1021952", 4096), ("rows-16x4099", 200)):
        scores, _, orders = TC.group(name)
        jobs.append((name, scores.shape, k, _dev_scores(name)[1],
                     TC.ref_top(scores, k, None, orders)))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with S.ScoreBank() as bank:
        # the scratch at its final size first: growing it later would free the old buffers, which
        # waits for the device and would hide a missing order between the two calls
        Call(bank, jobs[1][3], *jobs[1][1], TC.TOP_MAX_K)
        Call(bank, jobs[0][3], *jobs[0][1], jobs[0][2])
        bank.sync()
        for order in ((0, 1), (1, 0), (0, 1), (0, 0)):
            calls = [Call(bank, jobs[x][3], *jobs[x][1], jobs[x][2], stream=st.cuda_stream,
                          issue=False) for x, st in zip(order, (s1, s2))]
            torch.cuda.synchronize()
            for call in calls:
                call.issue()
            torch.cuda.synchronize()
            for x, call in zip(order, calls):
                _check(call.result(), jobs[x][4], None, (jobs[x][0], order))


# ---- 4. score -> top hits -> align on one stream (golden) -----------------------------------------
def _golden():
    recs = O.read_fasta(O.golden_fasta("data500.fa"))
    q = O.encode_dna(O.read_fasta(O.golden_fasta("query100.fa"))[0][1])
    return q, [n for n, _ in recs], [O.encode_dna(s) for _, s in recs]


def test_pipeline_golden():
    torch = _torch()
    q, names, seqs = _golden()
    n, k = len(seqs), 12
    res, offs, lens = S.pack_targets(seqs)
    ids = np.arange(n, dtype=np.uint64) * 7 + np.uint64(1 << 40)
    max_len = int(lens.max())
    stride = 2 * max_len + 1
    dev = torch.device("cuda", 0)
    d_res, d_offs, d_lens, d_ids = _to_dev(res), _to_dev(offs), _to_dev(lens), _to_dev(ids)
    d_scores = torch.full((n,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    d_hits = torch.full((k * 8,), FILL, dtype=torch.uint8, device=dev)
    d_hsc = torch.full((k * 4,), FILL, dtype=torch.uint8, device=dev)
    d_out = torch.full((k * S.ALIGNMENT_DTYPE.itemsize,), FILL, dtype=torch.uint8, device=dev)
    d_cig = torch.full((k * stride,), 0x3C3C3C3C, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with S.ScoreBank() as bank:
        bank.set_penalties(*REF)
        bank.load_query(q)
        h = st.cuda_stream
        bank.score_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, max_len,
                                d_scores.data_ptr(), stream=h, d_ids=d_ids.data_ptr())
        bank.top_hits_device(d_scores.data_ptr(), n, k, d_hits.data_ptr(), d_ids=d_ids.data_ptr(),
                             d_hit_scores=d_hsc.data_ptr(), stream=h)
        bank.align_hits_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, max_len,
                               d_hits.data_ptr(), k, d_out.data_ptr(), d_cig.data_ptr(), stride,
                               stream=h, d_ids=d_ids.data_ptr())
        bank.sync()
        st.synchronize()
        hits = d_hits.cpu().numpy().view(np.uint64)
        hsc = d_hsc.cpu().numpy().view(np.int32)
        assert [(names[int(x)], int(s)) for x, s in zip(hits, hsc)] == TC.GOLDEN_TOP12
        assert bank.best()[2] == int(hits[0])
        got = S.alignments_from(d_out.cpu().numpy().view(S.ALIGNMENT_DTYPE),
                                d_cig.cpu().numpy().view(np.uint32))
        want = bank.align_hits(res, offs, lens, hits, ids=ids)
    assert got == want and len(got) == k
    rows = [ln.rstrip("\n").split("\t")
            for ln in open(os.path.join(O.GOLDEN, "alignments500.tsv"))][1:]
    for a, r in zip(got, rows):
        assert names[a.index] == r[0] and a.id == int(ids[a.index])
        assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end, a.n_columns,
                a.n_identities) == tuple(int(x) for x in r[1:8])
        assert a.cigar == r[8]


# ---- 5. a query set ------------------------------------------------------------------------------------
def test_query_set():
    torch = _torch()
    q, _, seqs = _golden()
    rng = np.random.default_rng(12)
    queries = [q, q[20:90].copy(), rng.integers(0, 4, 130).astype(np.uint8)]
    n, nq, k = len(seqs), 3, 40
    res, offs, lens = S.pack_targets(seqs)
    ores, ooffs, olens = O.pack_residues(seqs)
    oracle = np.stack([O.score_batch(x, ores, ooffs, olens, O.dna_matrix(), -12, -4, O.GAP_MERGED)
                       for x in queries]).astype(np.int32)
    d_res, d_offs, d_lens = _to_dev(res), _to_dev(offs), _to_dev(lens)
    d_scores = torch.full((nq * n,), 0x3C3C3C3C, dtype=torch.int32, device=torch.device("cuda", 0))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with S.ScoreBank() as bank:
        bank.set_penalties(*REF)
        bank.load_queries(queries)
        call = Call(bank, d_scores.data_ptr(), nq, n, k, stream=st.cuda_stream, issue=False)
        bank.score_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n,
                                int(lens.max()), d_scores.data_ptr(), stream=st.cuda_stream)
        call.issue()  # on the same stream, nothing between the two calls
        bank.sync()
        st.synchronize()
        assert np.array_equal(d_scores.cpu().numpy().reshape(nq, n), oracle)
        _check(call.result(), TC.ref_top(oracle, k), None, "query set")


# ---- 6. a multi-device bank runs it on its root ------------------------------------------------
def test_multi_device_bank():
    name = "rows-3x2049"
    scores, runs, orders = TC.group(name)
    nq, n = scores.shape
    _, d_scores = _dev_scores(name)
    ids = _perm_ids(n)
    with S.ScoreBank(devices=[0, 0]) as bank:
        for k, ms in runs:
            want = TC.ref_top(scores, k, ms, orders)
            call = Call(bank, d_scores, nq, n, k, ms, ids)
            assert bank.last_kernel() == f"top k={k} nq={nq} n={n}"
            bank.sync()
            _check(call.result(), want, ids, (k, ms))
            _check(bank.top_hits(scores, k, ids=ids, min_score=ms), want, ids, (k, ms, "host"))


# ---- 7. arguments ---------------------------------------------------------------------------------------
def test_arguments():
    torch = _torch()
    name = "sizes-2049"
    scores, _, orders = TC.group(name)
    n = scores.shape[1]
    _, d_scores = _dev_scores(name)
    d_hits = torch.full((S.TOP_MAX_K * 8,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    big = 1 << 62
    bad = [dict(d_scores=0), dict(d_hits=0), dict(n=0), dict(nq=0), dict(k=0),
           dict(k=S.TOP_MAX_K + 1), dict(n=(1 << 32) + 1),
           dict(nq=big, n=8, k=1),   # nq x n overflows, nq x k does not
           dict(nq=big, n=1, k=8)]   # nq x k overflows, nq x n does not
    with S.ScoreBank() as bank:
        for kw in bad:
            args = dict(d_scores=d_scores, n=n, k=12, d_hits=d_hits.data_ptr(), nq=1)
            args.update(kw)
            with pytest.raises(S.SwbankError) as e:
                bank.top_hits_device(**args)
            assert e.value.status == S.ERR_ARG, kw
        bank.sync()
        assert (d_hits.cpu().numpy() == FILL).all()  # nothing was written
        for kw in (dict(k=0), dict(k=S.TOP_MAX_K + 1)):
            with pytest.raises(S.SwbankError) as e:
                bank.top_hits(scores, **kw)
            assert e.value.status == S.ERR_ARG, kw
        st = S.lib().sw_top_hits_device(None, d_scores, None, n, 1, 12, S.INT32_MIN,
                                        d_hits.data_ptr(), None, None, None, None)
        assert st == S.ERR_ARG
        # k = SW_TOP_MAX_K works (here k > n: the row in order, then sentinels)
        bank.top_hits_device(d_scores, n, S.TOP_MAX_K, d_hits.data_ptr())
        bank.sync()
        want = TC.ref_top(scores, S.TOP_MAX_K, None, orders)[0]
        assert np.array_equal(d_hits.cpu().numpy().view(np.uint64), want[0])
    assert S.TOP_MAX_K == TC.TOP_MAX_K == 4096 and S.HIT_NONE == int(TC.HIT_NONE)
