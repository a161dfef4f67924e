"""The best query of every target on the GPU (sw_best_queries / sw_best_queries_device): every
shape and content family of tests/set_cases.py against numpy's column maximum and its first
occurrence, element for element; rows at every 4-byte phase; either output left out; a
non-default stream; the multi-device bank; the argument errors.  Every test runs with plain
and with poisoned device buffers."""
import numpy as np
import pytest

import swbank as S

import set_cases as SC

pytestmark = pytest.mark.gpu

FILL = 0x3C


@pytest.fixture(params=["plain", "poisoned"], autouse=True)
def buffers(request):
    if request.param == "poisoned":
        request.getfixturevalue("poisoned_buffers")


def _torch():
    import torch
    return torch


def _dev_scores(scores, pad):
    """The matrix on the device after `pad` scores of padding: (the tensor, row 0's pointer)."""
    torch = _torch()
    flat = np.concatenate([np.full(pad, 0x3C3C3C3C, np.int32), scores.reshape(-1)])
    t = torch.from_numpy(flat).to(torch.device("cuda", 0))
    return t, t.data_ptr() + 4 * pad


def _device(bank, d_scores, nq, n, min_score, outs=("query", "score"), stream=0):
    """One sw_best_queries_device call over 0x3C-filled outputs -> (best_query | None,
    best_score | None)."""
    torch = _torch()
    dev = torch.device("cuda", 0)
    buf = {name: torch.full((n * 4,), FILL, dtype=torch.uint8, device=dev) for name in outs}
    torch.cuda.synchronize()
    ptr = lambda name: buf[name].data_ptr() if name in buf else 0
    bank.best_queries_device(d_scores, n, nq, ptr("query"), ptr("score"), min_score=min_score,
                             stream=stream)
    assert bank.last_kernel() == f"best-query nq={nq} n={n}"
    bank.sync()
    if stream:
        torch.cuda.synchronize()
    get = lambda name, t: buf[name].cpu().numpy().view(t) if name in buf else None
    return get("query", np.uint32), get("score", np.int32)


def _check(got, want, what):
    if got[0] is not None:
        assert np.array_equal(got[0], want[0]), what
    if got[1] is not None:
        assert np.array_equal(got[1], want[1]), what


@pytest.mark.parametrize("nq,n", SC.BQ_SHAPES)
def test_shapes(nq, n):
    torch = _torch()
    st = torch.cuda.Stream()
    with S.ScoreBank() as bank:  # neither penalties nor a query: the call needs none
        for shift in SC.bq_shifts(n):
            scores = SC.bq_scores(nq, n, shift)
            pad = (nq + n + shift) % 4
            keep, d_scores = _dev_scores(scores, pad)
            base = SC.ref_best(scores)
            marks = SC.bq_thresholds(scores, shift)
            for x, ms in enumerate(marks):
                want = SC.thresholded(base, ms)
                outs = (("query", "score"), ("query",), ("score",))[x % 3]
                got = _device(bank, d_scores, nq, n, ms, outs,
                              stream=st.cuda_stream if x % 2 else 0)
                assert [g is not None for g in got] == [o in outs for o in ("query", "score")]
                _check(got, want, (nq, n, shift, ms, "device"))
            del keep
            _check(bank.best_queries(scores, min_score=marks[3]), SC.thresholded(base, marks[3]),
                   (nq, n, shift, marks[3], "host"))
            assert bank.last_kernel() == f"best-query nq={nq} n={n}"
            bq, bs = bank.best_queries(scores, min_score=marks[4], want_score=False)
            assert bs is None and np.array_equal(bq, SC.thresholded(base, marks[4])[0])
            bq, bs = bank.best_queries(scores, want_query=False)
            assert bq is None and np.array_equal(bs, base[1])


def test_repeatable():
    """The split form (atomicMax on scratch keys) gives one result however the parts arrive."""
    scores = SC.bq_scores(4097, 257)
    _, d_scores = keep = _dev_scores(scores, 1)
    want = SC.ref_best(scores)
    with S.ScoreBank() as bank:
        for _ in range(4):
            _check(_device(bank, d_scores, 4097, 257, None), want, "repeat")
    del keep


def test_two_streams():
    """Two calls that both use the bank's key scratch, issued on two streams with nothing
    between them."""
    torch = _torch()
    dev = torch.device("cuda", 0)
    jobs = []
    for nq, n in ((4097, 8191), (257, 65)):
        scores = SC.bq_scores(nq, n)
        jobs.append((nq, n, _dev_scores(scores, 3), SC.ref_best(scores)))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with S.ScoreBank() as bank:
        _device(bank, jobs[0][2][1], jobs[0][0], jobs[0][1], None)  # the scratch at its final size
        for order in ((0, 1), (1, 0)):
            outs = [[torch.full((jobs[x][1] * 4,), FILL, dtype=torch.uint8, device=dev)
                     for _ in range(2)] for x in order]
            torch.cuda.synchronize()
            for x, o, st in zip(order, outs, (s1, s2)):
                bank.best_queries_device(jobs[x][2][1], jobs[x][1], jobs[x][0], o[0].data_ptr(),
                                         o[1].data_ptr(), stream=st.cuda_stream)
            torch.cuda.synchronize()
            for x, o in zip(order, outs):
                _check((o[0].cpu().numpy().view(np.uint32), o[1].cpu().numpy().view(np.int32)),
                       jobs[x][3], (order, x))


def test_multi_device_bank():
    with S.ScoreBank(devices=[0, 0]) as bank:
        for nq, n in ((17, 257), (4097, 65), (3, 8193)):
            scores = SC.bq_scores(nq, n)
            keep, d_scores = _dev_scores(scores, 2)
            for ms in SC.bq_thresholds(scores)[2:]:
                want = SC.ref_best(scores, ms)
                _check(_device(bank, d_scores, nq, n, ms), want, (nq, n, ms))
                _check(bank.best_queries(scores, min_score=ms), want, (nq, n, ms, "host"))
                assert bank.last_kernel() == f"best-query nq={nq} n={n}"
            del keep


def test_arguments():
    torch = _torch()
    scores = SC.bq_scores(3, 65)
    keep, d_scores = _dev_scores(scores, 0)
    d_out = torch.full((65 * 4,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    bad = [dict(d_scores=0), dict(d_best_query=0), dict(n=0), dict(nq=0), dict(nq=65537),
           dict(n=(1 << 32) + 1, nq=1), dict(n=1 << 31, nq=1 << 40)]
    with S.ScoreBank() as bank:
        for kw in bad:
            args = dict(d_scores=d_scores, n=65, nq=3, d_best_query=d_out.data_ptr())
            args.update(kw)
            with pytest.raises(S.SwbankError) as e:
                bank.best_queries_device(**args)
            assert e.value.status == S.ERR_ARG, kw
        bank.sync()
        assert (d_out.cpu().numpy() == FILL).all()  # nothing was written
        with pytest.raises(S.SwbankError) as e:
            bank.best_queries(scores, want_query=False, want_score=False)
        assert e.value.status == S.ERR_ARG
        assert S.lib().sw_best_queries_device(None, d_scores, 65, 3, S.INT32_MIN,
                                              d_out.data_ptr(), None, None) == S.ERR_ARG
        # nq = 65536, the limit, works
        thin = SC.bq_scores(65536, 1)
        assert np.array_equal(bank.best_queries(thin)[0], SC.ref_best(thin)[0])
    del keep
    assert S.QUERY_NONE == int(SC.QUERY_NONE)
