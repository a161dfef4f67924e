"""GPU: every hand-off of column or row state with a live gap crossing it.

Each seam family of tests/seam_cases.py is a batch of straddle targets whose single indel lies
over the seam's own rows (deletions: a vertical gap run) or columns (insertions: a horizontal
one).  tests/test_param_envelope.py shows on the CPU that losing the gap value alone at the
first or the last seam of a family changes at least half of that seam's scores, so a kernel that
hands H over but loses, delays or mis-indexes the gap value fails here.  Every item runs the
path's usual penalties, free extension (-8/0) and an asymmetric matrix, both gap models where
the path has both, on poisoned device buffers; it asserts from last_kernel() (and the counters)
that the intended path ran, then bit-exact scores for every target."""
import re

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

import align_check as AC
import seam_cases as SC

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_buffers")]

MODELS = [S.GAP_MERGED, S.GAP_GOTOH]
PSETS = ["ref", "free", "asym"]
_WANT = {}


def _omodel(model):
    return O.GAP_GOTOH if model == S.GAP_GOTOH else O.GAP_MERGED


def _params(name, pset, model):
    """(matrix, open, extend) of a family's parameter set."""
    alphabet = SC.SEAMS[name].alphabet
    _, mat, go, ge = next(p for p in SC.seam_params(alphabet, _omodel(model)) if p[0] == pset)
    return SC.MATRICES[mat](), go, ge


def _bank(name, pset, model):
    sub, go, ge = _params(name, pset, model)
    bank = S.ScoreBank(alphabet=S.ALPHABET_PROTEIN if SC.SEAMS[name].alphabet == SC.PROTEIN
                       else S.ALPHABET_DNA, gap_model=model)
    bank.set_matrix(sub, go, ge)
    return bank


def _want(name, pset, model, q=None, key=None):
    """Oracle scores of the family's targets (its template for a uniform family), computed once
    and shared read-only; q: another query of a set."""
    k = (name, pset, model, key)
    if k not in _WANT:
        fq, tg, _ = SC.seam_family(name)
        sub, go, ge = _params(name, pset, model)
        _WANT[k] = SC.oracle_scores(O, fq if q is None else q, list(tg), sub, go, ge,
                                    _omodel(model))
        _WANT[k].setflags(write=False)
    return _WANT[k]


def _exact(got, want, kern, *ctx):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (kern, ctx, int(bad.size),
                           [(int(i), int(got[i]), int(want[i])) for i in bad[:8]])


def _arith_env(monkeypatch, arith):
    monkeypatch.setenv("SWBANK_F16", "0" if arith == "u16" else "1")


def _host(monkeypatch, name, pset, model, check, seqs=None, want=None):
    """score_targets of the family's ragged batch; check(kernel name) proves the path."""
    q, tg, _ = SC.seam_family(name)
    with _bank(name, pset, model) as bank:
        bank.load_query(q)
        got = bank.score_targets(tg if seqs is None else seqs)
        kern = bank.last_kernel()
    check(kern)
    _exact(got, _want(name, pset, model) if want is None else want, kern, name, pset, model)
    return kern


# ---- tile kernel: wave to wave through the LDS ring --------------------------------------------
@pytest.mark.parametrize("arith", ["f16", "u16"])
@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("R", [32, 16])
@pytest.mark.parametrize("name", ["ring100", "ring130"])
def test_tile_ring(name, R, model, pset, arith, monkeypatch):
    """Deletions over every multiple of 16 rows that can carry a live gap (96 of 100 included;
    128 of 130 cannot, tests/seam_cases.py): with R = 16 every one is a wave boundary, with
    R = 32 every other one (the rest lie inside a wave's register column)."""
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    monkeypatch.setenv("SWBANK_R", str(R))
    _arith_env(monkeypatch, arith)
    qlen = SC.SEAMS[name].qlen

    def check(kern):
        m = re.match(r"tile (\S+?)(-profile| pair)? R=(\d+) W=(\d+) segs=(\d+)", kern)
        assert m and m.group(1) == arith, kern
        r, w, segs = int(m.group(3)), int(m.group(4)), int(m.group(5))
        # (a u16 Gotoh pass that follows no f16 pass runs 16 rows per wave whatever SWBANK_R)
        assert r == (16 if arith == "u16" and model == S.GAP_GOTOH else R), kern
        assert w == -(-qlen // r) and w > 1 and segs == 1, kern

    _host(monkeypatch, name, pset, model, check)


# ---- tile kernel: query segments through HBM edge rows -----------------------------------------
@pytest.mark.parametrize("arith", ["f16", "u16"])
@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name,seg,segs", [("seg300", "64", 5), ("seg600", None, 2)])
def test_tile_segments(name, seg, segs, model, pset, arith, monkeypatch):
    """Deletions over every segment boundary.  SWBANK_SEG applies to queries taller than one
    workgroup (16 waves), so the 64-row segments run at 16 rows per wave on a 300-row query
    (boundaries 64, 128, 192, 256); the 600-row query takes the default segments."""
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    if seg:
        monkeypatch.setenv("SWBANK_SEG", seg)
        monkeypatch.setenv("SWBANK_R", "16")
    _arith_env(monkeypatch, arith)

    def check(kern):
        m = re.search(r" R=(\d+) W=(\d+) segs=(\d+)", kern)
        assert kern.startswith(f"tile {arith}") and m, kern
        if seg:
            assert int(m.group(3)) == segs and int(m.group(1)) * int(m.group(2)) == 64, kern
        else:  # u16 Gotoh: 16 rows per wave, 256-row segments
            assert int(m.group(3)) >= segs and 512 % (int(m.group(1)) * int(m.group(2))) == 0, kern

    _host(monkeypatch, name, pset, model, check)


@pytest.mark.parametrize("model", MODELS)
def test_tile_segments_in_position_ranges(model, monkeypatch):
    """SWBANK_EDGE_MB=1: the segmented batch runs as position ranges, each with its own edge
    rows (the batch is repeated until it is longer than one range)."""
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    monkeypatch.setenv("SWBANK_EDGE_MB", "1")
    q, tg, _ = SC.seam_family("seg600")
    seqs = list(tg) * 5
    ecols = (max(len(t) for t in seqs) + 7) // 8 * 8
    span = max(1, (1 << 20) // (ecols * 64 * 8)) * 128  # (the launch's own rule)
    assert len(seqs) > span
    want = np.tile(_want("seg600", "free", model), 5)

    def check(kern):
        assert kern.startswith("tile f16") and "segs=2" in kern, kern

    _host(monkeypatch, "seg600", "free", model, check, seqs=seqs, want=want)


# ---- wave kernel: lane rows (DPP), 1024-row segments -------------------------------------------
@pytest.mark.parametrize("arith", ["f16", "u16"])
@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name,K,segs", [("lane100", 4, 1), ("lane300", 8, 1), ("lane600", 16, 1),
                                         ("lane1020", 16, 1), ("wseg1100", 16, 2)])
def test_wave_lanes_and_segments(name, K, segs, model, pset, arith, monkeypatch):
    """K rows per lane: every multiple of K is a lane boundary.  Deletions over every multiple
    of 16 and over K and 2K (rows 4 and 8 at K = 4, 8 and 16 at K = 8, 16 and 32 at K = 16) and,
    in the 1020-row query, 63K = 1008; past 1024 rows the bottom row of the first segment goes
    through HBM (a deletion over row 1024)."""
    monkeypatch.setenv("SWBANK_KERNEL", "wave")
    monkeypatch.setenv("SWBANK_WAVE_SPLIT", "0")
    _arith_env(monkeypatch, arith)

    def check(kern):
        assert kern.startswith(f"wave {arith}") and kern.endswith(f" K={K} segs={segs}"), kern

    _host(monkeypatch, name, pset, model, check)


# ---- wave kernel: split tail ---------------------------------------------------------------------
@pytest.mark.parametrize("arith", ["f16", "u16"])
@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name,P", [("strip300", 2), ("strip300", 4), ("strip600", 2),
                                    ("strip600", 4)])
def test_wave_split_tail(name, P, model, pset, arith, monkeypatch):
    """Every pair split into P row segments of 64 K / P rows: deletions over rows 128 and 256
    (K = 8) and 256 and 512 (K = 16) cross the segment boundaries of P = 2 and P = 4."""
    monkeypatch.setenv("SWBANK_KERNEL", "wave")
    monkeypatch.setenv("SWBANK_WAVE_SPLIT", "1000000")
    monkeypatch.setenv("SWBANK_WAVE_SPLIT_P", str(P))
    _arith_env(monkeypatch, arith)
    n = len(SC.seam_family(name)[1])

    def check(kern):
        assert kern.startswith(f"wave {arith}") and f" split={(n + 1) // 2}/{P}" in kern, kern

    _host(monkeypatch, name, pset, model, check)


@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("model", MODELS)
def test_wave_tail_of_eight_segments(model, pset, monkeypatch):
    """Protein, 400 rows, two pairs per wave with every pair as 8 segments of 64 rows, one wave
    each, handed on through global memory: deletions over every multiple of 64 rows."""
    monkeypatch.setenv("SWBANK_KERNEL", "wave")
    monkeypatch.setenv("SWBANK_WAVE_SPLIT", "1000000")
    monkeypatch.setenv("SWBANK_WAVE_SPLIT_P", "8")
    n = len(SC.seam_family("split8")[1])

    def check(kern):
        assert "pairs/wave=2" in kern and f" tail={(n + 1) // 2}/8" in kern, kern

    _host(monkeypatch, "split8", pset, model, check)


# ---- wave kernel: two pairs per wave ------------------------------------------------------------
@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n", [3, 333])
@pytest.mark.parametrize("name", ["half257", "half512"])
def test_wave_two_pairs(name, n, model, pset, monkeypatch):
    """Two pairs per wave: lanes 0-31 on one pair and 32-63 on the next, so a lane holds 16
    rows (the kernel name's K = 8 is the table layout, 64 K = 512 rows, shared with the
    one-pair form of 8 rows per lane).  Deletions over every multiple of 16 rows, 8 targets
    each; 3 targets (a last wave with one real half) and 333."""
    monkeypatch.setenv("SWBANK_KERNEL", "wave")
    monkeypatch.setenv("SWBANK_WAVE_SPLIT", "0")
    q, tg, mt = SC.seam_family(name)
    want = _want(name, pset, model)
    if n == 3:
        pick = [k for k, m in enumerate(mt) if m is not None][5:8]
        seqs, want = [tg[k] for k in pick], want[pick]
    else:
        seqs = tg
    assert len(seqs) == n

    def check(kern):
        assert kern.startswith("wave f16") and kern.endswith("K=8 segs=1 pairs/wave=2"), kern

    _host(monkeypatch, name, pset, model, check, seqs=seqs, want=want)


# ---- uniform device batches: a template of whole tiles, repeated ---------------------------------
def _uniform_device(name, pset, model, n, calls=2):
    """The family's template repeated to n targets, scored `calls` times back to back through
    score_batch_device_range: ([scores], kernel name, counters, expected scores of all n)."""
    import torch
    q, tpl, _ = SC.seam_family(name)
    L = tpl.shape[1]
    idx = np.arange(n) % len(tpl)
    res = np.ascontiguousarray(tpl[idx]).reshape(-1)
    dev = torch.device("cuda", 0)
    d_res = torch.from_numpy(res).to(dev)
    d_offs = torch.arange(n, dtype=torch.int64, device=dev) * L
    d_lens = torch.full((n,), L, dtype=torch.int32, device=dev)
    out = []
    with _bank(name, pset, model) as bank:
        bank.load_query(q)
        st = torch.cuda.Stream()
        for _ in range(calls):
            sc = torch.full((n,), -7, dtype=torch.int32, device=dev)
            bank.score_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, L,
                                    sc.data_ptr(), st.cuda_stream, min_len=L)
            out.append(sc)
        st.synchronize()
        bank.sync()
        kern, ctr = bank.last_kernel(), bank.counters()
    return [x.cpu().numpy() for x in out], kern, ctr, _want(name, pset, model)[idx]


@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name,n,W", [("wbal48", 18_000, 4), ("wbal48", 26_000, 8),
                                      ("wbal64", 18_000, 4), ("wbal64", 26_000, 8),
                                      ("wbal1000", 12_500, 4), ("wbal1000", 12_500, 8)])
def test_wave_balanced_ranges(name, n, W, model, pset, monkeypatch):
    """Balanced 32-step block ranges of the two-pairs wave kernel, the lane state handed over
    through global memory and a flag: insertions over every multiple of 32 columns (and, at
    L = 1000, deletions over every multiple of 16 rows); the smallest admitted shapes of
    tests/test_gpu_wave_balanced_short.py and the shape of tests/test_gpu_wave_balanced.py."""
    monkeypatch.setenv("SWBANK_KERNEL", "wave")
    monkeypatch.setenv("SWBANK_WAVE_W", str(W))
    gots, kern, ctr, want = _uniform_device(name, pset, model, n)
    assert "pairs/wave=2" in kern and re.search(rf"balanced grid=\d+x{W}$", kern), kern
    assert ctr["wave_balanced_timeouts"] == 0 and ctr["tail_timeouts"] == 0, ctr
    for got in gots:
        _exact(got, want, kern, name, n, W, pset, model)


@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("name,n", [("tbal40x24", 600_001), ("tbal40x64", 600_001),
                                    ("tbal40x128", 600_001), ("tbal100x24", 300_001),
                                    ("tbal100x64", 300_001), ("tbal100x128", 300_001)])
def test_tile_balanced_ranges_uniform(name, n, pset, monkeypatch):
    """Balanced chunk ranges of the pair-table tile kernel (merged gaps): insertions over every
    8-column chunk boundary, so wherever a range boundary cuts a tile the gap value T is live
    in some of its lanes; every target of the batch is checked."""
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    gots, kern, ctr, want = _uniform_device(name, pset, S.GAP_MERGED, n)
    m = re.search(r"balanced grid=(\d+)$", kern)
    assert kern.startswith("tile f16 pair R=32") and m, kern
    assert (n + 127) // 128 >= 2 * int(m.group(1))
    assert ctr["balanced_calls"] == 2 and ctr["balanced_timeouts"] == 0, ctr
    for got in gots:
        _exact(got, want, kern, name, n, pset)


@pytest.mark.parametrize("pset", PSETS)
def test_tile_balanced_ranges_ragged(pset, monkeypatch):
    """The device sort's plan: 1.5 million straddle targets of 30-61 letters (4,096 distinct
    ones, repeated), every target checked."""
    import torch
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    q, tpl, _ = SC.seam_family("rbal40")
    n, reps = 1_500_000, -(-1_500_000 // len(tpl))
    lens_t = np.array([len(t) for t in tpl], np.uint32)
    assert lens_t.min() >= 30 and lens_t.max() <= 61
    res = np.tile(np.concatenate(tpl), reps)
    lens = np.tile(lens_t, reps)[:n]
    offs = np.zeros(n, np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    want = np.tile(_want("rbal40", pset, S.GAP_MERGED), reps)[:n]
    dev = torch.device("cuda", 0)
    d_res = torch.from_numpy(res).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
    sc = torch.full((n,), -7, dtype=torch.int32, device=dev)
    with _bank("rbal40", pset, S.GAP_MERGED) as bank:
        bank.load_query(q)
        st = torch.cuda.Stream()
        bank.score_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, 61,
                                sc.data_ptr(), st.cuda_stream, min_len=30)
        st.synchronize()
        kern, ctr = bank.last_kernel(), bank.counters()
    assert "balanced" in kern and "dsort" in kern, kern
    assert ctr["balanced_calls"] == 1 and ctr["balanced_timeouts"] == 0, ctr
    _exact(sc.cpu().numpy(), want, kern, pset)


# ---- streamed host call ---------------------------------------------------------------------------
@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("model", MODELS)
def test_streamed_host_call(model, pset, monkeypatch):
    """The streamed kernel (chunks of whole tiles published while it runs) on 40,000 targets of
    120 letters built from the tile template; every target checked."""
    monkeypatch.setenv("SWBANK_STREAM", "2")
    monkeypatch.delenv("SWBANK_KERNEL", raising=False)
    q, tpl, _ = SC.seam_family("stream100x120")
    n, L = 40_000, tpl.shape[1]
    idx = np.arange(n) % len(tpl)
    res = np.ascontiguousarray(tpl[idx]).reshape(-1)
    with _bank("stream100x120", pset, model) as bank:
        bank.load_query(q)
        got = bank.score_batch(res, np.arange(n, dtype=np.uint64) * L, np.full(n, L, np.uint32))
        kern, ctr = bank.last_kernel(), bank.counters()
    assert "streamed=" in kern and ctr["stream_calls"] == 1 and ctr["stream_reruns"] == 0, (kern, ctr)
    _exact(got, _want("stream100x120", pset, model)[idx], kern, pset, model)


# ---- the 256-row strips of the int32 and alignment kernels -----------------------------------------
@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ["strip300", "strip600"])
def test_int32_strips(name, model, pset, monkeypatch):
    """Every pair again through the int32 kernel, whose column state passes from one 256-row
    strip to the next: deletions over rows 256 and 512."""
    monkeypatch.setenv("SWBANK_I32", "1")

    def check(kern):
        assert kern.endswith("+i32-rescore"), kern

    _host(monkeypatch, name, pset, model, check)


@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("name", ["strip300", "strip600"])
def test_alignment_strips(name, model, pset):
    """align_targets on the deletion targets over rows 256 (and 512): coordinates against the
    brute-force tie rules, the CIGAR re-scored, and a query-only run (I) in every path."""
    q, tg, mt = SC.seam_family(name)
    sub, go, ge = _params(name, pset, model)
    om = _omodel(model)
    hits = [k for k, m in enumerate(mt) if m is not None and m.cut % 256 == 0] + [1, 2]
    assert len(hits) >= 6
    brute = AC.brute_ends_batch(O, q, [tg[h] for h in hits], sub, go, ge, om)
    with _bank(name, pset, model) as bank:
        bank.load_query(q)
        alns = bank.align_targets(tg, hits)
        kern = bank.last_kernel()
    assert kern.startswith(f"align i32 hits={len(hits)}"), kern
    for h, a, b in zip(hits, alns, brute):
        AC.check_alignment(O, q, tg[h], sub, go, ge, om, a)
        assert (a.score, a.q_start, a.q_end, a.t_start, a.t_end) == b, (h, a, b)
        if mt[h] is not None:
            assert a.q_start < mt[h].cut < a.q_end, (h, a)
            assert any(op & 15 == AC.I for op in a.ops), (h, a.cigar)


# ---- query sets -------------------------------------------------------------------------------------
@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("qlens", [(130, 600, 40), (130, 513, 40)])
def test_query_set_segments(qlens, model, pset, monkeypatch):
    """One launch per query segment for a set of three queries: deletions over row 512, the
    segment boundary of the longest.  (130, 513, 40) is tests/test_gpu_queries.py's shape, but a
    gap cannot lie over the last row but one, so the set with a 600-row query carries the live
    gaps; the 513-row query is the 600-row one cut short.)  The one-launch variant is exact
    16-bit arithmetic: u16 at these lengths."""
    import torch
    monkeypatch.setenv("SWBANK_KERNEL", "tile")
    q, tg, _ = SC.seam_family("qset600")
    queries = [q[300:300 + qlens[0]].copy(), q[:qlens[1]].copy(), q[500:500 + qlens[2]].copy()]
    res, offs, lens = S.pack_targets(tg)
    dev = torch.device("cuda", 0)
    d_res = torch.from_numpy(res).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_sc = torch.full((3, len(tg)), -7, dtype=torch.int32, device=dev)
    with _bank("qset600", pset, model) as bank:
        bank.load_queries(queries)
        st = torch.cuda.Stream()
        bank.score_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), len(tg),
                                int(lens.max()), d_sc.data_ptr(), st.cuda_stream)
        st.synchronize()
        kern = bank.last_kernel()
    m = re.search(r" segs=(\d+) queries=3$", kern)
    assert kern.startswith("tile u16") and m and int(m.group(1)) >= 2, kern
    got = d_sc.cpu().numpy()
    for k, qq in enumerate(queries):
        want = _want("qset600", pset, model, q=qq, key=(qlens, k))
        _exact(got[k], want, kern, qlens, k, pset, model)
