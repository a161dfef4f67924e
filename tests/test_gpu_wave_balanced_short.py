"""GPU: balanced ranges of the two-pairs protein wave kernel at short targets.

tests/test_gpu_wave_balanced.py sits at L = 850-1300 (B = ⌈(L + 31)/32⌉ of about 33 blocks per
unit).  Here B is 1-5, where every cut of a unit lies inside the 31-step fill or drain of the
lane pipeline, and the range is the 4-block minimum of the launch rule U B >= 4 W grid (U units
of four targets on grid blocks of W waves), the rule the host's kernel choice and the launch
guard share (swk_wbal_admissible).

 a. the library's own choice (no SWBANK_KERNEL, no SWBANK_WAVE_W) at the batch sizes where the
    host used to pick a balanced launch the guard refused (SW_ERR_HIP before any launch);
 b. each side of every step of B from 1 to 5, the balanced path forced and reached;
 c. ranges of exactly 4 blocks, every unit cut three times (middle visits chained), and the
    first batch size below the rule;
 d. a seeded sweep of the library's own choice over short targets and large batches.

Every case: protein, BLOSUM62, poisoned device buffers, two calls back to back on one bank (the
flags' generation), every target against the oracle, no hand-off wait run out."""
import functools
import os
import re

import numpy as np
import pytest

import swbank as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

MODELS = (S.GAP_GOTOH, S.GAP_MERGED)


def _batch(rng, n, qlen, L):
    """The recipe of tests/test_gpu_wave_balanced.py: random targets, some near-copies of the
    query (scores past the optimistic f16 threshold when L allows)."""
    q = rng.integers(0, 20, qlen, dtype=np.uint8)
    res = rng.integers(0, 20, n * L, dtype=np.uint8)
    for k in rng.choice(n, max(4, n // 400), replace=False):
        t = np.resize(q, L).copy()
        t[::9] = rng.integers(0, 20, len(t[::9]))
        res[k * L:(k + 1) * L] = t
    return q, res, np.arange(n, dtype=np.uint64) * L, np.full(n, L, np.uint32)


def _blocks(L):
    return (L + 62) // 32  # B: 32-step blocks of a unit (L + 31 steps)


def _omodel(model):
    return O.GAP_GOTOH if model == S.GAP_GOTOH else O.GAP_MERGED


def _parse(kern):
    """(grid, W) of a balanced two-pairs launch, None otherwise."""
    m = re.search(r"balanced grid=(\d+)x(\d+)", kern)
    return (int(m.group(1)), int(m.group(2))) if m else None


def _check_rule(kern, n, L):
    grid, W = _parse(kern)
    U = ((n + 1) // 2 + 1) // 2
    assert U * _blocks(L) >= 4 * W * grid, (kern, n, L, U, _blocks(L))
    return grid, W


def _no_timeouts(bank, kern):
    ctr = bank.counters()
    assert (ctr["tail_timeouts"] == 0 and ctr["balanced_timeouts"] == 0
            and ctr["wave_balanced_timeouts"] == 0), (kern, ctr)


def _device_twice(n, L, q, res, offs, lens, model, go=-11, ge=-1):
    """Two back-to-back device calls on one bank: ([scores, scores], kernel name)."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    d_res = torch.from_numpy(res).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
    out = []
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=model) as bank:
        bank.set_matrix(O.BLOSUM62, go, ge)
        bank.load_query(q)
        for _ in range(2):
            sc = torch.full((n,), -7, dtype=torch.int32, device=dev)
            bank.score_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, L,
                                    sc.data_ptr(), min_len=L)
            out.append(sc)
        bank.sync()
        kern = bank.last_kernel()
        _no_timeouts(bank, kern)
    return [x.cpu().numpy() for x in out], kern


def _exact(gots, want, kern, *ctx):
    for got in gots:
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (kern, ctx, int(bad.size),
                               [(int(i), int(got[i]), int(want[i])) for i in bad[:8]])


@functools.lru_cache(maxsize=None)
def _grid(W, model):
    """Resident blocks of the W-wave balanced launch, read from the kernel name of one forced
    launch on one-letter targets with 8 units per nominal wave slot (any rule holds)."""
    torch = pytest.importorskip("torch")
    n = 4 * (8 * (4096 if W == 8 else 3072) + 1)
    rng = np.random.default_rng(W)
    q, res, offs, lens = _batch(rng, n, 512, 1)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SWBANK_KERNEL", "wave")
        mp.setenv("SWBANK_WAVE_W", str(W))
        _, kern = _device_twice(n, 1, q, res, offs, lens, model)
    got = _parse(kern)
    assert got is not None and got[1] == W, kern
    return got[0]


# ---- a. the library's own choice where the launch guard used to refuse the host's choice ----

_REFUSED = [(14_000, 48), (14_000, 64), (12_289, 65), (16_380, 65), (20_000, 48), (21_844, 34),
            (30_000, 33), (40_000, 2)]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n,L", _REFUSED)
def test_short_unforced_device(n, L, model, monkeypatch, poisoned_buffers):
    """No kernel forced: a 512-row query against n targets of L residues.  Before the host and
    the launch guard shared one rule, each of these failed with SW_ERR_HIP (the host chose 8- or
    4-wave balanced blocks by units per slot alone; the guard wants ranges of 4 blocks)."""
    monkeypatch.delenv("SWBANK_KERNEL", raising=False)
    monkeypatch.delenv("SWBANK_WAVE_W", raising=False)
    q, res, offs, lens = _batch(np.random.default_rng(n + L), n, 512, L)
    gots, kern = _device_twice(n, L, q, res, offs, lens, model)
    print(f"a device n={n} L={L} model={model}: {kern}")
    if "balanced" in kern and "pairs/wave=2" in kern:
        _check_rule(kern, n, L)
    want = O.score_batch(q, res, offs, lens, O.BLOSUM62, -11, -1, _omodel(model))
    _exact(gots, want, kern, n, L)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("n,L", [(14_000, 64), (16_401, 65)])
def test_short_unforced_host(n, L, model, monkeypatch, poisoned_buffers):
    """The same through the host-buffer API: the feeder's equal-length chunks reach the kernel
    without offset or length arrays (ScoreArgs.ulen / ustride)."""
    monkeypatch.delenv("SWBANK_KERNEL", raising=False)
    monkeypatch.delenv("SWBANK_WAVE_W", raising=False)
    q, res, offs, lens = _batch(np.random.default_rng(n + L), n, 512, L)
    with S.ScoreBank(alphabet=S.ALPHABET_PROTEIN, gap_model=model) as bank:
        bank.set_matrix(O.BLOSUM62, -11, -1)
        bank.load_query(q)
        gots = [bank.score_batch(res, offs, lens).copy() for _ in range(2)]
        kern = bank.last_kernel()
        _no_timeouts(bank, kern)
    print(f"a host n={n} L={L} model={model}: {kern}")
    want = O.score_batch(q, res, offs, lens, O.BLOSUM62, -11, -1, _omodel(model))
    _exact(gots, want, kern, n, L)


# ---- b. each side of every step of B from 1 to 5, the balanced path reached ----

_EDGE_L = (1, 2, 33, 34, 65, 66, 97, 98)
_QLENS = (257, 400, 512)  # 257: the shortest query with K = 8 tables (two pairs per wave)


def _edge_cases():
    """(L, W, model, qlen, r): W = 4 and 8 with both gap models, the library's choice (W = 0) with
    the models alternating; qlen and r (the last unit holds 4 - r targets) spread over the cases."""
    out, i = [], 0
    for w in (4, 8, 0):
        for L in _EDGE_L:
            for model in (MODELS if w else (MODELS[(i // 2) % 2],)):
                out.append((L, w, model, _QLENS[i % 3], (i + i // 4) % 4))
                i += 1
    return out


@pytest.mark.parametrize("L,w,model,qlen,r", _edge_cases())
def test_short_block_count_edges(L, w, model, qlen, r, monkeypatch, poisoned_buffers):
    """U = the fewest units the W-wave launch admits + 2, so ranges are just past 4 blocks: with
    B <= 4 every range boundary falls in a unit's fill or drain steps (a unit has L + 31 steps).
    W = 8 needs U B >= 4 G only; W = 4 (and the library's choice) also a unit per slot, U >= G,
    and U % G != 0, so U = max(ceil(4 G / B), G) + 2 there (bumped when a multiple of G)."""
    monkeypatch.setenv("SWBANK_KERNEL", "wave")
    if w:
        monkeypatch.setenv("SWBANK_WAVE_W", str(w))
    else:
        monkeypatch.delenv("SWBANK_WAVE_W", raising=False)
    B = _blocks(L)
    G = (w or 4) * _grid(w or 4, model)
    U = -(-4 * G // B) + 2 if w == 8 else max(-(-4 * G // B), G) + 2
    if U % G == 0:
        U += 1
    n = 4 * U - r
    q, res, offs, lens = _batch(np.random.default_rng(n + L), n, qlen, L)
    gots, kern = _device_twice(n, L, q, res, offs, lens, model)
    print(f"b L={L} B={B} w={w} model={model} qlen={qlen} n={n}: {kern}")
    assert "pairs/wave=2" in kern and "balanced" in kern, kern
    grid, W = _check_rule(kern, n, L)
    assert w == 0 or W == w, kern
    want = O.score_batch(q, res, offs, lens, O.BLOSUM62, -11, -1, _omodel(model))
    _exact(gots, want, kern, n, L, qlen)


# ---- c. ranges of exactly 4 blocks: chained middle visits ----

# (L, units past ceil(4 G / B), targets missing from the last unit): with G = 4,096 slots these
# are n = 4,096 and 4,093 at L = 480, 4,100 at L = 450 (B = 16: every range exactly / nearly 4
# blocks, every unit cut three times) and 6,000 at L = 290 (B = 11: ranges of 4.03 blocks, the
# cuts at no fixed place in a unit)
_CHAIN = [(480, 0, 0), (480, 0, 3), (450, 1, 0), (290, 10, 0)]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("L,extra,r", _CHAIN)
def test_short_min_range_chained(L, extra, r, model, monkeypatch, poisoned_buffers):
    monkeypatch.setenv("SWBANK_KERNEL", "wave")
    monkeypatch.setenv("SWBANK_WAVE_W", "8")
    B = _blocks(L)
    U = -(-32 * _grid(8, model) // B) + extra
    n = 4 * U - r
    q, res, offs, lens = _batch(np.random.default_rng(n + L), n, 512, L)
    gots, kern = _device_twice(n, L, q, res, offs, lens, model)
    print(f"c L={L} B={B} model={model} n={n}: {kern}")
    assert "pairs/wave=2" in kern and "balanced" in kern and "x8" in kern, kern
    _check_rule(kern, n, L)
    want = O.score_batch(q, res, offs, lens, O.BLOSUM62, -11, -1, _omodel(model))
    if L >= 450:  # the finishing visit of a thrice-cut unit re-scores it in u16
        assert want.max() > 2048, int(want.max())
    _exact(gots, want, kern, n, L)


@pytest.mark.parametrize("model", MODELS)
def test_short_below_min_range_not_balanced(model, monkeypatch, poisoned_buffers):
    """One unit fewer than the rule admits (n = 4,092 at L = 480 on 4,096 slots): the host takes
    the unbalanced launch instead, and the scores are exact."""
    monkeypatch.setenv("SWBANK_KERNEL", "wave")
    monkeypatch.setenv("SWBANK_WAVE_W", "8")
    L = 480
    U = -(-32 * _grid(8, model) // _blocks(L)) - 1
    n = 4 * U
    q, res, offs, lens = _batch(np.random.default_rng(n + L), n, 512, L)
    gots, kern = _device_twice(n, L, q, res, offs, lens, model)
    print(f"c negative L={L} model={model} n={n}: {kern}")
    assert "balanced" not in kern, kern
    want = O.score_batch(q, res, offs, lens, O.BLOSUM62, -11, -1, _omodel(model))
    assert want.max() > 2048, int(want.max())
    _exact(gots, want, kern, n, L)


# ---- d. seeded sweep of the library's own choice ----

#  SWBANK_WBALS_SEEDS=n (default 16) / SWBANK_WBALS_BASE=b: seeds b .. b+n-1
_SS_BASE = int(os.environ.get("SWBANK_WBALS_BASE", "0"))
_SS_SEEDS = int(os.environ.get("SWBANK_WBALS_SEEDS", "16"))


@pytest.mark.parametrize("seed", range(_SS_BASE, _SS_BASE + _SS_SEEDS))
def test_short_unforced_sweep(seed, monkeypatch, poisoned_buffers):
    """Short equal-length targets in batches of 12,000-70,000, where the kernel choice and the
    balanced launch's predicates flip: whatever the library picks is exact on every target."""
    monkeypatch.delenv("SWBANK_KERNEL", raising=False)
    monkeypatch.delenv("SWBANK_WAVE_W", raising=False)
    rng = np.random.default_rng(90_000 + seed)
    qlen = int(rng.integers(257, 513))
    L = int(rng.integers(1, 201))
    n = int(rng.integers(12_000, min(70_000, int(3e9) // (L * qlen)) + 1))
    model = S.GAP_GOTOH if rng.random() < 0.5 else S.GAP_MERGED
    go, ge = -int(rng.integers(10, 15)), -int(rng.integers(1, 4))
    q, res, offs, lens = _batch(rng, n, qlen, L)
    gots, kern = _device_twice(n, L, q, res, offs, lens, model, go, ge)
    print(f"d seed={seed} n={n} L={L} qlen={qlen} model={model} gaps={go}/{ge}: {kern}")
    if "balanced" in kern and "pairs/wave=2" in kern:
        _check_rule(kern, n, L)
    want = O.score_batch(q, res, offs, lens, O.BLOSUM62, go, ge, _omodel(model))
    _exact(gots, want, kern, seed, n, L, qlen, model, go, ge)
