"""The shuffle of long targets on the GPU (swbank_kstat.hip): targets past a
lane's LDS row are shuffled by a workgroup of their own in LDS sized by their class, those past
the largest class in place in global memory.  Every byte is compared with the header's
Fisher-Yates definition as tests/stat_cases.py restates it: each side of the lane row and of every
class limit (the limits come from the library), short and long targets mixed in one batch, odd
offsets with gaps, a 0x3C fill that nothing else may touch, the caller's layout
(sw_shuffle_batch_device) and the estimate's stride layout at a batch position other than 0
(swk_shuffle_batch as the estimates call it), DNA and protein codes.

The two layouts share one reference: the batch starts with HEAD empty targets, the caller's
layout shuffles all of it from position 0, the stride layout its rest from position HEAD."""
import ctypes

import numpy as np
import pytest

import swbank as S

import stat_cases as SC

pytestmark = pytest.mark.gpu

FILL = 0x3C
HEAD = 5
SHORT = [0, 1, 2, 3, 64, 128, 255]
MID = [261, 262, 323, 324, 325, 1021, 4099]


def _limit(i):
    f = S.lib().swk_shuffle_class_limit
    f.restype = ctypes.c_uint32
    f.argtypes = [ctypes.c_int]
    return int(f(i))


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


def _filled(nbytes):
    torch = _torch()
    return torch.full((max(nbytes, 1),), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))


def _around(x):
    return [x - 1, x, x + 1]


def _batch(lens, alpha, seed):
    """HEAD empty targets, then targets of the given lengths at odd byte offsets with gaps
    between them: (residues, offsets, lengths, the mask of the targets' bytes)."""
    rng = np.random.default_rng([seed, alpha, len(lens)])
    lens = np.array([0] * HEAD + list(lens), np.uint32)
    offs = np.zeros(len(lens), np.int64)
    pos = 0
    for k in range(len(lens)):
        pos += 2 * int(rng.integers(0, 4)) + 1
        pos += (pos + 1) % 2  # every start is odd
        offs[k] = pos
        pos += int(lens[k])
    res = rng.integers(0, alpha, pos + 5).astype(np.uint8)
    mask = np.zeros(len(res), bool)
    for k in range(len(lens)):
        mask[offs[k]:offs[k] + int(lens[k])] = True
    assert (offs % 2 == 1).all()
    return res, offs.astype(np.uint64), lens, mask


def _check_caller_layout(res, offs, lens, mask, seed, want):
    """sw_shuffle_batch_device over the whole batch."""
    torch = _torch()
    d_res, d_offs, d_lens = _to_dev(res), _to_dev(offs), _to_dev(lens)
    d_out = _filled(len(res))
    torch.cuda.synchronize()
    with S.ScoreBank() as bank:
        bank.shuffle_batch_device(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), len(lens),
                                  int(lens.max()), seed, d_out.data_ptr())
        assert bank.last_kernel() == f"shuffle n={len(lens)}"
        bank.sync()
    got = d_out.cpu().numpy()
    exp = np.where(mask, want, FILL).astype(np.uint8)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (seed, bad[:8], got[bad[:8]], exp[bad[:8]])
    assert np.array_equal(d_res.cpu().numpy(), res)  # the input is left alone


def _check_stride_layout(res, offs, lens, seed, want):
    """swk_shuffle_batch as the estimates call it: the targets past HEAD, keyed from position
    HEAD, each at a fixed stride of a scratch, its offset written beside it."""
    torch = _torch()
    fn = S.lib().swk_shuffle_batch
    P = ctypes.c_void_p
    fn.restype = ctypes.c_int
    fn.argtypes = [P, P, P, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, P, P,
                   ctypes.c_uint32, P]
    n = len(lens) - HEAD
    max_len = int(lens.max())
    stride = (max_len + 15) // 16 * 16 + 16
    d_res, d_offs, d_lens = _to_dev(res), _to_dev(offs[HEAD:]), _to_dev(lens[HEAD:])
    d_out = _filled(n * stride + 64)
    d_oo = _to_dev(np.full(n, 0x3C3C3C3C3C3C3C3C, np.uint64))
    torch.cuda.synchronize()
    assert fn(d_res.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), n, max_len, HEAD, seed,
              d_out.data_ptr(), d_oo.data_ptr(), stride, None) == 0
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(d_oo.cpu().numpy().view(np.uint64),
                          np.arange(n, dtype=np.uint64) * np.uint64(stride))
    exp = np.full(len(got), FILL, np.uint8)
    for k in range(n):
        o, ln = int(offs[HEAD + k]), int(lens[HEAD + k])
        exp[k * stride:k * stride + ln] = want[o:o + ln]
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (seed, bad[:8], got[bad[:8]], exp[bad[:8]])


def test_class_limits_are_exported():
    row, limits = _limit(-1), [_limit(i) for i in range(4)]
    assert row == 260 and limits[3] == 0
    assert row < limits[0] < limits[1] < limits[2] <= 160 << 10  # a CU's LDS
    assert 4099 > limits[0] and limits[1] < 70000 <= limits[2]   # the lengths below meet each class


@pytest.mark.parametrize("alpha", [5, 24], ids=["dna", "protein"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_lane_row_and_first_class(n, alpha):
    """n targets walking through short lengths, each side of the lane row and of the first
    class's limit, and the lengths between: one, and more than one, wave of the lane tier with
    the long targets' workgroups beside it."""
    pool = _around(_limit(-1)) + _around(_limit(0)) + MID + SHORT
    pool = sorted(set(pool), key=lambda x: (x * 7919) % 104729)  # mixed, the same every time
    lens = [_limit(0) + 1] if n == 1 else [pool[k % len(pool)] for k in range(n)]
    if n >= 63:
        assert set(pool) <= set(lens)
    res, offs, lens, mask = _batch(lens, alpha, n)
    for seed in (11, 0xFFFFFFFFFFFFFFF5) if n == 65 else (11,):
        want = SC.shuffle(res, offs, lens, seed)
        _check_caller_layout(res, offs, lens, mask, seed, want)
        _check_stride_layout(res, offs, lens, seed, want)


def test_upper_classes_and_the_global_tier():
    """Each side of the second and third class's limits, 70,000 bases, and short targets between
    them; the one target past the largest class is shuffled in global memory."""
    lens = [100] + _around(_limit(1)) + [300, 70000] + _around(_limit(2)) + [1021, 0, 261]
    assert sum(l > _limit(2) for l in lens) == 1
    res, offs, lens, mask = _batch(lens, 24, 3)
    want = SC.shuffle(res, offs, lens, 7)
    _check_caller_layout(res, offs, lens, mask, 7, want)
    _check_stride_layout(res, offs, lens, 7, want)
