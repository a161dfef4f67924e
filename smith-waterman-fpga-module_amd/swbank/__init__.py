"""swbank — Python host over libswbank.so (ctypes), mirroring the reference ScoreBank surface.

The reference's "host" for this path is the ScoreBank testbench (ScoreBank/ScoreBank_v1_tb.sv)
and the CAPI C host (capi_sample_aligner/software-C,C++/src/main_test.c).  This module keeps
their order of operations:

    bank = ScoreBank()                                  # ScoreBank_v2 instance + reset
    bank.set_penalties(5, -4, -12, -4)                  # ld_penalties   (ScoreBank_v2.v:161)
    bank.load_query(encode("AGGGCG..."))                # ld_sequence q  (ScoreBank_v2.v:162)
    scores = bank.score_batch(targets)                  # target records -> results/IDs/vld

Everything goes through the C ABI declared in include/swbank.h; there is no Python compute
path and no CPU fallback: if libswbank.so is missing, or no gfx950 device is present,
construction raises.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("SWBANK_LIB", os.path.join(_PKG, "lib", "libswbank.so"))
CLI_PATH = os.path.join(_PKG, "bin", "swbank")

OK = 0
ERR_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_RANGE, ERR_STATE, ERR_NOMEM, ERR_IO, ERR_UNSUPPORTED = \
    -1, -2, -3, -4, -5, -6, -7, -8
ERR_TIMEOUT = -9  # a device-side hand-off wait ran out (ABI 5): the call's scores are invalid
ALPHABET_DNA, ALPHABET_PROTEIN = 0, 1
GAP_MERGED, GAP_GOTOH = 0, 1
DNA_ALPHA, PROTEIN_ALPHA = 5, 24

# Every symbol include/swbank.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "sw_abi_version", "sw_status_string", "sw_device_count", "sw_max_query_len",
    "sw_config_default", "sw_bank_create", "sw_bank_destroy", "sw_last_error",
    "sw_set_penalties", "sw_set_matrix", "sw_load_query", "sw_score_batch",
    "sw_score_batch_device", "sw_best_hit", "sw_encode_ascii", "sw_pack_2bit",
    "sw_unpack_2bit", "sw_fill_matrix", "sw_bank_set_timing", "sw_bank_timing",
    "sw_last_kernel", "sw_load_query_record", "sw_score_records", "sw_score_records_device",
    "sw_best_hit_device", "sw_batch_best", "sw_bank_devices", "sw_load_queries",
    "sw_query_count", "sw_score_batch_device_range", "sw_bank_counters",
    "sw_bank_counters_ex", "sw_bank_sync", "sw_score_batch_device_multi",
    "sw_align_hits", "sw_align_hits_device", "sw_cigar_string",
    "sw_top_hits", "sw_top_hits_device",
    "sw_best_queries", "sw_best_queries_device",
    "sw_align_set_hits", "sw_align_set_hits_device",
    "sw_shuffle_batch_device", "sw_score_histogram_device", "sw_fit_statistics",
    "sw_estimate_statistics", "sw_estimate_statistics_device",
    "sw_hit_significance", "sw_hit_significance_device",
    "sw_revcomp_codes", "sw_revcomp_batch_device", "sw_score_strands",
    "sw_score_strands_device", "sw_align_strand_hits", "sw_align_strand_hits_device",
    "sw_translate_codes", "sw_translate_batch_device", "sw_score_frames",
    "sw_score_frames_device", "sw_align_frame_hits", "sw_align_frame_hits_device",
    "sw_score_fshift", "sw_score_fshift_device",
    "sw_align_fshift_hits", "sw_align_fshift_hits_device",
    "sw_estimate_fshift_statistics", "sw_estimate_fshift_statistics_device",
    "sw_score_glocal", "sw_score_glocal_device",
    "sw_align_glocal_hits", "sw_align_glocal_hits_device",
    "sw_align_disjoint_hits", "sw_align_disjoint_hits_device",
    "sw_align_disjoint_frame_hits", "sw_align_disjoint_frame_hits_device",
)
ABI_VERSION = 6
COUNTERS = ("stream_calls", "stream_reruns", "stream_declined", "chunked_calls", "device_sorts",
            "gather_timeouts", "mixed_chunks", "mixed_runs", "balanced_calls",
            "balanced_timeouts", "tail_timeouts", "handoff_reruns", "wave_balanced_timeouts",
            "h2d_bytes")
MAX_DEVICES = 16
CIGAR_M, CIGAR_I, CIGAR_D = 0, 1, 2          # BAM codes: I consumes query only, D target only
CIGAR_FS_SKIP, CIGAR_FS_BACK = 3, 4          # frameshift hits: the next codon starts one base
#                                              later ('/') or one base earlier ('\'), length 1
ALIGN_EMPTY, ALIGN_NO_PATH = 1, 2            # sw_alignment.flags
ALIGN_NO_HIT = 4                             # ... the slot named no pair (with ALIGN_EMPTY)
ALIGN_REVERSE = 8                            # ... aligned against the target's reverse complement
ALIGN_FRAME_SHIFT, ALIGN_FRAME_MASK = 4, 0x30  # ... f % 3 of a translated hit's reading frame
_ALIGN_WHERE = ALIGN_REVERSE | ALIGN_FRAME_MASK  # (flags that say where a hit lies, not how)
FRAME_COUNT = 6                              # SW_FRAME_COUNT: reading frames of a DNA target
FRAME_TAGS = ("+1", "+2", "+3", "-1", "-2", "-3")
FSHIFT_MAX_QUERY = 1024                      # SW_FSHIFT_MAX_QUERY: query rows of score_frameshift
GLOCAL_MAX_QUERY = 1024                      # SW_GLOCAL_MAX_QUERY: query rows of score_glocal
ENDS_QUERY, ENDS_TARGET, ENDS_BOTH = 1, 2, 3  # SW_ENDS_*: what score_glocal aligns end to end
DISJOINT_MAX_QUERY = 1024                    # SW_DISJOINT_MAX_QUERY: query rows of align_disjoint_hits
DISJOINT_MAX_ROUNDS = 64                     # SW_DISJOINT_MAX_ROUNDS: alignments per hit
END_NONE = 0xFFFFFFFF                        # SW_END_NONE: the score is the boundary's
STANDARD_CODE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
RECORD_BYTES, RECORD_MAX_BASES = 64, 232
TOP_MAX_K = 4096                             # SW_TOP_MAX_K: the largest k of the top-hits calls
HIT_NONE = 0xFFFFFFFFFFFFFFFF                # SW_HIT_NONE: a hit slot past the row's count
QUERY_NONE = 0xFFFFFFFF                      # SW_QUERY_NONE: "no query" in a hit-query list
INT32_MIN = -(1 << 31)                       # min_score: no threshold; the score of such a slot
STAT_BINS = 4096                             # SW_STAT_BINS: score bins of a histogram row
STAT_DEGENERATE, STAT_CLAMPED = 1, 2         # sw_statistics.flags


class SwbankError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"swbank status {status}: {msg}")
        self.status = status


class DeviceBatch(ctypes.Structure):
    """sw_device_batch (ABI 6): one device's resident batch for sw_score_batch_device_multi."""
    _fields_ = [("d_residues", ctypes.c_void_p), ("d_offsets", ctypes.c_void_p),
                ("d_lens", ctypes.c_void_p), ("n", ctypes.c_size_t),
                ("min_len", ctypes.c_uint32), ("max_len", ctypes.c_uint32),
                ("d_scores", ctypes.c_void_p), ("stream", ctypes.c_void_p)]


class AlignmentRecord(ctypes.Structure):
    """sw_alignment: one hit's record as the C ABI writes it (56 bytes)."""
    _fields_ = [("index", ctypes.c_uint64), ("id", ctypes.c_uint64), ("score", ctypes.c_int32),
                ("flags", ctypes.c_uint32), ("q_start", ctypes.c_uint32),
                ("q_end", ctypes.c_uint32), ("t_start", ctypes.c_uint32),
                ("t_end", ctypes.c_uint32), ("n_columns", ctypes.c_uint32),
                ("n_identities", ctypes.c_uint32), ("cigar_offset", ctypes.c_uint32),
                ("cigar_len", ctypes.c_uint32)]


class Statistics(ctypes.Structure):
    """sw_statistics: lambda and K of one query's shuffled-library fit (48 bytes)."""
    _fields_ = [("lambda_", ctypes.c_double), ("K", ctypes.c_double),
                ("n_samples", ctypes.c_uint64), ("n_clamped", ctypes.c_uint64),
                ("query_len", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("min_score", ctypes.c_int32), ("max_score", ctypes.c_int32)]

    @property
    def degenerate(self) -> bool:
        return bool(self.flags & STAT_DEGENERATE)

    @property
    def clamped(self) -> bool:
        return bool(self.flags & STAT_CLAMPED)

    def __repr__(self):
        return (f"Statistics(lambda_={self.lambda_!r}, K={self.K!r}, n_samples={self.n_samples}, "
                f"n_clamped={self.n_clamped}, query_len={self.query_len}, flags={self.flags}, "
                f"min_score={self.min_score}, max_score={self.max_score})")


ALIGNMENT_DTYPE = np.dtype([(n, np.dtype(t)) for n, t in AlignmentRecord._fields_])


@dataclasses.dataclass
class Alignment:
    """One aligned hit (sw_alignment with its ops): coordinates 0-based and inclusive; `ops`
    the CIGAR as len << 4 | code, `cigar` its text (empty without a path)."""
    index: int
    id: int
    score: int
    flags: int
    q_start: int
    q_end: int
    t_start: int
    t_end: int
    n_columns: int
    n_identities: int
    ops: Tuple[int, ...] = ()
    cigar: str = ""

    @property
    def empty(self) -> bool:
        return bool(self.flags & ALIGN_EMPTY)

    @property
    def has_path(self) -> bool:
        return self.flags & ~_ALIGN_WHERE == 0

    @property
    def reverse(self) -> bool:
        """The hit lies on the reverse strand (ALIGN_REVERSE): aligned against the reverse
        complement of its target, t_start / t_end given on the forward target."""
        return bool(self.flags & ALIGN_REVERSE)

    @property
    def frame(self) -> int:
        """The reading frame 0..5 of a translated hit (align_frame_hits): frames 0..2 forward,
        3..5 those of the reverse complement; t_start / t_end are nucleotide positions."""
        return ((self.flags & ALIGN_FRAME_MASK) >> ALIGN_FRAME_SHIFT) + (3 if self.reverse else 0)


def cigar_string(ops) -> str:
    """CIGAR ops (len << 4 | code) -> text, e.g. "15M2I17M4D13M" (sw_cigar_string)."""
    a = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1)
    need = lib().sw_cigar_string(_p(a) if a.size else None, a.size, None, 0)
    buf = ctypes.create_string_buffer(need + 1)
    lib().sw_cigar_string(_p(a) if a.size else None, a.size, buf, need + 1)
    return buf.value.decode()


def alignments_from(records: np.ndarray, cigar: np.ndarray) -> list:
    """Alignment objects from an ALIGNMENT_DTYPE array and the op buffer its offsets index."""
    out = []
    for r in records:
        ops = ()
        if int(r["flags"]) & ~_ALIGN_WHERE == 0:
            ops = tuple(int(x) for x in cigar[int(r["cigar_offset"]):
                                              int(r["cigar_offset"]) + int(r["cigar_len"])])
        out.append(Alignment(int(r["index"]), int(r["id"]), int(r["score"]), int(r["flags"]),
                             int(r["q_start"]), int(r["q_end"]), int(r["t_start"]),
                             int(r["t_end"]), int(r["n_columns"]), int(r["n_identities"]), ops,
                             cigar_string(ops) if ops else ""))
    return out


class _Config(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("alphabet", ctypes.c_int32),
                ("gap_model", ctypes.c_int32), ("max_query_len", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("n_devices", ctypes.c_int32),
                ("devices", ctypes.c_int32 * 16)]


_LIB: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    """Load libswbank.so (raises if it has not been built)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise SwbankError(ERR_UNSUPPORTED, f"{LIB_PATH} not built (run make in {_PKG})")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (same SONAME). If
    # torch is imported first, libswbank binds to that copy, so torch tensors and streams can
    # be handed across the ABI; loading /opt/rocm's copy first would leave torch unable to
    # initialise its own.  So import torch (when present) before dlopen-ing the library.
    if os.environ.get("SWBANK_STANDALONE_HIP") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = ctypes.CDLL(LIB_PATH)
    if L.sw_abi_version() != ABI_VERSION:
        raise SwbankError(ERR_UNSUPPORTED, f"{LIB_PATH}: ABI {L.sw_abi_version()}, want {ABI_VERSION}")
    P, i32, u32, u64, sz = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64,
                            ctypes.c_size_t)
    sig = {
        "sw_abi_version": (i32, []),
        "sw_status_string": (ctypes.c_char_p, [i32]),
        "sw_device_count": (i32, []),
        "sw_max_query_len": (u32, []),
        "sw_config_default": (i32, [P]),
        "sw_bank_create": (i32, [ctypes.POINTER(P), P]),
        "sw_bank_destroy": (None, [P]),
        "sw_last_error": (ctypes.c_char_p, [P]),
        "sw_set_penalties": (i32, [P, i32, i32, i32, i32]),
        "sw_set_matrix": (i32, [P, P, i32, i32, i32]),
        "sw_load_query": (i32, [P, u64, P, u32]),
        "sw_score_batch": (i32, [P, P, sz, P, P, P, sz, P]),
        "sw_score_batch_device": (i32, [P, P, P, P, P, sz, u32, P, P]),
        "sw_score_batch_device_range": (i32, [P, P, P, P, P, sz, u32, u32, P, P]),
        "sw_bank_counters": (i32, [P, P]),
        "sw_bank_counters_ex": (i32, [P, P, sz]),
        "sw_bank_sync": (i32, [P]),
        "sw_batch_best": (i32, [P, P, P, P]),
        "sw_bank_devices": (i32, [P, P, i32]),
        "sw_best_hit": (i32, [P, P, P, sz, P, P]),
        "sw_encode_ascii": (sz, [i32, ctypes.c_char_p, sz, P]),
        "sw_pack_2bit": (sz, [ctypes.c_char_p, sz, P]),
        "sw_unpack_2bit": (sz, [P, sz, P]),
        "sw_fill_matrix": (i32, [i32, i32, i32, P]),
        "sw_bank_set_timing": (i32, [P, i32]),
        "sw_bank_timing": (i32, [P, P, P, P]),
        "sw_last_kernel": (ctypes.c_char_p, [P]),
        "sw_load_query_record": (i32, [P, P]),
        "sw_score_records": (i32, [P, P, sz, P]),
        "sw_score_records_device": (i32, [P, P, sz, P, P]),
        "sw_best_hit_device": (i32, [P, P, P, sz, P, P]),
        "sw_load_queries": (i32, [P, sz, P, P, P, P]),
        "sw_query_count": (sz, [P]),
        "sw_score_batch_device_multi": (i32, [P, P, sz, P, P]),
        "sw_align_hits": (i32, [P, P, sz, P, P, P, sz, P, sz, P, P, sz, P]),
        "sw_align_hits_device": (i32, [P, P, P, P, P, sz, u32, P, sz, P, P, u32, P]),
        "sw_cigar_string": (sz, [P, sz, P, sz]),
        "sw_top_hits": (i32, [P, P, P, sz, sz, sz, i32, P, P, P, P]),
        "sw_top_hits_device": (i32, [P, P, P, sz, sz, sz, i32, P, P, P, P, P]),
        "sw_best_queries": (i32, [P, P, sz, sz, i32, P, P]),
        "sw_best_queries_device": (i32, [P, P, sz, sz, i32, P, P, P]),
        "sw_align_set_hits": (i32, [P, P, sz, P, P, P, sz, P, sz, P, sz, P, P, sz, P]),
        "sw_align_set_hits_device": (i32, [P, P, P, P, P, sz, u32, P, sz, P, sz, P, P, u32, P]),
        "sw_shuffle_batch_device": (i32, [P, P, P, P, sz, u32, u64, P, P]),
        "sw_score_histogram_device": (i32, [P, P, P, sz, sz, P, P, P, P]),
        "sw_fit_statistics": (i32, [P, P, u32, P]),
        "sw_estimate_statistics_device": (i32, [P, P, P, P, sz, u32, u32, u64, u32, P, P]),
        "sw_estimate_statistics": (i32, [P, P, sz, P, P, sz, u64, u32, P]),
        "sw_hit_significance": (i32, [P, P, P, sz, u64, P, P]),
        "sw_hit_significance_device": (i32, [P, P, P, P, P, sz, sz, u64, P, P, P]),
        "sw_revcomp_codes": (sz, [P, sz, P]),
        "sw_revcomp_batch_device": (i32, [P, P, P, P, sz, P, P]),
        "sw_score_strands": (i32, [P, P, sz, P, P, sz, P, P]),
        "sw_score_strands_device": (i32, [P, P, P, P, P, sz, u32, u32, P, P, P]),
        "sw_align_strand_hits": (i32, [P, P, sz, P, P, P, sz, P, P, sz, P, sz, P, P, sz, P]),
        "sw_align_strand_hits_device": (i32, [P, P, P, P, P, sz, u32, P, P, sz, P, sz, P, P, u32,
                                              P]),
        "sw_translate_codes": (sz, [P, sz, u32, P, P]),
        "sw_translate_batch_device": (i32, [P, P, P, P, sz, u32, P, P, sz, P, P, P]),
        "sw_score_frames": (i32, [P, P, sz, P, P, sz, P, P, P]),
        "sw_score_frames_device": (i32, [P, P, P, P, sz, u32, u32, P, P, P, P]),
        "sw_align_frame_hits": (i32, [P, P, sz, P, P, P, sz, P, P, P, sz, P, sz, P, P, sz, P]),
        "sw_align_frame_hits_device": (i32, [P, P, P, P, P, sz, u32, P, P, P, sz, P, sz, P, P, u32,
                                             P]),
        "sw_score_fshift": (i32, [P, P, sz, P, P, sz, P, i32, P, P]),
        "sw_score_fshift_device": (i32, [P, P, P, P, sz, u32, P, i32, P, P, P]),
        "sw_score_glocal": (i32, [P, P, sz, P, P, sz, i32, i32, P, P, P]),
        "sw_score_glocal_device": (i32, [P, P, P, P, sz, u32, i32, i32, P, P, P, P]),
        "sw_align_glocal_hits": (i32, [P, P, sz, P, P, P, sz, i32, i32, P, sz, P, sz, P, P, sz, P]),
        "sw_align_glocal_hits_device": (i32, [P, P, P, P, P, sz, u32, i32, i32, P, sz, P, sz, P, P,
                                              u32, P]),
        "sw_align_disjoint_hits": (i32, [P, P, sz, P, P, P, sz, u32, i32, P, sz, P, sz, P, P, sz,
                                         P]),
        "sw_align_disjoint_hits_device": (i32, [P, P, P, P, P, sz, u32, u32, i32, P, sz, P, sz, P,
                                                P, u32, P]),
        "sw_align_disjoint_frame_hits": (i32, [P, P, sz, P, P, P, sz, P, u32, i32, P, sz, P, sz, P,
                                               P, sz, P]),
        "sw_align_disjoint_frame_hits_device": (i32, [P, P, P, P, P, sz, u32, P, u32, i32, P, sz,
                                                      P, sz, P, P, u32, P]),
        "sw_align_fshift_hits": (i32, [P, P, sz, P, P, P, sz, P, i32, P, sz, P, sz, P, P, sz, P]),
        "sw_align_fshift_hits_device": (i32, [P, P, P, P, P, sz, u32, P, i32, P, sz, P, sz, P, P,
                                              u32, P]),
        "sw_estimate_fshift_statistics": (i32, [P, P, sz, P, P, sz, P, i32, u64, u32, P]),
        "sw_estimate_fshift_statistics_device": (i32, [P, P, P, P, sz, u32, P, i32, u64, u32, P,
                                                       P]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = L
    return L


def _p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def status_string(st: int) -> str:
    return lib().sw_status_string(st).decode()


def device_count() -> int:
    return int(lib().sw_device_count())


# ---- host helpers (no device) --------------------------------------------------------------
def encode(seq: str | bytes, alphabet: int = ALPHABET_DNA) -> np.ndarray:
    """ASCII -> codes (sw_encode_ascii; ConvertToBase for DNA)."""
    b = seq.encode() if isinstance(seq, str) else bytes(seq)
    out = np.zeros(max(len(b), 1), dtype=np.uint8)
    lib().sw_encode_ascii(alphabet, b, len(b), _p(out))
    return out[:len(b)]


def pack_2bit(seq: str | bytes) -> np.ndarray:
    """charTo2bit packing (sw_pack_2bit)."""
    b = seq.encode() if isinstance(seq, str) else bytes(seq)
    out = np.zeros(max((len(b) + 3) // 4, 1), dtype=np.uint8)
    lib().sw_pack_2bit(b, len(b), _p(out))
    return out[:(len(b) + 3) // 4]


def unpack_2bit(packed: np.ndarray, n: int) -> np.ndarray:
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    out = np.zeros(max(n, 1), dtype=np.uint8)
    lib().sw_unpack_2bit(_p(packed), n, _p(out))
    return out[:n]


def make_records(seqs: Sequence[np.ndarray], ids: Optional[Sequence[int]] = None) -> np.ndarray:
    """DNA code arrays (0..3) -> CAPI `sequence_t` records, one 64-byte row each
    (aligner_Header.h:19-24: u32 ID, u16 length, 58 bytes of 2-bit codes LSB-first)."""
    out = np.zeros((len(seqs), RECORD_BYTES), dtype=np.uint8)
    if isinstance(seqs, np.ndarray) and seqs.ndim == 2:  # equal lengths: vectorised
        n, L = seqs.shape
        if L > RECORD_MAX_BASES or (seqs.size and seqs.max() > 3):
            raise ValueError(f"records need <= {RECORD_MAX_BASES} ACGT codes")
        idv = np.arange(n, dtype=np.uint32) if ids is None else np.asarray(ids, np.uint32)
        out[:, 0:4] = idv.view(np.uint8).reshape(n, 4)
        out[:, 4:6] = np.full(n, L, np.uint16).view(np.uint8).reshape(n, 2)
        q = np.zeros((n, (L + 3) // 4 * 4), dtype=np.uint8)
        q[:, :L] = seqs
        q = q.reshape(n, -1, 4)
        out[:, 6:6 + q.shape[1]] = q[..., 0] | q[..., 1] << 2 | q[..., 2] << 4 | q[..., 3] << 6
        return out
    for k, sq in enumerate(seqs):
        c = np.asarray(sq, dtype=np.uint8)
        if len(c) > RECORD_MAX_BASES or (len(c) and c.max() > 3):
            raise ValueError(f"record {k}: needs <= {RECORD_MAX_BASES} ACGT codes")
        out[k, 0:4] = np.frombuffer(np.uint32(k if ids is None else ids[k]).tobytes(), np.uint8)
        out[k, 4:6] = np.frombuffer(np.uint16(len(c)).tobytes(), np.uint8)
        q = np.zeros((len(c) + 3) // 4 * 4, dtype=np.uint8)
        q[:len(c)] = c
        q = q.reshape(-1, 4)
        out[k, 6:6 + len(q)] = q[:, 0] | q[:, 1] << 2 | q[:, 2] << 4 | q[:, 3] << 6
    return out


def revcomp(codes) -> np.ndarray:
    """sw_revcomp_codes: the reverse complement of DNA codes (T <-> A, C <-> G; N stays N)."""
    a = np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1)
    out = np.empty(a.size, dtype=np.uint8)
    if a.size:
        lib().sw_revcomp_codes(_p(a), a.size, _p(out))
    return out


def _codon_table(table) -> Optional[np.ndarray]:
    """A caller's genetic code as the 64 protein codes the C ABI takes (None: the standard
    code): 64 letters of ARNDCQEGHILKMFPSTWYVBZX*, or 64 codes."""
    if table is None:
        return None
    t = encode(table, ALPHABET_PROTEIN) if isinstance(table, (str, bytes)) else \
        np.ascontiguousarray(table, dtype=np.uint8).reshape(-1)
    if t.size != 64:
        raise ValueError("a codon table has 64 entries")
    return t


def translate_codes(codes, frame: int, codon_table=None) -> np.ndarray:
    """sw_translate_codes: the protein codes of reading frame `frame` (0..2 forward, 3..5 those
    of the reverse complement) of DNA codes; a codon holding N is X, a stop is *."""
    a = np.ascontiguousarray(codes, dtype=np.uint8).reshape(-1)
    tab = _codon_table(codon_table)
    if not 0 <= frame < FRAME_COUNT or (tab is not None and tab.max() >= PROTEIN_ALPHA):
        raise ValueError("frame 0..5 and a table of protein codes")
    out = np.empty(max(a.size // 3, 1), dtype=np.uint8)
    n = lib().sw_translate_codes(_p(a), a.size, frame, _p(tab) if tab is not None else None,
                                 _p(out)) if a.size else 0
    return out[:n]


def fill_matrix(alphabet: int, match: int = 5, mismatch: int = -4) -> np.ndarray:
    a = DNA_ALPHA if alphabet == ALPHABET_DNA else PROTEIN_ALPHA
    m = np.zeros((a, a), dtype=np.int8)
    st = lib().sw_fill_matrix(alphabet, match, mismatch, _p(m))
    if st != OK:
        raise SwbankError(st, status_string(st))
    return m


def pack_targets(seqs: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Concatenate code arrays -> (residues, offsets u64, lens u32)."""
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    offs = np.zeros(len(seqs), dtype=np.uint64)
    if len(seqs) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    res = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs]) if len(seqs) else None
    if res is None or res.size == 0:
        res = np.zeros(1, dtype=np.uint8)
    return res, offs, lens


def validate_batch(residues, offsets, lens, ids=None):
    """Host batch -> contiguous (residues u8, offsets u64, lens u32, ids u64 | None), or
    ValueError when the arrays disagree: the C feeder reads offsets[k], lens[k] (and ids[k])
    for every k < len(lens), so a short array would be a host over-read inside the library
    rather than a Python error.  Each target's range against the residues is checked by the
    library itself (sw_score_batch takes the residue count; SW_ERR_ARG, nothing read past it),
    inside the feeder pass that reads the offsets anyway."""
    res = np.ascontiguousarray(residues, dtype=np.uint8).reshape(-1)
    ln = np.ascontiguousarray(lens, dtype=np.uint32).reshape(-1)
    off_in = np.asarray(offsets).reshape(-1)
    if off_in.size != ln.size:
        raise ValueError(f"{off_in.size} offsets for {ln.size} lengths")
    if off_in.size and np.issubdtype(off_in.dtype, np.signedinteger) and off_in.min() < 0:
        raise ValueError("negative offset")
    offs = np.ascontiguousarray(off_in, dtype=np.uint64)
    idv = None
    if ids is not None:
        idv = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        if idv.size != ln.size:
            raise ValueError(f"{idv.size} ids for {ln.size} targets")
    return res, offs, ln, idv


# ---- hit statistics on the host (no device) -----------------------------------------------
def fit_statistics(counts, len_sums, query_len: int) -> Statistics:
    """sw_fit_statistics: the maximum-likelihood lambda and K of one histogram row (STAT_BINS
    counts and length sums, as score_histogram_device writes them)."""
    c = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    ls = np.ascontiguousarray(len_sums, dtype=np.uint64).reshape(-1)
    if c.size != STAT_BINS or ls.size != STAT_BINS:
        raise ValueError(f"a histogram row holds {STAT_BINS} bins")
    out = Statistics()
    st = lib().sw_fit_statistics(_p(c), _p(ls), query_len, ctypes.byref(out))
    if st != OK:
        raise SwbankError(st, status_string(st))
    return out


def make_statistics(lambda_: float, K: float, query_len: int) -> Statistics:
    """Given statistics (e.g. the Lambda and K another tool printed) for hit_significance."""
    return Statistics(lambda_=lambda_, K=K, query_len=query_len)


def hit_significance(stats: Statistics, scores, target_lens, db_size: int):
    """sw_hit_significance: (bits float64 [n], evalues float64 [n]) of hits with the given
    scores and target lengths in a library of db_size sequences."""
    sc = np.ascontiguousarray(scores, dtype=np.int32).reshape(-1)
    tl = np.ascontiguousarray(target_lens, dtype=np.uint32).reshape(-1)
    if sc.size != tl.size:
        raise ValueError(f"{sc.size} scores for {tl.size} target lengths")
    bits = np.empty(max(sc.size, 1), np.float64)
    ev = np.empty(max(sc.size, 1), np.float64)
    st = lib().sw_hit_significance(ctypes.byref(stats), _p(sc) if sc.size else _p(bits),
                                   _p(tl) if tl.size else _p(bits), sc.size, db_size, _p(bits),
                                   _p(ev))
    if st != OK:
        raise SwbankError(st, status_string(st))
    return bits[:sc.size], ev[:sc.size]


# ---- the bank ----------------------------------------------------------------------------
class ScoreBank:
    """One ScoreBank_v2 instance (sw_bank_create): on one GPU, or with ``devices=[...]`` a
    multi-device bank that deals every host batch over those GPUs (the RTL's MODULES,
    ScoreBank_v2.v:76-148) and gathers the scores back with RCCL."""

    def __init__(self, device: int = -1, alphabet: int = ALPHABET_DNA,
                 gap_model: int = GAP_MERGED, max_query_len: int = 0,
                 devices: Optional[Sequence[int]] = None):
        L = lib()
        cfg = _Config()
        L.sw_config_default(ctypes.byref(cfg))
        cfg.device, cfg.alphabet, cfg.gap_model, cfg.max_query_len = (
            device, alphabet, gap_model, max_query_len)
        if devices is not None:
            devices = list(devices)
            if not 1 <= len(devices) <= MAX_DEVICES:
                raise ValueError(f"devices: 1..{MAX_DEVICES} ordinals")
            cfg.n_devices = len(devices)
            for i, d in enumerate(devices):
                cfg.devices[i] = d
        h = ctypes.c_void_p()
        st = L.sw_bank_create(ctypes.byref(h), ctypes.byref(cfg))
        if st != OK:
            raise SwbankError(st, status_string(st))
        self._h = h
        self.alphabet = alphabet
        self.gap_model = gap_model

    # errors
    def _check(self, st: int):
        if st != OK:
            raise SwbankError(st, f"{status_string(st)}: {lib().sw_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None):
            lib().sw_bank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ld_penalties
    def set_penalties(self, match: int, mismatch: int, gap_open: int, gap_extend: int):
        self._check(lib().sw_set_penalties(self._h, match, mismatch, gap_open, gap_extend))

    def set_matrix(self, matrix: np.ndarray, gap_open: int, gap_extend: int):
        m = np.ascontiguousarray(matrix, dtype=np.int8)
        self._check(lib().sw_set_matrix(self._h, _p(m), m.shape[0], gap_open, gap_extend))

    # ld_sequence (query)
    def load_query(self, codes: np.ndarray, qid: int = 0):
        c = np.ascontiguousarray(codes, dtype=np.uint8)
        buf = c if c.size else np.zeros(1, np.uint8)
        self._check(lib().sw_load_query(self._h, qid, _p(buf), len(c)))

    def load_queries(self, queries, ids=None):
        """A query set (sw_load_queries): every following score_batch_device call scores the
        batch against each query, scores query-major (len(queries) x n)."""
        qs = [np.ascontiguousarray(q, dtype=np.uint8) for q in queries]
        if not qs:
            raise ValueError("an empty query set")
        codes, offs, lens = pack_targets(qs)
        idv = None
        if ids is not None:
            idv = np.ascontiguousarray(ids, dtype=np.uint64)
            if idv.size != len(qs):
                raise ValueError(f"{idv.size} ids for {len(qs)} queries")
        buf = codes if codes.size else np.zeros(1, np.uint8)
        self._check(lib().sw_load_queries(self._h, len(qs), None if idv is None else _p(idv),
                                          _p(buf), _p(offs), _p(lens)))

    def query_count(self) -> int:
        return int(lib().sw_query_count(self._h))

    # target stream
    def score_batch(self, residues: np.ndarray, offsets: np.ndarray, lens: np.ndarray,
                    ids: Optional[np.ndarray] = None,
                    out: Optional[np.ndarray] = None) -> np.ndarray:
        """Scores of targets residues[offsets[k] : offsets[k] + lens[k]] in input order; ids
        (optional, one per target) tag the batch best hit (best()); out (optional, int32,
        contiguous, one per target) is filled and returned instead of a new array."""
        res, offs, ln, idv = validate_batch(residues, offsets, lens, ids)
        if out is None:
            out = np.empty(len(ln), dtype=np.int32)  # every entry written by the library
        elif (out.dtype != np.int32 or out.shape != (len(ln),)
              or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]):
            raise ValueError("out: a writable contiguous int32 array with one entry per target")
        if len(ln) == 0:
            return out
        self._check(lib().sw_score_batch(self._h, _p(res), res.size, _p(offs), _p(ln),
                                         _p(idv) if idv is not None else None, len(ln), _p(out)))
        return out

    def best(self) -> Tuple[int, int, int]:
        """Best hit of the last batch call (sw_batch_best, ≙ max / vld_max):
        (id, score, index) — lowest index among equal maxima."""
        bid, bsc, bix = ctypes.c_uint64(), ctypes.c_int32(), ctypes.c_uint64()
        self._check(lib().sw_batch_best(self._h, ctypes.byref(bid), ctypes.byref(bsc),
                                        ctypes.byref(bix)))
        return int(bid.value), int(bsc.value), int(bix.value)

    def devices(self) -> list:
        arr = (ctypes.c_int32 * MAX_DEVICES)()
        n = lib().sw_bank_devices(self._h, arr, MAX_DEVICES)
        return [int(arr[i]) for i in range(n)]

    def score_targets(self, seqs: Iterable[np.ndarray]) -> np.ndarray:
        return self.score_batch(*pack_targets(list(seqs)))

    def score_batch_device(self, d_res: int, d_offs: int, d_lens: int, n: int, max_len: int,
                           d_scores: int, stream: int = 0, d_ids: int = 0,
                           min_len: Optional[int] = None):
        """Device pointers (ints, e.g. torch.Tensor.data_ptr()); async on `stream`.  With d_ids
        the call also records the batch best hit on the device (best()).  With min_len (every
        length in [min_len, max_len]) the call is sw_score_batch_device_range: a range of one
        length skips the on-device length sort.  stream 0 is the BANK's own non-blocking stream
        (the C ABI's NULL), not HIP's default stream; torch's default current stream has handle
        0 on ROCm, so pass a torch.cuda.Stream's cuda_stream (or sync()) before torch reads the
        scores."""
        if min_len is None:
            self._check(lib().sw_score_batch_device(self._h, d_res, d_offs, d_lens,
                                                    d_ids or None, n, max_len, d_scores,
                                                    stream or None))
        else:
            self._check(lib().sw_score_batch_device_range(self._h, d_res, d_offs, d_lens,
                                                          d_ids or None, n, min_len, max_len,
                                                          d_scores, stream or None))

    def score_batch_device_multi(self, batches, d_gathered: int = 0, stream: int = 0):
        """sw_score_batch_device_multi (ABI 6): batches[d] = dict(d_res, d_offs, d_lens, n,
        max_len, min_len=0, d_scores=0, stream=0) resident on the bank's d-th device; each device
        scores its own batch in place, the int32 scores are gathered to the root into d_gathered
        (query-major over the concatenated batch) and/or left in each d_scores.  Async."""
        arr = (DeviceBatch * len(batches))()
        for i, bt in enumerate(batches):
            arr[i] = DeviceBatch(bt["d_res"] or None, bt["d_offs"] or None, bt["d_lens"] or None,
                                 bt["n"], bt.get("min_len", 0), bt["max_len"],
                                 bt.get("d_scores", 0) or None, bt.get("stream", 0) or None)
        self._check(lib().sw_score_batch_device_multi(self._h, arr, len(batches),
                                                      d_gathered or None, stream or None))

    # alignments of chosen hits
    def align_hits(self, residues: np.ndarray, offsets: np.ndarray, lens: np.ndarray, hits,
                   ids: Optional[np.ndarray] = None, cigar_cap: Optional[int] = None) -> list:
        """sw_align_hits: Alignment objects for targets hits[0..) (batch positions, any order,
        repeats allowed) of the host batch.  cigar_cap: ops the call may return in all (default:
        enough for every path; 0: coordinates only, every non-empty hit ALIGN_NO_PATH)."""
        res, offs, ln, idv = validate_batch(residues, offsets, lens, ids)
        hv = np.ascontiguousarray(hits, dtype=np.uint64).reshape(-1)
        out = np.zeros(max(len(hv), 1), dtype=ALIGNMENT_DTYPE)
        if cigar_cap is None:  # runs alternate with M runs: at most 2 x columns + 1 ops a path
            sel = hv[hv < len(ln)].astype(np.int64)
            cigar_cap = 2 * int(ln[sel].astype(np.int64).sum()) + len(hv)
        cig = np.zeros(max(cigar_cap, 1), dtype=np.uint32)
        used = ctypes.c_size_t()
        self._check(lib().sw_align_hits(self._h, _p(res), res.size, _p(offs), _p(ln),
                                        _p(idv) if idv is not None else None, len(ln), _p(hv),
                                        len(hv), _p(out), _p(cig) if cigar_cap else None,
                                        cigar_cap, ctypes.byref(used)))
        return alignments_from(out[:len(hv)], cig)

    def align_targets(self, seqs: Iterable[np.ndarray], hits) -> list:
        return self.align_hits(*pack_targets(list(seqs)), hits)

    def align_hits_device(self, d_res: int, d_offs: int, d_lens: int, n: int, max_len: int,
                          d_hits: int, n_hits: int, d_out: int, d_cigar: int = 0,
                          cigar_stride: int = 0, stream: int = 0, d_ids: int = 0):
        """sw_align_hits_device: device pointers (ints); d_out receives n_hits sw_alignment
        records (ALIGNMENT_DTYPE, 56 bytes each), hit h's ops go to d_cigar + h * cigar_stride.
        Async on `stream` (0: the bank's own stream; sync() before reading)."""
        self._check(lib().sw_align_hits_device(self._h, d_res or None, d_offs or None,
                                               d_lens or None, d_ids or None, n, max_len,
                                               d_hits or None, n_hits, d_out or None,
                                               d_cigar or None, cigar_stride, stream or None))

    # alignments of chosen hits against a query set
    def align_set_hits(self, residues: np.ndarray, offsets: np.ndarray, lens: np.ndarray,
                       hits=None, hit_queries=None, hits_per_query: int = 0,
                       ids: Optional[np.ndarray] = None, cigar_cap: Optional[int] = None,
                       n_hits: Optional[int] = None) -> list:
        """sw_align_set_hits: Alignment objects for the pairs of the loaded query set.  Hit h is
        query hit_queries[h] (or h // hits_per_query, the [nq, k] layout of top_hits) against
        target hits[h] (or target h when hits is None; n_hits then defaults to the number of
        hit_queries, or of targets).  A hit whose query is QUERY_NONE or whose target is HIT_NONE
        names no pair: index = id = HIT_NONE, flags ALIGN_EMPTY | ALIGN_NO_HIT.  cigar_cap as
        for align_hits."""
        res, offs, ln, idv = validate_batch(residues, offsets, lens, ids)
        hv = None if hits is None else np.ascontiguousarray(hits, dtype=np.uint64).reshape(-1)
        hq = None if hit_queries is None else \
            np.ascontiguousarray(hit_queries, dtype=np.uint32).reshape(-1)
        if n_hits is None:
            n_hits = len(hv) if hv is not None else len(hq) if hq is not None else len(ln)
        if (hv is not None and len(hv) < n_hits) or (hq is not None and len(hq) < n_hits):
            raise ValueError("hits / hit_queries shorter than n_hits")
        out = np.zeros(max(n_hits, 1), dtype=ALIGNMENT_DTYPE)
        if cigar_cap is None:  # runs alternate with M runs: at most 2 x columns + 1 ops a path
            tv = hv[:n_hits] if hv is not None else np.arange(min(n_hits, len(ln)), dtype=np.uint64)
            sel = tv[tv < len(ln)].astype(np.int64)
            cigar_cap = 2 * int(ln[sel].astype(np.int64).sum()) + n_hits
        cig = np.zeros(max(cigar_cap, 1), dtype=np.uint32)
        used = ctypes.c_size_t()
        self._check(lib().sw_align_set_hits(
            self._h, _p(res), res.size, _p(offs), _p(ln), _p(idv) if idv is not None else None,
            len(ln), _p(hq) if hq is not None else None, hits_per_query,
            _p(hv) if hv is not None else None, n_hits, _p(out), _p(cig) if cigar_cap else None,
            cigar_cap, ctypes.byref(used)))
        return alignments_from(out[:n_hits], cig)

    def align_set_hits_device(self, d_res: int, d_offs: int, d_lens: int, n: int, max_len: int,
                              n_hits: int, d_out: int, d_hits: int = 0, d_hit_queries: int = 0,
                              hits_per_query: int = 0, d_cigar: int = 0, cigar_stride: int = 0,
                              stream: int = 0, d_ids: int = 0):
        """sw_align_set_hits_device: device pointers (ints).  Hit h's query is d_hit_queries[h]
        (uint32) or h // hits_per_query, its target d_hits[h] (uint64) or h when d_hits is 0;
        d_out, d_cigar and cigar_stride as for align_hits_device.  Async on `stream` (0: the
        bank's own stream; sync() before reading)."""
        self._check(lib().sw_align_set_hits_device(
            self._h, d_res or None, d_offs or None, d_lens or None, d_ids or None, n, max_len,
            d_hit_queries or None, hits_per_query, d_hits or None, n_hits, d_out or None,
            d_cigar or None, cigar_stride, stream or None))

    # the best query of every target
    def best_queries(self, scores: np.ndarray, min_score: Optional[int] = None,
                     want_query: bool = True, want_score: bool = True):
        """sw_best_queries: for every column of `scores` [nq, n] the lowest query with the
        column's maximum and that maximum, (best_query uint32 [n], best_score int32 [n]);
        QUERY_NONE / INT32_MIN where the maximum is < min_score (None: no threshold).  An output
        not wanted is None."""
        s = np.ascontiguousarray(scores, dtype=np.int32)
        if s.ndim != 2:
            raise ValueError("scores: 2-D [nq, n]")
        nq, n = s.shape
        bq = np.empty(max(n, 1), np.uint32) if want_query else None
        bs = np.empty(max(n, 1), np.int32) if want_score else None
        self._check(lib().sw_best_queries(self._h, _p(s), n, nq,
                                          INT32_MIN if min_score is None else min_score,
                                          _p(bq) if bq is not None else None,
                                          _p(bs) if bs is not None else None))
        return (bq[:n] if bq is not None else None, bs[:n] if bs is not None else None)

    def best_queries_device(self, d_scores: int, n: int, nq: int, d_best_query: int = 0,
                            d_best_score: int = 0, min_score: Optional[int] = None,
                            stream: int = 0):
        """sw_best_queries_device: device pointers (ints); d_scores holds nq rows of n int32
        scores, d_best_query (uint32) and d_best_score (int32) receive n entries each (either
        may be 0).  Async on `stream` (0: the bank's own stream; sync() before reading)."""
        self._check(lib().sw_best_queries_device(self._h, d_scores or None, n, nq,
                                                 INT32_MIN if min_score is None else min_score,
                                                 d_best_query or None, d_best_score or None,
                                                 stream or None))

    # the k best hits of a score matrix
    def top_hits(self, scores: np.ndarray, k: int, ids: Optional[np.ndarray] = None,
                 min_score: Optional[int] = None):
        """sw_top_hits: the k best of every row of `scores` (1-D: one row; 2-D [nq, n]), score
        descending, then batch position ascending, among the scores >= min_score (None: all).
        Returns (hits uint64, hit_scores int32, hit_ids uint64, counts uint32): [k] and a scalar
        count for 1-D scores, [nq, k] and [nq] for 2-D; slots past a row's count hold HIT_NONE /
        INT32_MIN / HIT_NONE."""
        s = np.ascontiguousarray(scores, dtype=np.int32)
        if s.ndim not in (1, 2):
            raise ValueError("scores: 1-D, or 2-D [nq, n]")
        rows = s.reshape(1, -1) if s.ndim == 1 else s
        nq, n = rows.shape
        idv = None
        if ids is not None:
            idv = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
            if idv.size != n:
                raise ValueError(f"{idv.size} ids for {n} targets")
        kk = max(int(k), 1)
        hits = np.empty((nq, kk), np.uint64)
        hsc = np.empty((nq, kk), np.int32)
        hid = np.empty((nq, kk), np.uint64)
        cnt = np.empty(nq, np.uint32)
        self._check(lib().sw_top_hits(self._h, _p(rows), _p(idv) if idv is not None else None, n,
                                      nq, k, INT32_MIN if min_score is None else min_score,
                                      _p(hits), _p(hsc), _p(hid), _p(cnt)))
        if s.ndim == 1:
            return hits[0], hsc[0], hid[0], cnt[0]
        return hits, hsc, hid, cnt

    def top_hits_device(self, d_scores: int, n: int, k: int, d_hits: int, nq: int = 1,
                        d_ids: int = 0, min_score: Optional[int] = None, d_hit_scores: int = 0,
                        d_hit_ids: int = 0, d_counts: int = 0, stream: int = 0):
        """sw_top_hits_device: device pointers (ints); d_scores holds nq rows of n int32 scores,
        d_hits receives nq x k uint64 batch positions (the hit list align_hits_device takes),
        d_hit_scores / d_hit_ids / d_counts (optional) nq x k int32, nq x k uint64, nq uint32.
        Async on `stream` (0: the bank's own stream; sync() before reading)."""
        self._check(lib().sw_top_hits_device(self._h, d_scores or None, d_ids or None, n, nq, k,
                                             INT32_MIN if min_score is None else min_score,
                                             d_hits or None, d_hit_scores or None,
                                             d_hit_ids or None, d_counts or None, stream or None))

    # hit statistics: shuffle, histogram, estimate, significance
    def shuffle_batch_device(self, d_res: int, d_offs: int, d_lens: int, n: int, max_len: int,
                             seed: int, d_out: int, stream: int = 0):
        """sw_shuffle_batch_device: device pointers (ints); d_out[d_offs[k] .. + d_lens[k])
        receives the seeded shuffle of target k, nothing else of d_out is written.  Async on
        `stream` (0: the bank's own stream; sync() before reading)."""
        self._check(lib().sw_shuffle_batch_device(self._h, d_res or None, d_offs or None,
                                                  d_lens or None, n, max_len, seed,
                                                  d_out or None, stream or None))

    def score_histogram_device(self, d_scores: int, n: int, d_counts: int, nq: int = 1,
                               d_lens: int = 0, d_len_sums: int = 0, d_clamped: int = 0,
                               stream: int = 0):
        """sw_score_histogram_device: device pointers (ints); adds the score / length histogram
        of every row of d_scores [nq, n] to d_counts and d_len_sums (uint64 [nq, STAT_BINS]) and
        the clamped scores to d_clamped (uint64 [nq]); the caller zeroes them.  Async."""
        self._check(lib().sw_score_histogram_device(self._h, d_scores or None, d_lens or None, n,
                                                    nq, d_counts or None, d_len_sums or None,
                                                    d_clamped or None, stream or None))

    def estimate_statistics_device(self, d_res: int, d_offs: int, d_lens: int, n: int,
                                   max_len: int, seed: int = 0, rounds: int = 1,
                                   min_len: int = 0, stream: int = 0) -> list:
        """sw_estimate_statistics_device: one Statistics per loaded query from `rounds` shuffles
        of the device batch (seeds seed .. seed + rounds - 1).  Returns after synchronising."""
        out = (Statistics * max(self.query_count(), 1))()
        self._check(lib().sw_estimate_statistics_device(self._h, d_res or None, d_offs or None,
                                                        d_lens or None, n, min_len, max_len, seed,
                                                        rounds, out, stream or None))
        return list(out)[:self.query_count()]

    def estimate_statistics(self, residues: np.ndarray, offsets: np.ndarray, lens: np.ndarray,
                            seed: int = 0, rounds: int = 1) -> list:
        """sw_estimate_statistics: the same for a host batch (uploaded once)."""
        res, offs, ln, _ = validate_batch(residues, offsets, lens)
        out = (Statistics * max(self.query_count(), 1))()
        self._check(lib().sw_estimate_statistics(self._h, _p(res), res.size, _p(offs), _p(ln),
                                                 len(ln), seed, rounds, out))
        return list(out)[:self.query_count()]

    def hit_significance_device(self, stats, d_hit_scores: int, d_hits: int, d_lens: int,
                                hits_per_query: int, db_size: int, d_bits: int = 0,
                                d_evalues: int = 0, stream: int = 0):
        """sw_hit_significance_device: device pointers (ints); stats one Statistics per row of the
        [nq, hits_per_query] layout top_hits_device writes; d_bits / d_evalues (float64, either
        may be 0) receive bits and E-values, -inf / +inf in a HIT_NONE slot.  Async."""
        stats = [stats] if isinstance(stats, Statistics) else list(stats)
        arr = (Statistics * max(len(stats), 1))(*stats)
        self._check(lib().sw_hit_significance_device(self._h, arr, d_hit_scores or None,
                                                     d_hits or None, d_lens or None,
                                                     hits_per_query, len(stats), db_size,
                                                     d_bits or None, d_evalues or None,
                                                     stream or None))

    # both DNA strands: reverse complement, strand-merged scores, strand-aware alignments
    def revcomp_batch_device(self, d_res: int, d_offs: int, d_lens: int, n: int, d_out: int,
                             stream: int = 0):
        """sw_revcomp_batch_device: device pointers (ints); d_out[d_offs[k] .. + d_lens[k])
        receives the reverse complement of target k, nothing else of d_out is written.  Async on
        `stream` (0: the bank's own stream; sync() before reading)."""
        self._check(lib().sw_revcomp_batch_device(self._h, d_res or None, d_offs or None,
                                                  d_lens or None, n, d_out or None,
                                                  stream or None))

    def score_strands_device(self, d_res: int, d_offs: int, d_lens: int, n: int, max_len: int,
                             d_scores: int, d_strands: int = 0, d_rc: int = 0, min_len: int = 0,
                             stream: int = 0):
        """sw_score_strands_device: device pointers (ints); d_scores receives the nq x n int32
        strand-merged scores, d_strands (optional) the nq x n uint8 strands (1: the reverse
        score is strictly greater).  d_rc: the caller's resident reverse complement at the same
        offsets (0: the bank makes it in its scratch).  Async on `stream`."""
        self._check(lib().sw_score_strands_device(self._h, d_res or None, d_rc or None,
                                                  d_offs or None, d_lens or None, n, min_len,
                                                  max_len, d_scores or None, d_strands or None,
                                                  stream or None))

    def score_strands(self, residues: np.ndarray, offsets: np.ndarray, lens: np.ndarray):
        """sw_score_strands: (scores int32, strands uint8) of the host batch on both strands,
        [n] for one loaded query, [nq, n] for a query set."""
        res, offs, ln, _ = validate_batch(residues, offsets, lens)
        nq, n = max(self.query_count(), 1), len(ln)
        sc = np.zeros(nq * max(n, 1), np.int32)
        sd = np.zeros(nq * max(n, 1), np.uint8)
        self._check(lib().sw_score_strands(self._h, _p(res), res.size, _p(offs), _p(ln), n,
                                           _p(sc), _p(sd)))
        scores = sc[:nq * n].reshape(nq, n)
        strands = sd[:nq * n].reshape(nq, n)
        return (scores[0], strands[0]) if nq == 1 else (scores, strands)

    def align_strand_hits(self, residues: np.ndarray, offsets: np.ndarray, lens: np.ndarray,
                          strands=None, hits=None, hit_queries=None, hits_per_query: int = 0,
                          ids: Optional[np.ndarray] = None, cigar_cap: Optional[int] = None,
                          n_hits: Optional[int] = None) -> list:
        """sw_align_strand_hits: align_set_hits with the [nq, n] strand matrix of score_strands
        (None: every hit on the forward strand).  A hit on the reverse strand is aligned against
        the reverse complement of its target: Alignment.reverse is set and t_start / t_end are
        given on the forward target."""
        res, offs, ln, idv = validate_batch(residues, offsets, lens, ids)
        sv = None
        if strands is not None:
            sv = np.ascontiguousarray(strands, dtype=np.uint8).reshape(-1)
            if sv.size != max(self.query_count(), 1) * len(ln):
                raise ValueError("strands: nq x n entries")
        hv = None if hits is None else np.ascontiguousarray(hits, dtype=np.uint64).reshape(-1)
        hq = None if hit_queries is None else \
            np.ascontiguousarray(hit_queries, dtype=np.uint32).reshape(-1)
        if n_hits is None:
            n_hits = len(hv) if hv is not None else len(hq) if hq is not None else len(ln)
        if (hv is not None and len(hv) < n_hits) or (hq is not None and len(hq) < n_hits):
            raise ValueError("hits / hit_queries shorter than n_hits")
        out = np.zeros(max(n_hits, 1), dtype=ALIGNMENT_DTYPE)
        if cigar_cap is None:  # runs alternate with M runs: at most 2 x columns + 1 ops a path
            tv = hv[:n_hits] if hv is not None else np.arange(min(n_hits, len(ln)), dtype=np.uint64)
            sel = tv[tv < len(ln)].astype(np.int64)
            cigar_cap = 2 * int(ln[sel].astype(np.int64).sum()) + n_hits
        cig = np.zeros(max(cigar_cap, 1), dtype=np.uint32)
        used = ctypes.c_size_t()
        self._check(lib().sw_align_strand_hits(
            self._h, _p(res), res.size, _p(offs), _p(ln), _p(idv) if idv is not None else None,
            len(ln), _p(sv) if sv is not None else None, _p(hq) if hq is not None else None,
            hits_per_query, _p(hv) if hv is not None else None, n_hits, _p(out),
            _p(cig) if cigar_cap else None, cigar_cap, ctypes.byref(used)))
        return alignments_from(out[:n_hits], cig)

    def align_strand_hits_device(self, d_res: int, d_offs: int, d_lens: int, n: int, max_len: int,
                                 n_hits: int, d_out: int, d_strands: int = 0, d_hits: int = 0,
                                 d_hit_queries: int = 0, hits_per_query: int = 0,
                                 d_cigar: int = 0, cigar_stride: int = 0, stream: int = 0,
                                 d_ids: int = 0):
        """sw_align_strand_hits_device: align_set_hits_device with d_strands, the nq x n uint8
        strand matrix score_strands_device writes (0: every hit on the forward strand).  Async on
        `stream` (0: the bank's own stream; sync() before reading)."""
        self._check(lib().sw_align_strand_hits_device(
            self._h, d_res or None, d_offs or None, d_lens or None, d_ids or None, n, max_len,
            d_strands or None, d_hit_queries or None, hits_per_query, d_hits or None, n_hits,
            d_out or None, d_cigar or None, cigar_stride, stream or None))

    # the translated search: a protein query against DNA in six reading frames
    def translate_batch_device(self, d_res: int, d_offs: int, d_lens: int, n: int, max_len: int,
                               d_out: int, out_stride: int, d_out_offs: int, d_out_lens: int,
                               codon_table=None, stream: int = 0):
        """sw_translate_batch_device: device pointers (ints); the 6 n translations of the DNA
        batch, frame-major (f * n + k), at d_out + (f * n + k) * out_stride, with their offsets
        and lengths in d_out_offs / d_out_lens.  Async on `stream` (0: the bank's own stream;
        sync() before reading)."""
        tab = _codon_table(codon_table)
        self._check(lib().sw_translate_batch_device(
            self._h, d_res or None, d_offs or None, d_lens or None, n, max_len,
            _p(tab) if tab is not None else None, d_out or None, out_stride, d_out_offs or None,
            d_out_lens or None, stream or None))

    def score_frames_device(self, d_res: int, d_offs: int, d_lens: int, n: int, max_len: int,
                            d_scores: int, d_frames: int = 0, min_len: int = 0,
                            codon_table=None, stream: int = 0):
        """sw_score_frames_device: device pointers (ints); d_scores receives the nq x n int32
        best-frame scores of the DNA batch against the protein queries, d_frames (optional) the
        nq x n uint8 frames (the lowest frame that reaches the score).  Async on `stream`."""
        tab = _codon_table(codon_table)
        self._check(lib().sw_score_frames_device(
            self._h, d_res or None, d_offs or None, d_lens or None, n, min_len, max_len,
            _p(tab) if tab is not None else None, d_scores or None, d_frames or None,
            stream or None))

    def score_frames(self, residues: np.ndarray, offsets: np.ndarray, lens: np.ndarray,
                     codon_table=None):
        """sw_score_frames: (scores int32, frames uint8) of the host DNA batch over its six
        reading frames, [n] for one loaded query, [nq, n] for a query set."""
        res, offs, ln, _ = validate_batch(residues, offsets, lens)
        tab = _codon_table(codon_table)
        nq, n = max(self.query_count(), 1), len(ln)
        sc = np.zeros(nq * max(n, 1), np.int32)
        fr = np.zeros(nq * max(n, 1), np.uint8)
        self._check(lib().sw_score_frames(self._h, _p(res), res.size, _p(offs), _p(ln), n,
                                          _p(tab) if tab is not None else None, _p(sc), _p(fr)))
        scores = sc[:nq * n].reshape(nq, n)
        frames = fr[:nq * n].reshape(nq, n)
        return (scores[0], frames[0]) if nq == 1 else (scores, frames)

    # the frameshift-tolerant translated search: one score over the three frames of a strand
    def score_frameshift_device(self, d_dna: int, d_offs: int, d_lens: int, n: int, max_len: int,
                                frameshift: int, d_scores: int, d_strands: int = 0,
                                codon_table=None, stream: int = 0):
        """sw_score_fshift_device: device pointers (ints); d_scores receives the nq x n int32
        scores of the DNA batch against the protein queries under the frameshift penalty
        `frameshift` (0 .. -32767), d_strands (optional) the nq x n uint8 strands (1: the reverse
        strand is strictly better).  Async on `stream`."""
        tab = _codon_table(codon_table)
        self._check(lib().sw_score_fshift_device(
            self._h, d_dna or None, d_offs or None, d_lens or None, n, max_len,
            _p(tab) if tab is not None else None, frameshift, d_scores or None, d_strands or None,
            stream or None))

    def score_frameshift(self, targets, frameshift: int, codon_table=None):
        """sw_score_fshift: (scores int32, strands uint8) of host DNA targets, [n] for one loaded
        query, [nq, n] for a query set.  `targets`: a sequence of DNA code arrays, or a packed
        batch as the tuple (residues, offsets, lens)."""
        if not (isinstance(targets, tuple) and len(targets) == 3):
            targets = pack_targets([np.asarray(t, np.uint8) for t in targets])
        res, offs, ln, _ = validate_batch(*targets)
        tab = _codon_table(codon_table)
        nq, n = max(self.query_count(), 1), len(ln)
        sc = np.zeros(nq * max(n, 1), np.int32)
        sd = np.zeros(nq * max(n, 1), np.uint8)
        self._check(lib().sw_score_fshift(self._h, _p(res), res.size, _p(offs), _p(ln), n,
                                          _p(tab) if tab is not None else None, frameshift,
                                          _p(sc), _p(sd)))
        scores = sc[:nq * n].reshape(nq, n)
        strands = sd[:nq * n].reshape(nq, n)
        return (scores[0], strands[0]) if nq == 1 else (scores, strands)

    # the global-local search: the query, the target or both scored end to end
    def score_glocal_device(self, d_res: int, d_offs: int, d_lens: int, n: int, max_len: int,
                            ends: int, d_scores: int, d_end_pos: int = 0, d_strands: int = 0,
                            both_strands: bool = False, stream: int = 0):
        """sw_score_glocal_device: device pointers (ints); d_scores receives the nq x n int32
        scores of the batch under `ends` (ENDS_QUERY, ENDS_TARGET, ENDS_BOTH), d_end_pos
        (optional) the nq x n uint32 end positions (END_NONE: the boundary), d_strands (optional)
        the nq x n uint8 strands.  Async on `stream`."""
        self._check(lib().sw_score_glocal_device(
            self._h, d_res or None, d_offs or None, d_lens or None, n, max_len, ends,
            1 if both_strands else 0, d_scores or None, d_end_pos or None, d_strands or None,
            stream or None))

    def score_glocal(self, targets, ends: int, both_strands: bool = False):
        """sw_score_glocal: (scores int32, end positions uint32, strands uint8) of host targets,
        [n] for one loaded query, [nq, n] for a query set.  `targets`: a sequence of code arrays,
        or a packed batch as the tuple (residues, offsets, lens)."""
        if not (isinstance(targets, tuple) and len(targets) == 3):
            targets = pack_targets([np.asarray(t, np.uint8) for t in targets])
        res, offs, ln, _ = validate_batch(*targets)
        nq, n = max(self.query_count(), 1), len(ln)
        sc = np.zeros(nq * max(n, 1), np.int32)
        ep = np.zeros(nq * max(n, 1), np.uint32)
        sd = np.zeros(nq * max(n, 1), np.uint8)
        self._check(lib().sw_score_glocal(self._h, _p(res), res.size, _p(offs), _p(ln), n, ends,
                                          1 if both_strands else 0, _p(sc), _p(ep), _p(sd)))
        out = tuple(a[:nq * n].reshape(nq, n) for a in (sc, ep, sd))
        return tuple(a[0] for a in out) if nq == 1 else out

    # alignments of global-local hits: where a pair of score_glocal starts, its CIGAR, identities
    def align_glocal_hits(self, residues: np.ndarray, offsets: np.ndarray, lens: np.ndarray,
                          ends: int, both_strands: bool = False, hits=None, hit_queries=None,
                          hits_per_query: int = 0, ids: Optional[np.ndarray] = None,
                          cigar_cap: Optional[int] = None, n_hits: Optional[int] = None) -> list:
        """sw_align_glocal_hits: the pair list of align_set_hits over a host batch, each pair
        aligned as score_glocal scores it under `ends`.  Alignment.score may be 0 or negative; an
        empty Alignment (the boundary won) carries the boundary's score.  The first and the last
        op of a CIGAR need not be M; t_start / t_end of a reverse hit are given on the forward
        target and its CIGAR runs along the reverse strand."""
        res, offs, ln, idv = validate_batch(residues, offsets, lens, ids)
        hv = None if hits is None else np.ascontiguousarray(hits, dtype=np.uint64).reshape(-1)
        hq = None if hit_queries is None else \
            np.ascontiguousarray(hit_queries, dtype=np.uint32).reshape(-1)
        if n_hits is None:
            n_hits = len(hv) if hv is not None else len(hq) if hq is not None else len(ln)
        if (hv is not None and len(hv) < n_hits) or (hq is not None and len(hq) < n_hits):
            raise ValueError("hits / hit_queries shorter than n_hits")
        out = np.zeros(max(n_hits, 1), dtype=ALIGNMENT_DTYPE)
        if cigar_cap is None:  # an op consumes a query row or a target column
            tv = hv[:n_hits] if hv is not None else np.arange(min(n_hits, len(ln)), dtype=np.uint64)
            sel = tv[tv < len(ln)].astype(np.int64)
            cigar_cap = int(ln[sel].astype(np.int64).sum()) + n_hits * (GLOCAL_MAX_QUERY + 1)
        cig = np.zeros(max(cigar_cap, 1), dtype=np.uint32)
        used = ctypes.c_size_t()
        self._check(lib().sw_align_glocal_hits(
            self._h, _p(res), res.size, _p(offs), _p(ln), _p(idv) if idv is not None else None,
            len(ln), ends, 1 if both_strands else 0, _p(hq) if hq is not None else None,
            hits_per_query, _p(hv) if hv is not None else None, n_hits, _p(out),
            _p(cig) if cigar_cap else None, cigar_cap, ctypes.byref(used)))
        return alignments_from(out[:n_hits], cig)

    def align_glocal_hits_device(self, d_res: int, d_offs: int, d_lens: int, n: int, max_len: int,
                                 ends: int, n_hits: int, d_out: int, both_strands: bool = False,
                                 d_hits: int = 0, d_hit_queries: int = 0,
                                 hits_per_query: int = 0, d_cigar: int = 0,
                                 cigar_stride: int = 0, stream: int = 0, d_ids: int = 0):
        """sw_align_glocal_hits_device: device pointers (ints), the pair list of
        align_set_hits_device over the batch score_glocal_device scored under the same `ends` and
        `both_strands`.  Async on `stream` (0: the bank's own stream; sync() before reading)."""
        self._check(lib().sw_align_glocal_hits_device(
            self._h, d_res or None, d_offs or None, d_lens or None, d_ids or None, n, max_len,
            ends, 1 if both_strands else 0, d_hit_queries or None, hits_per_query,
            d_hits or None, n_hits, d_out or None, d_cigar or None, cigar_stride,
            stream or None))

    # non-intersecting local alignments: the next best hits of a pair
    def align_disjoint_hits(self, residues: np.ndarray, offsets: np.ndarray, lens: np.ndarray,
                            rounds: int, min_score: int = 1, hits=None, hit_queries=None,
                            hits_per_query: int = 0, ids: Optional[np.ndarray] = None,
                            cigar_cap: Optional[int] = None,
                            n_hits: Optional[int] = None) -> list:
        """sw_align_disjoint_hits: the pair list of align_set_hits over a host batch; for each
        hit a list of `rounds` Alignments in order, no two of which share a matrix cell: the best
        local alignment, then the best one that avoids its cells, and so on.  A round that scores
        less than min_score (>= 1) and every later one is empty.  Returns one list per hit."""
        res, offs, ln, idv = validate_batch(residues, offsets, lens, ids)
        hv = None if hits is None else np.ascontiguousarray(hits, dtype=np.uint64).reshape(-1)
        hq = None if hit_queries is None else \
            np.ascontiguousarray(hit_queries, dtype=np.uint32).reshape(-1)
        if n_hits is None:
            n_hits = len(hv) if hv is not None else len(hq) if hq is not None else len(ln)
        if (hv is not None and len(hv) < n_hits) or (hq is not None and len(hq) < n_hits):
            raise ValueError("hits / hit_queries shorter than n_hits")
        nrec = n_hits * max(int(rounds), 0)
        out = np.zeros(max(nrec, 1), dtype=ALIGNMENT_DTYPE)
        if cigar_cap is None:  # M runs alternate with gap runs, and an M run takes a row and a column
            tv = hv[:n_hits] if hv is not None else np.arange(min(n_hits, len(ln)), dtype=np.uint64)
            sel = tv[tv < len(ln)].astype(np.int64)
            per = 2 * np.minimum(ln[sel].astype(np.int64), DISJOINT_MAX_QUERY)
            cigar_cap = max(int(rounds), 0) * int(per.sum()) + nrec
        cig = np.zeros(max(cigar_cap, 1), dtype=np.uint32)
        used = ctypes.c_size_t()
        self._check(lib().sw_align_disjoint_hits(
            self._h, _p(res), res.size, _p(offs), _p(ln), _p(idv) if idv is not None else None,
            len(ln), rounds, min_score, _p(hq) if hq is not None else None, hits_per_query,
            _p(hv) if hv is not None else None, n_hits, _p(out), _p(cig) if cigar_cap else None,
            cigar_cap, ctypes.byref(used)))
        flat = alignments_from(out[:nrec], cig)
        return [flat[h * rounds:(h + 1) * rounds] for h in range(n_hits)]

    def align_disjoint_hits_device(self, d_res: int, d_offs: int, d_lens: int, n: int,
                                   max_len: int, rounds: int, n_hits: int, d_out: int,
                                   min_score: int = 1, d_hits: int = 0, d_hit_queries: int = 0,
                                   hits_per_query: int = 0, d_cigar: int = 0,
                                   cigar_stride: int = 0, stream: int = 0, d_ids: int = 0):
        """sw_align_disjoint_hits_device: device pointers (ints), the pair list of
        align_set_hits_device; d_out receives n_hits x rounds records, (hit h, round r) at
        h * rounds + r, its ops at d_cigar + (h * rounds + r) * cigar_stride.  Async on `stream`
        (0: the bank's own stream; sync() before reading)."""
        self._check(lib().sw_align_disjoint_hits_device(
            self._h, d_res or None, d_offs or None, d_lens or None, d_ids or None, n, max_len,
            rounds, min_score, d_hit_queries or None, hits_per_query, d_hits or None, n_hits,
            d_out or None, d_cigar or None, cigar_stride, stream or None))

    # non-intersecting alignments over the six reading frames: every exon of a hit, best first
    def align_disjoint_frame_hits(self, residues: np.ndarray, offsets: np.ndarray,
                                  lens: np.ndarray, rounds: int, min_score: int = 1, hits=None,
                                  hit_queries=None, hits_per_query: int = 0,
                                  ids: Optional[np.ndarray] = None,
                                  cigar_cap: Optional[int] = None, n_hits: Optional[int] = None,
                                  codon_table=None) -> list:
        """sw_align_disjoint_frame_hits: the pair list of align_set_hits over a host DNA batch;
        for each hit a list of `rounds` Alignments, best first, merged from the non-intersecting
        alignments of the query with each of the target's six translations (a tie goes to the
        lowest frame).  Alignment.frame is the record's frame, t_start / t_end are nucleotides on
        the forward target, the CIGAR runs in amino-acid columns.  Returns one list per hit."""
        res, offs, ln, idv = validate_batch(residues, offsets, lens, ids)
        tab = _codon_table(codon_table)
        hv = None if hits is None else np.ascontiguousarray(hits, dtype=np.uint64).reshape(-1)
        hq = None if hit_queries is None else \
            np.ascontiguousarray(hit_queries, dtype=np.uint32).reshape(-1)
        if n_hits is None:
            n_hits = len(hv) if hv is not None else len(hq) if hq is not None else len(ln)
        if (hv is not None and len(hv) < n_hits) or (hq is not None and len(hq) < n_hits):
            raise ValueError("hits / hit_queries shorter than n_hits")
        nrec = n_hits * max(int(rounds), 0)
        out = np.zeros(max(nrec, 1), dtype=ALIGNMENT_DTYPE)
        if cigar_cap is None:  # M runs alternate with gap runs, and an M run takes a row and a codon
            tv = hv[:n_hits] if hv is not None else np.arange(min(n_hits, len(ln)), dtype=np.uint64)
            sel = tv[tv < len(ln)].astype(np.int64)
            per = 2 * np.minimum(ln[sel].astype(np.int64) // 3, DISJOINT_MAX_QUERY)
            cigar_cap = max(int(rounds), 0) * int(per.sum()) + nrec
        cig = np.zeros(max(cigar_cap, 1), dtype=np.uint32)
        used = ctypes.c_size_t()
        self._check(lib().sw_align_disjoint_frame_hits(
            self._h, _p(res), res.size, _p(offs), _p(ln), _p(idv) if idv is not None else None,
            len(ln), _p(tab) if tab is not None else None, rounds, min_score,
            _p(hq) if hq is not None else None, hits_per_query,
            _p(hv) if hv is not None else None, n_hits, _p(out), _p(cig) if cigar_cap else None,
            cigar_cap, ctypes.byref(used)))
        flat = alignments_from(out[:nrec], cig)
        return [flat[h * rounds:(h + 1) * rounds] for h in range(n_hits)]

    def align_disjoint_frame_hits_device(self, d_res: int, d_offs: int, d_lens: int, n: int,
                                         max_len: int, rounds: int, n_hits: int, d_out: int,
                                         min_score: int = 1, d_hits: int = 0,
                                         d_hit_queries: int = 0, hits_per_query: int = 0,
                                         d_cigar: int = 0, cigar_stride: int = 0, stream: int = 0,
                                         d_ids: int = 0, codon_table=None):
        """sw_align_disjoint_frame_hits_device: device pointers (ints), the pair list of
        align_set_hits_device over the DNA batch score_frames_device scored; d_out receives
        n_hits x rounds records, (hit h, round r) at h * rounds + r, its ops at
        d_cigar + (h * rounds + r) * cigar_stride.  Async on `stream` (0: the bank's own stream;
        sync() before reading)."""
        tab = _codon_table(codon_table)
        self._check(lib().sw_align_disjoint_frame_hits_device(
            self._h, d_res or None, d_offs or None, d_lens or None, d_ids or None, n, max_len,
            _p(tab) if tab is not None else None, rounds, min_score, d_hit_queries or None,
            hits_per_query, d_hits or None, n_hits, d_out or None, d_cigar or None, cigar_stride,
            stream or None))

    def estimate_frameshift_statistics_device(self, d_dna: int, d_offs: int, d_lens: int, n: int,
                                              max_len: int, frameshift: int, seed: int = 0,
                                              rounds: int = 1, codon_table=None,
                                              stream: int = 0) -> list:
        """sw_estimate_fshift_statistics_device: one Statistics per loaded query from `rounds`
        shuffles of the device DNA batch (seeds seed .. seed + rounds - 1), each scored as
        score_frameshift_device scores it.  Returns after synchronising.  hit_significance with
        the targets' lengths in nucleotides gives the bits and E-values of frameshift hits."""
        tab = _codon_table(codon_table)
        out = (Statistics * max(self.query_count(), 1))()
        self._check(lib().sw_estimate_fshift_statistics_device(
            self._h, d_dna or None, d_offs or None, d_lens or None, n, max_len,
            _p(tab) if tab is not None else None, frameshift, seed, rounds, out, stream or None))
        return list(out)[:self.query_count()]

    def estimate_frameshift_statistics(self, targets, frameshift: int, seed: int = 0,
                                       rounds: int = 1, codon_table=None) -> list:
        """sw_estimate_fshift_statistics: the same for host DNA targets (uploaded once), a
        sequence of DNA code arrays or a packed batch as the tuple (residues, offsets, lens)."""
        if not (isinstance(targets, tuple) and len(targets) == 3):
            targets = pack_targets([np.asarray(t, np.uint8) for t in targets])
        res, offs, ln, _ = validate_batch(*targets)
        tab = _codon_table(codon_table)
        out = (Statistics * max(self.query_count(), 1))()
        self._check(lib().sw_estimate_fshift_statistics(
            self._h, _p(res), res.size, _p(offs), _p(ln), len(ln),
            _p(tab) if tab is not None else None, frameshift, seed, rounds, out))
        return list(out)[:self.query_count()]

    def align_frame_hits(self, residues: np.ndarray, offsets: np.ndarray, lens: np.ndarray,
                         frames, hits=None, hit_queries=None, hits_per_query: int = 0,
                         ids: Optional[np.ndarray] = None, cigar_cap: Optional[int] = None,
                         n_hits: Optional[int] = None, codon_table=None) -> list:
        """sw_align_frame_hits: align_set_hits on the translation of each hit's frame, `frames`
        the [nq, n] matrix of score_frames.  Alignment.frame is the hit's frame, t_start / t_end
        are nucleotide positions on the forward target; the query coordinates, the counts and the
        CIGAR stay in amino-acid columns."""
        res, offs, ln, idv = validate_batch(residues, offsets, lens, ids)
        tab = _codon_table(codon_table)
        fv = None
        if frames is not None:
            fv = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
            if fv.size != max(self.query_count(), 1) * len(ln):
                raise ValueError("frames: nq x n entries")
        hv = None if hits is None else np.ascontiguousarray(hits, dtype=np.uint64).reshape(-1)
        hq = None if hit_queries is None else \
            np.ascontiguousarray(hit_queries, dtype=np.uint32).reshape(-1)
        if n_hits is None:
            n_hits = len(hv) if hv is not None else len(hq) if hq is not None else len(ln)
        if (hv is not None and len(hv) < n_hits) or (hq is not None and len(hq) < n_hits):
            raise ValueError("hits / hit_queries shorter than n_hits")
        out = np.zeros(max(n_hits, 1), dtype=ALIGNMENT_DTYPE)
        if cigar_cap is None:  # runs alternate with M runs: at most 2 x columns + 1 ops a path
            tv = hv[:n_hits] if hv is not None else np.arange(min(n_hits, len(ln)), dtype=np.uint64)
            sel = tv[tv < len(ln)].astype(np.int64)
            cigar_cap = 2 * int((ln[sel].astype(np.int64) // 3).sum()) + n_hits
        cig = np.zeros(max(cigar_cap, 1), dtype=np.uint32)
        used = ctypes.c_size_t()
        self._check(lib().sw_align_frame_hits(
            self._h, _p(res), res.size, _p(offs), _p(ln), _p(idv) if idv is not None else None,
            len(ln), _p(tab) if tab is not None else None, _p(fv) if fv is not None else None,
            _p(hq) if hq is not None else None, hits_per_query,
            _p(hv) if hv is not None else None, n_hits, _p(out),
            _p(cig) if cigar_cap else None, cigar_cap, ctypes.byref(used)))
        return alignments_from(out[:n_hits], cig)

    def align_frame_hits_device(self, d_res: int, d_offs: int, d_lens: int, n: int, max_len: int,
                                n_hits: int, d_out: int, d_frames: int, d_hits: int = 0,
                                d_hit_queries: int = 0, hits_per_query: int = 0,
                                d_cigar: int = 0, cigar_stride: int = 0, stream: int = 0,
                                d_ids: int = 0, codon_table=None):
        """sw_align_frame_hits_device: align_set_hits_device on the translation of each hit's
        frame, d_frames the nq x n uint8 frame matrix score_frames_device writes.  Async on
        `stream` (0: the bank's own stream; sync() before reading)."""
        tab = _codon_table(codon_table)
        self._check(lib().sw_align_frame_hits_device(
            self._h, d_res or None, d_offs or None, d_lens or None, d_ids or None, n, max_len,
            _p(tab) if tab is not None else None, d_frames or None, d_hit_queries or None,
            hits_per_query, d_hits or None, n_hits, d_out or None, d_cigar or None, cigar_stride,
            stream or None))

    # alignments of frameshift hits: where a hit of score_frameshift lies and where it shifts
    def align_frameshift_hits(self, residues: np.ndarray, offsets: np.ndarray, lens: np.ndarray,
                              frameshift: int, hits=None, hit_queries=None,
                              hits_per_query: int = 0, ids: Optional[np.ndarray] = None,
                              cigar_cap: Optional[int] = None, n_hits: Optional[int] = None,
                              codon_table=None) -> list:
        """sw_align_fshift_hits: the pair list of align_set_hits over a host DNA batch; the call
        scores both strands itself.  Alignment.frame is the frame of the hit's first codon on its
        strand, t_start / t_end are nucleotide positions on the forward target; the CIGAR is in
        amino-acid columns with CIGAR_FS_SKIP ('/') and CIGAR_FS_BACK ('\\') ops of length 1 where
        the next codon starts one base later or earlier than the frame says."""
        res, offs, ln, idv = validate_batch(residues, offsets, lens, ids)
        tab = _codon_table(codon_table)
        hv = None if hits is None else np.ascontiguousarray(hits, dtype=np.uint64).reshape(-1)
        hq = None if hit_queries is None else \
            np.ascontiguousarray(hit_queries, dtype=np.uint32).reshape(-1)
        if n_hits is None:
            n_hits = len(hv) if hv is not None else len(hq) if hq is not None else len(ln)
        if (hv is not None and len(hv) < n_hits) or (hq is not None and len(hq) < n_hits):
            raise ValueError("hits / hit_queries shorter than n_hits")
        out = np.zeros(max(n_hits, 1), dtype=ALIGNMENT_DTYPE)
        if cigar_cap is None:  # m M runs between shifts and I runs span at least 2 m + 1 bases
            tv = hv[:n_hits] if hv is not None else np.arange(min(n_hits, len(ln)), dtype=np.uint64)
            sel = tv[tv < len(ln)].astype(np.int64)
            cigar_cap = 2 * int(ln[sel].astype(np.int64).sum()) + n_hits
        cig = np.zeros(max(cigar_cap, 1), dtype=np.uint32)
        used = ctypes.c_size_t()
        self._check(lib().sw_align_fshift_hits(
            self._h, _p(res), res.size, _p(offs), _p(ln), _p(idv) if idv is not None else None,
            len(ln), _p(tab) if tab is not None else None, frameshift,
            _p(hq) if hq is not None else None, hits_per_query,
            _p(hv) if hv is not None else None, n_hits, _p(out),
            _p(cig) if cigar_cap else None, cigar_cap, ctypes.byref(used)))
        return alignments_from(out[:n_hits], cig)

    def align_frameshift_hits_device(self, d_res: int, d_offs: int, d_lens: int, n: int,
                                     max_len: int, frameshift: int, n_hits: int, d_out: int,
                                     d_hits: int = 0, d_hit_queries: int = 0,
                                     hits_per_query: int = 0, d_cigar: int = 0,
                                     cigar_stride: int = 0, stream: int = 0, d_ids: int = 0,
                                     codon_table=None):
        """sw_align_fshift_hits_device: device pointers (ints), the pair list of
        align_set_hits_device over the DNA batch score_frameshift_device scored.  Async on
        `stream` (0: the bank's own stream; sync() before reading)."""
        tab = _codon_table(codon_table)
        self._check(lib().sw_align_fshift_hits_device(
            self._h, d_res or None, d_offs or None, d_lens or None, d_ids or None, n, max_len,
            _p(tab) if tab is not None else None, frameshift, d_hit_queries or None,
            hits_per_query, d_hits or None, n_hits, d_out or None, d_cigar or None, cigar_stride,
            stream or None))

    def counters(self) -> dict:
        """sw_bank_counters: feeder / fallback counts since the bank was created."""
        c = (ctypes.c_uint64 * len(COUNTERS))()
        self._check(lib().sw_bank_counters_ex(self._h, ctypes.byref(c), ctypes.sizeof(c)))
        return dict(zip(COUNTERS, (int(x) for x in c)))

    def sync(self):
        """sw_bank_sync: wait for the bank's last scoring call; raises SwbankError(ERR_TIMEOUT)
        when a device call since the last synchronising call had a hand-off wait run out."""
        self._check(lib().sw_bank_sync(self._h))

    # CAPI record path (sequence_t arrays, 2-bit codes)
    def load_query_record(self, record: np.ndarray):
        r = np.ascontiguousarray(record, dtype=np.uint8).reshape(-1)
        if r.size != RECORD_BYTES:
            raise ValueError("a record is 64 bytes")
        self._check(lib().sw_load_query_record(self._h, _p(r)))

    def score_records(self, records: np.ndarray) -> np.ndarray:
        r = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, RECORD_BYTES)
        out = np.zeros(len(r), dtype=np.int32)
        if len(r):
            self._check(lib().sw_score_records(self._h, _p(r), len(r), _p(out)))
        return out

    def score_records_device(self, d_records: int, n: int, d_scores: int, stream: int = 0):
        self._check(lib().sw_score_records_device(self._h, d_records, n, d_scores,
                                                  stream or None))

    def best_hit(self, scores: np.ndarray, ids: Optional[np.ndarray] = None) -> Tuple[int, int]:
        """ScoreBank max / vld_max: (id of the best target, its score)."""
        s = np.ascontiguousarray(scores, dtype=np.int32)
        bid, bsc = ctypes.c_uint64(), ctypes.c_int32()
        ida = np.ascontiguousarray(ids, dtype=np.uint64) if ids is not None else None
        self._check(lib().sw_best_hit(self._h, _p(s), _p(ida) if ida is not None else None,
                                      len(s), ctypes.byref(bid), ctypes.byref(bsc)))
        return int(bid.value), int(bsc.value)

    def best_hit_device(self, d_scores: int, n: int, d_out: int, d_ids: int = 0,
                        stream: int = 0):
        """Device best hit: d_out (2 x uint64) <- (best id, best score); async on `stream`."""
        self._check(lib().sw_best_hit_device(self._h, d_scores, d_ids or None, n, d_out,
                                             stream or None))

    # profiling
    def set_timing(self, enable: bool = True):
        self._check(lib().sw_bank_set_timing(self._h, 1 if enable else 0))

    def last_kernel(self) -> str:
        """The kernel the last score call ran (e.g. "tile f16 R=32 W=4 segs=1 grid=998")."""
        return lib().sw_last_kernel(self._h).decode()

    def timing(self) -> Tuple[int, float, float]:
        """(launches, pack_ms, score_ms) accumulated since the previous call."""
        n, pm, sm = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double()
        self._check(lib().sw_bank_timing(self._h, ctypes.byref(n), ctypes.byref(pm),
                                         ctypes.byref(sm)))
        return int(n.value), float(pm.value), float(sm.value)
