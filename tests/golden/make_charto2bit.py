#!/usr/bin/env python3
"""Record the reference's charTo2bit on seeded sequences as ``charto2bit_random.tsv``.

Run where the reference tree is present, after ``make -C oracle ref`` has compiled its
charTo2bit (aligner_Header.c:14-47) into ``oracle/_ref/libaligner_ref.so``:

    python tests/golden/make_charto2bit.py

One row per sequence: the sequence (letters of ``ACGTacgtN``, lengths 1, 3, 4, 31, 32, 128 and
232 = the longest a CAPI record holds) and the ceil(n / 4) bytes the reference wrote for it,
as hex.  DATA only: inputs and what the reference's program returned for them.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF_LIB = os.path.join(REPO, "oracle", "_ref", "libaligner_ref.so")
LENGTHS = (1, 3, 4, 31, 32, 128, 232)


def sequences():
    rng = np.random.default_rng(1)
    return ["".join(rng.choice(list("ACGTacgtN"), n)) for n in LENGTHS]


def reference_bytes(ref, seq: str) -> np.ndarray:
    """charTo2bit(seq) -> its first ceil(n / 4) bytes.  The reference prints a debug trace per
    base (_DEBUGGING_), so stdout is muted at the fd level around the call."""
    libc = ctypes.CDLL(None)
    libc.fflush.argtypes = [ctypes.c_void_p]
    buf = np.zeros(64, np.uint8)
    fd = os.dup(1)
    with open(os.devnull, "w") as dn:
        os.dup2(dn.fileno(), 1)
        try:
            ref.charTo2bit(seq.encode(), buf.ctypes.data)
            libc.fflush(None)
        finally:
            os.dup2(fd, 1)
            os.close(fd)
    return buf[:(len(seq) + 3) // 4]


def load_reference():
    ref = ctypes.CDLL(REF_LIB)
    ref.charTo2bit.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    return ref


def main():
    ref = load_reference()
    with open(os.path.join(HERE, "charto2bit_random.tsv"), "w") as out:
        out.write("sequence\tbytes\n")
        for seq in sequences():
            out.write(seq + "\t" + reference_bytes(ref, seq).tobytes().hex() + "\n")
    print(f"wrote {len(LENGTHS)} sequences")


if __name__ == "__main__":
    main()
