"""The cases the Reed-Solomon tests share (tests/test_rs_cpu.py on the host,
tests/test_gpu_rs.py on the device): the frame lengths at which the layout
changes, and the error patterns planted in every codeword of a frame.
"""
import numpy as np

import frames_check_ref as C
import rs_ref as R

KINDS = (C.CRC16, C.CRC32)
FLAGS = (R.FLAG16, R.FLAG32)
BAD_MODES = (0, 2, 0x10, 0x31, 0x81)
PATTERNS = ("none", "one", "t", "t+1", "parity", "ends", "header")


def edge_lengths(h, c, P):
    """0, 1, the last len with D = 1, the first with D = 2, one with D = 3 and
    unequal k_j, and 4096 (the last two need h = 2)."""
    kmax = 255 - P
    out = [0, 1, kmax - h - c, kmax - h - c + 1]
    if h == 2:
        n3 = 2 * kmax + 2
        n3 += n3 % 3 == 0
        assert R.codewords(n3, P) == 3 and n3 % 3 != 0
        out += [n3 - h - c, 4096]
    return out


def corrupt(row, n, P, h, pattern, rng):
    """`pattern` in every codeword of the frame of n bytes in `row` (a
    bytearray), the header bytes spared except by "header"."""
    t, D = P // 2, R.codewords(n, P)
    if pattern == "header":
        row[h - 1] ^= 0x04
        return
    for j in range(D):
        off = R.offsets(n, P, j)
        free = [x for x in range(len(off)) if off[x] >= h]
        if pattern == "none":
            xs = []
        elif pattern == "one":
            xs = [free[int(rng.integers(len(free)))]]
        elif pattern in ("t", "t+1"):
            k = min(t + (pattern == "t+1"), len(free))
            xs = rng.choice(free, k, replace=False).tolist()
        elif pattern == "parity":
            xs = rng.choice(np.arange(len(off) - P, len(off)), t, replace=False).tolist()
        else:   # "ends": the first and the last symbol of the codeword
            xs = [free[0], len(off) - 1]
        for x in xs:
            row[off[x]] ^= int(rng.integers(1, 256))
