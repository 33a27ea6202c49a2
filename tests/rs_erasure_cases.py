"""The cases the erasure-decoding tests share (tests/test_rs_erasures_cpu.py on
the host, tests/test_gpu_rs_erasures.py on the device): what is planted in each
codeword of a frame, flags and wrong bytes together.
"""
import itertools

import numpy as np

import rs_ref as R


def combos(P):
    """(f, 2 e + f) for f in {0, 1, P - 1, P, P + 1} and 2 e + f at the limit (P
    - 1 or P: the sum has f's parity), one error past it (P + 1 or P + 2) and
    two past it."""
    out = []
    for f in (0, 1, P - 1, P, P + 1):
        at = P if (P - f) % 2 == 0 else P - 1
        out += [(f, at), (f, at + 2), (f, at + 4)]
    return out


def plant(row, flags, n, P, h, rng, plan):
    """In codeword j of the frame of n bytes in `row` (a bytearray; `flags` a
    bool array a row byte): plan[j % len(plan)] = (f, 2 e + f). f random
    positions are flagged, about half of them hold a wrong byte and the others
    are right; e positions outside the flags hold a wrong byte. Header bytes
    are flagged but never made wrong; parity bytes take part like any other.
    Returns [(f, e) a codeword] as planted (clipped to the codeword's room)."""
    D = R.codewords(n, P)
    done = []
    for j in range(D):
        f, total = plan[j % len(plan)]
        off = R.offsets(n, P, j)
        N = len(off)
        f = min(f, N)
        e = min(max((total - f) // 2, 0), N - f)
        flagged = rng.choice(N, f, replace=False) if f else np.zeros(0, dtype=int)
        rest = np.setdiff1d(np.arange(N), flagged)
        rest = rest[[off[x] >= h for x in rest]] if len(rest) else rest
        e = min(e, len(rest))
        wrong = rng.choice(rest, e, replace=False) if e else np.zeros(0, dtype=int)
        for x in flagged:
            flags[off[x]] = True
            if off[x] >= h and rng.integers(2):
                row[off[x]] ^= int(rng.integers(1, 256))
        for x in wrong:
            row[off[x]] ^= int(rng.integers(1, 256))
        done.append((int(f), int(e)))
    return done


def rounds(P, D):
    """Rotations of combos(P) so that D codewords a round meet every combination."""
    base = combos(P)
    k = -(-len(base) // D)
    return [list(itertools.islice(itertools.cycle(base), r * D, r * D + D)) for r in range(k)]
