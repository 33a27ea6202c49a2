"""An independent reference of the Reed-Solomon outer code (include/demod.h
"Reed-Solomon outer code"), in plain Python.

Nothing here follows the product's route. The field tables come from the
reduction polynomial by shift and XOR; the encoder is polynomial long
division; the decoder is Peterson-Gorenstein-Zierler: for v = t down to 1 the
v x v syndrome matrix is solved for the locator by Gaussian elimination over
the field, the roots are found by trying every position of the codeword, and
the error values come from a second linear solve. No Berlekamp-Massey, no
Forney. A candidate is accepted only when the corrected word has zero
syndromes, so what is accepted is a codeword within t of the received word:
the unique one, whatever algorithm finds it.

`check_codeword` uses no decoder at all: a decoded codeword has zero syndromes
by direct evaluation and differs from the received one in at most t places; a
failed one is unchanged.
"""
import frames_check_ref as C

POLY = 0x11D
FLAG16, FLAG32 = 0x100, 0x200
PARITY = {FLAG16: 16, FLAG32: 32}
OK, BAD_LENGTH, FAILED = 0, 1, 2

EXP = [0] * 510
LOG = [0] * 256
_v = 1
for _e in range(255):
    EXP[_e] = EXP[_e + 255] = _v
    LOG[_v] = _e
    _v <<= 1
    if _v & 0x100:
        _v ^= POLY


def mul(a, b):
    return EXP[LOG[a] + LOG[b]] if a and b else 0


def div(a, b):
    assert b
    return EXP[LOG[a] + 255 - LOG[b]] if a else 0


def apow(e):
    return EXP[e % 255]


def generator(P):
    """g(x) = prod_{i<P} (x - alpha^i), highest coefficient first."""
    g = [1]
    for i in range(P):
        r = apow(i)
        g = [a ^ mul(b, r) for a, b in zip(g + [0], [0] + g)]
    return g


def parity(msg, P):
    """The remainder of msg(x) x^P by g, highest degree first (long division)."""
    g = generator(P)
    rem = list(msg) + [0] * P
    for i in range(len(msg)):
        f = rem[i]
        if f:
            for d in range(1, P + 1):
                rem[i + d] ^= mul(f, g[d])
    return rem[len(msg):]


def mode_parity(fec):
    return PARITY.get(fec & (FLAG16 | FLAG32), 0)


def codewords(n, P):
    return -(-n // (255 - P))


def frame_size(n, P):
    return n + codewords(n, P) * P if P else n


def offsets(n, P, j):
    """Where the symbols of codeword j sit in the frame, highest degree first."""
    D = codewords(n, P)
    return list(range(j, n, D)) + [n + i * D + j for i in range(P)]


def max_len(W, h, c, P):
    """The greatest len with n'(len) <= W, by counting; -1 when none fits."""
    best = -1
    for length in range(0, W + 1):
        if frame_size(h + length + c, P) <= W:
            best = length
        else:
            break
    return best


def frame_encode(data, h, kind, P):
    frame = list(C.encode(bytes(data), h, kind))
    n = len(frame)
    if not P:
        return bytes(frame)
    D = codewords(n, P)
    out = frame + [0] * (D * P)
    for j in range(D):
        off = offsets(n, P, j)
        par = parity([frame[o] for o in off[:-P]], P)
        for o, v in zip(off[-P:], par):
            out[o] = v
    return bytes(out)


def syndromes(word, P):
    """S_i = word(alpha^i) by direct evaluation: symbol x has power N - 1 - x."""
    N = len(word)
    return [_xor(mul(c, apow(i * (N - 1 - x))) for x, c in enumerate(word) if c) for i in range(P)]


def _xor(it):
    v = 0
    for a in it:
        v ^= a
    return v


def _solve(M, rhs):
    """x with M x = rhs over the field, or None when M is singular."""
    v = len(M)
    A = [row[:] + [r] for row, r in zip(M, rhs)]
    for col in range(v):
        piv = next((r for r in range(col, v) if A[r][col]), None)
        if piv is None:
            return None
        A[col], A[piv] = A[piv], A[col]
        inv = div(1, A[col][col])
        A[col] = [mul(a, inv) for a in A[col]]
        for r in range(v):
            if r != col and A[r][col]:
                f = A[r][col]
                A[r] = [a ^ mul(f, b) for a, b in zip(A[r], A[col])]
    return [A[r][v] for r in range(v)]


def decode_codeword(word, P):
    """(the codeword, the places changed), or None when no codeword of the
    shortened code lies within t = P / 2 of `word`."""
    word = list(word)
    N, t = len(word), P // 2
    S = syndromes(word, P)
    if not any(S):
        return word, 0
    for v in range(t, 0, -1):
        lam = _solve([[S[i + j] for j in range(v)] for i in range(v)], [S[i + v] for i in range(v)])
        if lam is None:
            continue
        loc = [1] + lam[::-1]                       # Lambda_0 .. Lambda_v
        places = []
        for x in range(N):
            z = (255 - (N - 1 - x)) % 255           # X^-1 = alpha^z
            if _xor(mul(c, apow(l * z)) for l, c in enumerate(loc) if c) == 0:
                places.append(x)
        if len(places) != v:
            return None
        X = [apow(N - 1 - x) for x in places]
        vals = _solve([[apow(LOG[Xk] * i) for Xk in X] for i in range(v)], S[:v])
        if vals is None:
            return None
        out = word[:]
        for x, e in zip(places, vals):
            out[x] ^= e
        if any(syndromes(out, P)):
            return None
        return out, sum(a != b for a, b in zip(out, word))
    return None


def frame_decode(row, h, kind, P):
    """The decoder on a row of W = len(row) bytes: (the row, the record)."""
    row = list(row)
    c = C.CRC_BYTES[kind]
    length = int.from_bytes(bytes(row[:h]), "big")
    most = max_len(len(row), h, c, P)
    assert most >= 0
    if length > most:
        return bytes(row), dict(status=BAD_LENGTH, codewords=0, corrected=0, failed=0)
    n = h + length + c
    D = codewords(n, P)
    rec = dict(status=OK, codewords=D, corrected=0, failed=0)
    for j in range(D):
        off = offsets(n, P, j)
        got = decode_codeword([row[o] for o in off], P)
        if got is None:
            rec["failed"] += 1
            continue
        for o, v in zip(off, got[0]):
            row[o] = v
        rec["corrected"] += got[1]
    if rec["failed"]:
        rec["status"] = FAILED
    return bytes(row), rec


def check_codeword(received, result, failed, P):
    """No decoder: a decoded codeword has zero syndromes and differs from the
    received one in at most t places; a failed one is unchanged. Returns the
    places changed."""
    received, result = list(received), list(result)
    assert len(received) == len(result)
    changed = sum(a != b for a, b in zip(received, result))
    if failed:
        assert changed == 0, "a failed codeword was changed"
        assert any(syndromes(result, P)), "a codeword was reported as failed"
        return 0
    assert changed <= P // 2, ("more than t places changed", changed)
    assert not any(syndromes(result, P)), "a decoded word is not a codeword"
    return changed


def check_frame(before, after, record, h, kind, P):
    """check_codeword over every codeword of a decoded row, and the record's
    sums. `before` and `after` are the whole rows."""
    c = C.CRC_BYTES[kind]
    length = int.from_bytes(bytes(before[:h]), "big")
    if record["status"] == BAD_LENGTH:
        assert length > max_len(len(before), h, c, P)
        assert bytes(before) == bytes(after) and record["codewords"] == record["corrected"] == record["failed"] == 0
        return
    n = h + length + c
    D = codewords(n, P)
    assert record["codewords"] == D
    assert bytes(before[frame_size(n, P):]) == bytes(after[frame_size(n, P):]), "bytes past n' changed"
    changed = failed = 0
    for j in range(D):
        off = offsets(n, P, j)
        r, o = [before[x] for x in off], [after[x] for x in off]
        bad = any(syndromes(o, P))
        failed += bad
        changed += check_codeword(r, o, bad, P)
    assert (record["corrected"], record["failed"]) == (changed, failed)
    assert record["status"] == (FAILED if failed else OK)
