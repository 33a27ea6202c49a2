"""An independent reference of the Reed-Solomon decoder with an erasure mask
(include/demod.h "erasure decoding"), in plain Python, in the manner of
tests/rs_ref.py and on its field, layout and errors-only decoder.

Nothing here follows the product's route. The first attempt is
Peterson-Gorenstein-Zierler on the Forney syndromes: with f flagged positions
the erasure locator Gamma is multiplied out, T = S Gamma mod x^P, and for v =
floor((P - f) / 2) down to 0 the v x v matrix of T_f .. T_(P-1) is solved for
the error locator by Gaussian elimination; its roots are found by trying every
position that is not flagged; the values of all v + f errata come from one
linear solve on the first v + f syndromes. No Berlekamp-Massey, no Forney. A
candidate is accepted only when the corrected word has zero syndromes by direct
evaluation and 2 e + f <= P for the e places outside the flags that changed:
the unique such codeword, whatever algorithm finds it. Otherwise the fallback
is rs_ref's errors-only decoder on the same word.

`check_frame` uses no decoder at all.
"""
import frames_check_ref as C
import rs_ref as R

mul, div, apow, LOG = R.mul, R.div, R.apow, R.LOG


def mask_words(row_bytes):
    return -(-row_bytes // 64)


def pack_mask(flags, row_bytes):
    """A bool a row byte -> the Wm words: byte b is bit b & 63 of word b >> 6."""
    words = [0] * mask_words(row_bytes)
    for b, f in enumerate(flags[:row_bytes]):
        if f:
            words[b >> 6] |= 1 << (b & 63)
    return words


def first_attempt(word, P, flagged):
    """(the codeword, the places changed), or None when no codeword c has 2 e +
    f <= P. `flagged`: the flagged positions of the word, 1 <= f <= P of them."""
    word = list(word)
    N, f = len(word), len(flagged)
    assert 1 <= f <= P
    S = R.syndromes(word, P)
    gam = [1]
    for x in flagged:                                   # times (1 - X x), X = alpha^(N - 1 - x)
        X = apow(N - 1 - x)
        gam = [a ^ mul(b, X) for a, b in zip(gam + [0], [0] + gam)]
    T = [R._xor(mul(gam[l], S[k - l]) for l in range(min(k, f) + 1)) for k in range(P)][f:]
    for v in range((P - f) // 2, -1, -1):
        places = []
        if v:
            lam = R._solve([[T[i + j] for j in range(v)] for i in range(v)], [T[i + v] for i in range(v)])
            if lam is None:
                continue
            loc = [1] + lam[::-1]
            for x in range(N):
                if x in flagged:
                    continue
                z = (255 - (N - 1 - x)) % 255
                if R._xor(mul(c, apow(l * z)) for l, c in enumerate(loc) if c) == 0:
                    places.append(x)
            if len(places) != v:
                continue
        errata = list(flagged) + places
        X = [apow(N - 1 - x) for x in errata]
        vals = R._solve([[apow(LOG[Xk] * i) for Xk in X] for i in range(len(X))], S[:len(X)])
        if vals is None:
            continue
        out = word[:]
        for x, e in zip(errata, vals):
            out[x] ^= e
        if any(R.syndromes(out, P)):
            continue
        e = sum(out[x] != word[x] for x in range(N) if x not in flagged)
        if 2 * e + f > P:
            continue
        return out, sum(a != b for a, b in zip(out, word))
    return None


def decode_codeword(word, P, flagged):
    """(the codeword or None when it failed, the places changed, the branch:
    "clean", "errors" (f = 0), "used" or "fallback")."""
    word = list(word)
    f = len(flagged)
    if not any(R.syndromes(word, P)):
        return word, 0, "clean"
    if f == 0:
        got = R.decode_codeword(word, P)
        return (got[0], got[1], "errors") if got else (None, 0, "errors")
    if f <= P:
        got = first_attempt(word, P, flagged)
        if got:
            return got[0], got[1], "used"
    got = R.decode_codeword(word, P)
    return (got[0], got[1], "fallback") if got else (None, 0, "fallback")


def frame_decode(row, h, kind, P, flags):
    """The decoder on a row of W = len(row) bytes with a bool a row byte (or
    None): (the row, the record, the erasure record)."""
    row = list(row)
    W = len(row)
    flags = list(flags) if flags is not None else [False] * W
    c = C.CRC_BYTES[kind]
    length = int.from_bytes(bytes(row[:h]), "big")
    erec = dict(erased=0, used=0, fallback=0, reserved=0)
    most = R.max_len(W, h, c, P)
    assert most >= 0
    if length > most:
        return bytes(row), dict(status=R.BAD_LENGTH, codewords=0, corrected=0, failed=0), erec
    n = h + length + c
    D = R.codewords(n, P)
    rec = dict(status=R.OK, codewords=D, corrected=0, failed=0)
    for j in range(D):
        off = R.offsets(n, P, j)
        flagged = [x for x, o in enumerate(off) if flags[o]]
        erec["erased"] += len(flagged)
        out, changed, branch = decode_codeword([row[o] for o in off], P, flagged)
        if branch in ("used", "fallback"):
            erec[branch] += 1
        if out is None:
            rec["failed"] += 1
            continue
        for o, v in zip(off, out):
            row[o] = v
        rec["corrected"] += changed
    if rec["failed"]:
        rec["status"] = R.FAILED
    return bytes(row), rec, erec


def check_frame(before, after, flags, record, erec, h, kind, P):
    """No decoder. Every codeword of the row after the decoder: zero syndromes
    by direct evaluation unless it failed, and a failed one unchanged; a word
    that was clean unchanged; a result with 1 <= f <= P and 2 e + f <= P is the
    first attempt's (it is unique, so the first attempt had to find it); any
    other result changed at most t places (errors only, or the fallback); and
    the two records are the sums."""
    W = len(before)
    flags = list(flags) if flags is not None else [False] * W
    c = C.CRC_BYTES[kind]
    t = P // 2
    length = int.from_bytes(bytes(before[:h]), "big")
    assert erec["reserved"] == 0
    if record["status"] == R.BAD_LENGTH:
        assert length > R.max_len(W, h, c, P)
        assert bytes(before) == bytes(after)
        assert record["codewords"] == record["corrected"] == record["failed"] == 0
        assert erec == dict(erased=0, used=0, fallback=0, reserved=0)
        return
    n = h + length + c
    D = R.codewords(n, P)
    assert record["codewords"] == D
    assert bytes(before[R.frame_size(n, P):]) == bytes(after[R.frame_size(n, P):]), "bytes past n' changed"
    tot = dict(corrected=0, failed=0, erased=0, used=0, fallback=0)
    for j in range(D):
        off = R.offsets(n, P, j)
        r, o = [before[x] for x in off], [after[x] for x in off]
        fl = [flags[x] for x in off]
        f = sum(fl)
        tot["erased"] += f
        changed = sum(a != b for a, b in zip(r, o))
        if not any(R.syndromes(r, P)):
            assert changed == 0, "a clean codeword was changed"
            continue
        if any(R.syndromes(o, P)):
            assert changed == 0, "a failed codeword was changed"
            tot["failed"] += 1
            tot["fallback"] += f >= 1
            continue
        e = sum(a != b for a, b, g in zip(r, o, fl) if not g)
        tot["corrected"] += changed
        if 1 <= f <= P and 2 * e + f <= P:
            tot["used"] += 1
        else:
            assert changed <= t, ("more than t places changed without the flags' help", changed, f)
            tot["fallback"] += f >= 1
    assert (record["corrected"], record["failed"]) == (tot["corrected"], tot["failed"])
    assert record["status"] == (R.FAILED if tot["failed"] else R.OK)
    assert (erec["erased"], erec["used"], erec["fallback"]) == (tot["erased"], tot["used"], tot["fallback"])
