"""Without a GPU: the reference plumbing of the coded modes (tests/rx_ref.py
takes a mode directly) and the fixture conditions of the GPU tests that hold
the stages behind the decode in every mode (tests/test_gpu_fec_stages.py,
test_collect_modes of tests/test_gpu_rx.py), on the reference alone.

The fixture conditions are what makes those tests bite: a device check that
took another span than the mode's gives another `covered` vector on the very
rows the GPU test uses (so check, kept, body and summary differ), and a
collect that did gives another hold. The other spans are the ones a per-mode
slip would produce (test_gpu_fec_stages.alt_spans).
"""
import numpy as np
import pytest

import fec_modes_ref as Z
import frames_check_ref as C
import frames_fec_ref as X
import frames_ref as F
import rx_ref as RX
import test_gpu_fec_stages as TS
import test_gpu_frames_fec as TF
import test_gpu_rx as TR

KINDS = (C.CRC16, C.CRC32)


# ---- 1. the plumbing ---------------------------------------------------------------------------

def test_modes_0_and_1_are_unchanged():
    """span, row_symbols and sizes at fec 0 and 1 give what they gave before
    they took a mode: the plain byte count and frames_fec_ref's closed forms."""
    for h in (1, 2):
        for kind in KINDS:
            c = C.CRC_BYTES[kind]
            for bits in (1, 2, 3, 4):
                for length in list(range(0, 12)) + [38, 40, 255]:
                    assert RX.span(length, bits, h, kind, 0) == C.frame_symbols(h + length + c, bits)
                    assert RX.span(length, bits, h, kind, 1) == X.coded_symbols(length, h, kind, bits)
                for max_len in (0, 3, 7, 40):
                    assert RX.row_symbols(h, kind, 0, bits, max_len) == C.frame_symbols(h + max_len + c, bits)
                    assert RX.row_symbols(h, kind, 1, bits, max_len) == \
                        min(N for N in range(1, 800) if (X.row_shape(N, bits, h, kind) or (0, 0, -1))[2] >= max_len)
                for N in range(150 // bits, 420, 13):
                    assert Z.row_shape(N, bits, h, kind, 1) == X.row_shape(N, bits, h, kind)
                    if X.row_shape(N, bits, h, kind) is None:
                        continue
                    St, Bd, max_len = X.row_shape(N, bits, h, kind)
                    got = RX.sizes(1 << bits, 4, 65, 16, N, h, kind, 1, 7, 5000)
                    assert (got["max_len"], got["row_bytes"]) == (max_len, Bd)
                    assert got["decode_work_bytes"] == 65 * 7 * St * 8
                    assert got["bodies_bytes"] == 65 * 7 * max_len


@pytest.mark.parametrize("fec", Z.MODES)
def test_sizes_every_mode(A, fec):
    """demod_rx_sizes against rx_ref.sizes with the mode: the row width and
    max_len every later stage gets (47 or 63 bytes wide interleaved where rate
    1/2 has 43), the decode workspace by the mode's step count."""
    for freqs, h, kind in ((F.FSK2, 1, C.CRC16), (F.FSK8, 2, C.CRC32)):
        K, R, L = len(freqs), 4, 16
        bits = F.bits_per_symbol(K)
        cfg = A.make_cfg(n=1024, hop=256, freqs=freqs)
        N0 = Z.symbols_for(40, bits, h, kind, fec)
        for N, S, mf in ((N0, 1, 5), (N0 + 1, 65, 130), (N0 + 85, 20000, 3)):
            ring = RX.min_ring(L, N, R)
            got = A.rx_sizes(cfg, A.make_rx_cfg(np.arange(L) % K, 1, N, h, kind, fec, mf, ring), S)
            assert got == RX.sizes(K, R, S, L, N, h, kind, fec, mf, ring), (hex(fec), K, N, S)
            assert got["decode_work_bytes"] == A.fec_decode_workspace_size(cfg, S, mf, N, fec)
    widths = {f: Z.row_shape(Z.symbols_for(40, 1, 1, C.CRC16, f), 1, 1, C.CRC16, f)[1] for f in Z.MODES}
    assert widths == {0x01: 43, 0x11: 43, 0x21: 43, 0x41: 47, 0x51: 63, 0x61: 47}


def test_spans_of_the_modes():
    """The spans the fixtures rely on, counted: 40- and 30-byte frames at 1 bit
    a symbol (h 1, CRC-16), and one block at 3 bits ending inside a symbol."""
    assert [Z.span(40, 1, 1, C.CRC16, f) for f in Z.MODES] == [700, 525, 467, 768, 768, 512]
    assert [Z.span(30, 1, 1, C.CRC16, f) for f in Z.MODES] == [540, 405, 360, 768, 512, 512]
    assert Z.span(0, 3, 1, C.CRC16, 0x41) == 86
    for f in Z.MODES:
        for n in (0, 30, 40):
            assert RX.span(n, 1, 1, C.CRC16, f) == Z.span(n, 1, 1, C.CRC16, f)


def test_receiver_takes_a_mode():
    """rx_ref.Rx in a mapped mode, no swap of module functions: in mode 0x11 a
    frame that touches the end of the one before (405 symbols behind its word,
    where the rate-1/2 span has 540) is kept, and hold is its own end."""
    fec, K, R, h, kind, L = 0x11, 2, 2, 1, C.CRC16, 16
    rng = np.random.default_rng(5)
    word = rng.integers(0, K, L).astype(np.uint8)
    N = RX.row_symbols(h, kind, fec, 1, 30)
    a, b = bytes(range(30)), b"touching"
    assert (RX.span(30, 1, h, kind, fec), X.coded_symbols(30, h, kind, 1)) == (405, 540)
    fa, fb = RX.frame_symbols(a, word, 1, h, kind, fec), RX.frame_symbols(b, word, 1, h, kind, fec)
    assert len(fa) == L + 405
    symbols = np.concatenate([rng.integers(0, K, 7).astype(np.uint8), fa, fb,
                              rng.integers(0, K, N + 9).astype(np.uint8)])
    sym, P = RX.windows_of(symbols, K, R, 1, rng)
    rx = RX.Rx(1, K, R, word, 0, N, h, kind, fec, 8, len(sym) + 64)
    fr, bodies, summ = rx.push([(sym, P)])
    assert bodies == [a, b] and fr["window"].tolist() == [1 + 7 * R, 1 + (7 + len(fa)) * R]
    assert int(rx.state["hold"][0]) == 1 + (7 + len(fa) + len(fb)) * R
    assert RX.Rx(1, K, R, word, 0, N, h, kind, fec, 8, len(sym) + 64).push([(sym, P)])[1] == bodies
    assert RX.one_shot(sym, P, R, word, 0, N, h, kind, fec) == [(int(f["window"]), 0, d) for f, d in zip(fr, bodies)]


# ---- 2. the coded check's fixtures ----------------------------------------------------------------

def group_under(case, g, Rn, h, kind, span):
    nw = min(case["counts"][g], case["hits"].shape[1])
    return TS.covered_under(case["hits"]["window"][g, :nw], case["rows"][g, :nw], TS.L0, Rn, h, kind, span)


@pytest.mark.parametrize("fec,K,Rn,h,kind", TS.CHECK_CASES)
def test_check_fixture(fec, K, Rn, h, kind):
    """On the rows test_coded_check_modes uses: `covered` under the mode's span
    differs from `covered` under (a) the rate-1/2 span, (b) the kept bits
    without block rounding and (c) block rounding without puncturing, wherever
    that span differs from the mode's at one of the lengths; each placement
    gives what it is named for; at least four rows covered and four kept."""
    case = TS.check_case(fec, K, Rn, h, kind)
    bits, gaps = case["bits"], case["gaps"]
    chk, kept, bodies, summ = C.check_group(case["hits"]["window"][0, :case["counts"][0]],
                                            case["rows"][0, :case["counts"][0]], TS.L0, Rn,
                                            Z.span_of(bits, h, kind, fec), None, h, kind)
    cov = chk["covered"]
    own = group_under(case, 0, Rn, h, kind, lambda n: Z.span(n, bits, h, kind, fec))
    assert np.array_equal(own, cov)
    assert int(cov.sum()) >= 4 and len(kept) >= 4 and len(kept) + int(cov.sum()) == int(summ["n_valid"])
    for i, gap in enumerate(gaps):
        if gap in ("first", "touch", "past", "behind long", "behind invalid"):
            assert chk["status"][i] == C.OK and not cov[i], (i, gap)
        elif gap == "inside":
            assert chk["status"][i] == C.OK and cov[i], (i, gap)
    assert chk["status"][gaps.index("long")] == C.BAD_LENGTH and chk["length"][gaps.index("long")] == \
        case["rows"].shape[2] - h - C.CRC_BYTES[kind] + 1
    assert chk["status"][gaps.index("invalid")] == C.BAD_CRC
    names = set()
    for n in case["lens"]:
        for name, alt in TS.alt_spans(n, bits, h, kind, fec).items():
            if alt != Z.span(n, bits, h, kind, fec):
                names.add(name)
    if fec == 0x01:
        assert not names                                  # the control: every alternative is its own span
    else:
        assert "a" in names and (not fec & Z.INTERLEAVE or fec == 0x41 or {"b", "c"} <= names)
        assert fec != 0x41 or TS.alt_spans(30, bits, h, kind, fec)["b"] == TS.alt_spans(30, bits, h, kind, fec)["a"]
    for name in sorted(names):
        other = group_under(case, 0, Rn, h, kind, lambda n: TS.alt_spans(n, bits, h, kind, fec)[name])
        differ = np.flatnonzero(other != cov)
        assert differ.size >= 1, (hex(fec), name)
        assert {gaps[i] for i in differ} >= {"between " + name}, (hex(fec), name, {gaps[i] for i in differ})


def test_check_fixture_tells_0x41_from_0x51():
    """Their spans coincide at 40 bytes (768 symbols at 1 bit): the cases hold
    lengths where they differ, and `covered` differs there."""
    K, Rn, h, kind = 2, 1, 1, C.CRC16
    for fec, other in ((0x41, 0x51), (0x51, 0x41)):
        case = TS.check_case(fec, K, Rn, h, kind)
        assert Z.span(40, 1, h, kind, fec) == Z.span(40, 1, h, kind, other)
        assert any(Z.span(n, 1, h, kind, fec) != Z.span(n, 1, h, kind, other) for n in case["lens"])
        a = group_under(case, 0, Rn, h, kind, lambda n: Z.span(n, 1, h, kind, fec))
        b = group_under(case, 0, Rn, h, kind, lambda n: Z.span(n, 1, h, kind, other))
        assert not np.array_equal(a, b)


@pytest.mark.parametrize("fec", Z.NEW_MODES)
def test_groups_fixture(fec):
    """test_coded_check_groups' 65 groups: an empty one, one stored above
    max_frames, every status, covered and kept rows; under the rate-1/2 span
    `covered` differs in some group; and rows read at another mode's width
    (the groups laid 43, 47 or 63 bytes apart) give other statuses."""
    g = TS.GROUPS_SHAPE
    Rn, h, kind, mf = g["Rn"], g["h"], g["kind"], g["max_frames"]
    case = TS.groups_case(fec)
    bits = case["bits"]
    assert case["counts"][1] == 0 and case["counts"][2] > mf and len(case["counts"]) == 65
    want, refs = TS.expected(case, Rn, h, kind, fec, 0xFF)
    status = np.concatenate([r[0]["status"] for r in refs])
    cov = np.concatenate([r[0]["covered"] for r in refs])
    assert {C.OK, C.BAD_CRC} <= set(status.tolist()) and cov.sum() >= 4 and sum(len(r[1]) for r in refs) >= 4
    half = [group_under(case, s, Rn, h, kind, lambda n: X.coded_symbols(n, h, kind, bits)) for s in range(65)]
    assert any(not np.array_equal(a, r[0]["covered"]) for a, r in zip(half, refs))
    Bd = case["rows"].shape[2]
    for wrong in {43, 47, 63} - {Bd}:
        flat = case["rows"].reshape(-1)
        n = flat.size // (mf * wrong)
        again = np.resize(flat, (max(n, 65), mf, wrong))[:65]     # what a kernel with that row pitch would see
        wrong_status = [C.check_row(again[s, i], h, kind)[2]
                        for s in range(3, 65) for i in range(min(case["counts"][s], mf))]
        right_status = [int(v) for s in range(3, 65) for v in refs[s][0]["status"]]
        assert wrong_status != right_status, (hex(fec), wrong)


# ---- 3. the collect's fixtures ---------------------------------------------------------------------

@pytest.mark.parametrize("S,mf,K", TR.COLLECT_MODE_CASES)
@pytest.mark.parametrize("fec", Z.NEW_MODES)
def test_collect_fixture(fec, S, mf, K):
    """On the inputs test_collect_modes uses: the new hold differs from the one
    the rate-1/2 span gives (and from the ones of the other alternative spans)
    for at least one stream, and at least one emitted record has its length
    clamped at the mode's max_len, which is the counted one."""
    c = TR.collect_case(S, mf, K, fec, TR.collect_seed(S, mf, K, fec), TR.MODE_LEN)
    bits, h, kind = c["bits"], c["h"], c["kind"]
    assert c["N"] == Z.symbols_for(TR.MODE_LEN, bits, h, kind, fec)
    assert c["max_len"] == Z.row_shape(c["N"], bits, h, kind, fec)[2] >= TR.MODE_LEN
    state, frames, bodies, summary = TR.collect_reference(c, fec)
    half = TR.collect_reference(c, 1)[0]
    moved = state["hold"] != c["state"]["hold"]
    assert moved.any() and (state["hold"][moved] != half["hold"][moved]).any()
    assert (state["hold"] != half["hold"]).any()
    n = int(summary["n_frames"])
    assert n >= 1
    fr = frames[:n]
    assert (fr["length"] <= c["max_len"]).all() and (fr["length"] == c["max_len"]).any()
    clamped = 0
    for s in range(S):
        nk = min(int(c["summ"]["n_kept"][s]), mf)
        for r in range(nk):
            i = int(c["kept"][s, r])
            if i < mf and int(c["state"]["base"][s]) + int(c["hits"]["window"][s, i]) >= int(c["state"]["hold"][s]):
                clamped += int(c["check"]["length"][s, i]) == c["max_len"] + 9
    assert clamped >= 1


@pytest.mark.parametrize("fec", Z.NEW_MODES)
def test_collect_bites(fec, monkeypatch):
    """A collect that took one of the alternative spans leaves another hold on
    test_collect_modes' inputs: the reference run with that span (the only
    place this module replaces a function of the reference) differs in the
    state the GPU test compares whole."""
    S, mf, K = 65, 130, 2
    c = TR.collect_case(S, mf, K, fec, TR.collect_seed(S, mf, K, fec), TR.MODE_LEN)
    right = TR.collect_reference(c, fec)[0]
    names = [k for k, v in TS.alt_spans(TR.MODE_LEN, c["bits"], c["h"], c["kind"], fec).items()
             if v != Z.span(TR.MODE_LEN, c["bits"], c["h"], c["kind"], fec)]
    assert "a" in names
    for name in names:
        monkeypatch.setattr(RX, "span", lambda length, bits, h, kind, f, name=name:
                            TS.alt_spans(length, bits, h, kind, f)[name])
        wrong = TR.collect_reference(c, fec)[0]
        monkeypatch.undo()
        assert (wrong["hold"] != right["hold"]).any(), (hex(fec), name)
        for f in ("base", "dropped", "cut_hits", "fill", "keep"):
            assert np.array_equal(wrong[f], right[f])


# ---- 4. the end-to-end fixture -----------------------------------------------------------------------

@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("fec", Z.NEW_MODES)
def test_e2e_wrong_symbols_are_corrected(fec, K):
    """The rows test_frames_coded_modes sends, on clean powers (six draws and
    saturated ones): the reference's decode recovers all five frames with the
    wrong-tone symbols of test_gpu_fec_stages.E2E_WRONG, three where no entry
    reduces them."""
    truth, word, N, at, datas, sent, wrong = TS.e2e_symbols(K, fec)
    assert wrong == TS.E2E_WRONG.get((fec, K), 3)
    bits, h, kind = F.bits_per_symbol(K), TS.E2E_H, TS.E2E_KIND
    Bd = Z.row_shape(N, bits, h, kind, fec)[1]
    for f, a in enumerate(at):
        Sc = Z.span(len(datas[f]), bits, h, kind, fec)
        hard = truth[a + TS.E2E_L:a + TS.E2E_L + Sc]
        assert int((hard != sent[f][:Sc]).sum()) == (wrong if f in TS.E2E_HIT else 0)
    windows = np.array(at, np.uint64) * 4
    for seed in range(7):
        P = TF.powers_for(truth, K, np.random.default_rng(seed))
        if seed == 6:
            P = np.where(P >= 1000, 1000.0, 1.0).astype(np.float32)
        soft = X.soft_bits(P)
        q = np.stack([soft[a + TS.E2E_L:a + TS.E2E_L + N].reshape(-1) for a in at])
        written, dec = Z.decode_rows(q, h, kind, fec)
        rows = np.zeros((len(at), Bd), np.uint8)
        for i, b in enumerate(written):
            rows[i, :len(b)] = np.frombuffer(b, np.uint8)
        chk, kept, bodies, summ = C.check_group(windows, rows, TS.E2E_L, 4, Z.span_of(bits, h, kind, fec), None, h,
                                                kind)
        assert bodies == datas and kept.tolist() == list(range(5)), seed
