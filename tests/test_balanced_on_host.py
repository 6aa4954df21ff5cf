"""The balanced pair search of full-size verify passes (libeddsa_amd/csrc/halve.h: halve_balanced_lane - pairs (u, v) with both
at most B33 = 0x777...7, 33 nibbles, so that the evaluation runs 33 windows instead of 34), the part that needs no GPU: the
device source compiled for the host with every bound asserted (tests/host_check/balanced_check.cpp) against the integer model
of the rule (tests/balanced_model.py) and against the oracle's verdicts."""
import ctypes

import numpy as np
import pytest

import balanced_model as bm
from balanced_model import B33, CRAFTED, L, N8L, lane_pairs, rows_of
from ed_model import H
from hostlib import build_check

SZ = ctypes.c_size_t
GIVE_UP_CAP = 0.0025          # the condition under which the arrangement is worth its exact-path items; the rule gives 0.0017-0.0019


@pytest.fixture(scope="module")
def balancedcheck(tmp_path_factory):
    h = build_check(tmp_path_factory, "balanced")
    h.bc_violations.restype = ctypes.c_long
    h.bc_first_violation.restype = ctypes.c_char_p
    h.bc_reset()
    return h


def clean(h):
    assert h.bc_violations() == 0, h.bc_first_violation()


def test_b33_is_the_33_window_bound():
    """recoding adds 8 to every nibble: B33 leaves windows 33 .. 63 at digit 0 (nibble 8) with 15 = digit 7 below; B33 + 1 carries
    into window 33"""
    pattern = int("8" * 64, 16)
    digits = lambda x: [((x + pattern) >> (4 * w) & 15) - 8 for w in range(64)]   # noqa: E731
    assert digits(B33) == [7] * 33 + [0] * 31 and B33 == int("7" * 33, 16)
    assert digits(B33 + 1)[33] == 1
    assert B33 * B33 > 1 << 255 > (B33 >> 4) ** 2                                   # the lattice's determinant: 33 windows can hold a pair, 32 cannot hold one for every t


def test_a_million_random_scalars(balancedcheck):
    """10^6 random t below 2^252: every pair the lane returns has u t = v (mod 8 l) in Python integers, u odd, |u| and v <= B33;
    it gives up on at most 0.25 % of them; on the first 20 000 and on every t it gives up on, the integer model agrees item by
    item (found / not found, and the pair)"""
    n = 1000000
    rng = np.random.default_rng(20250133)
    tin = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    tin[:, 31] &= 0x0f
    raw = tin.tobytes()
    out = ctypes.create_string_buffer(48 * n)
    balancedcheck.bc_halve(out, raw, SZ(n))
    rows = rows_of(out.raw, n)
    given_up = []
    for i, (found, u, v) in enumerate(rows):
        if not found:
            given_up.append(i)
            continue
        t = int.from_bytes(raw[32 * i:32 * i + 32], "little")
        assert (u * t - v) % N8L == 0 and u & 1 and abs(u) <= B33 and 0 <= v <= B33, hex(t)
    print("give-ups: %d of %d = %.5f" % (len(given_up), n, len(given_up) / n))
    assert len(given_up) <= GIVE_UP_CAP * n
    ways = {}
    for i in list(range(20000)) + given_up:
        t = int.from_bytes(raw[32 * i:32 * i + 32], "little")
        found, u, v, way, big = bm.balanced_trace(t)
        ways[way] = ways.get(way, 0) + 1
        assert big < 1 << 24                                   # (far from the 31-bit quotients where the model does not apply)
        assert rows[i][0] == found, hex(t)
        if found:
            assert rows[i][1:] == (u, v), hex(t)
    assert ways["none"] >= len(given_up) and min(ways.get(w, 0) for w in ("odd", "before", "partial")) > 500
    # the step after an even cofactor is never the answer: beyond B33 the step before is more than seven times the remainder
    # below 2^128, so a partial step comes first (halve.h)
    assert "after" not in ways
    # most of the way by Lehmer rounds, the rest step by step (cf. test_device_source_on_host.py: test_halved_scalar_pairs)
    counters = (ctypes.c_long * 2)()
    balancedcheck.bc_halve_counters(counters, 1)
    assert counters[0] >= 4 * n and counters[1] <= 12 * n, list(counters)
    clean(balancedcheck)


def test_crafted_scalars(balancedcheck):
    ts = [t for t, _ in CRAFTED] + [N8L // k % L for k in (3, 5, 7, 9, 1000003, (1 << 61) - 1, (1 << 100) + 277, (1 << 125) + 1, (1 << 126) + 3, (1 << 128) + 51)]
    ts += [((1 << 127) * k + 1) % L for k in (2, 6, 10)] + [B33, B33 + 1, B33 + 2, B33 * 16 + 7]
    got = lane_pairs(balancedcheck, ts)
    for t, (found, u, v) in zip(ts, got):
        mf, mu, mv, way, big = bm.balanced_trace(t)
        assert found == mf, hex(t)
        if found:
            assert (u, v) == (mu, mv) and (u * t - v) % N8L == 0 and u & 1 and abs(u) <= B33 and v <= B33, hex(t)
    for (t, want), (found, u, v) in zip(CRAFTED, got):
        if want:
            assert bm.balanced_trace(t)[3] == want and found == (want != "none"), hex(t)
    by_t = {t: row for t, row in zip(ts, got)}
    assert by_t[0] == (True, 1, 0) and by_t[1] == (True, 1, 1)
    assert not by_t[L - 1][0]                                  # 8 l = 8 (l - 1) + 8, then a quotient of 249 bits: given up, as by every search here
    assert by_t[0xcd5e43aa6a59ff1c3f090a6d5b5f703bea3c6313c5fee44556a0184217a8ff5][2] == B33
    assert abs(by_t[0xd57995c7447399ddb97a9ccad81645fe6cf323ab7b81cb32578870752108fd0][1]) == B33
    # B33 + 1 as the step before, B33 + 2 as the deciding cofactor: what the model's walk meets on the way
    t = 0x72e17e74e66215804f091fbbe402dba499977feaa3834dc4531ebf70c12bab0
    r0, r1 = N8L, t
    while r1 >= 1 << 128:
        r0, r1 = r1, r0 % r1
    assert r0 == B33 + 1
    assert abs(bm.balanced_trace(0x6ce7b909a5d0e24431871af5f2124fee40d6a0a30dfd2cf84c2858d9a8ff7fe)[1]) == B33 + 2
    clean(balancedcheck)


def pair_of_digit_words(hd):
    """(u, v) as the 33-window evaluation reads them from an item's digit words (lanes.h: hd)"""
    pattern = int("8" * 64, 16)
    word = lambda k: sum(int(hd[k + j]) << (32 * j) for j in range(8))   # noqa: E731
    return (word(8) - pattern) * (-1 if hd[24] & 1 else 1), word(0) - pattern


def item_verdict(balancedcheck, hostcheck, sig, pub, msg):
    """(verdict, code, (u, v)): the 33-window evaluation's verdict, or the exact path's when the item goes there"""
    hd = (ctypes.c_uint32 * 28)()
    code = balancedcheck.bc_verify(sig, pub, msg, SZ(len(msg)), hd)
    if code & 2:
        return hostcheck.hc_verify_exact(sig, pub, msg, SZ(len(msg))), code, None
    return code & 1, code, pair_of_digit_words(hd)


def test_edges_and_torsion_through_33_windows(balancedcheck, hostcheck, golden):
    """scalars lane + 33-window main lane on the recorded edge and mixed-order vectors: the oracle's verdict, from the evaluation
    whenever it keeps the item and from the exact path otherwise; what the evaluation reads fits 33 windows"""
    kept = 0
    for c in golden("verify_edges.json") + golden("verify_torsion.json"):
        msg = H(c["msg"])
        verdict, code, pair = item_verdict(balancedcheck, hostcheck, H(c["sig"]), H(c["pub"]), msg)
        assert verdict == int(c["accept"]) and not code & 8, c["name"]
        if pair:
            kept += 1
            assert abs(pair[0]) <= B33 and 0 <= pair[1] <= B33 and pair[0] & 1, c["name"]
    assert kept > 350
    clean(balancedcheck)


def test_an_injected_wrong_quotient_never_lets_a_wrong_pair_through(balancedcheck, hostcheck, oracle):
    """the fault injections of the host build (halve.h: halve_fault) against the balanced search: a quotient one too large at the
    n-th working half-step (n > 0; the remainder wraps) or in the n-th cofactor update alone (n < 0; a plausible pair with a
    broken congruence).  The verdict is the oracle's every time; a pair that reaches the 33-window evaluation satisfies the
    congruence in Python integers and the bound; every broken pair the search returns is refused (+ 8) and the item goes long"""
    import hashlib
    sk = bytes(range(1, 33))
    pk = oracle.genpub(sk)
    refused = {1: 0, -1: 0}
    for i in range(40):
        msg = b"balanced fault injection %d" % i
        sig = oracle.sign(sk, pk, msg)
        bad = sig[:45] + bytes([sig[45] ^ 4]) + sig[46:]
        t = int.from_bytes(hashlib.sha512(sig[:32] + pk + msg).digest(), "little") % L
        for s_, want in ((sig, 1), (bad, 0)):
            for sign in (1, -1):
                balancedcheck.bc_halve_fault(sign * (1 + i % 4))
                verdict, code, pair = item_verdict(balancedcheck, hostcheck, s_, pk, msg)
                balancedcheck.bc_halve_fault(0)
                assert verdict == want, (i, sign, code)
                if code & 8:
                    assert code & 2
                    refused[sign] += 1
                if pair:
                    assert (pair[0] * t - pair[1]) % N8L == 0 and abs(pair[0]) <= B33 and 0 <= pair[1] <= B33 and pair[0] & 1, (i, sign)
    print("refused pairs:", refused)
    # n = -1 always fires and always leaves a pair to refuse: the Lehmer rounds stop above 2^129, so a t of 128 bits or more has a
    # working half-step in the plain loop, and a wrong cofactor there is in every pair that follows (ten i, two signatures each)
    assert refused[-1] >= 20, refused
    balancedcheck.bc_reset()                                  # the injected faults tripped the no-borrow assertions, as they must
    for i in range(200):
        msg = b"balanced, no fault %d" % i
        sig = oracle.sign(sk, pk, msg)
        assert balancedcheck.bc_verify(sig, pk, msg, SZ(len(msg)), None) in (1, 2)
    clean(balancedcheck)


def test_the_crafted_give_ups_as_signatures(balancedcheck, hostcheck, oracle):
    """signatures whose t has no balanced pair (searched with the model over one key's signatures): the item goes to the exact
    path, which gives the oracle's verdict for the genuine and for a corrupted signature"""
    import hashlib
    sk = bytes(range(32))
    pk = oracle.genpub(sk)
    hits = 0
    for i in range(20000):
        msg = b"no balanced pair %d" % i
        sig = oracle.sign(sk, pk, msg)
        t = int.from_bytes(hashlib.sha512(sig[:32] + pk + msg).digest(), "little") % L
        if bm.balanced_pair(t)[0]:
            continue
        hits += 1
        assert item_verdict(balancedcheck, hostcheck, sig, pk, msg)[:2] == (1, 2)
        bad = sig[:40] + bytes([sig[40] ^ 1]) + sig[41:]
        assert item_verdict(balancedcheck, hostcheck, bad, pk, msg)[:2] == (0, 2)
        if hits == 3:
            break
    assert hits == 3
    clean(balancedcheck)
