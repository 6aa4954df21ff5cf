"""Every evaluation of verification on CHOSEN scalars (tests/crafted_scalars.py: the digest forms let the caller pick
t = digest mod l), the part that needs no GPU: what the set covers, from the integer models alone, and the device source compiled
for the host with every bound asserted (tests/host_check/crafted_check.cpp) - the full-length chain, the three half-length
chains in their short loop and inside a long wave, and the comb - against the models' verdicts, pairs and digit words.
tests/test_gpu_crafted_scalars.py runs the same set through the kernels."""
import ctypes

import pytest

import crafted_scalars as cs
from balanced_model import B33
from ed_model import L
from hostlib import build_check

PAT4, PAT16 = int("8" * 64, 16), int("8000" * 16, 16)
BITS = {"h134": 134, "h138": 138, "bal": 131}       # the template argument of verify_half_scalars_lane (halve.h)
U_NEGATIVE, LONG = 1, 2                              # lanes.h: the status word


@pytest.fixture(scope="module")
def crafted():
    return cs.build()


@pytest.fixture(scope="module")
def craftedcheck(tmp_path_factory):
    h = build_check(tmp_path_factory, "crafted")
    h.cc_violations.restype = ctypes.c_long
    h.cc_first_violation.restype = ctypes.c_char_p
    return h


def clean(h):
    assert h.cc_violations() == 0, h.cc_first_violation()


def what(it):
    return "%s: t = %#x, S = %#x, key %d" % (it.kind, it.t, it.s, it.key)


# ---------------------------------------------------------------- the set itself

def test_the_scalars_are_the_listed_ones():
    named, pats, rand = cs.scalars()
    values = [v for _, v in named]
    assert len(set(values)) == len(values) and all(0 <= v < L for v in values) and len(rand) == 200 and len(values) >= 400
    for w, count in ((4, 64), (6, 43), (16, 16)):
        mx, mn = (1 << (w - 1)) - 1, -(1 << (w - 1))
        got = dict(cs.pattern_scalars(w))
        assert len(got) == 4 + 2 * count
        top = cs.reachable(w)
        assert cs.digits(got["w%d all max" % w], w)[:top + 1] == [mx] * top + [0]
        assert cs.digits(got["w%d all min" % w], w)[:top + 1] == [mn] * top + [1]
        for name in ("min/max", "max/min"):
            d = cs.digits(got["w%d %s" % (w, name)], w)
            n = cs.top_nonzero(d) + 1
            assert n >= top - 1 and set(d[:n:2]) | set(d[1:n:2]) == {mn, mx} and len(set(d[:n:2])) == len(set(d[1:n:2])) == 1
        for i in range(top):
            assert cs.digits(got["w%d max at %d" % (w, i)], w)[i] == mx and cs.digits(got["w%d min at %d" % (w, i)], w)[i:i + 2] == [mn, 1]
    # the digits are those of the models the kernels are held against
    for v in values[::7]:
        assert cs.comb_digits(v) == cs.digits(v, 6, 44) and sum(d << (4 * i) for i, d in enumerate(cs.nibbles(v))) == v


def test_every_item_has_the_verdict_it_was_built_for(crafted):
    """build() asserts it item by item (valid: accepted, near miss: rejected, under the default rule, by ed_model.verify_t); here:
    both kinds are there in numbers, the digests reduce to the chosen t, the keys are the six"""
    items, rep = crafted
    assert rep["items"] == len(items) <= cs.MAX_ITEMS and rep["valid"] >= 1000 and rep["near"] >= 64 * len(cs.ROUTES)
    assert all(it.accept == it.valid for it in items)
    assert all(int.from_bytes(it.digest, "little") % L == it.t for it in items)
    assert {int.from_bytes(it.digest, "little") // L == 0 for it in items} == {True, False}
    assert any(int.from_bytes(it.digest, "little") + L >= 1 << 512 for it in items)
    assert sum(it.s >= L for it in items if it.valid) >= 16 and {it.key for it in items} == set(range(6))
    assert [k[3] for k in cs.keys()] == ["honest"] * 4 + ["a B + T8", "a B + T2"]
    for route in cs.ROUTES:
        kinds = {it.kind for it in items if it.kind.startswith(route + ":")}
        assert len(kinds) >= 6, (route, kinds)
    # the strict rules and the cofactored equation tell the classes apart: S + l and the keys of mixed order; R + a small point
    import policy_model as pm
    strict = cs.verdicts(items, policy=pm.STRICT)
    assert 0 < strict.sum() < rep["valid"]
    tors = [it for it in items if it.kind == "R + a point of small order"]
    assert len(tors) == 14 and cs.verdicts(tors, cofactored=True).all() and not cs.verdicts(tors).any()


def test_coverage_from_the_models_alone(crafted):
    """conditions, not measurements: what the windowed kernels have to see at least once"""
    items, rep = crafted
    every = set(range(-8, 8))
    for route, (bound, windows) in cs.HALF.items():
        r = rep[route]
        assert r["v digits"] == every, route
        assert r["top window of v"] >= 3 and r["u < 0"] >= 20 and r["no pair"] >= 3, (route, r)
    assert rep["bal"]["v = B33"] >= 1 and rep["bal"]["|u| = B33"] >= 1 and rep["bal"]["max |u|"] == B33
    # The searches below 2^134 / 2^138 promise |u| < 2^bits.  A pair from the FIRST remainder below the bound has |u| < 2^(256 -
    # bits) (|u| times the remainder before it is below 8 l), so its top windows are empty; a pair from the second look, after an
    # even cofactor, can be up to 2^bits - and the set holds one whose |u| reaches window 33 of the 34
    assert rep["h134"]["max |u|"] < 1 << 134 and rep["h138"]["max |u|"] < 1 << 138
    for route in ("h134", "h138"):
        bound = cs.HALF[route][0]
        for t in {it.t for it in items}:
            u, v, found, _ = cs.pair_of(route, t)
            if found and t >= 1 << bound:
                r0, r1 = 8 * L, t
                while r1 >= 1 << bound:
                    r0, r1 = r1, r0 % r1
                assert abs(u) < 1 << (256 - bound) or r1 != v, hex(t)
    assert any(cs.nibbles(abs(cs.pair_of("h134", it.t)[0]))[33] for it in items)
    assert rep["t window 0"] == every and rep["t window 63"] == {0, 1} and rep["t all 7"] and rep["t all -8"]
    assert rep["S halfwords"] == [] and rep["S comb"] == [] and rep["t comb"] == []


# ---------------------------------------------------------------- the device source on the host

def expected_hd(route, it):
    """the digit words and the status word of lanes.h: verify_half_scalars_lane by the models -> the list of acceptable
    (words 0..7, 8..15, 16..23, status): one, or two where the walk has a quotient the model does not cover"""
    u, v, found, sure = cs.pair_of(route, it.t)
    s = it.s % L
    long_form = (it.t + PAT4, 1 + PAT4, s + PAT16, LONG)
    if not found:
        return [long_form]
    short_form = (v + PAT4, abs(u) + PAT4, abs(u) * s % L + PAT16, U_NEGATIVE if u < 0 else 0)
    return [short_form] if sure else [short_form, long_form]


def test_every_chain_on_every_item(crafted, craftedcheck):
    """the verdict of each chain = the model's for every item of the set; a hand-off to the exact path where the chain has one;
    the half-length digit words = the model's pair, s' = |u| S mod l and status; no pair refused, no bound violated"""
    items, _ = crafted
    h = craftedcheck
    assert h.cc_comb_build(cs.key_bytes().tobytes(), ctypes.c_size_t(6)) == 6
    hd = (ctypes.c_uint32 * 28)()
    word = lambda k: sum(int(hd[k + j]) << (32 * j) for j in range(8))   # noqa: E731
    wrong, handed = [], {r: 0 for r in cs.HALF}
    for it in items:
        want = int(it.accept)
        if h.cc_full(it.sig, it.pub, it.digest) != want:
            wrong.append(("full-length", what(it)))
        if h.cc_comb(it.key, it.sig, it.digest) != want:
            wrong.append(("comb", what(it)))
        for route, bits in BITS.items():
            for in_long_wave in (0, 1):
                code = h.cc_half(bits, it.sig, it.pub, it.digest, in_long_wave, hd)
                got = (word(0), word(8), word(16), int(hd[24]))
                forms = expected_hd(route, it)
                if got not in forms or any(hd[25:28]):
                    wrong.append((route + ": digit words", what(it)))
                    continue
                is_long = bool(got[3] & LONG)
                if route == "bal" and is_long and not in_long_wave:
                    handed[route] += 1
                    if code != 2:
                        wrong.append((route + ": no hand-off", what(it)))
                elif code != want + (4 if is_long else 0):
                    wrong.append(("%s%s: code %d" % (route, ", in a long wave" if in_long_wave else "", code), what(it)))
    assert not wrong, (len(wrong), wrong[:5])
    assert handed["bal"] >= 3
    clean(h)
