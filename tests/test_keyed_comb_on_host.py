"""Comb key sets (include/eddsa_amd.h: eddsa_amd_keyset_create_comb), the part that needs no GPU: the header and the shipped
library's exports, the argument checks that run before any device is touched, the integer model of the comb's digits and table
entries (tests/keyed_comb_model.py), and the lane steps of k_keyset_comb_build and k_verify_main_comb_keyed
(libeddsa_amd/csrc/keyed_lanes.h) compiled for the host with every bound asserted (tests/host_check/keyed_comb_check.cpp) over the
recorded edge and torsion vectors as ONE comb key set."""
import ctypes
import os
import random
import re

import pytest

import keyed_comb_model as cm
import keyed_model as km
from ed_model import H
from hostlib import ROOT, build_check, declared_names, exported_names, header_text

SZ = ctypes.c_size_t
NAMES = ("eddsa_amd_keyset_create_comb", "eddsa_amd_keyset_create_comb_dev", "eddsa_amd_keyset_is_comb", "eddsa_amd_keyset_bytes")
INVALID_VALUE = 1                                    # hipErrorInvalidValue


def _cases(golden):
    return golden("verify_edges.json") + golden("verify_torsion.json")


@pytest.fixture(scope="module")
def combcheck(tmp_path_factory):
    """tests/host_check/keyed_comb_check.cpp built with the flags of the hostcheck fixture (conftest.py), outside the tree"""
    h = build_check(tmp_path_factory, "keyed_comb")
    h.kcc_violations.restype = ctypes.c_long
    h.kcc_build.restype = ctypes.c_long
    return h


@pytest.fixture(scope="module")
def built(combcheck, golden):
    """the 273 + 192 recorded keys, the out-of-range key and the zero string as one comb key set, entry i = case i's key"""
    cases = _cases(golden)
    assert len(golden("verify_edges.json")) == 273 and len(golden("verify_torsion.json")) == 192
    keys = b"".join(H(c["pub"]) for c in cases) + km.NO_KEY + bytes(32)
    on = combcheck.kcc_build(keys, SZ(len(keys) // 32))
    assert 0 < on < len(keys) // 32                                  # both kinds of key are in the set
    return keys


# ---------------------------------------------------------------- the interface

def test_the_header_declares_the_names_and_the_library_exports_them():
    text = header_text(strip_comments=True)
    assert re.search(r"#define\s+EDDSA_AMD_KEYSET_COMB_MAX_KEYS\s+\(\(size_t\)1\s*<<\s*14\)", text)
    declared = declared_names(text, r"RFC8032_EDDSA_DECL")
    assert set(NAMES) <= declared
    exported = exported_names("libeddsa_amd.so")
    assert set(NAMES) <= exported
    assert "eddsa_amd_debug_keyset_comb_read" not in exported        # the read-back hook is the debug library's alone
    debug_h = open(os.path.join(ROOT, "include", "eddsa_amd_debug.h")).read()
    assert "eddsa_amd_debug_keyset_comb_read(const eddsa_amd_keyset *ks, size_t key, uint32_t *words)" in debug_h


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*", " ", header_text()).split())        # (a phrase may run over the comment's line break)
    for phrase in ("88 KiB of HBM per key", "EDDSA_AMD_KEYSET_COMB_MAX_KEYS = 2^14 keys", "1.375 GiB", "in every mode",
                   "at every size", "S mod l", "there is no new verify entry point", "under both equations",
                   "profiles/verify_keyed_comb.txt"):
        assert phrase in text, phrase


def test_the_layout_names_the_sizes_once_and_the_launcher_lives_in_edk_keyed():
    layout = open(os.path.join(ROOT, "libeddsa_amd", "csrc", "edk_layout.h")).read()
    assert len(re.findall(r"#define\s+KEYSET_COMB_ENTRIES\b", layout)) == 1 and len(re.findall(r"#define\s+KEYSET_COMB_WORDS\b", layout)) == 1
    assert "KEYSET_COMB_WORDS * 4 == 704 * 128" in layout
    kernels_h = open(os.path.join(ROOT, "libeddsa_amd", "csrc", "eddsa_kernels.h")).read()
    assert "edk_keyset_comb_build" not in kernels_h
    assert re.search(r"const uint32_t\*\s*ks_comb;[^}]*}\s*edk_verify_src;", kernels_h, flags=re.S)   # the last field
    assert "edk_keyset_comb_build(" in open(os.path.join(ROOT, "libeddsa_amd", "csrc", "edk_keyed.h")).read()
    assert cm.ENTRIES == 704 and cm.ENTRIES * cm.ENTRY_WORDS * 4 == 88 * 1024


def test_create_comb_checks_its_arguments_before_any_device_is_touched():
    """count == 0, count above the comb's limit (2^14 + 1, 2^63), out == NULL and keys == NULL: -hipErrorInvalidValue, *out left
    NULL - on a machine without a GPU too, which shows that no device was asked"""
    lib = ctypes.CDLL(os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd.so"))
    keys = (ctypes.c_uint8 * 64)()
    for fn, extra in ((lib.eddsa_amd_keyset_create_comb, ()), (lib.eddsa_amd_keyset_create_comb_dev, (ctypes.c_void_p(0),))):
        for k, count in ((keys, 0), (keys, (1 << 14) + 1), (None, 2), (keys, 2**63), (keys, 1 << 20)):
            out = ctypes.c_void_p(0xdead)
            assert fn(ctypes.byref(out), k, SZ(count), *extra) == -INVALID_VALUE
            assert out.value is None
        assert fn(None, keys, SZ(2), *extra) == -INVALID_VALUE
    lib.eddsa_amd_keyset_bytes.restype = ctypes.c_size_t
    assert lib.eddsa_amd_keyset_bytes(None) == 0 and lib.eddsa_amd_keyset_is_comb(None) == 0


# ---------------------------------------------------------------- the integer model

def _edge_scalars():
    """0, 1, l - 1, and the scalars below l with as many digits at the ends of the range as fit: digits 0..41 all 31 or all -32
    under top digits that keep 0 <= t < l (44 digits of 31 are 2^263, 44 of -32 are negative: no such t exists)"""
    out = [0, 1, cm.L - 1]
    for low in (31, -32):
        base = cm.digits_value([low] * 42)
        for top in range(-32 * 64 - 32, 31 * 64 + 32):
            t = base + (top << (cm.COMB_W * 42))
            if 0 <= t < cm.L:
                out.append(t)
    assert len(out) >= 3 + 2                                         # (2^252 = 64^42: the top digits are (0, 0) or (1, 0))
    return out


def test_the_comb_digits_sum_back_and_stay_in_range(combcheck):
    rng = random.Random(5)
    ts = _edge_scalars() + [rng.randrange(cm.L) for _ in range(10000)]
    saw = set()
    for n, t in enumerate(ts):
        d = cm.digits(t)
        assert len(d) == 44 and all(-32 <= x <= 31 for x in d) and cm.digits_value(d) == t
        saw.update(d)
        if n < 2000:                                                 # the lane cuts the same digits from both kinds of digit words
            for pat in (0x88888888, 0x80008000):
                out = (ctypes.c_int8 * 44)()
                combcheck.kcc_digits(out, t.to_bytes(32, "little"), ctypes.c_uint32(pat))
                assert list(out) == d, hex(t)
    assert saw == set(range(-32, 32))
    assert combcheck.kcc_violations() == 0


def test_table_entries_are_multiples_of_minus_a():
    """entry (row, m) = m * 4096^row * (-A) as an affine point; a small-order key has the neutral element among them"""
    rng = random.Random(7)
    b = (15112221349535400772501151409588531511454012693041857206046113283949847762202,
         46316835694926478169428394003475163141307993866256225615783033603165251855960)
    neg_a = cm.mul(rng.randrange(cm.L), b)
    for row, m in ((0, 1), (0, 32), (21, 1), (21, 32), (7, 13)):
        q = neg_a
        for _ in range(12 * row):
            q = cm.add(q, q)
        want = cm.NEUTRAL
        for _ in range(m):
            want = cm.add(want, q)                                   # the affine law, step by step
        assert cm.entry(neg_a, row, m) == want
    assert cm.entry(neg_a, 1, 1) == cm.mul(64, cm.mul(64, neg_a))
    order4 = cm.decode_neg(bytes(32))                                # (sqrt(-1), 0) up to sign
    assert order4 is not None and cm.mul(4, order4) == cm.NEUTRAL and cm.entry(order4, 0, 4) == cm.NEUTRAL and cm.entry(order4, 3, 9) == cm.NEUTRAL
    assert cm.decode_neg(km.NO_KEY) is None


# ---------------------------------------------------------------- the lanes on the host

SAMPLE = [(0, 1), (0, 32), (21, 1), (21, 32), (0, 2), (1, 1), (10, 17), (20, 31)]


def test_the_built_comb_matches_the_model(combcheck, built):
    """every key of the two files, the out-of-range key and the zero string: rows 0 and 21, m = 1 and 32 and a sample between;
    a key that decodes to no point has entries too (what ge_frombytes yields), which nothing compares"""
    compared = 0
    for k in range(len(built) // 32):
        neg_a = cm.decode_neg(built[32 * k:32 * k + 32])
        assert (neg_a is not None) == bool(combcheck.kcc_on_curve(SZ(k))), k
        if neg_a is None:
            continue
        for row, m in SAMPLE:
            words = (ctypes.c_uint32 * 32)()
            combcheck.kcc_entry(words, SZ(k), row, m)
            assert cm.entry_point(list(words)) == cm.entry(neg_a, row, m), (k, row, m)
        compared += 1
    assert compared > 400
    assert combcheck.kcc_violations() == 0


@pytest.mark.parametrize("order", ["arange", "shuffled"])
def test_recorded_verdicts_through_the_comb_lane(combcheck, golden, order):
    """the 273 + 192 recorded cases (S + k l, S = 2^256 - 1, small-order keys and non-canonical encodings among them) as ONE comb
    key set: prepare, comb lane and finish return the recorded verdicts; off-curve keys go through the exact path"""
    cases = _cases(golden)
    place = list(range(len(cases)))
    if order == "shuffled":
        random.Random(11).shuffle(place)                             # entry place[i] holds case i's key
    keys = bytearray(32 * len(cases))
    for i, c in enumerate(cases):
        keys[32 * place[i]:32 * place[i] + 32] = H(c["pub"])
    combcheck.kcc_build(bytes(keys), SZ(len(cases)))
    exact = 0
    for i, c in enumerate(cases):
        msg, sig = H(c["msg"]), H(c["sig"])
        got = combcheck.kcc_verify(ctypes.c_uint32(place[i]), sig, msg, SZ(len(msg)))
        assert got & 1 == int(c["accept"]), c["name"]
        exact += (got & 2) != 0
    assert 0 < exact < len(cases)
    for idx in (len(cases), 0xFFFFFFFF):                             # no key: rejected, nothing of the set read
        assert combcheck.kcc_verify(ctypes.c_uint32(idx), H(cases[0]["sig"]), H(cases[0]["msg"]), SZ(len(H(cases[0]["msg"])))) == 0
    assert combcheck.kcc_violations() == 0


def test_the_comb_lane_computes_verify_main_lanes_point(combcheck, built):
    """2 000 random (t, S, key), keys on the curve (small-order ones included): S B + t (-A) from the two combs is the projective
    point the 64-window chain gives"""
    rng = random.Random(13)
    on = [k for k in range(len(built) // 32) if combcheck.kcc_on_curve(SZ(k))]
    for n in range(2000):
        t, s = rng.randrange(cm.L), rng.randrange(cm.L)
        if n < 8:
            t, s = ((0, 0), (0, 1), (1, 0), (cm.L - 1, cm.L - 1), (cm.L - 1, 0), (0, cm.L - 1), (1, 1), (2**252, 2**252))[n]
        k = rng.choice(on)
        assert combcheck.kcc_same_point(ctypes.c_uint32(k), t.to_bytes(32, "little"), s.to_bytes(32, "little")) == 1, (k, hex(t), hex(s))
    assert combcheck.kcc_violations() == 0
