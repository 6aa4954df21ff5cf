"""Key-set verification (include/eddsa_amd.h: eddsa_amd_keyset, ed25519_verify_keyed), the part that needs no GPU: the header
and the shipped library's exports, the argument checks that run before any device is touched, the lane steps of the keyed
kernels (libeddsa_amd/csrc/keyed_lanes.h, keyed_kernels.h) compiled for the host with every bound asserted
(tests/host_check/keyed_check.cpp) over the recorded edge and torsion vectors with tab_a read from ONE shared table, the key
bytes of an out-of-range item, and the integer model of the pair search that the GPU tests rely on (tests/keyed_model.py)."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import keyed_model as km
import ed_model as em
from ed_model import D, H, P, le
from hostlib import ROOT, build_check, declared_names, exported_names, header_text

SZ = ctypes.c_size_t
NAMES = ("eddsa_amd_keyset_create", "eddsa_amd_keyset_create_dev", "eddsa_amd_keyset_destroy", "eddsa_amd_keyset_count",
         "eddsa_amd_keyset_device", "ed25519_verify_keyed", "ed25519_verify_keyed_dev")
INVALID_VALUE = 1                                    # hipErrorInvalidValue


@pytest.fixture(scope="module")
def keyedcheck(tmp_path_factory):
    """tests/host_check/keyed_check.cpp built with the flags of the hostcheck fixture (conftest.py), outside the tree"""
    h = build_check(tmp_path_factory, "keyed")
    h.kc_violations.restype = ctypes.c_long
    h.kc_build.restype = ctypes.c_long
    return h


# ---------------------------------------------------------------- the interface

def test_the_header_declares_the_names_and_the_library_exports_them():
    """the opaque type and the seven functions, each with RFC8032_EDDSA_DECL (the EDDSA_AMD_DECL names are counted by the tests of
    earlier additions); the shipped library exports every one of them"""
    text = header_text(strip_comments=True)
    assert re.search(r"typedef\s+struct\s+eddsa_amd_keyset\s+eddsa_amd_keyset\s*;", text)
    assert re.search(r"#define\s+EDDSA_AMD_KEYSET_MAX_KEYS\s+\(\(size_t\)1\s*<<\s*20\)", text)
    declared = declared_names(text, r"RFC8032_EDDSA_DECL")
    assert set(NAMES) <= declared
    assert not set(NAMES) & declared_names(text, r"(?<![0-9A-Z_])EDDSA_AMD_DECL")
    exported = exported_names("libeddsa_amd.so")
    assert set(NAMES) <= exported


def test_the_header_states_the_contract():
    text = " ".join(header_text().split())
    for phrase in ("key_idx[i] >= count is rejected", "SURVIVES eddsa_amd_shutdown", "never merged by the small-call combiner",
                   "Out of scope: _rlc, _multi, records, digest", "one-lane", "profiles/verify_keyed.txt"):
        assert phrase in text, phrase


def test_the_internal_header_does_not_name_the_keyset_launcher():
    """eddsa_kernels.h keeps its eighteen launchers; the one that builds a key set lives in edk_keyed.h"""
    kernels_h = open(os.path.join(ROOT, "libeddsa_amd", "csrc", "eddsa_kernels.h")).read()
    assert "edk_keyset_build" not in kernels_h and "edk_keyed" not in kernels_h
    assert len(set(re.findall(r"\b(edk_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", kernels_h, flags=re.S)))) == 18
    assert "edk_keyset_build(" in open(os.path.join(ROOT, "libeddsa_amd", "csrc", "edk_keyed.h")).read()


def test_create_checks_its_arguments_before_any_device_is_touched():
    """count == 0, count above the limit, out == NULL and keys == NULL: -hipErrorInvalidValue, *out left NULL - on a machine
    without a GPU too, which shows that no device was asked"""
    lib = ctypes.CDLL(os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd.so"))
    keys = (ctypes.c_uint8 * 64)()
    for fn, extra in ((lib.eddsa_amd_keyset_create, ()), (lib.eddsa_amd_keyset_create_dev, (ctypes.c_void_p(0),))):
        for k, count in ((keys, 0), (keys, (1 << 20) + 1), (None, 2), (keys, 2**63)):
            out = ctypes.c_void_p(0xdead)
            assert fn(ctypes.byref(out), k, SZ(count), *extra) == -INVALID_VALUE
            assert out.value is None
        assert fn(None, keys, SZ(2), *extra) == -INVALID_VALUE
    lib.eddsa_amd_keyset_destroy(None)                               # NULL allowed
    lib.eddsa_amd_keyset_count.restype = ctypes.c_size_t
    assert lib.eddsa_amd_keyset_count(None) == 0 and lib.eddsa_amd_keyset_device(None) == -1
    ok = (ctypes.c_uint8 * 4)()
    assert lib.ed25519_verify_keyed(ok, None, None, None, None, None, SZ(0), SZ(4)) == -INVALID_VALUE
    assert lib.ed25519_verify_keyed_dev(ok, None, None, None, None, None, SZ(0), SZ(4), None) == -INVALID_VALUE


# ---------------------------------------------------------------- the out-of-range key

def test_the_out_of_range_key_does_not_decode(keyedcheck):
    """y = 2: 3 / (4 d + 1) is no square mod p, so no rule decodes the string - while the all-zero string, the obvious other
    choice, is the point (sqrt(-1), 0) of order 4, for which R = [S]B verifies under the cofactored equation"""
    out = ctypes.create_string_buffer(32)
    keyedcheck.kc_no_key(out)
    assert out.raw == km.NO_KEY == le(2)
    x2 = em.x_squared(2)
    assert x2 == 3 * em.inv(4 * D + 1) % P
    assert pow(x2, (P - 1) // 2, P) == P - 1                         # Euler: a non-residue
    assert not km.decodes(km.NO_KEY)
    assert km.decodes(bytes(32))                                     # y = 0: x^2 = -1, a point of order 4
    assert (em.SQRT_M1 * em.SQRT_M1 + 1) % P == 0


# ---------------------------------------------------------------- the lanes, from a shared table

def _cases(golden):
    return golden("verify_edges.json") + golden("verify_torsion.json")


def test_the_keyset_table_is_verify_table_lanes(keyedcheck, golden):
    cases = _cases(golden)
    assert len(golden("verify_edges.json")) == 273 and len(golden("verify_torsion.json")) == 192
    keys = b"".join(H(c["pub"]) for c in cases) + km.NO_KEY + bytes(32)
    on = keyedcheck.kc_build(keys, SZ(len(keys) // 32))
    assert 0 < on < len(keys) // 32                                  # both kinds of key are in the set
    for k in range(len(keys) // 32):
        assert keyedcheck.kc_table_matches(SZ(k)) == 1, k
    assert keyedcheck.kc_violations() == 0


@pytest.mark.parametrize("order", ["arange", "shuffled"])
def test_recorded_verdicts_from_a_shared_table(keyedcheck, golden, order):
    """the 273 + 192 recorded cases as ONE key set (entry i = case i's key): the keyed prepare, halve and main steps - both
    routes, both pair bounds - return the recorded verdicts with tab_a read from the shared table, and leave it as built"""
    cases = _cases(golden)
    place = list(range(len(cases)))
    if order == "shuffled":
        random.Random(11).shuffle(place)                             # entry place[i] holds case i's key
    keys = bytearray(32 * len(cases))
    for i, c in enumerate(cases):
        keys[32 * place[i]:32 * place[i] + 32] = H(c["pub"])
    keyedcheck.kc_build(bytes(keys), SZ(len(cases)))
    exact = long_items = 0
    for i, c in enumerate(cases):
        msg, sig = H(c["msg"]), H(c["sig"])
        for wide in (0, 1):
            got = keyedcheck.kc_verify(ctypes.c_uint32(place[i]), sig, msg, SZ(len(msg)), 0, wide)
            assert got & 1 == int(c["accept"]), (c["name"], wide)
            exact += (got & 2) != 0
            long_items += (got & 4) != 0
        assert keyedcheck.kc_verify(ctypes.c_uint32(place[i]), sig, msg, SZ(len(msg)), 1, 0) == int(c["accept"]), c["name"]
    assert exact > 0                                                 # off-curve keys went through the item's own table
    for idx in (len(cases), len(cases) + 1, 0xFFFFFFFF):             # no key: rejected on both routes, nothing of the set read
        c = cases[0]
        for form in (0, 1):
            assert keyedcheck.kc_verify(ctypes.c_uint32(idx), H(c["sig"]), H(c["msg"]), SZ(len(H(c["msg"]))), form, 0) == 0
    assert keyedcheck.kc_keyset_untouched() == 1
    assert keyedcheck.kc_violations() == 0


# ---------------------------------------------------------------- the model of the pair search

def test_the_pair_model_agrees_with_the_lane(hostcheck):
    """keyed_model.short_pair against halve_scalar_lane (tests/host_check: hc_halve), both bounds: the same t have no pair, and
    the pairs the model returns satisfy v = u t (mod 8 l) with u odd"""
    rng = random.Random(3)
    none = {134: 0, 138: 0}
    for k in range(30000):
        t = rng.randrange(km.L)
        for bits, wide in ((134, 0), (138, 1)):
            if bits == 138 and k >= 3000:
                continue
            pair = km.short_pair(t, bits)
            v, u, neg = ctypes.create_string_buffer(20), ctypes.create_string_buffer(20), ctypes.c_int(0)
            found = hostcheck.hc_halve(v, u, ctypes.byref(neg), t.to_bytes(32, "little"), wide)
            assert bool(found) == (pair is not None), (hex(t), bits)
            if pair is None:
                none[bits] += 1
                continue
            assert km.check_pair(t, pair) and pair[0] < 1 << bits and abs(pair[1]) < 1 << bits
            assert int.from_bytes(v.raw, "little") == pair[0] and int.from_bytes(u.raw, "little") == abs(pair[1])
            assert bool(neg.value) == (pair[1] < 0)
    assert none[134] >= 1                                            # 8.5 in 10^5: about 2.5 of 30000


def test_as_keyset_round_trips():
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    pubs = base[rng.integers(0, 5, 40)]
    pubs[7, 0] ^= 1
    keys, idx = km.as_keyset(pubs, base)
    assert np.array_equal(keys[:5], base) and len(keys) == 6 and np.array_equal(keys[idx], pubs) and idx.dtype == np.uint32
