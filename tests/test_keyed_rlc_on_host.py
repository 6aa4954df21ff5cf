"""Batch verification over a key set (include/eddsa_amd.h: ed25519_verify_keyed_rlc), the part that needs no GPU: the header and
the shipped library's exports, the argument checks that run before any device is touched, and the lane steps of the keyed
combination (libeddsa_amd/csrc/rlc_keyed_lanes.h) compiled for the host with every bound asserted
(tests/host_check/keyed_rlc_check.cpp): the per-key scalar against Python integers, the item's term, and a whole small group
evaluated the keyed way against the unkeyed evaluation of the same items (hc_rlc_group)."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from ed_model import H, L
from hostlib import ROOT, build_check, declared_names, exported_names, header_text

SZ = ctypes.c_size_t
N8L = 8 * L
NAMES = ("ed25519_verify_keyed_rlc", "ed25519_verify_keyed_rlc_dev")
INVALID_VALUE = 1                                    # hipErrorInvalidValue


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """tests/host_check/keyed_rlc_check.cpp built with the flags of the hostcheck fixture (conftest.py), outside the tree"""
    h = build_check(tmp_path_factory, "keyed_rlc")
    h.krc_violations.restype = ctypes.c_long
    return h


# ---------------------------------------------------------------- the interface

def test_the_header_declares_the_two_names_and_the_library_exports_them():
    text = header_text(strip_comments=True)
    declared = declared_names(text, r"RFC8032_EDDSA_DECL")
    assert set(NAMES) <= declared
    assert set(NAMES) <= exported_names("libeddsa_amd.so")


def test_the_header_states_the_contract():
    text = " ".join(header_text().split())
    for phrase in ("key_idx[i] >= count gets ok[i] = 0 under every setting", "it contributes to no sum",
                   "does not send its group to the per-item kernels", "more than 8192 keys is not combined",
                   "eddsa_amd_set_rlc_min_items", "64 bytes per item of workspace capacity", "profiles/verify_keyed_rlc.txt",
                   "Still out of scope: the digest, records, _multi"):
        assert phrase in text, phrase


def test_the_calls_check_their_arguments_before_any_device_is_touched():
    lib = ctypes.CDLL(os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd.so"))
    ok = (ctypes.c_uint8 * 4)()
    st = (ctypes.c_uint32 * 4)()
    assert lib.ed25519_verify_keyed_rlc(ok, st, None, None, None, None, None, SZ(0), SZ(4)) == -INVALID_VALUE
    assert lib.ed25519_verify_keyed_rlc_dev(ok, None, None, None, None, None, None, SZ(0), SZ(4), None) == -INVALID_VALUE


def test_the_launchers_are_the_existing_ones():
    """no new edk_* symbol: the keyed pass enters through edk_verify_rlc and edk_verify_rlc_fallback"""
    kernels_h = open(os.path.join(ROOT, "libeddsa_amd", "csrc", "eddsa_kernels.h")).read()
    assert len(set(re.findall(r"\b(edk_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", kernels_h, flags=re.S)))) == 18
    rlc = open(os.path.join(ROOT, "libeddsa_amd", "csrc", "rlc.hip")).read()
    assert '#include "rlc_keyed.h"' in rlc and "sub.key_idx += lo" in rlc
    assert "gok[i / RLC_G] == 1" in rlc and "h_gok[g] == 1" in rlc           # an undecided group fails closed


# ---------------------------------------------------------------- the per-key scalar

def signed_value(dig):
    assert all(-128 <= d <= 127 for d in dig)
    return sum(d << (8 * j) for j, d in enumerate(dig))


def key_sum(check, terms):
    """the digits' value for the accumulator the kernels would hold after adding `terms` word by word"""
    acc = (ctypes.c_uint64 * 8)(*[sum((t >> (32 * q)) & 0xffffffff for t in terms) for q in range(8)])
    assert all(a < 2**45 for a in acc)
    dig = (ctypes.c_int8 * 32)()
    check.krc_key_sum(dig, acc)
    return signed_value(list(dig))


def centred(v):
    v %= N8L
    return v - N8L if v >= 4 * L else v


def test_key_scalar_lane_against_integers(check):
    rng = np.random.default_rng(41)
    rnd = lambda: int.from_bytes(bytes(rng.integers(0, 256, 40, dtype=np.uint8)), "little") % N8L  # noqa: E731
    cases = [[0], [1], [N8L - 1], [rnd()], [rnd(), rnd()], [N8L - 1, N8L - 1], [N8L - 1] * 8192, [rnd() for _ in range(8192)]]
    a = rnd()
    cases += [[a, N8L - a], [L, 7 * L], [N8L - 1, 1]]                                  # sums = 0 (mod 8 l)
    for edge in (4 * L, -4 * L):                                                      # both sides of + 4 l and of - 4 l
        for delta in (-2, -1, 0, 1, 2):
            v = (edge + delta) % N8L
            cases += [[v], [v - a if v >= a else v + N8L - a, a], [(v - 5 * a) % N8L] + [a] * 5]
    cases += [[k * L + d] for k in range(8) for d in (0, 1, L - 1)]                    # every k of z t = a0 + k l
    for terms in cases:
        assert all(0 <= t < N8L for t in terms)
        c = key_sum(check, terms)
        assert abs(c) <= 4 * L and (c - sum(terms)) % N8L == 0, (len(terms), terms[:3])
        assert c == centred(sum(terms)), (len(terms), terms[:3])
    assert key_sum(check, []) == 0
    assert check.krc_violations() == 0


def test_the_items_term_is_z_t_mod_8l(check):
    rng = np.random.default_rng(42)
    term, zs = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    dr = (ctypes.c_int8 * 16)()
    for k in range(60):
        seed = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        i = int(rng.integers(0, 2**40)) if k % 2 else k
        t = int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), "little") % L if k > 3 else (0, 1, L - 1, L - 2)[k]
        s = int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), "little") % L if k > 3 else (L - 1, 0, 1, 7)[k]
        check.krc_term(term, dr, zs, seed, ctypes.c_uint64(i), t.to_bytes(32, "little"), s.to_bytes(32, "little"))
        h = hashlib.sha512(seed + i.to_bytes(8, "little") + b"rlc\0" + bytes(20)).digest()
        z = (int.from_bytes(h[:16], "little") & (2**126 - 1)) | 1
        assert int.from_bytes(term.raw, "little") == z * t % N8L
        assert signed_value(list(dr)) == z and int.from_bytes(zs.raw, "little") == z * s % L
    assert check.krc_violations() == 0


# ---------------------------------------------------------------- a whole group, the keyed way

P_ = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def both_ways(check, hostcheck, sig, keys, idx, msg, mlen):
    """(keyed evaluation, unkeyed evaluation of the same items) -> each 0 or 1"""
    n = len(sig)
    sig, keys, msg = np.ascontiguousarray(sig), np.ascontiguousarray(keys), np.ascontiguousarray(msg)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    fl = (ctypes.c_uint8 * n)()
    valid = (ctypes.c_uint8 * n)()
    got = check.krc_group(fl, P_(sig), P_(keys), len(keys), P_(idx), P_(msg), SZ(mlen), n)
    ref = hostcheck.hc_rlc_group(valid, P_(sig), P_(np.ascontiguousarray(keys[idx])), P_(msg), SZ(mlen), n)
    assert [f & 1 for f in fl] == list(valid)
    return got, ref


@pytest.mark.parametrize("nkeys", [1, 3])
def test_whole_group_the_keyed_way(check, hostcheck, oracle, nkeys):
    rng = np.random.default_rng(43 + nkeys)
    n, mlen = 24, 20
    ksk = rng.integers(0, 256, (nkeys, 32), dtype=np.uint8)
    kpk = oracle.genpub_batch(ksk)
    idx = (np.arange(n) * 7 % nkeys).astype(np.uint32)
    msg = rng.integers(0, 256, (n, mlen), dtype=np.uint8)
    sig = oracle.sign_batch(np.ascontiguousarray(ksk[idx]), np.ascontiguousarray(kpk[idx]), msg, mlen)
    assert both_ways(check, hostcheck, sig, kpk, idx, msg, mlen) == (1, 1)             # honest items
    s2 = sig.copy(); s2[5, 40] ^= 1
    assert both_ways(check, hostcheck, s2, kpk, idx, msg, mlen) == (0, 0)              # a forged item
    m2 = msg.copy(); m2[7, 0] ^= 1
    assert both_ways(check, hostcheck, sig, kpk, idx, m2, mlen) == (0, 0)
    s2 = sig.copy(); s2[3, 32:] = np.frombuffer((int.from_bytes(sig[3, 32:].tobytes(), "little") + L).to_bytes(32, "little"), np.uint8)
    assert both_ways(check, hostcheck, s2, kpk, idx, msg, mlen) == (1, 1)              # S + l: reduced, not range-checked
    # a key set may hold a key of order 2 and a string that is no curve point: combined while no item refers to them
    wide = np.concatenate([kpk, np.frombuffer((2**255 - 20).to_bytes(32, "little") + (2).to_bytes(32, "little"), np.uint8).reshape(2, 32)])
    assert both_ways(check, hostcheck, sig, wide, idx, msg, mlen) == (1, 1)
    for bad in (nkeys, nkeys + 1):
        i2 = idx.copy(); i2[11] = bad
        assert both_ways(check, hostcheck, sig, wide, i2, msg, mlen) == (0, 0)         # flagged for the per-item route
    # an index outside the key set: flags 0, no term, the group still passes
    i2 = idx.copy(); i2[9] = len(wide)
    fl = (ctypes.c_uint8 * n)()
    assert check.krc_group(fl, P_(sig), P_(wide), len(wide), P_(i2), P_(msg), SZ(mlen), n) == 1
    assert fl[9] == 0 and all(fl[i] == 1 for i in range(n) if i != 9)
    assert check.krc_violations() == 0 and hostcheck.hc_violations() == 0


def test_single_item_groups_are_exact_on_mixed_order_points(check, hostcheck, golden):
    """the mixed-order vectors of verify_torsion.json as one-item groups under a one-key set: the per-key scalar is exact mod
    8 l, so the keyed group decides what the reference decides, like the unkeyed one"""
    fl = (ctypes.c_uint8 * 1)()
    idx = np.zeros(1, np.uint32)
    for c in golden("verify_torsion.json"):
        msg, key = H(c["msg"]), np.frombuffer(H(c["pub"]), np.uint8)
        got = check.krc_group(fl, H(c["sig"]), P_(key), 1, P_(idx), msg, SZ(len(msg)), 1)
        ref = hostcheck.hc_rlc_group((ctypes.c_uint8 * 1)(), H(c["sig"]), H(c["pub"]), msg, SZ(len(msg)), 1)
        assert got == ref == int(c["accept"]) and fl[0] & 1, c["name"]
    assert check.krc_violations() == 0
