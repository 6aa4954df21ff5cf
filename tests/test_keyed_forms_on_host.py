"""The digest, Ed25519ctx and Ed25519ph forms of key-set verification (include/eddsa_amd.h: ed25519_verify_keyed_digests[_rlc],
ed25519ctx_verify_keyed, ed25519ph_verify_keyed), the part that needs no GPU: the header and the shipped library's exports, the
argument checks that run before any device is touched, and the lane sequences of the three new kernel forms
(libeddsa_amd/csrc/keyed_kernels.h, rlc_keyed.h) compiled for the host with every bound asserted
(tests/host_check/keyed_forms_check.cpp), over the recorded edge and torsion vectors as one key set: what the keyed sequence
leaves for an item against what the unkeyed sequence leaves for (sig, keys[idx], ...), against hashlib and tests/dom2_model.py."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import dom2_model as dm
import keyed_model as km
from ed_model import H
from hostlib import ROOT, build_check, declared_names, exported_names, header_text

SZ = ctypes.c_size_t
L = km.L
NAMES = ("ed25519_verify_keyed_digests", "ed25519_verify_keyed_digests_dev", "ed25519_verify_keyed_digests_rlc",
         "ed25519_verify_keyed_digests_rlc_dev", "ed25519ctx_verify_keyed", "ed25519ctx_verify_keyed_dev", "ed25519ph_verify_keyed",
         "ed25519ph_verify_keyed_dev")
INVALID_VALUE = 1                                    # hipErrorInvalidValue
WINDOWED = 1                                         # kernel_io.h: VERIFY_WINDOWED


# ---------------------------------------------------------------- the interface

def test_the_header_declares_the_eight_names_and_the_library_exports_them():
    text = header_text(strip_comments=True)
    declared = declared_names(text, r"RFC8032_EDDSA_DECL")
    assert set(NAMES) <= declared
    assert set(NAMES) <= exported_names("libeddsa_amd.so")
    # no new debug name: what the debug library exports on top of the shipped one is what its header declares
    debug_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eddsa_amd_debug.h")).read(), flags=re.S)
    extra = exported_names("libeddsa_amd_debug.so") - exported_names("libeddsa_amd.so")
    assert extra <= set(re.findall(r"\b(eddsa_amd_\w+)\s*\(", debug_h)), extra
    assert not [n for n in extra if "keyed_digests" in n or "ctx" in n or "ph_" in n]


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*", " ", header_text()).split())
    for phrase in ("ok[i] is byte for byte what the unkeyed form of the same name returns",
                   "ed25519_verify_digests, ed25519_verify_digests_rlc, ed25519ctx_verify_batch, ed25519ph_verify_batch",
                   "over plain key sets and over comb key sets", "A comb set takes the comb route in the per-item forms",
                   "the combination does not use the comb",
                   "digests[i] = SHA-512(R_i || keys[key_idx[i]] || M_i)", "any 64 bytes are legal input",
                   "key_idx[i] >= count gives ok[i] = 0 under every setting", "nothing outside the key set is read for that item",
                   "it contributes to no sum and does not send its group to the per-item kernels",
                   "so the cofactored re-evaluation rejects it too",
                   "checked before any device is touched", "never merged by the small-call combiner",
                   "more than 8192 keys makes the _rlc form run as the per-item form", "eddsa_amd_set_rlc_min_items",
                   "synchronises `stream` once per pass", "`context` is a host pointer in every form",
                   "context_len > 255", "_rlc forms of ctx / ph", "profiles/verify_keyed_forms.txt"):
        assert phrase in text, phrase


def test_the_old_out_of_scope_sentences_stand_with_a_note_of_what_was_added():
    text = " ".join(re.sub(r"\n \*", " ", header_text()).split())
    for sentence in ("Out of scope: _rlc, _multi, records, digest, Ed25519ctx / Ed25519ph and single-item forms; tables wider than nine entries.",
                     "Still out of scope: the digest, records, _multi, Ed25519ctx / Ed25519ph and single-item forms of keyed verification.",
                     "Out of scope: four-lane forms of the comb route, combs wider than 6 bits, the digest, records, _multi and ctx / ph keyed forms."):
        at = text.index(sentence) + len(sentence)
        note = text[at:at + 420]
        assert note.lstrip().startswith("(") and "since been added" in note and "end of this header" in note, sentence


def test_the_calls_check_their_arguments_before_any_device_is_touched():
    """against the shipped library on a machine without a GPU: -hipErrorInvalidValue shows that no device was asked.  The key set
    handle of the NULL-argument cases is never looked into: the NULL checks come first."""
    lib = ctypes.CDLL(os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd.so"))
    ok, st = (ctypes.c_uint8 * 4)(), (ctypes.c_uint32 * 4)()
    idx, sig, dig = (ctypes.c_uint32 * 4)(), (ctypes.c_uint8 * 256)(), (ctypes.c_uint8 * 256)()
    ks = ctypes.cast((ctypes.c_uint8 * 256)(), ctypes.c_void_p)                          # "a key set"
    ctx = ctypes.c_char_p(b"abc")
    n = SZ(4)
    calls = {                                        # name -> (arguments in front of n, arguments behind n)
        "ed25519_verify_keyed": ([ok, ks, idx, sig, dig, None, SZ(64)], []),
        "ed25519_verify_keyed_dev": ([ok, ks, idx, sig, dig, None, SZ(64)], [None]),
        "ed25519_verify_keyed_rlc": ([ok, st, ks, idx, sig, dig, None, SZ(64)], []),
        "ed25519_verify_keyed_rlc_dev": ([ok, None, ks, idx, sig, dig, None, SZ(64)], [None]),
        "ed25519_verify_keyed_digests": ([ok, ks, idx, sig, dig], []),
        "ed25519_verify_keyed_digests_dev": ([ok, ks, idx, sig, dig], [None]),
        "ed25519_verify_keyed_digests_rlc": ([ok, st, ks, idx, sig, dig], []),
        "ed25519_verify_keyed_digests_rlc_dev": ([ok, None, ks, idx, sig, dig], [None]),
        "ed25519ctx_verify_keyed": ([ok, ks, idx, sig, dig, None, SZ(64)], [ctx, SZ(3)]),
        "ed25519ctx_verify_keyed_dev": ([ok, ks, idx, sig, dig, None, SZ(64)], [ctx, SZ(3), None]),
        "ed25519ph_verify_keyed": ([ok, ks, idx, sig, dig], [ctx, SZ(3)]),
        "ed25519ph_verify_keyed_dev": ([ok, ks, idx, sig, dig], [ctx, SZ(3), None]),
    }
    for name, (front, back) in calls.items():
        fn = getattr(lib, name)
        pointers = [k for k, a in enumerate(front) if a in (ok, ks, idx, sig, dig)]
        assert len(pointers) == 5
        for k in pointers:                           # NULL key set, ok, key_idx, sigs, digests / messages / prehashes
            args = list(front)
            args[k] = None
            assert fn(*args, n, *back) == -INVALID_VALUE, (name, k)
        if back and back[0] is ctx:
            tail = back[2:]
            assert fn(*front, n, ctx, SZ(256), *tail) == -INVALID_VALUE, name          # a context of 256 bytes
            assert fn(*front, n, None, SZ(3), *tail) == -INVALID_VALUE, name           # no context where a length is given
            front0 = list(front); front0[1] = None
            assert fn(*front0, SZ(0), ctx, SZ(256), *tail) == -INVALID_VALUE, name     # ... before the batch size is looked at
        front0 = list(front)
        front0[front.index(ks)] = None
        assert fn(*front0, SZ(0), *back) == -INVALID_VALUE, name                       # a NULL key set with an empty batch, as ed25519_verify_keyed


def test_the_launchers_and_the_python_mirror():
    """no new edk_* function and no new field of edk_verify_src: the passes enter through edk_verify and edk_verify_rlc"""
    csrc = os.path.join(ROOT, "libeddsa_amd", "csrc")
    kernels_h = open(os.path.join(csrc, "eddsa_kernels.h")).read()
    assert len(set(re.findall(r"\b(edk_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", kernels_h, flags=re.S)))) == 18
    kernels, rlc = open(os.path.join(csrc, "kernels.hip")).read(), open(os.path.join(csrc, "rlc.hip")).read()
    assert "k_verify_prepare_keyed<true>" in kernels and "k_dom_challenge_keyed" in kernels and "k_rlc_hash_keyed<true>" in rlc
    assert "keyed && (src.dom ||" in rlc                                               # the keyed combination still refuses ctx / ph
    import sys
    sys.path.insert(0, ROOT)
    import libeddsa_amd
    for name in NAMES[0::2]:
        assert callable(getattr(libeddsa_amd, name)), name


# ---------------------------------------------------------------- the lane sequences on the host

class Prepared(ctypes.Structure):
    _fields_ = [("t", ctypes.c_uint8 * 32), ("s", ctypes.c_uint8 * 32), ("key", ctypes.c_uint8 * 32), ("flags", ctypes.c_uint8),
                ("on", ctypes.c_uint8), ("off", ctypes.c_uint8), ("ok", ctypes.c_uint8)]

    def same(self, other, fields=("t", "s", "key", "flags", "on", "off")):
        return all(bytes(getattr(self, f)) == bytes(getattr(other, f)) if f in ("t", "s", "key") else getattr(self, f) == getattr(other, f)
                   for f in fields)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """tests/host_check/keyed_forms_check.cpp built with the flags of the hostcheck fixture (conftest.py), outside the tree"""
    h = build_check(tmp_path_factory, "keyed_forms")
    h.kfc_violations.restype = ctypes.c_long
    return h


OFF_CURVE = km.NO_KEY                                # y = 2: a registered key that is no curve point


@pytest.fixture(scope="module")
def items(golden, check):
    """the 273 + 192 recorded vectors as one key set with shuffled placement, one off-curve key behind them (item 7 refers to it),
    and one item (11) whose index is out of range -> (cases in item order, keys, idx)"""
    cases = golden("verify_edges.json") + golden("verify_torsion.json")
    assert len(cases) == 273 + 192
    rng = np.random.default_rng(2025)
    place = rng.permutation(len(cases))              # case c's key is entry place[c]
    keys = [None] * len(cases)
    for c, case in enumerate(cases):
        keys[place[c]] = H(case["pub"])
    keys.append(OFF_CURVE)
    order = rng.permutation(len(cases))
    idx = [int(place[c]) for c in order]
    cases = [cases[c] for c in order]
    idx[7] = len(keys) - 1
    idx[11] = len(keys)
    assert not km.decodes(OFF_CURVE) and any(not km.decodes(k) for k in keys[:-1])
    check.kfc_keyset(b"".join(keys), len(keys))
    assert [check.kfc_key_flag(k) for k in range(len(keys))] == [int(km.decodes(k)) for k in keys]
    return cases, keys, idx


def digits(v, pattern):
    return ((v + pattern * (2**256 // 0xffffffff)) % 2**256).to_bytes(32, "little")


T_PATTERN, S_PATTERN = 0x88888888, 0x80008000        # lanes.h: verify_digest_lane, verify_s_lane


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_keyed_digest_prepare_against_the_unkeyed_one_and_hashlib(check, items, mode):
    cases, keys, idx = items
    count = len(keys)
    for i, c in enumerate(cases):
        sig, msg = H(c["sig"]), H(c["msg"])
        known = idx[i] < count
        key = keys[idx[i]] if known else km.NO_KEY
        dig = hashlib.sha512(sig[:32] + key + msg).digest()
        got, ref = Prepared(), Prepared()
        check.kfc_prepare_keyed(ctypes.byref(got), sig, ctypes.c_uint32(idx[i]), dig, mode)
        check.kfc_prepare_unkeyed(ctypes.byref(ref), sig, key, dig, int(mode == 2))
        assert bytes(got.t) == digits(int.from_bytes(dig, "little") % L, T_PATTERN), c["name"]
        assert bytes(got.s) == digits(int.from_bytes(sig[32:], "little") % L, S_PATTERN), c["name"]
        assert bytes(got.key) == key
        if known:
            assert got.same(ref) and got.ok == 0xff, c["name"]
            assert got.on == int(km.decodes(key) and mode != 2) and got.off == 1 - got.on and got.flags == got.on * WINDOWED
        else:                                        # decided by the prepare kernel: ok = 0, on neither list
            assert got.same(ref, ("t", "s", "key")) and (got.flags, got.on, got.off, got.ok) == (0, 0, 0, 0)
    assert check.kfc_violations() == 0


def test_keyed_dom_challenge_against_the_unkeyed_one_and_the_model(check, items):
    cases, keys, idx = items
    count = len(keys)
    for flag, context in ((dm.CTX, b""), (dm.CTX, b"abc"), (dm.PH, bytes(range(255)))):
        dom = dm.dom2(flag, context)
        for i, c in enumerate(cases):
            sig, msg = H(c["sig"]), H(c["msg"])
            mprime = hashlib.sha512(msg).digest() if flag == dm.PH else msg
            key = keys[idx[i]] if idx[i] < count else km.NO_KEY
            got, ref = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
            check.kfc_dom_keyed(got, dom, len(dom), sig, ctypes.c_uint32(idx[i]), mprime, SZ(len(mprime)))
            check.kfc_dom_unkeyed(ref, dom, len(dom), sig, key, mprime, SZ(len(mprime)))
            assert got.raw == ref.raw == dm.challenge_digest(sig, key, mprime, flag, context), (flag, len(context), c["name"])
            if i % 16 == 0:                          # behind it the pass is a keyed digest pass over these 64 bytes
                p = Prepared()
                check.kfc_prepare_keyed(ctypes.byref(p), sig, ctypes.c_uint32(idx[i]), got.raw, 1)
                assert bytes(p.t) == digits(dm.challenge(sig[:32], key, mprime, flag, context), T_PATTERN)
    assert check.kfc_violations() == 0


def test_keyed_digest_combination_hash_against_the_unkeyed_one_and_hashlib(check, items):
    cases, keys, idx = items
    count = len(keys)
    for i, c in enumerate(cases):
        sig, msg = H(c["sig"]), H(c["msg"])
        key = keys[idx[i]] if idx[i] < count else km.NO_KEY
        dig = hashlib.sha512(sig[:32] + key + msg).digest()
        got, ref = ctypes.create_string_buffer(128), ctypes.create_string_buffer(96)
        check.kfc_rlc_hash_keyed(got, sig, ctypes.c_uint32(idx[i]), dig)
        check.kfc_rlc_hash_unkeyed(ref, sig, dig)
        assert got.raw[:96] == ref.raw and got.raw[96:] == key, c["name"]
        assert got.raw[:32] == (int.from_bytes(dig, "little") % L).to_bytes(32, "little")
        assert got.raw[32:64] == (int.from_bytes(sig[32:], "little") % L).to_bytes(32, "little")
        assert got.raw[64:96] == hashlib.sha512(dig + sig[32:]).digest()[:32], c["name"]   # the leaf: the digest's bytes, then S's
    assert check.kfc_violations() == 0
