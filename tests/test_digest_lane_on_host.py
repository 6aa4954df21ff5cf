"""Verification from caller-supplied digests (include/eddsa_amd.h: ed25519_verify_digests*), the part that needs no GPU:
the lane function of the digest kernels (libeddsa_amd/csrc/lanes.h: verify_digest_lane; rlc_lanes.h: rlc_digest_lane) compiled for
the host with every bound asserted (tests/host_check/digest_check.cpp), the Python wrappers' argument checks, and the header."""
import ctypes
import hashlib
import os
import random
import re

import numpy as np
import pytest

from ed_model import L
from hostlib import ROOT, build_check, declared_names

PATTERN = int("88" * 32, 16)                       # what the prepare kernels add: nibble - 8 is the signed digit
NAMES = ("ed25519_verify_digests", "ed25519_verify_digests_dev", "ed25519_verify_digests_rlc", "ed25519_verify_digests_rlc_dev",
         "ed25519_verify_digests_multi")


@pytest.fixture(scope="module")
def digestcheck(tmp_path_factory):
    """tests/host_check/digest_check.cpp built with the flags of the hostcheck fixture (conftest.py), outside the tree"""
    h = build_check(tmp_path_factory, "digest")
    h.dc_violations.restype = ctypes.c_long
    return h


def _lane(h, digests):
    buf = b"".join(digests)
    out = ctypes.create_string_buffer(32 * len(digests))
    h.dc_verify_digest(out, buf, ctypes.c_size_t(len(digests)))
    return [out.raw[32 * i:32 * i + 32] for i in range(len(digests))]


def _want(d):
    return ((int.from_bytes(d, "little") % L) + PATTERN).to_bytes(32, "little")


def test_verify_digest_lane_against_python_integers(digestcheck):
    """t = (the 64 bytes as a little-endian integer) mod l, the sc_import(t, h, 64) of the reference's ed25519_verify, plus the
    digit pattern: the edges of the 512-bit range and of the reduction, and 2000 seeded random digests"""
    top = ((1 << 512) - 1) // L * L                 # the largest multiple of l below 2^512
    edges = [0, (1 << 512) - 1, L - 1, L, L + 1, top, top - 1, top + 1, 1 << 252, (1 << 256) - 1, 1 << 511]
    assert top + 1 < 1 << 512 and top % L == 0 and top + L >= 1 << 512
    rng = random.Random(20261017)
    digests = [v.to_bytes(64, "little") for v in edges] + [rng.randbytes(64) for _ in range(2000)]
    got = _lane(digestcheck, digests)
    for d, g in zip(digests, got):
        assert g == _want(d), d.hex()
    assert _want(L.to_bytes(64, "little")) == PATTERN.to_bytes(32, "little")          # (l reduces to 0: the check checks)
    assert digestcheck.dc_violations() == 0


def test_verify_digest_lane_word_for_word_against_verify_hash_lane(digestcheck):
    """hashlib's SHA-512(R || A || M) through verify_digest_lane = what verify_hash_lane leaves for (R, A, M): 200 seeded items,
    len(M) from 0 to 300 (one, two and three blocks); the same for the batch verification's lane, leaf included"""
    rng = random.Random(7)
    lens = list(range(0, 301, 3)) + [47, 48, 49, 111, 112, 113, 175, 176, 177, 239, 240, 241] + [rng.randrange(301) for _ in range(87)]
    assert len(lens) == 200 and min(lens) == 0 and max(lens) == 300
    for mlen in lens:
        sig, a, m = rng.randbytes(64), rng.randbytes(32), rng.randbytes(mlen)
        d = hashlib.sha512(sig[:32] + a + m).digest()
        hashed = ctypes.create_string_buffer(32)
        digestcheck.dc_verify_hash(hashed, sig[:32], a, m, ctypes.c_size_t(mlen))
        assert _lane(digestcheck, [d])[0] == hashed.raw == _want(d), mlen
        from_msg, from_digest = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
        digestcheck.dc_rlc_both(from_msg, from_digest, sig, a, m, ctypes.c_size_t(mlen), d)
        assert from_msg.raw == from_digest.raw, mlen
        assert from_digest.raw[:32] == (int.from_bytes(d, "little") % L).to_bytes(32, "little")
        assert from_digest.raw[32:64] == (int.from_bytes(sig[32:], "little") % L).to_bytes(32, "little")
        assert from_digest.raw[64:] == hashlib.sha512(d + sig[32:]).digest()[:32]      # the leaf: from the digest BYTES, not from t
    assert digestcheck.dc_violations() == 0


def test_wrappers_validate_before_the_c_call():
    """uint8 data (TypeError), digests a multiple of 64 bytes, all three arrays agreeing on n (ValueError) - raised before the
    library is called (no GPU here: a call that got through would raise EddsaAmdError instead)"""
    import libeddsa_amd as ed
    sigs, pubs, digs = np.zeros((3, 64), np.uint8), np.zeros((3, 32), np.uint8), np.zeros((3, 64), np.uint8)
    for fn in (ed.ed25519_verify_digests, ed.ed25519_verify_digests_rlc, ed.ed25519_verify_digests_multi):
        with pytest.raises(TypeError):
            fn(sigs, pubs, digs.astype(np.int32))
        with pytest.raises(TypeError):
            fn(sigs.astype(np.float32), pubs, digs)
        with pytest.raises(TypeError):
            fn(sigs, pubs.astype(np.uint16), digs)
        with pytest.raises(ValueError):
            fn(sigs, pubs, np.zeros(3 * 64 - 1, np.uint8))                 # not a multiple of 64
        with pytest.raises(ValueError):
            fn(sigs, pubs, np.zeros((2, 64), np.uint8))                    # digests: other n
        with pytest.raises(ValueError):
            fn(sigs, pubs[:2], digs)                                       # pubs: other n
        with pytest.raises(ValueError):
            fn(sigs[:2], pubs, digs)                                       # sigs: other n
        with pytest.raises(ValueError):
            fn(sigs, pubs, np.zeros((3, 32), np.uint8))                    # 32-byte digests: 96 bytes is no multiple of 64
    with pytest.raises(ValueError):
        ed.ed25519_verify_digests_rlc(sigs, pubs, digs[:1], return_stats=True)


def test_the_header_declares_the_five_names():
    text = open(os.path.join(ROOT, "include", "eddsa_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = declared_names(code, r"EDDSA_AMD_DECL")
    assert set(NAMES) <= declared
    for name in NAMES:
        (args,) = re.findall(r"\b" + name + r"\s*\(([^)]*)\)", code)
        assert "const uint8_t *digests" in args and "msg" not in args, name
        assert ("void *stream" in args) == name.endswith("_dev"), name
    ref = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eddsa.h")).read(), flags=re.S)
    single = declared_names(ref, r"EDDSA_DECL")
    assert len(single) == 13 and len(declared | single) == 52              # the reference's 13 stay 13; 47 exported names become 52
    # the vouching rule and the combiner rule are stated where the caller reads them
    flat = " ".join(text.split())
    assert "CALLER VOUCHES" in flat and "never merged by the small-call combiner" in flat
