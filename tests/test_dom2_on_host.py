"""Ed25519ctx and Ed25519ph (include/eddsa_amd.h: ed25519ctx_*, ed25519ph_*), the part that needs no GPU: the model the GPU
tests compare with (tests/dom2_model.py) against RFC 8032's vectors; the prefixed hash lane of the kernels (libeddsa_amd/csrc/
sha512.h: sha512_dom_msg) and the lanes built on it, compiled for the host with every bound asserted (tests/host_check/
dom2_check.cpp), against hashlib and the model; the Python wrappers' argument checks; the header."""
import ctypes
import hashlib
import os
import random
import re

import numpy as np
import pytest

import dom2_model as dm
from hostlib import ROOT, build_check, declared_names

L = dm.L
PATTERN = int("88" * 32, 16)
NAMES = ("ed25519ctx_sign_batch", "ed25519ctx_verify_batch", "ed25519ph_sign_batch", "ed25519ph_verify_batch",
         "ed25519ctx_sign_batch_dev", "ed25519ctx_verify_batch_dev", "ed25519ph_sign_batch_dev", "ed25519ph_verify_batch_dev")
# P = 34 + len(C) takes every residue mod 4 and lands on, just below and just above 64, 128 and 256
CONTEXT_LENS = (0, 1, 2, 3, 29, 30, 31, 93, 94, 95, 221, 222, 223, 254, 255)
TOTALS_MOD_128 = (110, 111, 112, 113, 127, 128, 129)      # the edges of one- and two-block padding


@pytest.fixture(scope="module")
def domcheck(tmp_path_factory):
    """tests/host_check/dom2_check.cpp built with the flags of the hostcheck fixture (conftest.py), outside the tree"""
    h = build_check(tmp_path_factory, "dom2")
    h.d2_violations.restype = ctypes.c_long
    return h


def test_the_model_reproduces_rfc8032(oracle):
    """both vectors: the key pair, the signature bytes, acceptance; and what must NOT verify: the other flag, another context
    ("fo" against "foo", empty), one bit of R, S, A or M', and the same bytes as plain Ed25519 in either direction"""
    orc = oracle.lib
    vectors = dm.rfc_vectors()
    assert [v["flag"] for v in vectors] == [dm.CTX, dm.PH] and vectors[0]["context"] == b"foo" and vectors[1]["context"] == b""
    assert vectors[1]["mprime"] == hashlib.sha512(b"abc").digest()
    for v in vectors:
        sk, pk, m, c, f, sig = (v[k] for k in ("sk", "pk", "mprime", "context", "flag", "sig"))
        assert dm.genpub(orc, sk) == pk == oracle.genpub(sk)
        assert dm.sign(orc, sk, pk, m, f, c) == sig
        assert dm.verify(orc, sig, pk, m, f, c) and dm.response_ok(sig, sk, pk, m, f, c)
        assert not dm.verify(orc, sig, pk, m, 1 - f, c)
        for other in (b"fo", b"foo"[:len(c)] + b"o", b"", b"bar"):
            assert dm.verify(orc, sig, pk, m, f, other) == (other == c)
        flip = lambda b, at: b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]                    # noqa: E731
        assert not dm.verify(orc, flip(sig, 3), pk, m, f, c) and not dm.verify(orc, flip(sig, 40), pk, m, f, c)
        assert not dm.verify(orc, sig, flip(pk, 7), m, f, c) and not dm.verify(orc, sig, pk, flip(m, len(m) - 1), f, c)
        assert not oracle.verify(sig, pk, m)                                             # not an Ed25519 signature ...
        assert not dm.verify(orc, oracle.sign(sk, pk, m), pk, m, f, c)                   # ... and an Ed25519 one is not one of these
    assert dm.dom2(0, b"") == dm.TAG + b"\0\0" and len(dm.dom2(1, b"x" * 255)) == 289


def _lens_for(header):
    extra = [(t - header) % 128 + 384 for t in TOTALS_MOD_128]
    return list(range(301)) + extra


def test_the_prefixed_hash_lane_against_hashlib(domcheck):
    """sha512_dom_msg<8> and <16> = SHA-512(dom2 || register words || message): every context length of CONTEXT_LENS, both flags,
    message lengths 0..300 and the padding edges past them, the message at all four alignments"""
    rng = random.Random(20261019)
    room = 600
    bufs = [ctypes.create_string_buffer(room + 8) for _ in range(4)]
    base = [(-ctypes.addressof(b)) % 4 for b in bufs]                 # to a 4-byte boundary, then a bytes further
    out = ctypes.create_string_buffer(64)
    data = rng.randbytes(room)
    ptrs = []
    for a in range(4):
        ctypes.memmove(ctypes.addressof(bufs[a]) + base[a] + a, data, room)
        ptrs.append(ctypes.c_void_p(ctypes.addressof(bufs[a]) + base[a] + a))
        assert ptrs[a].value % 4 == a
    checked = 0
    for clen in CONTEXT_LENS:
        context = rng.randbytes(clen)
        for flag in (dm.CTX, dm.PH):
            dom = dm.dom2(flag, context)
            for npre in (8, 16):
                pre = rng.randbytes(4 * npre)
                head = hashlib.sha512(dom + pre)
                lens = _lens_for(len(dom) + 4 * npre)
                assert {(len(dom) + 4 * npre + n) % 128 for n in lens[301:]} == {t % 128 for t in TOTALS_MOD_128}
                for mlen in lens:
                    want = head.copy()
                    want.update(data[:mlen])
                    want = want.digest()
                    for a in range(4):
                        assert domcheck.d2_hash(out, npre, dom, ctypes.c_uint32(len(dom)), pre, ptrs[a], ctypes.c_size_t(mlen)) == 0
                        assert out.raw == want, (clen, flag, npre, mlen, a)
                        checked += 1
    assert checked == len(CONTEXT_LENS) * 2 * 2 * 308 * 4
    assert domcheck.d2_violations() == 0


def test_a_null_message_of_length_zero_is_never_read(domcheck):
    out = ctypes.create_string_buffer(64)
    for clen in (0, 3, 94, 255):
        dom = dm.dom2(dm.PH, b"c" * clen)
        for npre in (8, 16):
            pre = bytes(range(4 * npre))
            assert domcheck.d2_hash(out, npre, dom, ctypes.c_uint32(len(dom)), pre, None, ctypes.c_size_t(0)) == 0
            assert out.raw == hashlib.sha512(dom + pre).digest()
    assert domcheck.d2_violations() == 0


def test_the_sign_and_verify_lanes_against_the_model(domcheck, oracle):
    """sign_dom_scalars_lane leaves (a, r) of the model, sign_dom_challenge_lane + sign_response_lane its S, and the verify
    kernel's lane the digest ed25519_verify_digests is handed in the model, as the digit words of t: the RFC's vectors and 120
    seeded items over context lengths 0..255 and message lengths 0..400"""
    orc = oracle.lib
    rng = random.Random(8032)
    items = [(v["sk"], v["pk"], v["mprime"], v["flag"], v["context"]) for v in dm.rfc_vectors()]
    for k in range(120):
        sk = rng.randbytes(32)
        flag = k & 1
        m = rng.randbytes(64) if flag == dm.PH else rng.randbytes(rng.randrange(401))
        items.append((sk, oracle.genpub(sk), m, flag, rng.randbytes(rng.choice(CONTEXT_LENS + (rng.randrange(256),)))))
    for sk, pk, m, flag, context in items:
        dom = dm.dom2(flag, context)
        p = ctypes.c_uint32(len(dom))
        ar = ctypes.create_string_buffer(64)
        domcheck.d2_sign_scalars(ar, dom, p, sk, m, ctypes.c_size_t(len(m)))
        a, r = dm.secret_scalar(sk)[0] % L, dm.nonce(sk, m, flag, context)
        assert ar.raw == dm.le(a) + dm.le(r)
        sig = dm.sign(orc, sk, pk, m, flag, context)
        s = ctypes.create_string_buffer(32)
        domcheck.d2_sign_response(s, dom, p, sig[:32], pk, ar.raw[:32], ar.raw[32:], m, ctypes.c_size_t(len(m)))
        assert s.raw == sig[32:]
        tw, dig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
        domcheck.d2_verify_digits(tw, dig, dom, p, sig[:32], pk, m, ctypes.c_size_t(len(m)))
        assert dig.raw == dm.challenge_digest(sig, pk, m, flag, context)
        assert tw.raw == dm.le(dm.challenge(sig[:32], pk, m, flag, context) + PATTERN)
        assert dm.verify(orc, sig, pk, m, flag, context)
    assert domcheck.d2_violations() == 0


def test_wrappers_validate_before_the_c_call():
    """a context of more than 255 bytes, prehashes that are not 64 bytes per item, arrays that disagree on n: ValueError; data
    that is not uint8: TypeError - all before the library is called (no GPU here: a call that got through would raise
    EddsaAmdError instead)"""
    import libeddsa_amd as ed
    secs, sigs, pubs = np.zeros((3, 32), np.uint8), np.zeros((3, 64), np.uint8), np.zeros((3, 32), np.uint8)
    msgs, pre = np.zeros((3, 10), np.uint8), np.zeros((3, 64), np.uint8)
    long = b"x" * 256
    for fn, first in ((ed.ed25519ctx_sign_batch, secs), (ed.ed25519ctx_verify_batch, sigs)):
        with pytest.raises(ValueError):
            fn(first, pubs, msgs, long)
        with pytest.raises(ValueError):
            fn(first, pubs[:2], msgs, b"foo")
        with pytest.raises(ValueError):
            fn(first, pubs, np.zeros(31, np.uint8), b"foo")                 # 31 bytes: no multiple of three items
        with pytest.raises(TypeError):
            fn(first.astype(np.int32), pubs, msgs, b"foo")
    for fn, first in ((ed.ed25519ph_sign_batch, secs), (ed.ed25519ph_verify_batch, sigs)):
        with pytest.raises(ValueError):
            fn(first, pubs, pre, long)
        with pytest.raises(ValueError):
            fn(first, pubs, np.zeros((3, 32), np.uint8))                    # 32-byte prehashes: 96 bytes is no multiple of 64
        with pytest.raises(ValueError):
            fn(first, pubs, pre[:2], b"foo")
        with pytest.raises(ValueError):
            fn(first, pubs[:2], pre)
        with pytest.raises(TypeError):
            fn(first, pubs, pre.astype(np.uint16))


def test_the_header_declares_the_eight_names():
    text = open(os.path.join(ROOT, "include", "eddsa_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = declared_names(code, r"EDDSA(?:_AMD)?_DECL")
    assert set(NAMES) <= declared
    for name in NAMES:
        (args,) = re.findall(r"\b" + name + r"\s*\(([^)]*)\)", code)
        assert args.rstrip().endswith("void *stream") == name.endswith("_dev"), name
        assert "const uint8_t *context, size_t context_len" in " ".join(args.split()), name
        assert ("const uint8_t *prehashes" in args and "msg" not in args) == ("ph_" in name), name
        assert ("const uint64_t *msg_off, size_t msg_len" in " ".join(args.split())) == ("ctx_" in name), name
    flat = " ".join(text.split())
    for words in ("SHOULD NOT", "HOST pointer", "never merged by the small-call combiner", "Out of scope"):
        assert words in flat, words
