"""Ed25519ctx and Ed25519ph (RFC 8032 5.1, include/eddsa_amd.h: ed25519ctx_*, ed25519ph_*) as a model the tests share
(tests/test_dom2_on_host.py on the CPU, tests/test_gpu_dom2.py on the GPU): dom2, sign and verify from hashlib, Python integers
mod l and the oracle's two curve operations (orc_ed_scale_base, orc_ed_dual_scale).  Nothing here comes from the engine or from
its source.  `orc` is the ctypes handle of oracle/liboracle.so (the `oracle` fixture's .lib).  Honestly generated keys only."""
import ctypes
import json
import os

import numpy as np

import ed_model as em
from ed_model import DOM2_TAG as TAG, L, clamped, dom2, le, num, sha  # noqa: F401  (for this model's users)

CTX, PH = 0, 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rfc8032_dom2.json")


def secret_scalar(sk):
    """(a, prefix) of ed25519_key_setup: h = SHA-512(sk), a = h[0..32) clamped, prefix = h[32..64)"""
    return clamped(sk), sha(sk)[32:]


def scale_base(orc, k):
    out = ctypes.create_string_buffer(32)
    orc.orc_ed_scale_base(out, le(k % L))
    return out.raw


def genpub(orc, sk):
    return scale_base(orc, secret_scalar(sk)[0])


def nonce(sk, mprime, flag, context):
    return num(sha(dom2(flag, context), secret_scalar(sk)[1], mprime)) % L


def challenge(r_bytes, pk, mprime, flag, context):
    return em.challenge(r_bytes, pk, mprime, dom2(flag, context))


def sign(orc, sk, pk, mprime, flag, context):
    """mprime: the message (CTX) or the caller's SHA-512(M) (PH)"""
    a, _ = secret_scalar(sk)
    r = nonce(sk, mprime, flag, context)
    r_bytes = scale_base(orc, r)
    return r_bytes + le((r + challenge(r_bytes, pk, mprime, flag, context) * a) % L)


def verify(orc, sig, pk, mprime, flag, context):
    """the reference's permissive check (lib/ed25519-sha512.c:148-181) with t from the prefixed hash: S B + t (-A) == R as bytes"""
    t = challenge(sig[:32], pk, mprime, flag, context)
    minus_a = pk[:31] + bytes([pk[31] ^ 0x80])
    out = ctypes.create_string_buffer(32)
    orc.orc_ed_dual_scale(out, le(num(sig[32:]) % L), le(t), minus_a)
    return out.raw == sig[:32]


def challenge_digest(sig, pk, mprime, flag, context):
    """what ed25519_verify_digests takes for the item: the variants' verify IS that call on this digest"""
    return sha(dom2(flag, context), sig[:32], pk, mprime)


def response_ok(sig, sk, pk, mprime, flag, context):
    """S == (r + t a) mod l in Python integers, t taken from the signature's own R: pins S for every item of a large batch
    without a scalar multiplication (R = r B is pinned by a verify over the same signature)"""
    a, _ = secret_scalar(sk)
    return num(sig[32:]) == (nonce(sk, mprime, flag, context) + challenge(sig[:32], pk, mprime, flag, context) * a) % L


def rfc_vectors():
    """the two vectors of tests/golden/rfc8032_dom2.json as dicts of bytes; `mprime` is what the library is handed"""
    out = []
    for v in json.load(open(GOLDEN))["vectors"]:
        v = dict(v, **{k: bytes.fromhex(v[k]) for k in ("sk", "pk", "msg", "context", "sig")})
        v["mprime"] = sha(v["msg"]) if v["flag"] == PH else v["msg"]
        out.append(v)
    return out


def keys(orc, n, seed):
    """n honest key pairs -> (secs (n, 32), pubs (n, 32)) uint8, from the oracle's batched genpub"""
    rng = np.random.default_rng(seed)
    secs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pubs = np.zeros((n, 32), np.uint8)
    orc.orc_ed25519_genpub_batch(pubs.ctypes.data_as(ctypes.c_void_p), secs.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(n), 16)
    return secs, pubs
