"""Signer sets (include/eddsa_amd.h: eddsa_amd_signer, ed25519_sign_keyed and its ctx / ph forms) as a model the tests share
(tests/test_sign_keyed_on_host.py on the CPU, tests/test_gpu_sign_keyed.py on the GPU): hashlib, Python integers mod l and the
oracle's orc_ed_scale_base for arbitrary scalars.  Nothing here comes from the engine or from its source.  `orc` is the ctypes
handle of oracle/liboracle.so (the `oracle` fixture's .lib).  A key is its EXPANDED form, 64 bytes of scalar | prefix: the scalar
is any 256-bit little-endian integer, used mod l and not clamped."""
import numpy as np

import dom2_model as dm

L = dm.L
PLAIN, CTX, PH = None, dm.CTX, dm.PH                 # the variant: plain Ed25519 has no dom2 prefix at all
NEUTRAL = bytes([1]) + bytes(31)                     # the encoding of (0, 1)

# the scalars every test of expanded keys walks: the ends of the range, l and its neighbours, the clamping bits
EDGE_SCALARS = (0, 1, L - 1, L, L + 1, 2**255 - 1, 2**255, 2**256 - 1)


def expand(seed):
    """what eddsa_amd_signer_create derives from a seed: clamp(h[0..32)) | h[32..64) - the scalar as the clamped integer itself"""
    a, prefix = dm.secret_scalar(bytes(seed))
    return dm.le(a) + prefix


def expanded(a, prefix):
    assert 0 <= a < 2**256 and len(prefix) == 32
    return dm.le(a) + bytes(prefix)


def scalar(exp):
    return dm.num(exp[:32]) % L


def pub(orc, exp):
    """A = (a mod l) B, encoded"""
    a = scalar(exp)
    return NEUTRAL if a == 0 else dm.scale_base(orc, a)


def _dom(flag, context):
    return b"" if flag is PLAIN else dm.dom2(flag, context)


def nonce(exp, mprime, flag=PLAIN, context=b""):
    return dm.num(dm.sha(_dom(flag, context), exp[32:], mprime)) % L


def challenge(r_bytes, a_bytes, mprime, flag=PLAIN, context=b""):
    return dm.num(dm.sha(_dom(flag, context), r_bytes, a_bytes, mprime)) % L


def sign(orc, exp, mprime, flag=PLAIN, context=b"", a_bytes=None):
    """the signature of the expanded key over M' (the message; PH: the caller's SHA-512(M))"""
    a_bytes = pub(orc, exp) if a_bytes is None else a_bytes
    r = nonce(exp, mprime, flag, context)
    r_bytes = NEUTRAL if r == 0 else dm.scale_base(orc, r)
    return r_bytes + dm.le((r + challenge(r_bytes, a_bytes, mprime, flag, context) * scalar(exp)) % L)


def response_ok(sig, exp, a_bytes, mprime, flag=PLAIN, context=b""):
    """S == (r + t a) mod l in Python integers, t taken from the signature's own R (R = r B is pinned by a verify of the same
    signature)"""
    return dm.num(sig[32:]) == (nonce(exp, mprime, flag, context) + challenge(sig[:32], a_bytes, mprime, flag, context) * scalar(exp)) % L


def edge_keys(count, seed):
    """`count` expanded keys: the edge scalars first, then random unclamped 256-bit scalars; random prefixes -> (count, 64) uint8"""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(count):
        a = EDGE_SCALARS[k] if k < len(EDGE_SCALARS) else dm.num(rng.integers(0, 256, 32, dtype=np.uint8).tobytes())
        rows.append(expanded(a, rng.integers(0, 256, 32, dtype=np.uint8).tobytes()))
    return np.frombuffer(b"".join(rows), np.uint8).reshape(count, 64).copy()
