"""Plain-integer models for the tests of key-set verification (include/eddsa_amd.h: ed25519_verify_keyed): the pair search of the
half-length route (libeddsa_amd/csrc/halve.h: halve_scalar_lane), the decoding rule that the out-of-range key must fail, and
the construction of mixed keyed batches.  Test infrastructure only: Python integers, hashlib and numpy."""
import numpy as np

from ed_model import L, P, challenge, decode_reference, le  # noqa: F401  (P, challenge: for this model's users)

N8L = 8 * L

# the key bytes an item whose index names no key of the set is given (libeddsa_amd/csrc/keyed_lanes.h: keyed_no_key): y = 2
NO_KEY = le(2)


def decodes(enc):
    """whether 32 bytes decode to a curve point under the most permissive rule in use (the cofactored equation's, which is the
    reference import's test for "a root exists")"""
    return decode_reference(enc) is not None


def short_pair(t, bits=134):
    """The pair search of halve_scalar_lane as integers: the extended Euclidean algorithm on (8 l, t); every completed step's
    (remainder r, cofactor u) is a candidate with r = u t (mod 8 l).  The FIRST remainder below 2^bits decides: u odd -> the pair
    is (r, u), good when |u| < 2^bits; u even -> the next remainder is examined once more unless r is already below
    2^(256 - bits) (then |u'| >= 8 l / r cannot fit), and a second even u gives up.  Returns (v, u) or None = the item goes to
    the exact path.  (The kernel also gives up on a single quotient of 31 bits - one t in 2^31 - which this model does not.)"""
    r0, u0, r1, u1 = N8L, 0, t, 1
    tried = False
    while True:
        if r1 < (1 << bits):
            if u1 & 1:
                return (r1, u1) if abs(u1) < (1 << bits) else None
            if tried or r1 < (1 << (256 - bits)):
                return None
            tried = True
        if r1 == 0:
            return None
        q = r0 // r1
        r0, u0, r1, u1 = r1, u1, r0 - q * r1, u0 - q * u1


def check_pair(t, pair):
    v, u = pair
    return (u * t - v) % N8L == 0 and u & 1 == 1


def as_keyset(pubs, base_keys=None):
    """per-item keys (n, 32) -> (keys, idx): the distinct strings as a key set, base_keys (if given) first and in their order,
    and each item's index into it"""
    seen, keys = {}, []
    if base_keys is not None:
        for k in base_keys:
            b = k.tobytes()
            if b not in seen:
                seen[b] = len(keys)
                keys.append(b)
    idx = np.zeros(len(pubs), np.uint32)
    for i, p in enumerate(pubs):
        b = p.tobytes()
        if b not in seen:
            seen[b] = len(keys)
            keys.append(b)
        idx[i] = seen[b]
    return np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32).copy(), idx
