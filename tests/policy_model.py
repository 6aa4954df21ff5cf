"""The opt-in strict rules of verification (include/eddsa_amd.h: EDDSA_AMD_VERIFY_*) in Python integers, and the inputs the
policy tests share (tests/test_policy_lane_on_host.py on the CPU, tests/test_gpu_policy.py on the GPU).  Nothing here comes
from the engine or from its source: l and p are the curve's, the small-order y values are found by multiplying curve points by
l, the square test is Euler's criterion."""
import functools
import hashlib

import numpy as np

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, -1, P) % P
S_BELOW_L, A_CANONICAL, A_NOT_SMALL, R_NOT_SMALL, STRICT = 0x100, 0x200, 0x400, 0x800, 0xF00
BITS = (S_BELOW_L, A_CANONICAL, A_NOT_SMALL, R_NOT_SMALL)
POLICIES = (0,) + BITS + (STRICT,)
H = bytes.fromhex


# ---------------------------------------------------------------- the curve -x^2 + y^2 = 1 + d x^2 y^2, affine

def add(a, b):
    (x1, y1), (x2, y2) = a, b
    k = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * pow(1 + k, -1, P) % P, (y1 * y2 + x1 * x2) * pow(1 - k, -1, P) % P)


def mul(k, pt):
    acc = (0, 1)
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


def x_squared(y):
    return (y * y - 1) * pow(D * y * y + 1, -1, P) % P


def is_square(v):
    return v == 0 or pow(v, (P - 1) // 2, P) == 1


def sqrt(v):
    """a root of the square v (p = 5 mod 8)"""
    r = pow(v, (P + 3) // 8, P)
    if r * r % P != v:
        r = r * pow(2, (P - 1) // 4, P) % P
    assert r * r % P == v
    return r


@functools.lru_cache(maxsize=None)
def torsion_points():
    """the eight points of order dividing 8: l times a curve point is one of them; curve points with y = 2, 3, .. until all appeared"""
    found, y = set(), 2
    while len(found) < 8:
        if is_square(x_squared(y)):
            x = sqrt(x_squared(y))
            found.add(mul(L, (x, y)))
            found.add(mul(L, (P - x, y)))
        y += 1
        assert y < 1000
    for pt in found:
        assert mul(8, pt) == (0, 1)
    return frozenset(found)


@functools.lru_cache(maxsize=None)
def small_order_ys():
    ys = frozenset(y for _, y in torsion_points())
    assert len(ys) == 5 and {0, 1, P - 1} <= ys
    return ys


def torsion_encodings():
    """every 32-byte string whose low 255 bits are = the y of a point of order dividing 8 (mod p), with either sign bit"""
    out = []
    for y in sorted(small_order_ys()):
        for v in (y, y + P):
            if v < 2**255:
                out += [v.to_bytes(32, "little"), (v | 1 << 255).to_bytes(32, "little")]
    assert len(out) == 14
    return out


# ---------------------------------------------------------------- the four predicates

@functools.lru_cache(maxsize=1 << 16)
def canonical(enc):
    """RFC 8032 5.1.3 decodes these 32 bytes: y < p, x^2 = (y^2 - 1) / (d y^2 + 1) is a square, not (x = 0 with the sign bit set)"""
    v = int.from_bytes(enc, "little")
    y, sign = v & (2**255 - 1), v >> 255
    if y >= P:
        return False
    xx = x_squared(y)
    assert (xx == 0) == (y in (1, P - 1))
    return is_square(xx) and not (xx == 0 and sign)


def small_order(enc):
    return (int.from_bytes(enc, "little") & (2**255 - 1)) % P in small_order_ys()


def holds(policy, sig, pub):
    """every predicate whose bit is in `policy` holds for the item (64-byte signature, 32-byte key)"""
    sig, pub = bytes(sig), bytes(pub)
    assert len(sig) == 64 and len(pub) == 32 and not policy & ~STRICT
    return not ((policy & S_BELOW_L and int.from_bytes(sig[32:], "little") >= L) or
                (policy & A_CANONICAL and not canonical(pub)) or
                (policy & A_NOT_SMALL and small_order(pub)) or
                (policy & R_NOT_SMALL and small_order(sig[:32])))


def holds_batch(policy, sig, pk):
    return np.array([holds(policy, sig[i].tobytes(), pk[i].tobytes()) for i in range(len(sig))], np.uint8)


# ---------------------------------------------------------------- shared inputs

def arr(rows):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1).copy()


def vector_cases(golden):
    """verify_edges.json + verify_torsion.json -> (cases, sig (n, 64), pub (n, 32), accept (n,))"""
    cases = golden("verify_edges.json") + golden("verify_torsion.json")
    return cases, arr([H(c["sig"]) for c in cases]), arr([H(c["pub"]) for c in cases]), np.array([c["accept"] for c in cases], np.uint8)


MLEN = 40
IDENTITY = (b"\x01" + bytes(31), b"\x01" + bytes(30) + b"\x80", (P + 1).to_bytes(32, "little"))   # canonical, sign bit set, y = p + 1


def clamped(seed):
    """the secret scalar of a 32-byte seed: the clamped low half of SHA-512(seed)"""
    a = int.from_bytes(hashlib.sha512(bytes(seed)).digest()[:32], "little")
    return a & ((1 << 254) - 8) | 1 << 254


def policy_batch(oracle, n, seed=20261019):
    """n items over MLEN-byte messages, by item index mod 8 -> (sig, pk, msg, the oracle's verdicts).
    0, 7: valid.  1: valid with S + k l (below 2^256).  2: A = the identity in its three encodings in turn, R = genpub(seed),
    S = a mod l (a = the seed's clamped scalar): S B = R + t * 0 whatever t is.  3: R = the identity under the genuine key,
    S = t a mod l with t = SHA-512(R || A || M) mod l: S B - t A = 0.  4: one signature bit flipped.  5: a random key.
    6: 1 and 2 together."""
    rng = np.random.default_rng(seed)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (n, MLEN), dtype=np.uint8)
    pk = oracle.genpub_batch(sk)
    sig = oracle.sign_batch(sk, pk, msg, MLEN)

    def put(row, value):
        row[:] = np.frombuffer(value.to_bytes(32, "little"), np.uint8)

    for i in range(n):
        k = i % 8
        if k in (1, 6):
            mult = int(rng.integers(1, 15))
        if k in (2, 6):
            a = clamped(sk[i])
            sig[i, :32] = pk[i]
            pk[i] = np.frombuffer(IDENTITY[(i // 8) % 3], np.uint8)
            put(sig[i, 32:], a % L + (mult * L if k == 6 else 0))
        elif k == 1:
            put(sig[i, 32:], int.from_bytes(sig[i, 32:].tobytes(), "little") + mult * L)
        elif k == 3:
            sig[i, :32] = np.frombuffer(IDENTITY[0], np.uint8)
            t = int.from_bytes(hashlib.sha512(sig[i, :32].tobytes() + pk[i].tobytes() + msg[i].tobytes()).digest(), "little") % L
            put(sig[i, 32:], t * clamped(sk[i]) % L)
        elif k == 4:
            sig[i, rng.integers(0, 64)] ^= 1 << rng.integers(0, 8)
        elif k == 5:
            pk[i] = rng.integers(0, 256, 32, dtype=np.uint8)
    want = oracle.verify_batch(sig, pk, msg, MLEN)
    for a in (sig, pk, msg, want):
        a.setflags(write=False)
    return sig, pk, msg, want
