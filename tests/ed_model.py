"""Ed25519 in Python integers, once: the field, the group law in affine and in extended coordinates, the two ways of reading 32
bytes as a point, the hashes and the reference's cofactorless verification.  Every feature model (policy_model, cofactored_model,
keyed_model, keyed_comb_model, dom2_model, sign_keyed_model) and every test that needs the curve takes it from here;
tests/test_ed_model.py anchors it against the oracle, RFC 8032 and the reference's recorded verdicts.  Nothing here comes from the
engine or from its source: l and p are the curve's, the small-order y values are found by multiplying curve points by l, the
square test is Euler's criterion.  Python integers, hashlib and numpy only."""
import functools
import hashlib

import numpy as np

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
MASK255 = 2**255 - 1
H = bytes.fromhex


# ---------------------------------------------------------------- bytes

def le(x, n=32):
    return int(x).to_bytes(n, "little")


def num(b):
    return int.from_bytes(b, "little")


def arr(rows, width=-1):
    """byte strings (or uint8 rows) of one length -> (len(rows), width) uint8, writable; `width` is needed only for no rows"""
    return np.frombuffer(b"".join(bytes(r) for r in rows), np.uint8).reshape(len(rows), width).copy()


def sha(*parts):
    return hashlib.sha512(b"".join(parts)).digest()


# ---------------------------------------------------------------- the field

def inv(x):
    """1 / x, and 0 for x = 0 as in the reference (fld_inv)"""
    return pow(x, P - 2, P)


D = -121665 * inv(121666) % P
D2 = 2 * D % P
SQRT_M1 = pow(2, (P - 1) // 4, P)


def x_squared(y):
    return (y * y - 1) * inv(D * y * y + 1) % P


def is_square(v):
    return v == 0 or pow(v, (P - 1) // 2, P) == 1


def sqrt(v):
    """a root of the square v (p = 5 mod 8)"""
    r = pow(v, (P + 3) // 8, P)
    if r * r % P != v:
        r = r * SQRT_M1 % P
    assert r * r % P == v
    return r


# ---------------------------------------------------------------- the curve -x^2 + y^2 = 1 + d x^2 y^2, affine (x, y)

def add(a, b):
    """the complete addition"""
    (x1, y1), (x2, y2) = a, b
    k = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * inv(1 + k) % P, (y1 * y2 + x1 * x2) * inv(1 - k) % P)


def mul(k, pt):
    acc = (0, 1)
    while k:
        if k & 1:
            acc = add(acc, pt)
        pt = add(pt, pt)
        k >>= 1
    return acc


# ---------------------------------------------------------------- the same group in extended coordinates (X : Y : Z : T), a = -1

NEUTRAL = (0, 1, 1, 0)


def padd(p, q):
    """add-2008-hwcd-3: complete on this curve, so p = q and p = -q need no case"""
    x1, y1, z1, t1 = p
    x2, y2, z2, t2 = q
    a, b = (y1 - x1) * (y2 - x2) % P, (y1 + x1) * (y2 + x2) % P
    c, d = t1 * D2 % P * t2 % P, 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def pdbl(p):
    x1, y1, z1, _ = p
    a, b, c = x1 * x1 % P, y1 * y1 % P, 2 * z1 * z1 % P
    e, g, h = ((x1 + y1) ** 2 - a - b) % P, (b - a) % P, (-a - b) % P
    f = (g - c) % P
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def pneg(p):
    return (-p[0] % P, p[1], p[2], -p[3] % P)


def ext(pt):
    return (pt[0], pt[1], 1, pt[0] * pt[1] % P)


def affine(p):
    zi = inv(p[2])
    return (p[0] * zi % P, p[1] * zi % P)


def is_neutral(p):
    return p[0] % P == 0 and (p[1] - p[2]) % P == 0 and p[2] % P != 0


def pmul(k, p):
    acc = NEUTRAL
    for bit in bin(k)[2:] if k else "":
        acc = pdbl(acc)
        if bit == "1":
            acc = padd(acc, p)
    return acc


def pmul2(k1, p1, k2, p2):
    """k1 p1 + k2 p2 in one pass over the bits"""
    both = padd(p1, p2)
    acc = NEUTRAL
    for i in range(max(k1.bit_length(), k2.bit_length()) - 1, -1, -1):
        acc = pdbl(acc)
        pick = (k1 >> i & 1) | (k2 >> i & 1) << 1
        if pick:
            acc = padd(acc, (p1, p2, both)[pick - 1])
    return acc


def encode(p):
    x, y = affine(p)
    return le(y | (x & 1) << 255)


BY = 4 * inv(5) % P
BX = sqrt(x_squared(BY))
BX = BX if BX % 2 == 0 else P - BX
B = ext((BX, BY))


# ---------------------------------------------------------------- 32 bytes as a point

def decode_reference(enc):
    """the reference's import -> (x, y), or None when y is on no curve point: y = the low 255 bits mod p, x the root of
    u / w = (y^2 - 1) / (d y^2 + 1) whose parity is the sign bit; the sign bit is applied also when x = 0 (where it changes
    nothing).  The root by the one exponentiation of RFC 8032 5.1.3: u w^3 (u w^7)^((p - 5) / 8), times sqrt(-1) if need be"""
    v = num(enc)
    y, sign = (v & MASK255) % P, v >> 255
    u, w = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(w, 3, P) * pow(u * pow(w, 7, P) % P, (P - 5) // 8, P) % P
    if (w * x * x - u) % P:
        x = x * SQRT_M1 % P
    if (w * x * x - u) % P:
        return None
    return (-x % P if x & 1 != sign else x, y)


def decode_strict(enc):
    """RFC 8032 5.1.3 -> (x, y), or None: as above, but y >= p is refused, and so is x = 0 with the sign bit set"""
    v = num(enc)
    pt = decode_reference(enc) if v & MASK255 < P else None
    return None if pt is None or (pt[0] == 0 and v >> 255) else pt


# ---------------------------------------------------------------- the hashes

DOM2_TAG = b"SigEd25519 no Ed25519 collisions"


def dom2(flag, context):
    """the prefix of Ed25519ctx (flag 0) and Ed25519ph (flag 1), RFC 8032 5.1"""
    assert flag in (0, 1) and len(context) <= 255
    return DOM2_TAG + bytes([flag, len(context)]) + bytes(context)


def challenge(sig, pub, msg, prefix=b""):
    """t = SHA-512(prefix | R | A | M) mod l"""
    return num(sha(prefix, bytes(sig[:32]), bytes(pub), bytes(msg))) % L


def clamped(seed):
    """the secret scalar of a 32-byte seed: the clamped low half of SHA-512(seed)"""
    return num(sha(bytes(seed))[:32]) & ((1 << 254) - 8) | 1 << 254


# ---------------------------------------------------------------- the points of order dividing 8

@functools.lru_cache(maxsize=None)
def torsion_points():
    """the eight of them, affine: l times a curve point is one; curve points with y = 2, 3, .. until all appeared"""
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
                out += [le(v), le(v | 1 << 255)]
    assert len(out) == 14
    return out


# ---------------------------------------------------------------- verification

def verify_t(sig, pub, t):
    """the reference's cofactorless rule for a key that decodes, with the challenge scalar t given: the encoding of
    S B + t (-A) is R, byte for byte (S is used as its 256 bits say: B has order l, so S and S mod l give the same point)"""
    sig, pub = bytes(sig), bytes(pub)
    a = decode_reference(pub)
    assert a is not None, "a key on no curve point belongs to the exact path, not to this model"
    return encode(pmul2(num(sig[32:]), B, t, pneg(ext(a)))) == sig[:32]


def verify(sig, pub, msg, prefix=b""):
    """the same rule with t = SHA-512(prefix | R | A | M) mod l"""
    return verify_t(sig, pub, challenge(sig, pub, msg, prefix))
