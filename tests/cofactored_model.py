"""The opt-in cofactored equation of verification (include/eddsa_amd.h: eddsa_amd_set_verify_equation, the rules of ZIP-215)
in Python integers, and the vectors the cofactored tests share (tests/test_cofactor_lane_on_host.py on the CPU,
tests/test_gpu_cofactored.py on the GPU).  Nothing here comes from the engine or from its source: the curve helpers are those
of tests/policy_model.py, the group law is the textbook extended-coordinates one (checked against that file's affine law by the
CPU test), SHA-512 is hashlib's.

An item (R | S, A, M) is accepted exactly when S < l, A and R decode - y = the low 255 bits mod p, (y^2 - 1) / (d y^2 + 1) a
square, x takes the sign bit, x = 0 takes either - and [8]([S]B - [t]A - R) is the neutral element with
t = SHA-512(prefix | R | A | M) mod l (prefix: empty, or dom2 of Ed25519ctx / Ed25519ph)."""
import hashlib
import random

import numpy as np

import policy_model as pm
from policy_model import D, L, P

D2 = 2 * D % P
NEUTRAL = (0, 1, 1, 0)
DOM2_TAG = b"SigEd25519 no Ed25519 collisions"


# ---------------------------------------------------------------- the group in extended coordinates (X : Y : Z : T), a = -1

def padd(p, q):
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
    zi = pow(p[2], -1, P)
    return (p[0] * zi % P, p[1] * zi % P)


def is_neutral(p):
    return p[0] % P == 0 and (p[1] - p[2]) % P == 0


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


BY = 4 * pow(5, -1, P) % P
BX = pm.sqrt(pm.x_squared(BY))
BX = BX if BX % 2 == 0 else P - BX
B = ext((BX, BY))


def encode(p):
    x, y = affine(p)
    return (y | (x & 1) << 255).to_bytes(32, "little")


def decode(enc):
    """the point of these 32 bytes under the permissive rule, or None when y is on no curve point"""
    v = int.from_bytes(enc, "little")
    y, sign = (v & (2**255 - 1)) % P, v >> 255
    xx = pm.x_squared(y)
    if not pm.is_square(xx):
        return None
    x = pm.sqrt(xx)
    if x & 1 != sign:
        x = -x % P                                  # (x = 0 stays 0 under either sign bit)
    return ext((x, y))


# ---------------------------------------------------------------- the rule

def challenge(sig, pub, msg, prefix=b""):
    return int.from_bytes(hashlib.sha512(prefix + bytes(sig[:32]) + bytes(pub) + bytes(msg)).digest(), "little") % L


def accepts_t(sig, pub, t):
    """the cofactored verdict of (sig, pub) with the challenge scalar t given"""
    sig, pub = bytes(sig), bytes(pub)
    s = int.from_bytes(sig[32:], "little")
    if s >= L:
        return False
    a, r = decode(pub), decode(sig[:32])
    if a is None or r is None:
        return False
    q = padd(pmul2(s, B, t, pneg(a)), pneg(r))
    return is_neutral(pdbl(pdbl(pdbl(q))))


def accepts(sig, pub, msg, prefix=b""):
    return accepts_t(sig, pub, challenge(sig, pub, msg, prefix))


def dom2(flag, context):
    return DOM2_TAG + bytes([flag, len(context)]) + bytes(context)


# ---------------------------------------------------------------- the vectors

CLASSES = ("a_torsion", "b_honest", "c_mixed", "d_s_plus_kl", "e_bit_flip", "f_off_curve", "g_mixed_s_plus_l")


def _scalar(rng):
    return rng.randrange(1, L)


def _off_curve(rng):
    while True:
        enc = rng.randbytes(32)
        if decode(enc) is None:
            return enc


def vectors(prefix=b"", mlen=32, honest=16, seed=20261019):
    """-> list of dicts {sig, pub, msg (bytes), accept (the cofactored verdict, by the model), class}, all over mlen-byte
    messages hashed under `prefix`.
    a: the 14 x 14 encodings of the points of order dividing 8 as A and as R, S = 0 - accepted.
    b: honest signatures - accepted.  c: A = a B + T, R = r B + T' with T, T' running over the seven points of order 2, 4 and 8,
    S = r + t a mod l - accepted; the cofactorless check accepts only when t T + T' = 0.
    d: b with S + k l < 2^256.  e: b with one bit of the signature flipped.  f: A off the curve; R off the curve.
    g: c with S + l.  d - g are rejected."""
    rng = random.Random(seed)
    out = []

    def put(cls, sig, pub, msg):
        out.append({"sig": sig, "pub": pub, "msg": msg, "class": cls, "accept": accepts(sig, pub, msg, prefix)})

    def sign(a, pub_pt, r, r_pt, msg):
        pub, renc = encode(pub_pt), encode(r_pt)
        t = challenge(renc, pub, msg, prefix)
        return renc + ((r + t * a) % L).to_bytes(32, "little"), pub

    tors = pm.torsion_encodings()
    for a_enc in tors:
        for r_enc in tors:
            put(CLASSES[0], r_enc + bytes(32), a_enc, rng.randbytes(mlen))
    honest_items = []
    for _ in range(honest):
        a, r, msg = _scalar(rng), _scalar(rng), rng.randbytes(mlen)
        sig, pub = sign(a, pmul(a, B), r, pmul(r, B), msg)
        honest_items.append((sig, pub, msg))
        put(CLASSES[1], sig, pub, msg)
    small = [ext(pt) for pt in sorted(pm.torsion_points()) if pt != (0, 1)]
    mixed_items = []
    for t_a in small:
        for t_r in small:
            a, r, msg = _scalar(rng), _scalar(rng), rng.randbytes(mlen)
            sig, pub = sign(a, padd(pmul(a, B), t_a), r, padd(pmul(r, B), t_r), msg)
            mixed_items.append((sig, pub, msg))
            put(CLASSES[2], sig, pub, msg)
    for k, (sig, pub, msg) in enumerate(honest_items):
        s = int.from_bytes(sig[32:], "little") + (k % 14 + 1) * L
        if s >= 2**256:
            s = int.from_bytes(sig[32:], "little") + L
        put(CLASSES[3], sig[:32] + s.to_bytes(32, "little"), pub, msg)
    for sig, pub, msg in honest_items:
        bit = rng.randrange(512)
        flipped = bytearray(sig)
        flipped[bit >> 3] ^= 1 << (bit & 7)
        put(CLASSES[4], bytes(flipped), pub, msg)
    for k, (sig, pub, msg) in enumerate(honest_items[:8]):
        if k % 2:
            put(CLASSES[5], _off_curve(rng) + sig[32:], pub, msg)
        else:
            put(CLASSES[5], sig, _off_curve(rng), msg)
    for sig, pub, msg in mixed_items:
        s = int.from_bytes(sig[32:], "little") + L
        put(CLASSES[6], sig[:32] + s.to_bytes(32, "little"), pub, msg)
    return out


def as_json(vecs):
    return [{"sig": v["sig"].hex(), "pub": v["pub"].hex(), "msg": v["msg"].hex(), "accept": int(v["accept"]), "class": v["class"]}
            for v in vecs]


def from_json(rows):
    return [{"sig": bytes.fromhex(r["sig"]), "pub": bytes.fromhex(r["pub"]), "msg": bytes.fromhex(r["msg"]),
             "accept": bool(r["accept"]), "class": r["class"]} for r in rows]


def arrays(vecs):
    """-> sig (n, 64), pub (n, 32), msg (n, mlen), accept (n,) as uint8, read-only"""
    out = (pm.arr([v["sig"] for v in vecs]), pm.arr([v["pub"] for v in vecs]), pm.arr([v["msg"] for v in vecs]),
           np.array([v["accept"] for v in vecs], np.uint8))
    for a in out:
        a.setflags(write=False)
    return out


def tiled(arrs, n, seed=1):
    """the vectors tiled to n items and shuffled -> (sig, pub, msg, accept, the vector each item is)"""
    count = len(arrs[0])
    rng = np.random.default_rng(seed)
    pick = rng.permutation(rng.permutation(count)[np.arange(n) % count])
    return tuple(np.ascontiguousarray(a[pick]) for a in arrs) + (pick,)
