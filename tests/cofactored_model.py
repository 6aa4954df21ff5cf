"""The opt-in cofactored equation of verification (include/eddsa_amd.h: eddsa_amd_set_verify_equation, the rules of ZIP-215)
in Python integers, and the vectors the cofactored tests share (tests/test_cofactor_lane_on_host.py on the CPU,
tests/test_gpu_cofactored.py on the GPU).  The curve, the decoder and the hashes are those of tests/ed_model.py.

An item (R | S, A, M) is accepted exactly when S < l, A and R decode - y = the low 255 bits mod p, (y^2 - 1) / (d y^2 + 1) a
square, x takes the sign bit, x = 0 takes either - and [8]([S]B - [t]A - R) is the neutral element with
t = SHA-512(prefix | R | A | M) mod l (prefix: empty, or dom2 of Ed25519ctx / Ed25519ph)."""
import random

import numpy as np

import ed_model as em
from ed_model import B, L, P, affine, arr, challenge, dom2, encode, ext, is_neutral, le, num, padd, pdbl, pmul, pmul2, pneg  # noqa: F401


def decode(enc):
    """the point of these 32 bytes under the permissive rule (x = 0 takes either sign bit), or None when y is on no curve point"""
    pt = em.decode_reference(enc)
    return None if pt is None else ext(pt)


# ---------------------------------------------------------------- the rule

def accepts_t(sig, pub, t):
    """the cofactored verdict of (sig, pub) with the challenge scalar t given"""
    sig, pub = bytes(sig), bytes(pub)
    s = num(sig[32:])
    if s >= L:
        return False
    a, r = decode(pub), decode(sig[:32])
    if a is None or r is None:
        return False
    q = padd(pmul2(s, B, t, pneg(a)), pneg(r))
    return is_neutral(pdbl(pdbl(pdbl(q))))


def accepts(sig, pub, msg, prefix=b""):
    return accepts_t(sig, pub, challenge(sig, pub, msg, prefix))


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
        return renc + le((r + t * a) % L), pub

    tors = em.torsion_encodings()
    for a_enc in tors:
        for r_enc in tors:
            put(CLASSES[0], r_enc + bytes(32), a_enc, rng.randbytes(mlen))
    honest_items = []
    for _ in range(honest):
        a, r, msg = _scalar(rng), _scalar(rng), rng.randbytes(mlen)
        sig, pub = sign(a, pmul(a, B), r, pmul(r, B), msg)
        honest_items.append((sig, pub, msg))
        put(CLASSES[1], sig, pub, msg)
    small = [ext(pt) for pt in sorted(em.torsion_points()) if pt != (0, 1)]
    mixed_items = []
    for t_a in small:
        for t_r in small:
            a, r, msg = _scalar(rng), _scalar(rng), rng.randbytes(mlen)
            sig, pub = sign(a, padd(pmul(a, B), t_a), r, padd(pmul(r, B), t_r), msg)
            mixed_items.append((sig, pub, msg))
            put(CLASSES[2], sig, pub, msg)
    for k, (sig, pub, msg) in enumerate(honest_items):
        s = num(sig[32:]) + (k % 14 + 1) * L
        if s >= 2**256:
            s = num(sig[32:]) + L
        put(CLASSES[3], sig[:32] + le(s), pub, msg)
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
        s = num(sig[32:]) + L
        put(CLASSES[6], sig[:32] + le(s), pub, msg)
    return out


def as_json(vecs):
    return [{"sig": v["sig"].hex(), "pub": v["pub"].hex(), "msg": v["msg"].hex(), "accept": int(v["accept"]), "class": v["class"]}
            for v in vecs]


def from_json(rows):
    return [{"sig": bytes.fromhex(r["sig"]), "pub": bytes.fromhex(r["pub"]), "msg": bytes.fromhex(r["msg"]),
             "accept": bool(r["accept"]), "class": r["class"]} for r in rows]


def arrays(vecs):
    """-> sig (n, 64), pub (n, 32), msg (n, mlen), accept (n,) as uint8, read-only"""
    out = (arr([v["sig"] for v in vecs]), arr([v["pub"] for v in vecs]), arr([v["msg"] for v in vecs]),
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
