"""The opt-in strict rules of verification (include/eddsa_amd.h: EDDSA_AMD_VERIFY_*) in Python integers, and the inputs the
policy tests share (tests/test_policy_lane_on_host.py on the CPU, tests/test_gpu_policy.py on the GPU).  The curve, the strict
decoder and the points of small order are those of tests/ed_model.py."""
import functools

import numpy as np

from ed_model import H, L, P, arr, challenge, clamped, decode_strict, le, num, small_order_ys
from ed_model import D, add, is_square, mul, sqrt, torsion_encodings, torsion_points, x_squared  # noqa: F401  (for this model's users)

S_BELOW_L, A_CANONICAL, A_NOT_SMALL, R_NOT_SMALL, STRICT = 0x100, 0x200, 0x400, 0x800, 0xF00
BITS = (S_BELOW_L, A_CANONICAL, A_NOT_SMALL, R_NOT_SMALL)
POLICIES = (0,) + BITS + (STRICT,)


# ---------------------------------------------------------------- the four predicates

@functools.lru_cache(maxsize=1 << 16)
def canonical(enc):
    """RFC 8032 5.1.3 decodes these 32 bytes: y < p, x^2 = (y^2 - 1) / (d y^2 + 1) is a square, not (x = 0 with the sign bit set)"""
    return decode_strict(enc) is not None


def small_order(enc):
    return (num(enc) & (2**255 - 1)) % P in small_order_ys()


def holds(policy, sig, pub):
    """every predicate whose bit is in `policy` holds for the item (64-byte signature, 32-byte key)"""
    sig, pub = bytes(sig), bytes(pub)
    assert len(sig) == 64 and len(pub) == 32 and not policy & ~STRICT
    return not ((policy & S_BELOW_L and num(sig[32:]) >= L) or
                (policy & A_CANONICAL and not canonical(pub)) or
                (policy & A_NOT_SMALL and small_order(pub)) or
                (policy & R_NOT_SMALL and small_order(sig[:32])))


def holds_batch(policy, sig, pk):
    return np.array([holds(policy, sig[i].tobytes(), pk[i].tobytes()) for i in range(len(sig))], np.uint8)


# ---------------------------------------------------------------- shared inputs

def vector_cases(golden):
    """verify_edges.json + verify_torsion.json -> (cases, sig (n, 64), pub (n, 32), accept (n,))"""
    cases = golden("verify_edges.json") + golden("verify_torsion.json")
    return cases, arr([H(c["sig"]) for c in cases]), arr([H(c["pub"]) for c in cases]), np.array([c["accept"] for c in cases], np.uint8)


MLEN = 40
IDENTITY = (b"\x01" + bytes(31), b"\x01" + bytes(30) + b"\x80", le(P + 1))   # canonical, sign bit set, y = p + 1


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
        row[:] = np.frombuffer(le(value), np.uint8)

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
            put(sig[i, 32:], num(sig[i, 32:].tobytes()) + mult * L)
        elif k == 3:
            sig[i, :32] = np.frombuffer(IDENTITY[0], np.uint8)
            t = challenge(sig[i], pk[i], msg[i])
            put(sig[i, 32:], t * clamped(sk[i]) % L)
        elif k == 4:
            sig[i, rng.integers(0, 64)] ^= 1 << rng.integers(0, 8)
        elif k == 5:
            pk[i] = rng.integers(0, 256, 32, dtype=np.uint8)
    want = oracle.verify_batch(sig, pk, msg, MLEN)
    for a in (sig, pk, msg, want):
        a.setflags(write=False)
    return sig, pk, msg, want
