"""[m]P + [a]B (include/eddsa_amd.h: ed25519_point_muladd_batch) in Python integers: the vectors the CPU and the GPU tests share and
the 32 bytes each must give, from tests/ed_model.py alone - decode_reference, pmul, padd, encode, torsion_points.  m and a are
integers in [0, 2^256), used as they are: nothing is reduced here, so a reduction the engine must not make (m mod l on a point with
torsion) shows as a mismatch.  Nothing here comes from the engine.  Built once per process (about 3.5 ms of Python per item)."""
import functools

import numpy as np

import ed_model as em

NO_POINT = bytes([2]) + bytes(31)                    # y = 2: on no curve point
NEUTRAL = em.le(1)
L = em.L
SCALARS = (0, 1, 2, 7, 8, L - 1, L, L + 1, 4 * L - 1, 4 * L, 4 * L + 1, 8 * L - 1, 8 * L, 8 * L + 1,
           2**252, 2**255 - 1, 2**255, 2**256 - 1)


@functools.lru_cache(maxsize=None)
def _base_multiple(a):
    return em.pmul(a, em.B)


@functools.lru_cache(maxsize=None)
def one(point, m, a):
    """the 32 bytes of [m]P + [a]B for P = the 32 bytes `point`; NO_POINT when they are no curve point"""
    pt = em.decode_reference(point)
    if pt is None:
        return NO_POINT
    return em.encode(em.padd(em.pmul(m, em.ext(pt)), _base_multiple(a)))


def expected(points, mul=None, add=None):
    """points (n, 32) uint8; mul, add (n, 32) uint8 or None (every m = 1, every a = 0) -> (n, 32) uint8"""
    points = np.asarray(points).reshape(-1, 32)
    n = points.shape[0]
    ms = [1] * n if mul is None else [em.num(r.tobytes()) for r in np.asarray(mul).reshape(-1, 32)]
    az = [0] * n if add is None else [em.num(r.tobytes()) for r in np.asarray(add).reshape(-1, 32)]
    assert len(ms) == n and len(az) == n
    return em.arr([one(points[i].tobytes(), ms[i], az[i]) for i in range(n)], 32)


def encode_affine(pt):
    return em.le(pt[1] | (pt[0] & 1) << 255)


def order_of(enc):
    """the order of a point of the torsion subgroup given by its encoding: 1, 2, 4 or 8"""
    pt, k = em.ext(em.decode_reference(enc)), 1
    acc = pt
    while not em.is_neutral(acc):
        acc, k = em.pdbl(acc), 2 * k
    assert k <= 8
    return k


@functools.lru_cache(maxsize=None)
def vectors():
    """-> (names, points (n, 32), mul (n, 32), add (n, 32), out (n, 32)), uint8 and read-only; out = expected(points, mul, add)"""
    rows = []                                        # (name, 32 bytes of P, m, a)
    rng = np.random.default_rng(0x25519ADD)
    rand256 = lambda: em.num(rng.integers(0, 256, 32, dtype=np.uint8).tobytes())   # noqa: E731

    def put(name, point, m, a):
        assert 0 <= m < 2**256 and 0 <= a < 2**256, name
        rows.append((name, bytes(point), m, a))

    torsion = sorted(em.torsion_points())
    base = em.affine(em.B)
    kb = {k: em.mul(k, base) for k in (1, 2, 3, 7, 0x1234567)}
    # 1: k B + T for all eight torsion points T: small, boundary and random scalars on points with and without torsion
    mixed = {}
    for k, kpt in kb.items():
        for t, tp in enumerate(torsion):
            enc = encode_affine(em.add(kpt, tp))
            mixed[k, t] = enc
            put(f"{k} B + T{t}, random m, random a", enc, rand256(), rand256())
            put(f"{k} B + T{t}, m = {k + t}, a = 0", enc, k + t, 0)
    # 2: every scalar of the list as m and as a, on a point that carries torsion of order 8 where one exists
    order8 = [t for t, tp in enumerate(torsion) if order_of(encode_affine(tp)) == 8]
    assert len(order8) == 4
    for i, s in enumerate(SCALARS):
        enc = mixed[3, order8[i % 4]]
        put(f"scalar {i} as m on 3 B + T{order8[i % 4]}", enc, s, SCALARS[(i + 5) % len(SCALARS)])
        put(f"scalar {i} as a on 7 B + T{order8[(i + 1) % 4]}", mixed[7, order8[(i + 1) % 4]], SCALARS[(i + 11) % len(SCALARS)], s)
        put(f"scalar {i} as m on B", mixed[1, torsion.index((0, 1))], s, 0)
    # 3: the torsion encodings (14), the neutral element, x = 0 with the sign bit set, the non-canonical y = p + j
    for k, enc in enumerate(em.torsion_encodings()):
        put(f"torsion encoding {k}, m = 1, a = 0", enc, 1, 0)
        put(f"torsion encoding {k}, random m, random a", enc, rand256(), rand256())
    put("neutral, random m, random a", NEUTRAL, rand256(), rand256())
    put("neutral, m = 1, a = 0", NEUTRAL, 1, 0)
    for y, name in ((1, "y = 1"), (em.P - 1, "y = -1")):
        put(f"{name}, sign 1, m = 1, a = 0", em.le(y | 1 << 255), 1, 0)
        put(f"{name}, sign 1, m = 3, a = 5", em.le(y | 1 << 255), 3, 5)
    on = 0
    for y in range(em.P, 2**255):                    # the 19 non-canonical y, either sign bit
        on += em.decode_reference(em.le(y)) is not None
        for sign in (0, 1):
            put(f"y = p + {y - em.P}, sign {sign}", em.le(y | sign << 255), rand256() if y & 1 else 1, rand256() if y & 2 else 0)
    assert on == 12
    # 4: strings that are no curve point: the no-point string itself and random ones, under every kind of scalar
    put("the no-point string, m = 1, a = 0", NO_POINT, 1, 0)
    put("the no-point string, random m, random a", NO_POINT, rand256(), rand256())
    off = 0
    while off < 12:
        enc = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        if em.decode_reference(enc) is None:
            put(f"random string off the curve {off}", enc, SCALARS[off % len(SCALARS)] if off % 3 else rand256(), rand256())
            off += 1
    for k in range(24):
        enc = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        put(f"random string {k}", enc, rand256(), rand256())
    # 5: the required pairs
    for t in order8[:2] + [t for t in range(8) if t not in order8 and torsion[t] != (0, 1)][:2]:
        m = rand256() >> 4
        put(f"pair mod l: 2 B + T{t}, m", mixed[2, t], m, 9)
        put(f"pair mod l: 2 B + T{t}, m + l", mixed[2, t], m + L, 9)
        put(f"pair mod 8l: 2 B + T{t}, m", mixed[2, t], m, 9)
        put(f"pair mod 8l: 2 B + T{t}, m + 8 l", mixed[2, t], m + 8 * L, 9)
    plain = torsion.index((0, 1))
    for k in kb:
        put(f"{k} B, m = 1, a = l - {k}: the neutral element", mixed[k, plain], 1, L - k)
    for t, tp in enumerate(torsion):                 # k B + T - k B = T: every torsion point as a result, x = 0 or y = 0 among them
        put(f"3 B + T{t}, m = 1, a = l - 3: T{t}", mixed[3, t], 1, L - 3)
    t8 = encode_affine(torsion[order8[0]])
    put("a point of order 8, m = 2: order 4", t8, 2, 0)
    put("a point of order 8, m = 4: order 2", t8, 4, 0)
    put("a point of order 8, m = 2 + 8 l, a = l: order 4", t8, 2 + 8 * L, L)

    names = [r[0] for r in rows]
    assert len(set(names)) == len(names)
    points = em.arr([r[1] for r in rows], 32)
    mul = em.arr([em.le(r[2]) for r in rows], 32)
    add = em.arr([em.le(r[3]) for r in rows], 32)
    out = expected(points, mul, add)
    by = {n: out[i].tobytes() for i, n in enumerate(names)}
    # what the pairs are there to show, asserted on the model itself
    for n in names:
        if n.startswith("pair mod l:") and n.endswith(", m"):
            assert by[n] != by[n + " + l"], n        # a reduction mod l would make these equal
        if n.startswith("pair mod 8l:") and n.endswith(", m"):
            assert by[n] == by[n + " + 8 l"], n
        if n.endswith("the neutral element"):
            assert by[n] == NEUTRAL, n
    orders = sorted(order_of(by[f"3 B + T{t}, m = 1, a = l - 3: T{t}"]) for t in range(8))
    assert orders == [1, 2, 4, 4, 8, 8, 8, 8]
    assert order_of(by["a point of order 8, m = 2: order 4"]) == 4 and order_of(by["a point of order 8, m = 4: order 2"]) == 2
    assert by["a point of order 8, m = 2 + 8 l, a = l: order 4"] == by["a point of order 8, m = 2: order 4"]
    assert em.num(by["a point of order 8, m = 4: order 2"]) == em.P - 1                          # (0, -1): x = 0
    assert em.num(by["a point of order 8, m = 2: order 4"]) & em.MASK255 == 0                    # (+-sqrt(-1), 0): y = 0
    for a in (points, mul, add, out):
        a.setflags(write=False)
    return names, points, mul, add, out


def mismatches(got, want, names=None):
    """the first items whose 32 bytes are not the expected ones, readable"""
    got, want = np.asarray(got).reshape(-1, 32), np.asarray(want).reshape(-1, 32)
    assert got.shape == want.shape, (got.shape, want.shape)
    at = np.nonzero((got != want).any(axis=1))[0][:6]
    return [(int(i), names[i % len(names)] if names else None, got[i].tobytes().hex(), want[i].tobytes().hex()) for i in at]
