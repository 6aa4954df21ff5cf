"""X25519 on low-order and non-canonical points: a plain model of the operation, two pools of inputs, and placements that
put a zero denominator into chosen slots of the finish kernel's shared inversion (csrc/kernels.hip: finish_batch8,
x25519_finish_policy).  Pure Python integers and numpy indexing; no GPU, no library of the project.

model()                 the RFC 7748 ladder with this project's input rule, on Python integers: (x2, z2, out32)
DEGENERATE              the twelve 32-byte spellings of the five u-coordinates of order dividing 8 (z2 = 0, out = 0)
ORDINARY                60 inputs whose z2 is not 0: random points on the curve and on the twist, small and extreme u,
                        scalars 0, all-ones, 2^254, 8 and random ones
place(n, K)             a pool entry for every item of a pass of n items whose finish shares an inversion between K items:
                        in lane group (block b, lane t) exactly the slots named by the bits of (t + b) mod 2^K are degenerate
place_all_degenerate(n) every item degenerate: every shared product is 1
"""
import hashlib

import numpy as np

P = 2**255 - 19
A24 = 121665
BLOCK = 256                     # lanes of a tile of the point workspace (csrc/kernel_io.h: acc_column)

# the two u-coordinates of order 8 (the values tests/test_gpu_parity.py: test_x25519_random names)
ORDER8 = (325606250916557431795983626356110631294008115727848805560023387167927233504,
          39382357235489614581723060781553021112529911719440698176882885853963445705823)


def le(x, n=32):
    return int(x).to_bytes(n, "little")


def clamp(scalar32):
    """lib/x25519.c:137-140"""
    k = int.from_bytes(scalar32, "little")
    return (k & ~7 & (2**255 - 1)) | 2**254


def fold(point32):
    """the field's import: bit 255 is not masked but folded in as +19"""
    v = int.from_bytes(point32, "little")
    return ((v % 2**255) + 19 * (v >> 255)) % P


def model(scalar32, point32):
    """(x2, z2, out32): the ladder of RFC 7748 section 5 from bit 254 down on the clamped scalar, (x2 : z2) before the
    inversion, and out = x2 * z2^(p-2) mod p (0 when z2 = 0)"""
    k, x1 = clamp(scalar32), fold(point32)
    x2, z2, x3, z3, swap = 1, 0, x1, 1, 0
    for t in range(254, -1, -1):
        bit = (k >> t) & 1
        swap ^= bit
        if swap:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = bit
        a, b, c, d = (x2 + z2) % P, (x2 - z2) % P, (x3 + z3) % P, (x3 - z3) % P
        aa, bb, da, cb = a * a % P, b * b % P, d * a % P, c * b % P
        e = (aa - bb) % P
        x3, z3 = (da + cb) ** 2 % P, x1 * (da - cb) ** 2 % P
        x2, z2 = aa * bb % P, e * (aa + A24 * e) % P
    if swap:
        x2, x3, z2, z3 = x3, x2, z3, z2
    return x2, z2, le(x2 * pow(z2, P - 2, P) % P)


def _bytes(tag, i):
    return hashlib.sha512(b"libeddsa-amd x25519 cases " + tag + i.to_bytes(4, "little")).digest()[:32]


def on_curve(u):
    """u is the u-coordinate of a point of the curve v^2 = u^3 + 486662 u^2 + u (otherwise: of its twist)"""
    rhs = (u * u * u + 486662 * u * u + u) % P
    return rhs == 0 or pow(rhs, (P - 1) // 2, P) == 1


ONES = b"\xff" * 32
_SCALARS = (le(0), ONES, le(2**254), le(8))


def _degenerate_points():
    ws = (0, 1, P - 1) + ORDER8
    pts = [le(w) for w in ws]                                          # each canonical value
    pts += [le(w + P) for w in ws if w + P < 2**255]                   # p and p + 1
    pts += [le(((w - 19) % P) | 2**255) for w in ws]                   # bit 255 set: folded in as + 19
    return pts


def _ordinary_points():
    pts = [le(2), le(9), le(P - 2), le(2**255 - 1), le(2**256 - 1), bytes.fromhex("aa" * 32), bytes.fromhex("55" * 32)]
    curve, twist, i = [], [], 0
    while len(curve) < 4 or len(twist) < 4:
        b = _bytes(b"point", i)
        i += 1
        side = curve if on_curve(fold(b)) else twist
        if len(side) < 4:
            side.append(b)
    return pts + curve + twist


def _pool(points, rounds, tag):
    """every point under `rounds` scalars: the four fixed ones and a fresh random one, taken in turn"""
    out = []
    for j in range(rounds * len(points)):
        kind = (j % len(points) + j // len(points)) % 5
        out.append((_SCALARS[kind] if kind < 4 else _bytes(tag, j), points[j % len(points)]))
    return out


DEGENERATE = _pool(_degenerate_points(), 1, b"degenerate scalar")
ORDINARY = _pool(_ordinary_points(), 4, b"ordinary scalar")
assert len(DEGENERATE) == 12 and len({p for _, p in DEGENERATE}) == 12 and len(ORDINARY) == 60
DEGENERATE_MODEL = [model(s, p) for s, p in DEGENERATE]
ORDINARY_MODEL = [model(s, p) for s, p in ORDINARY]
assert all(z2 == 0 and out == bytes(32) for _, z2, out in DEGENERATE_MODEL)
assert all(z2 != 0 for _, z2, _ in ORDINARY_MODEL)
assert {fold(p) for _, p in DEGENERATE} == {0, 1, P - 1} | set(ORDER8)


def _rows(rows):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), 32).copy()


# the two pools in one table: entries 0 .. 11 degenerate, 12 .. 71 ordinary
_N_DEG, _N_ORD = len(DEGENERATE), len(ORDINARY)
_POOL_SC = _rows([s for s, _ in DEGENERATE + ORDINARY])
_POOL_PT = _rows([p for _, p in DEGENERATE + ORDINARY])
_POOL_OUT = _rows([m[2] for m in DEGENERATE_MODEL + ORDINARY_MODEL])
_DEG_STRIDE, _ORD_STRIDE = 5, 7                                       # coprime to 12 and to 60: every entry occurs in every slot
assert np.gcd(_DEG_STRIDE, _N_DEG) == 1 and np.gcd(_ORD_STRIDE, _N_ORD) == 1


def layout(i, K):
    """(tile, lane, block, slot) of item i in the finish kernel of a pass that shares an inversion between K items
    (csrc/kernels.hip: finish_at); i may be an array"""
    tile, lane = i // BLOCK, i % BLOCK
    return tile, lane, tile // K, tile % K


def degenerate_mask(n, K):
    """item i is degenerate exactly when bit `slot` of (lane + block) mod 2^K is set"""
    _, lane, block, slot = layout(np.arange(n, dtype=np.int64), K)
    return (((lane + block) % (1 << K)) >> slot) & 1 == 1


def _take(entry):
    return np.take(_POOL_SC, entry, axis=0), np.take(_POOL_PT, entry, axis=0), np.take(_POOL_OUT, entry, axis=0)


def place(n, K):
    """(scalars, points, expected), each (n, 32) uint8"""
    i = np.arange(n, dtype=np.int64)
    entry = np.where(degenerate_mask(n, K), (_DEG_STRIDE * i) % _N_DEG, _N_DEG + (_ORD_STRIDE * i) % _N_ORD)
    return _take(entry)


def place_all_degenerate(n):
    """(scalars, points, expected): every item degenerate, every expected output 32 zero bytes"""
    return _take((_DEG_STRIDE * np.arange(n, dtype=np.int64)) % _N_DEG)


def describe(bad, K, n):
    """the first items of `bad` (indices) as (i, tile, lane, block, slot, degenerate?) - a failure names the slot"""
    deg = degenerate_mask(n, K)
    return [(int(i),) + tuple(int(v) for v in layout(int(i), K)) + (bool(deg[i]),) for i in list(bad)[:8]]
