"""Plain-integer model of comb key sets (include/eddsa_amd.h: eddsa_amd_keyset_create_comb; libeddsa_amd/csrc/keyed_lanes.h): the
signed 6-bit digits the comb route cuts a scalar into, the table entries m * 4096^row * (-A) as affine points, and the reading
of a stored entry.  Test infrastructure only: Python integers."""
P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
D = (-121665 * pow(121666, P - 2, P)) % P
SQRT_M1 = pow(2, (P - 1) // 4, P)

COMB_W = 6
COMB_HALF = 1 << (COMB_W - 1)
COMB_DIGITS = 44
COMB_ROWS = COMB_DIGITS // 2
ENTRIES = COMB_ROWS * COMB_HALF
ENTRY_WORDS = 32
OFFSET = sum(COMB_HALF << (COMB_W * j) for j in range(COMB_DIGITS))

NEUTRAL = (0, 1)


def digits(x):
    """the comb's digits of x < 2^253: digit j of x + OFFSET, less COMB_HALF (the recoding of scale_base_lane)"""
    y = x + OFFSET
    assert y < 1 << (COMB_W * COMB_DIGITS)
    return [((y >> (COMB_W * j)) & (2 * COMB_HALF - 1)) - COMB_HALF for j in range(COMB_DIGITS)]


def digits_value(d):
    return sum(dj << (COMB_W * j) for j, dj in enumerate(d))


def add(p, q):
    """the complete addition of -x^2 + y^2 = 1 + d x^2 y^2, affine"""
    (x1, y1), (x2, y2) = p, q
    k = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + k, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - k, P - 2, P) % P)


def _ext_add(p, q):
    """the same addition in extended coordinates (X : Y : Z : T), no inversion (add-2008-hwcd-3, complete as well)"""
    (x1, y1, z1, t1), (x2, y2, z2, t2) = p, q
    a, b = (y1 - x1) * (y2 - x2) % P, (y1 + x1) * (y2 + x2) % P
    c, d = 2 * D * t1 * t2 % P, 2 * z1 * z2 % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def mul(n, p):
    q, r = (p[0], p[1], 1, p[0] * p[1] % P), (0, 1, 1, 0)
    while n:
        if n & 1:
            r = _ext_add(r, q)
        q = _ext_add(q, q)
        n >>= 1
    zi = pow(r[2], P - 2, P)
    return (r[0] * zi % P, r[1] * zi % P)


def decode_neg(enc):
    """-A for 32 key bytes under the reference's import (y = the low 255 bits mod p, the sign bit applied also when x = 0), or
    None when the bytes decode to no curve point"""
    v = int.from_bytes(enc, "little")
    sign, y = v >> 255, (v & (2**255 - 1)) % P
    x2 = (y * y - 1) * pow(D * y * y + 1, P - 2, P) % P
    x = pow(x2, (P + 3) // 8, P)
    if (x * x - x2) % P:
        x = x * SQRT_M1 % P
    if (x * x - x2) % P:
        return None
    if (x & 1) != sign:
        x = (P - x) % P
    return ((P - x) % P, y)


def entry(neg_a, row, m):
    """entry (row, m) of a key's comb: m * 2^(2 COMB_W row) * (-A)"""
    return mul(m << (2 * COMB_W * row), neg_a)


def entry_point(words):
    """the affine point of a stored entry: 32 little-endian words, Y-X | Y+X | 2dT | 2Z, eight words (a value below 2^255) each;
    also checks that 2dT belongs to the same point"""
    vals = [sum(int(w) << (32 * i) for i, w in enumerate(words[8 * k:8 * k + 8])) % P for k in range(4)]
    ymx, ypx, t2d, z2 = vals
    assert z2 != 0
    zi = pow(z2, P - 2, P)
    x, y = (ypx - ymx) * zi % P, (ypx + ymx) * zi % P
    assert (2 * t2d * zi - 2 * D * x * y) % P == 0             # T / Z = x y
    return (x, y)
