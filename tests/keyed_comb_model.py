"""Plain-integer model of comb key sets (include/eddsa_amd.h: eddsa_amd_keyset_create_comb; libeddsa_amd/csrc/keyed_lanes.h): the
signed 6-bit digits the comb route cuts a scalar into, the table entries m * 4096^row * (-A) as affine points, and the reading
of a stored entry.  Test infrastructure only: Python integers."""
import ed_model as em
from ed_model import D, L, P, add, inv  # noqa: F401  (L, add: for this model's users)

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


def mul(n, p):
    """n p for an affine p, through the extended coordinates (no inversion per step)"""
    return em.affine(em.pmul(n, em.ext(p)))


def decode_neg(enc):
    """-A for 32 key bytes under the reference's import, or None when the bytes decode to no curve point"""
    pt = em.decode_reference(enc)
    return None if pt is None else (-pt[0] % P, pt[1])


def entry(neg_a, row, m):
    """entry (row, m) of a key's comb: m * 2^(2 COMB_W row) * (-A)"""
    return mul(m << (2 * COMB_W * row), neg_a)


def entry_point(words):
    """the affine point of a stored entry: 32 little-endian words, Y-X | Y+X | 2dT | 2Z, eight words (a value below 2^255) each;
    also checks that 2dT belongs to the same point"""
    vals = [sum(int(w) << (32 * i) for i, w in enumerate(words[8 * k:8 * k + 8])) % P for k in range(4)]
    ymx, ypx, t2d, z2 = vals
    assert z2 != 0
    zi = inv(z2)
    x, y = (ypx - ymx) * zi % P, (ypx + ymx) * zi % P
    assert (2 * t2d * zi - 2 * D * x * y) % P == 0             # T / Z = x y
    return (x, y)
