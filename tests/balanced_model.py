"""The balanced pair search of libeddsa_amd/csrc/halve.h (halve_balanced_lane) on Python integers: what the CPU and GPU tests of
the 33-window arrangement hold the device source against."""
import ctypes

L = 2**252 + 27742317777372353535851937790883648493
N8L = 8 * L
B33 = 7 * (16**33 - 1) // 15            # 0x777...7, 33 nibbles: the largest value whose signed four-bit recoding ends at window 32
STOP = 1 << 128
SZ = ctypes.c_size_t


def balanced_trace(t):
    """(found, u, v, way, q): the pair with u t = v (mod 8 l), u odd, |u| and v <= B33, that the search settles on, how it got
    there - "odd": the first remainder below 2^128 came with an odd cofactor; "before" / "partial" / "after": its cofactor was
    even and the pair is the step before it, a partial step between the two, the step after; "none": no candidate fits - and the
    largest quotient the search divided by.  found is False for "none" and for a quotient of 31 bits or more (the device's
    quotients are 31-bit; no test drives one: the device may have used part of it up in partial steps)."""
    r0, u0, r1, u1, big = N8L, 0, t, 1, 0
    while r1 >= STOP:
        q = r0 // r1
        big = max(big, q)
        r0, r1, u0, u1 = r1, r0 - q * r1, u1, u0 - q * u1
    if u1 & 1:
        u, v, way = u1, r1, "odd"
    elif r0 <= B33:
        u, v, way = u0, r0, "before"
    else:
        j = (r0 - B33 - 1) // r1 + 1     # the smallest j with r0 - j r1 <= B33; r1 > 0: an even u1 is not the last cofactor
        big = max(big, j - 1)
        u, v, way = u0 - j * u1, r0 - j * r1, "after" if j == r0 // r1 else "partial"
    fits = abs(u) <= B33 and 0 <= v <= B33
    return fits and big < 1 << 31, u, v, way if fits else "none", big


def balanced_pair(t):
    """(found, u, v)"""
    return balanced_trace(t)[:3]


# Scalars found with the model (a search over random t, or t = v / u mod 8 l for a wanted pair until t < l and the search's way
# leads to that pair): what each one is stands beside it.
CRAFTED = [
    (0, "odd"), (1, "odd"), (L - 1, None), (2, "odd"), ((1 << 128) - 1, "odd"), (1 << 128, None), ((1 << 128) + 1, None), (L // 2, None), (L // 3, None),
    (0x2b8676df1461aaf8eb18b90074513021da8978206f5c6671e0c07e9e115e4b, "odd"),
    # even cofactor at the first remainder below 2^128, the step before fits
    (0xbe5bb2f1cfb10f62827688de6a16a3b0d464138a62332553fc1ea36f17fd374, "before"),
    # ... the step before is above B33: a partial step
    (0xd122da1d4042c36f000feb0bce240c658780d0aa4e15158461cb6e0590ef594, "partial"),
    (0x68a2b1b971503bd126d15699c9e8752a99b2c28615b43f359e1adc4771fe0ac, "partial"),
    # a quotient of 6520 across 2^128 with an even cofactor below it: no pair
    (0x51ece150d911c4a05c2703382000ad1786933c3afe385c7d6d46fe3f46abe22, "none"),
    (0x610ab0703b4bce576aa77d00e8ca9fa6cfc5b6225bf7c8400ad9227d733d669, "none"),
    # the step before an even cofactor is exactly B33 (taken: v = B33) / B33 + 1 (not taken: a partial step)
    (0xcd5e43aa6a59ff1c3f090a6d5b5f703bea3c6313c5fee44556a0184217a8ff5, "before"),
    (0x72e17e74e66215804f091fbbe402dba499977feaa3834dc4531ebf70c12bab0, "partial"),
    # the partial step that decides has |u| = B33 (taken) / B33 + 2, the next odd number (no pair)
    (0xd57995c7447399ddb97a9ccad81645fe6cf323ab7b81cb32578870752108fd0, "partial"),
    (0x6ce7b909a5d0e24431871af5f2124fee40d6a0a30dfd2cf84c2858d9a8ff7fe, "none"),
]


def lane_pairs(h, ts):
    """[(found, u, v)] of halve_balanced_lane for scalars ts; h: tests/host_check/balanced_check.cpp"""
    n = len(ts)
    tin = b"".join(int(t).to_bytes(32, "little") for t in ts)
    out = ctypes.create_string_buffer(48 * max(n, 1))
    h.bc_halve(out, tin, SZ(n))
    return rows_of(out.raw, n)


def rows_of(raw, n):
    res = []
    for i in range(n):
        row = raw[48 * i:48 * i + 48]
        res.append((bool(row[41]), int.from_bytes(row[20:40], "little") * (-1 if row[40] else 1), int.from_bytes(row[:20], "little")))
    return res
