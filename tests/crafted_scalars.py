"""Signatures whose challenge scalar t and whose S are CHOSEN, for the digest forms of verification (include/eddsa_amd.h:
ed25519_verify_digests*, ed25519_verify_keyed_digests*): the caller of those forms supplies the 64 digest bytes, so t = digest mod l
is whatever the builder wants.  With t, S and a key A = a B (+ a point of small order) chosen, R = S B - t A makes a signature that
is valid by construction, and solving the same equation with one window's digit set to zero makes the signature that would be
valid only if a kernel skipped that window.  tests/test_crafted_scalars_on_host.py runs the set through the device source
compiled for the host, tests/test_gpu_crafted_scalars.py through every verify route on the GPU.

Everything is seeded and deterministic; nothing comes from the engine or from its source.  The curve is tests/ed_model.py's, the
pair searches are tests/keyed_model.py's (short_pair) and tests/balanced_model.py's, the comb's digits tests/keyed_comb_model.py's,
the expected verdicts ed_model.verify_t, policy_model.holds and cofactored_model.accepts_t.  Python integers, hashlib and numpy.

The digits a kernel reads (lanes.h: the digit words x + 0x88..8 / x + 0x8000..8000, keyed_lanes.h: the comb's offset) are signed:
digit i of x at width w is ((x + sum_j 2^(w-1) 2^(w j)) >> w i & (2^w - 1)) - 2^(w-1), in [-2^(w-1), 2^(w-1) - 1], and
sum_i digit_i 2^(w i) = x.  A scalar below l < 2^253 cannot hold every digit everywhere: position i of width w takes the maximum
only when max 2^(w i) < l - nibbles 0..62, 16-bit digits 0..14, comb digits 0..41 - and the positions above take 0 or 1 (the top
16-bit digit: up to 2^12).  reachable(w) is that count; the coverage conditions are stated over it."""
import functools
import random

import numpy as np

import balanced_model as bm
import cofactored_model as cf
import ed_model as em
import keyed_comb_model as cm
import policy_model as pm
from balanced_model import B33
from ed_model import B, L, P, encode, ext, le, num, padd, pmul, pmul2, pneg
from keyed_model import short_pair

SEED = 20261021
MAX_ITEMS = 2048                                   # the window-sums route takes up to this many items in one pass
WIDTHS = (4, 6, 16)                                # the widths the kernels cut scalars into: windows, comb digits, base-table digits
ROUTES = ("full", "h134", "h138", "bal", "comb")   # the evaluations a near miss is built for
HALF = {"h134": (134, 34), "h138": (138, 35), "bal": ("bal", 33)}   # route -> (bound, windows)


# ---------------------------------------------------------------- signed digits

def digits(x, w, count=None):
    """the signed w-bit digits of 0 <= x < 2^256, lowest first"""
    count = count if count is not None else -(-256 // w)
    half = 1 << (w - 1)
    y = x + sum(half << (w * j) for j in range(count))
    assert 0 <= x and y < 1 << (w * count)
    return [((y >> (w * j)) & (2 * half - 1)) - half for j in range(count)]


def nibbles(x):
    return digits(x, 4, 64)


def halfwords(x):
    return digits(x, 16, 16)


def comb_digits(x):
    return cm.digits(x)


def top_nonzero(d):
    """the highest position with a non-zero digit, or None"""
    for j in range(len(d) - 1, -1, -1):
        if d[j]:
            return j
    return None


def reachable(w):
    """how many digit positions of width w can hold the maximum digit in a scalar below l"""
    mx = (1 << (w - 1)) - 1
    return max(i + 1 for i in range(-(-256 // w)) if mx << (w * i) < L)


assert (reachable(4), reachable(6), reachable(16)) == (63, 42, 15)


# ---------------------------------------------------------------- the scalars

def pattern_scalars(w):
    """the signed-digit patterns of width w, each in [0, l) -> [(name, value)]"""
    mx, mn = (1 << (w - 1)) - 1, -(1 << (w - 1))
    positions = -(-256 // w)                       # the positions that start below bit 256
    val = lambda ds: sum(d << (w * i) for i, d in enumerate(ds))   # noqa: E731
    out = []
    n = max(n for n in range(1, positions + 1) if val([mx] * n) < L)
    out.append(("w%d all max" % w, val([mx] * n)))
    n = max(n for n in range(1, positions) if val([mn] * n + [1]) < L)
    out.append(("w%d all min" % w, val([mn] * n + [1])))
    for first, name in ((mn, "min/max"), (mx, "max/min")):
        alt = lambda n: [first if i % 2 == 0 else mn + mx - first for i in range(n)]   # noqa: E731
        n = max(n for n in range(1, positions + 1) if alt(n)[-1] == mx and 0 < val(alt(n)) < L)
        out.append(("w%d %s" % (w, name), val(alt(n))))
    for i in range(positions):
        out.append(("w%d max at %d" % (w, i), (mx << (w * i)) % L))
        out.append(("w%d min at %d" % (w, i), ((1 << (w * (i + 1))) + (mn << (w * i))) % L))
    return out


@functools.lru_cache(maxsize=None)
def scalars():
    """-> (named, patterns, randoms): [(name, value)] of every chosen scalar, distinct values in the order listed; the subset that
    are digit patterns; the 200 seeded random ones"""
    named = [("edge", v) for v in (0, 1, 2, 7, 8, 9, 15, 16, L - 1, L - 2, (L + 1) // 2, (L - 1) // 2, 1 << 252, (1 << 252) - 1)]
    named += [("crafted %s" % way, t) for t, way in bm.CRAFTED]
    for b in (B33 - 1, B33, B33 + 1, (1 << 128) - 1, 1 << 128, (1 << 132) - 1, 1 << 132, (1 << 134) - 1, 1 << 134, (1 << 138) - 1, 1 << 138):
        named += [("bound", b), ("bound, l - b", L - b)]
    named += [("no short pair", t) for t in no_short_pair()]
    pats = [p for w in WIDTHS for p in pattern_scalars(w)]
    named += pats
    rng = random.Random(SEED)
    rand = [("random", rng.randrange(L)) for _ in range(200)]
    named += rand
    seen, out = set(), []
    for name, v in named:
        assert 0 <= v < L, name
        if v not in seen:
            seen.add(v)
            out.append((name, v))
    pat_values = {v for _, v in pats}
    return out, [(n, v) for n, v in out if v in pat_values], [v for _, v in rand]


# ---------------------------------------------------------------- the pairs of the half-length routes

def euclid_big(t, bits):
    """the largest quotient keyed_model.short_pair divides by on its way to an answer for t: those down to the first remainder
    below 2^bits, and one more where that remainder's cofactor is even and the rule looks at the next one.  The device's
    quotients are 31-bit (halve.h), and the model does not apply beyond them"""
    r0, u0, r1, u1, big = bm.N8L, 0, t, 1, 0
    while r1 >= 1 << bits:
        q = r0 // r1
        big = max(big, q)
        r0, u0, r1, u1 = r1, u1, r0 - q * r1, u0 - q * u1
    if u1 & 1 == 0 and r1 >= 1 << (256 - bits):
        big = max(big, r0 // r1)
    return big


def no_short_pair(bits=138, count=2):
    """scalars on which the searches below 2^134 and 2^138 give up after an ordinary walk (2 in 10^7 random t do under 2^138):
    t = (v / 2) / (u / 2) mod 4 l for an even u of 117 bits and an even v of 118 - then u t = v (mod 8 l), |u| v is far below
    8 l, so (v, u) is a step of the walk, the remainder before it is about 8 l / |u| > 2^138, and the first remainder below the
    bound comes with an even cofactor and is below 2^(256 - bits): no second look"""
    out, k = [], 0
    while len(out) < count:
        k += 1
        t = ((1 << 116) + 3 * k + 1) * pow((1 << 115) + 2 * k + 1, -1, 4 * L) % (4 * L)
        if t < L and short_pair(t, bits) is None and short_pair(t, 134) is None and euclid_big(t, bits) < 1 << 30:
            out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def pair_of(route, t):
    """(u, v, found, sure) for a half-length route: the pair of its search by the model, (1, t) with found False when it finds
    none ("long": the item keeps the reference's own equation).  sure is False where the walk has a quotient of 30 bits or more:
    there the device may give up on a pair the model finds, and both outcomes are right"""
    bound = HALF[route][0]
    if bound == "bal":
        found, u, v = bm.balanced_pair(t)
        sure = bm.balanced_trace(t)[4] < 1 << 30
        return (u, v, True, sure) if found else (1, t, False, sure)
    got = short_pair(t, bound)
    sure = euclid_big(t, bound) < 1 << 30
    return (got[1], got[0], True, sure) if got else (1, t, False, sure)


# ---------------------------------------------------------------- keys

@functools.lru_cache(maxsize=None)
def keys():
    """six keys -> [(a, the point A, its 32 bytes, what it is)]: four honest a B, one a B + T8, one a B + T2"""
    rng = random.Random(SEED + 1)
    tors = sorted(em.torsion_points())
    t8 = next(ext(pt) for pt in tors if em.mul(4, pt) != (0, 1))
    t2 = ext((0, P - 1))
    assert em.mul(2, (0, P - 1)) == (0, 1)
    out = []
    for k in range(6):
        a = rng.randrange(1, L)
        pt = pmul(a, B)
        what = "honest"
        if k == 4:
            pt, what = padd(pt, t8), "a B + T8"
        if k == 5:
            pt, what = padd(pt, t2), "a B + T2"
        out.append((a, pt, encode(pt), what))
    assert len({enc for _, _, enc, _ in out}) == 6
    return out


def key_bytes():
    return em.arr([enc for _, _, enc, _ in keys()])


# ---------------------------------------------------------------- items

class Item:
    """one (signature, key, digest): t = digest mod l and S as PRESENTED; valid = what the builder meant it to be"""
    __slots__ = ("sig", "key", "t", "digest", "valid", "kind", "accept")

    def __init__(self, r_enc, s, key, t, k, valid, kind):
        assert 0 <= s < 1 << 256 and 0 <= t < L and t + k * L < 1 << 512
        self.sig, self.key, self.t, self.valid, self.kind = r_enc + le(s), key, t, valid, kind
        self.digest = le(t + k * L, 64)

    @property
    def s(self):
        return num(self.sig[32:])

    @property
    def pub(self):
        return keys()[self.key][2]


def r_of(s, t, key):
    """R = S B - t A as a point"""
    return pmul2(s % L, B, t % L, pneg(keys()[key][1]))


def near_misses(item, route, kind_at):
    """the signature that is valid exactly when `route`'s evaluation skips one window, for the valid item (t, S, A): the first
    constructible kind from position kind_at of the route's list on -> (kind name, R bytes) or None.
    The evaluation adds  s' B + sigma v (-A) + |u| (-R)  with u t = v, s' = |u| S (u = 1, v = t, s' = S on the full-length and
    comb routes and for an item without a pair) digit by digit; with digit d of weight W left out of
      v:    it is neutral for the R of t* = (v - d W) / u            (then u t* is what the windows that remain add up to)
      |u|:  for R* = c (S B - t A), c = |u| / (|u| - d W)            (then (|u| - d W) R* = |u| (S B - t A))
      s':   for the R of S* = (s' - d W) / |u|
    all mod l, the order of B and of an honest A.  A zero digit changes nothing and is passed over."""
    t, s = item.t, item.s % L
    if route in HALF:
        u, v = pair_of(route, t)[:2]
        dv, du, ds, wbits, sbits = nibbles(v), nibbles(abs(u)), halfwords(abs(u) * s % L), 4, 16
    elif route == "full":
        u, v = 1, t
        dv, du, ds, wbits, sbits = nibbles(t), None, halfwords(s), 4, 16
    else:
        u, v = 1, t
        dv, du, ds, wbits, sbits = comb_digits(t), None, comb_digits(s), cm.COMB_W, cm.COMB_W
    au, sp = abs(u), abs(u) * s % L
    kinds = [("v", top_nonzero(dv)), ("v", 0)] + [("s", j) for j in (0, 7, 8, 15)]
    if du is not None:
        kinds[1:1] = [("u", top_nonzero(du))]
        kinds.insert(3, ("u", 0))
    for step in range(len(kinds)):
        what, j = kinds[(kind_at + step) % len(kinds)]
        if j is None:
            continue
        name = "%s: %s digit %d skipped" % (route, {"v": "t" if du is None else "v", "u": "|u|", "s": "S" if du is None else "s'"}[what], j)
        if what == "v" and dv[j]:
            t_star = (v - (dv[j] << (wbits * j))) * pow(u, -1, L) % L
            return name, encode(r_of(s, t_star, item.key))
        if what == "u" and du[j] and (au - (du[j] << (4 * j))) % L:
            c = au * pow(au - (du[j] << (4 * j)), -1, L) % L
            return name, encode(r_of(c * s, c * t, item.key))
        if what == "s" and ds[j]:
            s_star = (sp - (ds[j] << (sbits * j))) * pow(au, -1, L) % L
            return name, encode(r_of(s_star, t, item.key))
    return None


@functools.lru_cache(maxsize=None)
def build():
    """-> (items, report): the whole set with its expected verdicts, and the coverage report (coverage(items))"""
    named, _, rand = scalars()
    rng = random.Random(SEED + 2)
    items, uses, count = [], {}, [0]
    kmax = lambda t: ((1 << 512) - 1 - t) // L   # noqa: E731

    def valid(t, s, kind, key=None):
        n = count[0]
        count[0] += 1
        key = n % 6 if key is None else key
        k = (0, kmax(t), rng.randrange(kmax(t) + 1))[n % 3]
        shown = s + L if n % 16 == 5 else s        # a few items show S + l (< 2^256: S < l < 2^253)
        it = Item(encode(r_of(s, t, key)), shown, key, t, k, True, kind + (", S + l" if shown != s else ""))
        items.append(it)
        uses[t] = uses.get(t, 0) + 1
        return it

    everything = [v for _, v in named]
    chosen = [(n, v) for n, v in named if n != "random"]          # every S that is an edge, a crafted scalar, a bound or a pattern
    small = [v for v in everything if v < 1 << 128] + [rng.randrange(1 << 128) for _ in range(40)]
    full = [v for v in everything if v >= 1 << 248]
    assert len(small) >= 60 and len(full) >= 150
    # every chosen S under a t below 2^128 - every search then returns (u, v) = (1, t), so s' = S: the half-length kernels read
    # S's own digits - and under a full-size t
    for i, (name, s) in enumerate(chosen):
        t = small[i % len(small)]
        for route in HALF:
            assert pair_of(route, t)[:3] == (1, t, True), (route, hex(t))
        valid(t, s, "S = %s, t < 2^128" % name)
    for i, (name, s) in enumerate(chosen):
        valid(full[i % len(full)], s, "S = %s, full-size t" % name)
    # every t under a random S, and under a second S where it has not had two yet
    by_t = {}
    for i, (name, t) in enumerate(named):
        by_t[t] = valid(t, rand[(3 * i) % len(rand)], "t = %s" % name, key=i % 4 if name.startswith(("crafted", "random")) else None)
    for i, (name, t) in enumerate(named):
        if uses[t] < 2:
            valid(t, everything[(37 * i + 11) % len(everything)], "t = %s, second S" % name)
    assert all(uses[t] >= 2 for t in everything)

    # near misses: over the crafted scalars, the bounds' l - b and random t, under honest keys (the construction is exact there)
    bases = [by_t[t] for n, t in named if n.startswith("crafted")] + [by_t[t] for n, t in named if n == "bound, l - b"][:11]
    bases += [by_t[t] for t in rand[:64]]
    bases = [b for b in bases if b.key < 4]
    assert len(bases) >= 64
    for i, base in enumerate(bases):
        for r, route in enumerate(ROUTES):
            got = near_misses(base, route, i + r)
            if got:
                it = Item(got[1], base.s, base.key, base.t, 0, False, got[0])
                it.digest = base.digest
                items.append(it)
    for base in bases[21:25] + bases[40:42]:
        for w in (0, 31, 32, 33, 34, 63):
            for sign in (1, -1):
                items.append(Item(base.sig[:32], base.s, base.key, (base.t + sign * 16**w) % L, w, False, "t %+d * 16^%d" % (sign, w)))
    for base in bases[::12]:
        flipped = base.sig[:31] + bytes([base.sig[31] ^ 0x80])
        items.append(Item(flipped, base.s, base.key, base.t, 1, False, "R with the sign bit flipped"))
    for base in (bases[0], bases[30]):
        r_pt = r_of(base.s, base.t, base.key)
        for pt in sorted(em.torsion_points()):
            if pt != (0, 1):
                items.append(Item(encode(padd(r_pt, ext(pt))), base.s, base.key, base.t, 2, False, "R + a point of small order"))

    for it in items:
        it.accept = em.verify_t(it.sig, it.pub, it.t)
        # an item whose model verdict is not the intended one is a bug of this builder, not an expectation to record
        assert it.accept == it.valid, (it.kind, hex(it.t), it.sig.hex())
    assert len(items) <= MAX_ITEMS, len(items)
    return tuple(items), coverage(items)


def coverage(items):
    """what the set reaches, from the models alone -> dict (tests/test_crafted_scalars_on_host.py asserts the conditions)"""
    rep = {"items": len(items), "valid": sum(it.valid for it in items), "near": sum(not it.valid for it in items)}
    ts = sorted({it.t for it in items})
    for route, (bound, windows) in HALF.items():
        seen, top, neg, none, umax = set(), 0, 0, 0, 0
        for it in items:
            u, v, found, sure = pair_of(route, it.t)
            if not found:
                none += sure
                continue
            dv = nibbles(v)
            assert top_nonzero(dv) is None or top_nonzero(dv) < windows, hex(it.t)
            seen |= set(dv[:windows])
            top += dv[windows - 1] != 0
            neg += u < 0
            umax = max(umax, abs(u))
        rep[route] = {"v digits": seen, "top window of v": top, "u < 0": neg, "no pair": none, "max |u|": umax}
    rep["bal"]["v = B33"] = sum(pair_of("bal", t)[1] == B33 for t in ts)
    rep["bal"]["|u| = B33"] = sum(abs(pair_of("bal", t)[0]) == B33 for t in ts)
    rep["t window 0"] = {nibbles(t)[0] for t in ts}
    rep["t window 63"] = {nibbles(t)[63] for t in ts}
    rep["t all 7"] = any(nibbles(t)[:63] == [7] * 63 for t in ts)
    rep["t all -8"] = any(nibbles(t)[:63] == [-8] * 63 for t in ts)
    ss = sorted({it.s % L for it in items})
    for name, cut, vals, w in (("S halfwords", halfwords, ss, 16), ("S comb", comb_digits, ss, 6), ("t comb", comb_digits, ts, 6)):
        mx, mn = (1 << (w - 1)) - 1, -(1 << (w - 1))
        cols = list(zip(*[cut(x) for x in vals]))
        rep[name] = [j for j in range(reachable(w)) if not (mx in cols[j] and mn in cols[j])]      # positions that lack an extreme
    return rep


# ---------------------------------------------------------------- arrays for the tests

def arrays(items):
    """-> sig (n, 64), pub (n, 32), digest (n, 64), key index (n,) uint32, read-only"""
    out = (em.arr([it.sig for it in items]), em.arr([it.pub for it in items]), em.arr([it.digest for it in items]),
           np.array([it.key for it in items], np.uint32))
    for a in out:
        a.setflags(write=False)
    return out


def verdicts(items, policy=0, cofactored=False):
    """the models' verdicts under the default rule, the strict rules (policy_model) or the cofactored equation"""
    if cofactored:
        return np.array([cf.accepts_t(it.sig, it.pub, it.t) and pm.holds(policy, it.sig, it.pub) for it in items], np.uint8)
    return np.array([it.accept and pm.holds(policy, it.sig, it.pub) for it in items], np.uint8)
