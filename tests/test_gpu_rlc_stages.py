"""GPU tests of the opt-in batch verification, stage by stage (libeddsa_amd/csrc/rlc.hip): the verdict bytes and the four
statistics counters cannot tell a seed that ignores part of the batch from one that does not, nor a window point that is wrong in
a group that fails anyway.  So every device stage of a pass is read back (debug_rlc_snapshot: leaves, seed, t and S, flags, digit
rows, base-point digits, window points, group verdicts) and held against a model in plain Python integers and hashlib, written
below (the curve is that of tests/ed_model.py) from the description of the combination and from nothing of the device source.
Every comparison is exact: bytes, integers or affine points.

The conventions are the ones tests/test_device_source_on_host.py pins for the per-lane code on the host:
  leaf_i = SHA-512(SHA-512(R | A | M) | S)[:32]; a tree node = SHA-512(up to 16 children)[:32]; the seed is the root;
  z_i = (SHA-512(seed | i as 8 LE bytes | "rlc\\0" | 20 zero bytes)[:16] & (2^126 - 1)) | 1;
  the key's scalar is z t mod 8 l, centred; digits are signed bytes in [-128, 127]; the points are -A, -R and B.
"""
import functools

import numpy as np
import pytest

import ed_model as em
from ed_model import B as BASE, D, D2, L, NEUTRAL, P, affine, ext, inv, is_neutral, padd as add, pneg as neg
from gpu_kit import always_combine, dev  # noqa: F401  (always_combine: a fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("always_combine")]
G = 8192
H, LE = em.sha, em.num


def decode(enc):
    """(on the curve, x, y) of a 32-byte encoding, read permissively: y is taken mod p, any sign bit; x and y None off the curve"""
    pt = em.decode_reference(enc)
    return (False, None, None) if pt is None else (True,) + pt


def weighted_sum(digits, points):
    """sum of digits[k] * points[k], digits in [-128, 127]: one sum per magnitude, then the sums' running totals"""
    buckets = {}
    for k in np.nonzero(digits)[0]:
        d = int(digits[k])
        q = points[k] if d > 0 else neg(points[k])
        buckets[abs(d)] = add(buckets[abs(d)], q) if abs(d) in buckets else q
    run = total = NEUTRAL
    for m in range(max(buckets, default=0), 0, -1):
        if m in buckets:
            run = add(run, buckets[m])
        total = add(total, run)
    return total


def signed_digits(v, count):
    """the one way to write v as sum d_j 256^j with every d_j in [-128, 127]"""
    out = []
    for _ in range(count):
        d = (v + 128) % 256 - 128
        out.append(d)
        v = (v - d) >> 8
    assert v == 0
    return out


def tree_root(level):
    while True:
        level = [H(b"".join(level[j:j + 16]))[:32] for j in range(0, len(level), 16)]
        if len(level) == 1:
            return level[0]


class Model:
    """what a pass over the items (sig[i], pk[i], msgs[i]) has to compute, on integers; digests: the caller-supplied form"""

    def __init__(self, sig, pk, msgs=None, digests=None):
        self.n = len(sig)
        self.groups = (self.n + G - 1) // G
        self.r = [sig[i, :32].tobytes() for i in range(self.n)]
        self.a = [pk[i].tobytes() for i in range(self.n)]
        sb = [sig[i, 32:].tobytes() for i in range(self.n)]
        dg = digests if digests is not None else [H(self.r[i] + self.a[i] + bytes(msgs[i])) for i in range(self.n)]
        self.leaf = [H(dg[i] + sb[i])[:32] for i in range(self.n)]
        self.seed = tree_root(self.leaf)
        self.t = [LE(d) % L for d in dg]
        self.s = [LE(x) % L for x in sb]

    @functools.cached_property
    def z(self):
        return [(LE(H(self.seed + i.to_bytes(8, "little") + b"rlc\0" + bytes(20))[:16]) & (2**126 - 1)) | 1 for i in range(self.n)]

    @functools.cached_property
    def decoded(self):
        return [decode(x) for x in self.a], [decode(x) for x in self.r]

    @functools.cached_property
    def flags(self):
        """bit 0: R is the canonical encoding of a curve point; bit 1: the item sends its group to the per-item kernels (a key
        that is no curve point or has small order, a valid R of small order) - test_rlc_decoding_and_routing_flags"""
        out = []
        for i in range(self.n):
            (a_on, _, ay), (r_on, rx, ry) = self.decoded[0][i], self.decoded[1][i]
            v = LE(self.r[i])
            valid = r_on and (v & (2**255 - 1)) < P and not (rx == 0 and v >> 255)
            per_item = (not a_on or ay in em.small_order_ys()) or (valid and ry in em.small_order_ys())
            out.append((1 if valid else 0) | (2 if per_item else 0))
        return out

    @functools.cached_property
    def key_scalar(self):
        """z t mod 8 l, centred into [-4 l, 4 l)"""
        out = []
        for i in range(self.n):
            v = self.z[i] * self.t[i] % (8 * L)
            out.append(v - 8 * L if v >= 4 * L else v)
        return out

    @functools.cached_property
    def base_scalar(self):
        return [sum(self.z[i] * self.s[i] for i in range(g * G, min(self.n, (g + 1) * G)) if self.flags[i] & 1) % L
                for g in range(self.groups)]

    @functools.cached_property
    def dig(self):
        """(groups, 48, 8192) int8: rows 0..31 the digits of the key's scalar, 32..47 those of z; zero for an item whose R is
        rejected and for the slots past n"""
        out = np.zeros((self.groups, 48, G), np.int8)
        for i in range(self.n):
            if self.flags[i] & 1:
                out[i // G, :, i % G] = signed_digits(self.key_scalar[i], 32) + signed_digits(self.z[i], 16)
        return out

    @functools.cached_property
    def bdig(self):
        return np.array([signed_digits(v, 32) for v in self.base_scalar], np.int8)

    @functools.cached_property
    def neg_points(self):
        """(-A_i, -R_i) in extended coordinates (of encodings that decode: nothing else carries a non-zero digit here)"""
        return [[neg(ext((x, y))) if on else None for on, x, y in side] for side in self.decoded]

    def window_point(self, g, seg):
        """window point `seg` of group g: entries 0..31 are windows 31..0 of the keys and the base point, 32..47 windows 15..0
        of the R"""
        lo, hi = g * G, min(self.n, (g + 1) * G)
        if seg < 32:
            w = 31 - seg
            digits = np.append(self.dig[g, w, :hi - lo].astype(np.int64), int(self.bdig[g, w]))
            return weighted_sum(digits, self.neg_points[0][lo:hi] + [BASE])
        return weighted_sum(self.dig[g, 32 + 47 - seg, :hi - lo].astype(np.int64), self.neg_points[1][lo:hi])


def entry_point(entry):
    """a packed window point (Y-X | Y+X | 2dT | 2Z, 32 little-endian bytes each) as (X, Y, Z, T); it must be a curve point
    with Z != 0 and X Y = Z T"""
    ymx, ypx, t2d, z2 = (LE(entry[k].tobytes()) % P for k in range(4))
    half = inv(2)
    x, y, z, t = (ypx - ymx) * half % P, (ypx + ymx) * half % P, z2 * half % P, t2d * inv(D2) % P
    assert z != 0 and (x * y - z * t) % P == 0
    assert (-x * x * z * z + y * y * z * z - z**4 - D * x * x * y * y) % P == 0      # -x^2 + y^2 = 1 + d x^2 y^2, projectively
    return (x, y, z, t)


def horner(points):
    """the total of a group's 48 window points: windows 31..0, eight doublings between two windows"""
    r = NEUTRAL
    for w in range(31, -1, -1):
        if w != 31:
            for _ in range(8):
                r = add(r, r)
        r = add(r, points[31 - w])
        if w < 16:
            r = add(r, points[32 + 15 - w])
    return r


# ---------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------
def sign(engine, sk, msg):
    pk = engine.ed25519_genpub_batch(dev(sk))
    return engine.ed25519_sign_batch(dev(sk), pk, dev(msg)).cpu().numpy(), pk.cpu().numpy()


@pytest.fixture(scope="module")
def traffic(engine):
    """32 groups and a partial one of genuine signatures over 32-byte messages under distinct keys; never written to"""
    n = 32 * G + 300
    rng = np.random.default_rng(1001)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sig, pk = sign(engine, sk, msg)
    for a in (sig, pk, msg):
        a.setflags(write=False)
    return sig, pk, msg


def run(engine, sig, pk, msg):
    """one pass with device pointers -> (verdicts, statistics)"""
    n = len(sig)
    assert 0 < n <= 1 << 20
    ok, st = engine.ed25519_verify_batch_rlc(dev(sig), dev(pk), dev(msg), msg_len=msg.shape[1], return_stats=True)
    assert engine.debug_rlc_snapshot("info")[:2] == (n, (n + G - 1) // G)
    return ok.cpu().numpy(), st


def check_scalars_and_digits(engine, m):
    """stage R4 of the last pass against the model m: t and S, flags, digit rows, base-point digits"""
    n = m.n
    ts = engine.debug_rlc_snapshot("ts")
    assert [LE(ts[i, 0].tobytes()) for i in range(n)] == m.t
    assert [LE(ts[i, 1].tobytes()) for i in range(n)] == m.s
    flags = engine.debug_rlc_snapshot("flags")
    assert flags.tolist() == m.flags
    gflags = engine.debug_rlc_snapshot("gflags")
    assert [int(x != 0) for x in gflags] == [int(any(f & 2 for f in m.flags[g * G:(g + 1) * G])) for g in range(m.groups)]
    dig = engine.debug_rlc_snapshot("dig")
    assert dig.shape == (m.groups, 48, G) and dig.dtype == np.int8           # (so every digit lies in [-128, 127])
    weights_a = [1 << (8 * j) for j in range(32)]
    for i in range(n):
        col = dig[i // G, :, i % G].tolist()
        if m.flags[i] & 1:
            assert sum(d * w for d, w in zip(col[32:], weights_a)) == m.z[i], i
            av = sum(d * w for d, w in zip(col[:32], weights_a))
            zt = m.z[i] * m.t[i]
            assert (av - zt) % (8 * L) == 0 and abs(av) <= 4 * L and (av < 0) == ((zt // L) % 8 >= 4), i
        else:
            assert not any(col), i                                           # rejected outright: contributes nothing
    assert not dig.reshape(-1, G)[-48:, n - (m.groups - 1) * G:].any()       # the slots past the end of the batch
    assert np.array_equal(dig, m.dig)
    bdig = engine.debug_rlc_snapshot("bdig")
    for g in range(m.groups):
        assert sum(int(d) << (8 * j) for j, d in enumerate(bdig[g])) == m.base_scalar[g], g
    assert np.array_equal(bdig, m.bdig)
    return dig


def check_window_points(engine, m, which, accepted):
    """stage R5 and R6 of the last pass against the model m: the window points `which` = [(group, entry), ...] are the model's
    sums; EVERY dumped entry is a curve point; a group's Horner total over its 48 dumped points is the neutral element exactly
    when the device accepted the group, and that is what `accepted` expects"""
    assert np.array_equal(engine.debug_rlc_snapshot("dig"), m.dig) and np.array_equal(engine.debug_rlc_snapshot("bdig"), m.bdig)
    seg = engine.debug_rlc_snapshot("seg")
    gok = engine.debug_rlc_snapshot("gok")
    gflags = engine.debug_rlc_snapshot("gflags")
    assert seg.shape == (m.groups, 48, 4, 32) and gok.shape == (m.groups,)
    points = [[entry_point(seg[g, s]) for s in range(48)] for g in range(m.groups)]
    for g, s in which:
        assert affine(points[g][s]) == affine(m.window_point(g, s)), (g, s)
    for g in range(m.groups):
        assert gflags[g] == 0
        assert is_neutral(horner(points[g])) == (gok[g] == 1), g
    assert gok.tolist() == accepted
    return points


ALL_WINDOWS = list(range(48))


# ---------------------------------------------------------------------------------------------------------
# a. leaves and seed
# ---------------------------------------------------------------------------------------------------------
def leaves_and_seed(engine):
    return [x.tobytes() for x in engine.debug_rlc_snapshot("leaf")], engine.debug_rlc_snapshot("seed")


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65537])
def test_leaves_and_seed_are_the_hash_tree_of_the_whole_batch(engine, traffic, n):
    """one to five levels, full and partial last nodes on every level"""
    sig, pk, msg = (a[:n] for a in traffic)
    ok, st = run(engine, sig, pk, msg)
    assert ok.all() and st == (n, 0, 0, (n + G - 1) // G)
    m = Model(sig, pk, msg)
    leaf, seed = leaves_and_seed(engine)
    assert leaf == m.leaf
    assert seed == m.seed


@pytest.fixture(scope="module")
def ragged(engine):
    """257 genuine items with messages of 0..300 bytes"""
    import torch
    n = 257
    rng = np.random.default_rng(1002)
    lens = rng.integers(0, 301, n)
    lens[[3, 100, 256]] = (0, 300, 0)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pk = engine.ed25519_genpub_batch(dev(sk))
    sig = engine.ed25519_sign_batch(dev(sk), pk, dev(flat), msg_off=torch.from_numpy(off).cuda()).cpu().numpy()
    return sig, pk.cpu().numpy(), flat, off


@pytest.mark.parametrize("n", [255, 257])                    # two levels and three: the root in either buffer of the tree
def test_seed_of_ragged_messages(engine, ragged, n):
    """messages of different lengths are hashed in order of length (a permutation of the items): leaf i is still item i's"""
    import torch
    sig, pk, flat, off = ragged
    msgs = [flat[off[i]:off[i + 1]].tobytes() for i in range(n)]
    ok, st = engine.ed25519_verify_batch_rlc(dev(sig[:n]), dev(pk[:n]), dev(flat[:off[n]]), msg_off=torch.from_numpy(off[:n + 1].copy()).cuda(),
                                             return_stats=True)
    assert bool(ok.all()) and st == (n, 0, 0, 1)
    m = Model(sig[:n], pk[:n], msgs)
    leaf, seed = leaves_and_seed(engine)
    assert leaf == m.leaf
    assert seed == m.seed


def test_seed_from_caller_supplied_digests(engine, ragged):
    """ed25519_verify_digests_rlc over the same items: the same leaves and the same seed as from the messages"""
    sig, pk, flat, off = ragged
    n = len(sig)
    msgs = [flat[off[i]:off[i + 1]].tobytes() for i in range(n)]
    m = Model(sig, pk, msgs)
    digests = [H(m.r[i] + m.a[i] + msgs[i]) for i in range(n)]
    ok, st = engine.ed25519_verify_digests_rlc(dev(sig), dev(pk), dev(np.frombuffer(b"".join(digests), np.uint8)), return_stats=True)
    assert bool(ok.all()) and st == (n, 0, 0, 1)
    assert engine.debug_rlc_snapshot("info")[:2] == (n, 1)
    leaf, seed = leaves_and_seed(engine)
    assert leaf == Model(sig, pk, digests=digests).leaf == m.leaf
    assert seed == m.seed


def test_the_seed_changes_with_every_part_of_the_batch(engine, oracle, traffic):
    """one bit of the last item's S, of the last item's message, of the first item's key: the seed becomes the model's new
    value each time (4097 items: four levels, the last item alone in its node on every one)"""
    n = 4097
    base = [a[:n].copy() for a in traffic]
    seeds = {Model(*base).seed}
    for which, row, col in ((0, n - 1, 32 + 17), (2, n - 1, 31), (1, 0, 5)):
        sig, pk, msg = (a.copy() for a in base)
        (sig, pk, msg)[which][row, col] ^= 0x04
        ok, st = run(engine, sig, pk, msg)
        want = np.ones(n, np.uint8); want[row] = oracle.verify(sig[row].tobytes(), pk[row].tobytes(), msg[row].tobytes())
        assert np.array_equal(ok, want) and not want[row] and st == (0, n, 1, 0)
        m = Model(sig, pk, msg)
        leaf, seed = leaves_and_seed(engine)
        assert leaf == m.leaf and seed == m.seed
        seeds.add(seed)
    assert len(seeds) == 4


# ---------------------------------------------------------------------------------------------------------
# b. scalars and digits
# ---------------------------------------------------------------------------------------------------------
def with_rejected_r(traffic, n, rows):
    """the first n items with R strings that are no canonical encoding of a curve point in `rows`: those items are rejected at
    once, their group still passes"""
    sig, pk, msg = (a[:n].copy() for a in traffic)
    bad = [P + 1, 2, 1 | 1 << 255, 2**255 - 1]          # the neutral element as y = p + 1; no curve point; x = 0 with the sign bit; y >= p
    for k, row in enumerate(rows):
        sig[row, :32] = np.frombuffer(bad[k % 4].to_bytes(32, "little"), np.uint8)
    return sig, pk, msg


REJECTED_ROWS = {700: (0, 15, 16, 699), G + 300: (5, 1023, 1024, G - 1, G, G + 299)}


@pytest.fixture(scope="module")
def rejected(traffic):
    """n -> (sig, pk, msg, their model, computed once): the first n items of the traffic with REJECTED_ROWS[n]"""
    @functools.lru_cache(None)
    def case(n):
        sig, pk, msg = with_rejected_r(traffic, n, REJECTED_ROWS[n])
        return sig, pk, msg, Model(sig, pk, msg)
    return case


@pytest.mark.parametrize("n", [700, G + 300])
def test_scalars_flags_and_digit_rows(engine, rejected, n):
    sig, pk, msg, m = rejected(n)
    rows = REJECTED_ROWS[n]
    ok, st = run(engine, sig, pk, msg)
    want = np.ones(n, np.uint8); want[list(rows)] = 0
    assert np.array_equal(ok, want) and st == (n, 0, 0, (n + G - 1) // G)
    assert [i for i in range(n) if not m.flags[i] & 1] == list(rows) and not any(f & 2 for f in m.flags)
    dig = check_scalars_and_digits(engine, m)
    assert (dig[:, :32] == -128).any() and (dig[:, 32:] == -128).any()       # the digit that lands in bucket 128, on either side


# ---------------------------------------------------------------------------------------------------------
# c. window points and the Horner total
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129, 700])
def test_window_points_of_small_groups(engine, traffic, n):
    """a partial group: most buckets empty, the size ranks almost all ties, the base point alone in its bucket"""
    sig, pk, msg = (a[:n] for a in traffic)
    ok, st = run(engine, sig, pk, msg)
    assert ok.all() and st == (n, 0, 0, 1)
    check_window_points(engine, Model(sig, pk, msg), [(0, s) for s in ALL_WINDOWS], [1])


def test_window_points_of_a_full_group_and_a_partial_one(engine, rejected):
    """G + 300 items, some rejected for their R: the heaviest and lightest windows of the full group (the keys' windows 0, 15,
    16, 31, the R's 0 and 15) and all 48 of the partial one"""
    n = G + 300
    sig, pk, msg, m = rejected(n)
    ok, st = run(engine, sig, pk, msg)
    assert int(ok.sum()) == n - 6 and st == (n, 0, 0, 2)
    which = [(0, 31 - w) for w in (0, 15, 16, 31)] + [(0, 32 + 15 - w) for w in (0, 15)] + [(1, s) for s in ALL_WINDOWS]
    check_window_points(engine, m, which, [1, 1])


def test_window_points_of_a_group_that_fails(engine, traffic):
    """one S corrupted: the window points are still the model's sums (the base point's digits are those of the corrupted sum),
    their total is not the neutral element, the group is not accepted and its verdicts come from the per-item kernels"""
    n = 700
    sig, pk, msg = (a[:n].copy() for a in traffic)
    sig[333, 32 + 9] ^= 0x20
    ok, st = run(engine, sig, pk, msg)
    want = np.ones(n, np.uint8); want[333] = 0
    assert np.array_equal(ok, want) and st == (0, n, 1, 0)
    points = check_window_points(engine, Model(sig, pk, msg), [(0, s) for s in ALL_WINDOWS], [0])
    assert not is_neutral(horner(points[0]))


# ---------------------------------------------------------------------------------------------------------
# d. bucket loads unlike those of distinct random keys
# ---------------------------------------------------------------------------------------------------------
def degenerate(engine, kind, n):
    rng = np.random.default_rng(1003)
    if kind == "one key":                               # a single signer: a lane adds a point to itself and to its negative
        sk = np.repeat(rng.integers(0, 256, (1, 32), dtype=np.uint8), n, axis=0)
        msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    else:
        k = 1 if kind == "one item" else 2              # the very same item n times; two items in turn
        sk = np.tile(rng.integers(0, 256, (k, 32), dtype=np.uint8), (n // k + 1, 1))[:n]
        msg = np.tile(rng.integers(0, 256, (k, 32), dtype=np.uint8), (n // k + 1, 1))[:n]
    sig, pk = sign(engine, sk, msg)
    return sig, pk, msg


@pytest.mark.parametrize("kind", ["one key", "one item", "two items"])
def test_repeated_points_pass_by_combination(engine, kind):
    n = 2 * G + 5
    sig, pk, msg = degenerate(engine, kind, n)
    ok, st = run(engine, sig, pk, msg)
    assert ok.all() and st == (n, 0, 0, 3)
    for row in (G + 16, 2 * G + 4):                     # one copy corrupted: only its group goes per item, only its byte is 0
        bad = sig.copy(); bad[row, 32 + 3] ^= 1
        ok, st = run(engine, bad, pk, msg)
        want = np.ones(n, np.uint8); want[row] = 0
        cnt = G if row < 2 * G else 5
        assert np.array_equal(ok, want) and st == (n - cnt, cnt, 1, 2), row


def test_window_points_of_one_item_repeated(engine):
    n = 700
    sig, pk, msg = degenerate(engine, "one item", n)
    ok, st = run(engine, sig, pk, msg)
    assert ok.all() and st == (n, 0, 0, 1)
    check_window_points(engine, Model(sig, pk, msg), [(0, s) for s in ALL_WINDOWS], [1])


# ---------------------------------------------------------------------------------------------------------
# e. one corrupted item at every structural boundary of the bucket kernel
# ---------------------------------------------------------------------------------------------------------
def corrupt(sig, pk, msg, row, kind):
    if kind == 0:
        sig[row, 32 + 8] ^= 1                           # S
    elif kind == 1:
        msg[row, 0] ^= 1
    elif kind == 2:
        pk[row, 7] ^= 1                                 # another point, or none: the group fails or is flagged
    else:                                               # R: the first bit that leaves a canonical encoding of a curve point, so
        for bit in range(8, 248):                       # that the item is combined and its group fails (any other R is rejected
            r = bytearray(sig[row, :32].tobytes())      # at once, which test_scalars_flags_and_digit_rows covers)
            r[bit >> 3] ^= 1 << (bit & 7)
            if decode(bytes(r))[0]:
                sig[row, bit >> 3] ^= 1 << (bit & 7)
                return
        raise AssertionError("no bit of R leaves a curve point")


@pytest.mark.parametrize("pos", [0, 1, 15, 16, 63, 64, 255, 256, 1023, 1024, 4095, 4096, 8190, 8191])
def test_one_corrupted_item_at_every_boundary(engine, oracle, traffic, pos):
    """item `pos` of every second group (the ends of a lane's 16-byte digit load, of the 64-lane stride, of the group) and the
    last item of the partial last group, corrupted in S, message, key or R in turn"""
    sig, pk, msg = (a.copy() for a in traffic)
    n = len(sig)
    rows = [g * G + pos for g in range(0, 32, 2)] + [n - 1]
    for k, row in enumerate(rows):
        corrupt(sig, pk, msg, row, (k + pos) % 4)
    ok, st = run(engine, sig, pk, msg)
    want = np.ones(n, np.uint8)
    want[rows] = [oracle.verify(sig[r].tobytes(), pk[r].tobytes(), msg[r].tobytes()) for r in rows]
    assert not want[rows].any()
    assert np.array_equal(ok, want)
    assert st == (16 * G, 16 * G + 300, 17, 16)


# ---------------------------------------------------------------------------------------------------------
# the snapshot itself
# ---------------------------------------------------------------------------------------------------------
def test_the_snapshot_answers_only_for_a_pass_that_ran(engine, traffic):
    """no pass since the engine was created, or only a call that went to the per-item kernels: an error, not stale memory; an
    unknown region or a buffer that is too small: an error, and nothing is written"""
    import ctypes
    lib = engine.library()
    buf = np.full(64, 0xAA, np.uint8)
    snap = lambda region, nbytes: lib.eddsa_amd_debug_rlc_snapshot(ctypes.c_int(region), buf.ctypes.data_as(ctypes.c_void_p),  # noqa: E731
                                                                   ctypes.c_size_t(nbytes))
    sig, pk, msg = (a[:5] for a in traffic)
    engine.shutdown()
    engine.init(0)
    try:
        with pytest.raises(engine.EddsaAmdError):
            engine.debug_rlc_snapshot("seed")
        engine.set_rlc_min_items(6)                     # five items: the per-item kernels, no pass of the combination
        ok, st = engine.ed25519_verify_batch_rlc(dev(sig), dev(pk), dev(msg), msg_len=32, return_stats=True)
        assert bool(ok.all()) and st == (0, 5, 1, 0)
        assert snap(2, 32) == -600                      # hipErrorNotReady
    finally:
        engine.set_rlc_min_items(0)
    ok, st = run(engine, sig, pk, msg)
    assert ok.all() and st == (5, 0, 0, 1)
    assert engine.debug_rlc_snapshot("info") == (5, 1, 2048)
    assert snap(1, 5 * 32 - 1) == -1 and snap(0, 23) == -1 and snap(10, 64) == -1 and snap(-1, 64) == -1      # hipErrorInvalidValue
    assert (buf == 0xAA).all()
    assert snap(2, 64) == 32 and buf[:32].tobytes() == Model(sig, pk, msg).seed and (buf[32:] == 0xAA).all()
