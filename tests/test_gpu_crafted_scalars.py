"""GPU tests of every verify route on CHOSEN scalars (tests/crafted_scalars.py): the digest forms take the 64 digest bytes from
the caller, so t = digest mod l, S and the key are picked - digit patterns that random digests never show, the bounds of the three
pair searches, and for each evaluation the signatures that are valid exactly when one window is skipped.  Expected verdicts are
the integer models' (ed_model.verify_t, policy_model.holds, cofactored_model.accepts_t), never the engine's.  The same set runs
through the device source on the host in tests/test_crafted_scalars_on_host.py."""
import numpy as np
import pytest

import crafted_scalars as cs
import policy_model as pm
from gpu_kit import bad, dev, dev_idx, host, settings

pytestmark = pytest.mark.gpu


class Set:
    def __init__(self):
        self.items, self.report = cs.build()
        self.sig, self.pub, self.dig, self.key = cs.arrays(self.items)
        self.want = cs.verdicts(self.items)
        self.want.setflags(write=False)
        self.n = len(self.items)

    def pick(self, idx):
        idx = np.asarray(idx) % self.n
        return tuple(np.ascontiguousarray(a[idx]) for a in (self.sig, self.pub, self.dig, self.key, self.want))

    def tiled(self, n):
        """the set repeated up to n items"""
        return self.pick(np.arange(n))

    def kinds(self, where, idx=None):
        idx = np.arange(self.n) if idx is None else np.asarray(idx) % self.n
        return [(int(i), self.items[idx[i]].kind, hex(self.items[idx[i]].t)) for i in where]


@pytest.fixture(scope="module")
def crafted():
    return Set()


def check(c, got, want, idx=None):
    wrong = bad(got, want)
    assert np.array_equal(host(got), want), c.kinds(wrong, idx)


def both_forms(engine, c, sig, pub, dig, want, idx=None):
    check(c, engine.ed25519_verify_digests(sig, pub, dig), want, idx)
    check(c, engine.ed25519_verify_digests(dev(sig), dev(pub), dev(dig)), want, idx)


# ---------------------------------------------------------------- ed25519_verify_digests: every route of verify_route_of

def test_the_set_fits_one_window_sums_pass(crafted):
    assert 1000 < crafted.n <= 2048 and 0 < crafted.want.sum() < crafted.n


@pytest.mark.parametrize("n", [1, 64, 256])
def test_window_sums_pairs_below_2_134(engine, crafted, n):
    """algo 0 up to 256 items: three-lane preparation with pairs below 2^134, window sums, four-lane chain of 34 windows.
    256: the whole set in passes of 256; 64: three passes strided over the set; 1: a valid item, two near misses, two give-ups"""
    c = crafted
    if n == 256:
        passes = [np.arange(k, k + 256) for k in range(0, c.n, 256)]
    elif n == 64:
        passes = [np.arange(k, c.n, c.n // 64)[:64] for k in range(3)]
    else:
        near = [i for i, it in enumerate(c.items) if it.kind.startswith("h134:")]
        long_ = [i for i, it in enumerate(c.items) if not cs.pair_of("h134", it.t)[2]]
        passes = [np.array([i]) for i in (0, near[0], near[-1], long_[0], long_[-1])]
    with settings(engine, algo=0):
        for idx in passes:
            assert len(idx) == n
            sig, pub, dig, _, want = c.pick(idx)
            both_forms(engine, c, sig, pub, dig, want, idx)


def test_window_sums_pairs_below_2_138(engine, crafted):
    """algo 0, 257 .. 2048 items: the whole set in one pass"""
    c = crafted
    assert 256 < c.n <= 2048
    with settings(engine, algo=0):
        both_forms(engine, c, c.sig, c.pub, c.dig, c.want)


@pytest.mark.parametrize("algo,what", [(0, "four-lane half-length evaluation, 35 windows"), (3, "three-lane preparation, one-lane evaluation, long loop in place"),
                                       (2, "halve kernel, pairs below 2^138"), (4, "balanced pairs, 33 windows"), (1, "full-length, four lanes")])
def test_each_route_at_2049_items(engine, crafted, algo, what):
    c = crafted
    sig, pub, dig, _, want = c.tiled(2049)
    with settings(engine, algo=algo):
        both_forms(engine, c, sig, pub, dig, want)


def test_full_length_one_lane(engine, crafted):
    """algo 1 above 2^14 items: k_verify_main"""
    c = crafted
    sig, pub, dig, _, want = c.tiled(16385)
    with settings(engine, algo=1):
        both_forms(engine, c, sig, pub, dig, want)


@pytest.mark.parametrize("offcurve", [False, 2])
def test_reject_mode_and_replay_all(engine, crafted, offcurve):
    """off-curve mode 0 (the full-length route whatever the size) and 2 (every item through the exact path)"""
    c = crafted
    with settings(engine, offcurve=offcurve):
        both_forms(engine, c, c.sig, c.pub, c.dig, c.want)


# ---------------------------------------------------------------- ed25519_verify_keyed_digests

def keyed_forms(engine, c, ks, sig, key, dig, want, forms=("host", "dev")):
    if "host" in forms:
        check(c, engine.ed25519_verify_keyed_digests(sig, ks, np.ascontiguousarray(key, dtype=np.uint32), dig), want)
    if "dev" in forms:
        check(c, engine.ed25519_verify_keyed_digests(dev(sig), ks, dev_idx(key), dev(dig)), want)


@pytest.mark.parametrize("offcurve", [False, True])
@pytest.mark.parametrize("comb", [False, True])
def test_keyed_one_pass(engine, crafted, comb, offcurve):
    """the six keys as a key set, plain (half-length, 2^138 / 35 windows; reject mode: full-length, one lane) and with combs
    (k_verify_main_comb_keyed in both modes)"""
    c = crafted
    with engine.keyset_create(cs.key_bytes(), comb=comb) as ks, settings(engine, offcurve=offcurve):
        keyed_forms(engine, c, ks, c.sig, c.key, c.dig, c.want)


def test_keyed_pairs_below_2_134(engine, crafted):
    """a keyed pass of 2^19 items, the only way to the keyed kernel of 34 windows; device form"""
    c = crafted
    sig, _, dig, key, want = c.tiled(1 << 19)
    with engine.keyset_create(cs.key_bytes()) as ks, settings(engine):
        keyed_forms(engine, c, ks, sig, key, dig, want, forms=("dev",))


# ---------------------------------------------------------------- the batch verification

def test_rlc_forms(engine, crafted):
    """ed25519_verify_digests_rlc and ed25519_verify_keyed_digests_rlc with the combination from one item on: the valid items
    alone are all accepted; the whole set gets the models' verdicts"""
    c = crafted
    good = np.nonzero(c.want)[0]
    with engine.keyset_create(cs.key_bytes()) as ks, settings(engine, rlc_min=0):
        for idx in (good, np.arange(c.n)):
            sig, pub, dig, key, want = c.pick(idx)
            assert want.all() == (len(idx) == len(good))
            check(c, engine.ed25519_verify_digests_rlc(sig, pub, dig), want, idx)
            check(c, engine.ed25519_verify_digests_rlc(dev(sig), dev(pub), dev(dig)), want, idx)
            check(c, engine.ed25519_verify_keyed_digests_rlc(sig, ks, key, dig), want, idx)
            check(c, engine.ed25519_verify_keyed_digests_rlc(dev(sig), ks, dev_idx(key), dev(dig)), want, idx)


# ---------------------------------------------------------------- the strict rules, the cofactored equation

@pytest.mark.parametrize("cofactored", [False, True])
def test_strict_rules_and_cofactored_equation(engine, crafted, cofactored):
    """once each on the balanced route, the full-length route and the comb key set"""
    c = crafted
    policy = 0 if cofactored else pm.STRICT
    want = cs.verdicts(c.items, policy=policy, cofactored=cofactored)
    assert 0 < want.sum() and not np.array_equal(want, c.want)
    for algo in (4, 1):
        with settings(engine, algo=algo, policy=policy, cofactored=cofactored):
            both_forms(engine, c, c.sig, c.pub, c.dig, want)
    with engine.keyset_create(cs.key_bytes(), comb=True) as ks, settings(engine, policy=policy, cofactored=cofactored):
        keyed_forms(engine, c, ks, c.sig, c.key, c.dig, want)


# ---------------------------------------------------------------- counters

def test_no_pair_was_refused(engine, crafted):
    """after everything above: the integer check of verify_half_scalars_lane never had to refuse a pair"""
    assert engine.halve_rejected() == 0
