"""GPU tests of the opt-in cofactored equation of verification (include/eddsa_amd.h: eddsa_amd_set_verify_equation; kernels.hip:
k_cofactor_list / k_cofactor_points / k_cofactor_eval; rlc.hip: k_rlc_points): under it item i is accepted exactly when S < l, A
and R decode and [8](S B - t A - R) = 0.  Expected verdicts are the Python model's (tests/cofactored_model.py, the committed
vectors of tests/golden/verify_cofactored.json and their siblings under a dom2 prefix) - never the engine's.  Every test puts the
equation, the policy and the mode word back."""
import hashlib

import numpy as np
import pytest

import cofactored_model as cm
import policy_model as pm
from gpu_kit import bad, dev, host, settings
from policy_model import BITS, STRICT

pytestmark = pytest.mark.gpu
G = 8192                                            # items per group of the batch verification
MLEN = 32


@pytest.fixture(scope="module")
def vecs(golden):
    """the committed vectors (the CPU suite holds them against the model that generates them); shared, never modified"""
    return cm.from_json(golden("verify_cofactored.json"))


@pytest.fixture(scope="module")
def arrs(vecs):
    return cm.arrays(vecs)


@pytest.fixture(scope="module")
def cofactorless(arrs, oracle):
    """what the reference's check says of the vectors: the two equations differ on a third of them"""
    ok = oracle.verify_batch(arrs[0], arrs[1], arrs[2], MLEN)
    assert (ok != arrs[3]).sum() > len(ok) // 4
    return ok


def digests(sig, pk, msg, prefix=b""):
    return pm.arr([hashlib.sha512(prefix + sig[i, :32].tobytes() + pk[i].tobytes() + msg[i].tobytes()).digest() for i in range(len(sig))])


# ---------------------------------------------------------------- 1: parity with the model, every size, route and form

@pytest.mark.parametrize("algo,offcurve,n", [(0, True, 257), (0, True, 600), (1, True, 600), (2, True, 600), (3, True, 600),
                                             (0, False, 600), (0, 2, 600), (2, 2, 257)])
def test_device_form_at_every_size_route_and_mode(engine, arrs, cofactorless, algo, offcurve, n):
    """the vectors tiled and shuffled: 257 items put more than 64 rejected ones into two blocks of k_cofactor_list (its appends
    cross a wave boundary), 600 into three; under every algo; with off-curve keys rejected (mode 0 - what mode 1 runs as) and in
    the self-check mode 2, where the reference-order chain decides every item first and the algo chooses its companions"""
    sig, pk, msg, want, pick = cm.tiled(arrs, n)
    assert (cofactorless[pick] != want).sum() > 64 and 0 < want.sum() < n
    with settings(engine, cofactored=True, algo=algo, offcurve=offcurve):
        got = host(engine.ed25519_verify_batch(dev(sig), dev(pk), dev(msg), msg_len=MLEN))
    assert got.dtype == np.uint8 and np.array_equal(got, want), bad(got, want)


def test_single_items_and_the_single_item_call(engine, vecs, arrs, cofactorless):
    """n = 1 through the device form for one item of every class, and every vector through ed25519_verify (the small-call
    combiner's path)"""
    sig, pk, msg, want = arrs
    first = {}
    for i, v in enumerate(vecs):
        if v["class"] != "c_mixed" or not cofactorless[i]:           # (a mixed-order item the pass itself rejects)
            first.setdefault(v["class"], i)
    assert len(first) == len(cm.CLASSES)
    with settings(engine, cofactored=True):
        for cls, i in first.items():
            got = host(engine.ed25519_verify_batch(dev(sig[i:i + 1]), dev(pk[i:i + 1]), dev(msg[i:i + 1]), msg_len=MLEN))
            assert got.tolist() == [want[i]], cls
        single = [engine.ed25519_verify(v["sig"], v["pub"], v["msg"]) for v in vecs]
    assert not len(bad(np.array(single, np.uint8), want))


def test_host_records_and_digest_forms(engine, arrs, cofactorless):
    sig, pk, msg, want, pick = cm.tiled(arrs, 600, seed=2)
    dig = digests(sig, pk, msg)
    rec = np.ascontiguousarray(np.concatenate([sig, pk, msg], axis=1))
    with settings(engine, cofactored=True):
        assert not len(bad(engine.ed25519_verify_batch(sig, pk, msg, msg_len=MLEN), want)), "host"
        assert not len(bad(engine.ed25519_verify_records(rec, 0, 64, 96, MLEN), want)), "records, host"
        assert not len(bad(engine.ed25519_verify_records(dev(rec), 0, 64, 96, MLEN), want)), "records, device"
        assert not len(bad(engine.ed25519_verify_digests(sig, pk, dig), want)), "digests, host"
        assert not len(bad(engine.ed25519_verify_digests(dev(sig), dev(pk), dev(dig)), want)), "digests, device"
    assert (cofactorless[pick] != want).any()


@pytest.mark.parametrize("flag", [0, 1])
def test_ctx_and_ph_forms(engine, flag):
    """vectors made under dom2(flag, context): Ed25519ctx over 32-byte messages, Ed25519ph over 64-byte prehashes; t comes from
    the prefixed hash (the model hashes the prefix), and the same bytes under another context are rejected but for the torsion
    class, whose verdict does not depend on t"""
    context = b"cofactored"
    mlen = 64 if flag else MLEN
    dvecs = cm.vectors(cm.dom2(flag, context), mlen=mlen)
    sig, pk, msg, want, pick = cm.tiled(cm.arrays(dvecs), 600, seed=3)
    other = np.array([dvecs[i]["class"] == "a_torsion" for i in pick], np.uint8)
    assert 0 < other.sum() < want.sum() < 600

    def run(s, p, m, c):
        if flag:
            return engine.ed25519ph_verify_batch(s, p, m, c)
        return engine.ed25519ctx_verify_batch(s, p, m, c, msg_len=mlen)

    with settings(engine, cofactored=True):
        assert not len(bad(run(sig, pk, msg, context), want)), "host"
        assert not len(bad(run(dev(sig), dev(pk), dev(msg), context), want)), "device"
        assert not len(bad(run(dev(sig), dev(pk), dev(msg), b"another"), other)), "another context"


# ---------------------------------------------------------------- 2: the batch verification

def rlc_forms(engine, sig, pk, msg, dig):
    for put in (lambda a: a, dev):
        yield "messages", engine.ed25519_verify_batch_rlc(put(sig), put(pk), put(msg), msg_len=MLEN, return_stats=True)
        yield "digests", engine.ed25519_verify_digests_rlc(put(sig), put(pk), put(dig), return_stats=True)


def test_batch_verification_equals_the_per_item_rule(engine, vecs, arrs):
    """two groups: the first holds the vectors - small-order points in every encoding, non-canonical R, mixed orders - the second
    300 honest signatures.  Verdicts = the model's = the per-item kernels'; the second group is decided by the combination"""
    n = G + 300
    sig1, pk1, msg1, want1, _ = cm.tiled(arrs, G, seed=4)
    honest = np.array([i for i, v in enumerate(vecs) if v["class"] == "b_honest"])
    pick2 = honest[np.arange(300) % len(honest)]
    sig, pk, msg = (np.ascontiguousarray(np.concatenate([a, b[pick2]])) for a, b in ((sig1, arrs[0]), (pk1, arrs[1]), (msg1, arrs[2])))
    want = np.concatenate([want1, arrs[3][pick2]])
    assert want[G:].all() and 0 < want[:G].sum() < G
    dig = digests(sig, pk, msg)
    with settings(engine, cofactored=True, rlc_min=0):
        per_item = host(engine.ed25519_verify_batch(dev(sig), dev(pk), dev(msg), msg_len=MLEN))
        assert np.array_equal(per_item, want), bad(per_item, want)
        for form, (ok, st) in rlc_forms(engine, sig, pk, msg, dig):
            assert np.array_equal(host(ok), want), (form, bad(ok, want))
            assert tuple(st) == (300, G, 1, 1), (form, st)      # by the combination, per item; groups per item, by the combination


def test_a_non_canonical_r_sends_its_group_to_the_per_item_kernels(engine, vecs, arrs):
    """a group of honest signatures and ONE item with R = the neutral element in a non-canonical encoding (x = 0 with the sign
    bit set; y = p + 1) and S = t a under an honest key: the cofactored rule accepts it, the combination cannot carry it - the
    group is decided item by item instead of the item being rejected at once.  Under the cofactorless equation the routing is
    what it was: the item is rejected through its flag and the group stays with the combination"""
    honest = [v for v in vecs if v["class"] == "b_honest"]
    rng_a = 0x1234567890abcdef1234567890abcdef % pm.L
    pub = cm.encode(cm.pmul(rng_a, cm.B))
    for r_enc in ((1 | 1 << 255).to_bytes(32, "little"), (pm.P + 1).to_bytes(32, "little")):
        m = bytes(range(MLEN))
        t = cm.challenge(r_enc, pub, m)
        odd = r_enc + (t * rng_a % pm.L).to_bytes(32, "little")
        assert cm.accepts(odd, pub, m)
        n, at = 300, 123
        sig = pm.arr([odd if i == at else honest[i % len(honest)]["sig"] for i in range(n)])
        pk = pm.arr([pub if i == at else honest[i % len(honest)]["pub"] for i in range(n)])
        msg = pm.arr([m if i == at else honest[i % len(honest)]["msg"] for i in range(n)])
        with settings(engine, cofactored=True, rlc_min=0):
            ok, st = engine.ed25519_verify_batch_rlc(dev(sig), dev(pk), dev(msg), msg_len=MLEN, return_stats=True)
        assert host(ok).all() and tuple(st) == (0, n, 1, 0), st
        with settings(engine, cofactored=False, rlc_min=0):
            ok, st = engine.ed25519_verify_batch_rlc(dev(sig), dev(pk), dev(msg), msg_len=MLEN, return_stats=True)
        assert np.array_equal(host(ok), np.arange(n) != at) and tuple(st) == (n, 0, 0, 1), st


# ---------------------------------------------------------------- 3: composition with the strict rules, the default untouched

def test_the_strict_rules_compose_with_the_equation(engine, arrs):
    """(cofactored verdict) AND (every predicate of the policy): A_NOT_SMALL rejects the whole torsion class, and so on"""
    sig, pk, msg, want, pick = cm.tiled(arrs, 600, seed=5)
    for policy in BITS + (STRICT,):
        both = want & pm.holds_batch(policy, sig, pk)
        with settings(engine, cofactored=True, policy=policy):
            got_d = host(engine.ed25519_verify_batch(dev(sig), dev(pk), dev(msg), msg_len=MLEN))
            got_h = engine.ed25519_verify_batch(sig, pk, msg, msg_len=MLEN)
        assert np.array_equal(got_d, both) and np.array_equal(got_h, both), (hex(policy), bad(got_d, both))
        if policy != BITS[0]:                               # (S < l is part of the equation already)
            assert 0 < both.sum() < want.sum(), hex(policy)
        else:
            assert np.array_equal(both, want)


def test_the_default_is_untouched_and_a_refused_value_changes_nothing(engine, arrs, cofactorless):
    import ctypes
    from libeddsa_amd import api
    sig, pk, msg, want, pick = cm.tiled(arrs, 600, seed=6)
    ref = cofactorless[pick]
    run = lambda: host(engine.ed25519_verify_batch(dev(sig), dev(pk), dev(msg), msg_len=MLEN))
    fn = engine.library().eddsa_amd_set_verify_equation
    fn.restype = ctypes.c_int
    try:
        assert np.array_equal(run(), ref)                   # before anything was set
        engine.set_offcurve_mode(2)
        engine.set_verify_policy(BITS[0])
        engine.set_verify_equation(True)
        assert fn(ctypes.c_int(2)) == -1 and fn(ctypes.c_int(-1)) == -1      # refused: still cofactored
        assert np.array_equal(run(), want)
        engine.set_verify_equation(False)
        # the reference's verdicts again, under the policy and the mode set before the equation was
        assert (api._offcurve_mode, api._verify_policy) == (2, BITS[0])
        assert np.array_equal(run(), ref & pm.holds_batch(BITS[0], sig, pk))
        engine.set_verify_policy(0)
        engine.set_offcurve_mode(True)
        assert np.array_equal(run(), ref)
    finally:
        engine.set_verify_equation(False)
        engine.set_verify_policy(0)
        engine.set_offcurve_mode(True)
    assert (ref != want).sum() > 100 and (ref & ~pm.holds_batch(BITS[0], sig, pk) & 1).any()


# ---------------------------------------------------------------- 4: the multi-device host form

def test_multi_device_form(engine, arrs):
    """over a one-device set, like the suite's other multi tests"""
    assert engine.init_devices([0]) == 1
    sig, pk, msg, want, pick = cm.tiled(arrs, 5000, seed=7)
    dig = digests(sig, pk, msg)
    with settings(engine, cofactored=True):
        assert not len(bad(engine.ed25519_verify_batch_multi(sig, pk, msg, msg_len=MLEN), want))
        assert not len(bad(engine.ed25519_verify_digests_multi(sig, pk, dig), want))
