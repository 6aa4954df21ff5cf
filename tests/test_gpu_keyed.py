"""GPU tests of key-set verification (include/eddsa_amd.h: eddsa_amd_keyset, ed25519_verify_keyed[_dev]; keyed_kernels.h): ok[i] is
what the reference's ed25519_verify returns for (sigs[i], keys[key_idx[i]], message i), an index outside the key set rejects its
item.  Expected verdicts are the oracle's on (sig, keys[idx], msg) - under a policy or the cofactored equation those of
tests/policy_model.py and tests/cofactored_model.py - never the engine's own unkeyed call.  Every test puts the settings back."""
import ctypes
import subprocess

import numpy as np
import pytest

import cofactored_model as cm
import keyed_model as km
import policy_model as pm
import workload  # tools/ is on sys.path (conftest)
from gpu_kit import bad, dev, dev_idx, host, settings
from hostlib import build_c_program

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 63, 64, 65, 255, 257, 4099)
KEYSETS = (1, 3, 300)
MAXLEN = 150


def keyed(engine, form, ks, idx, sig, msgs, off=None, mlen=None):
    """form "dev": every array in HBM, the key set as it is; "host": numpy arrays"""
    if form == "dev":
        got = engine.ed25519_verify_keyed(dev(sig), ks, dev_idx(idx), dev(msgs), msg_off=None if off is None else dev(off.astype(np.int64)),
                                          msg_len=mlen)
        return host(got)
    return engine.ed25519_verify_keyed(sig, ks, np.ascontiguousarray(idx, dtype=np.uint32), msgs, msg_off=off, msg_len=mlen)


def oracle_verdicts(oracle, sig, pubs, msgs, off, mlen):
    if off is None:
        return oracle.verify_batch(np.ascontiguousarray(sig), np.ascontiguousarray(pubs), np.ascontiguousarray(msgs), mlen)
    flat = msgs.tobytes()
    return np.array([oracle.verify(sig[i].tobytes(), pubs[i].tobytes(), flat[int(off[i]):int(off[i + 1])]) for i in range(len(sig))], np.uint8)


# ---------------------------------------------------------------- shared inputs: built once, never modified

@pytest.fixture(scope="module")
def honest(engine):
    """300 secret keys and their public keys"""
    sk = workload.field_bytes(77, 2, workload.F_SK, 300, 32)
    pk = host(engine.ed25519_genpub_batch(dev(sk)))
    return sk, pk


_MIXED = {}


def mixed(engine, oracle, honest, n, nkeys, ragged):
    """n items signed by the engine under `nkeys` honest keys, then mixed by item index mod 8 - 0..4: untouched; 5: one bit of the
    signature flipped; 6: refers to a key-set entry that is its key with one bit flipped; 7: refers to a random 32-byte entry
    (about half of those are no curve point).  -> (keys, idx, sig, msgs, off, mlen, the oracle's verdicts)"""
    if (n, nkeys, ragged) in _MIXED:
        return _MIXED[(n, nkeys, ragged)]
    sk, pk = honest
    rng = np.random.default_rng(1000 * n + 10 * nkeys + ragged)
    who = rng.integers(0, nkeys, n)
    if ragged:
        lens = rng.integers(0, MAXLEN + 1, n)
        lens[: min(n, 3)] = (MAXLEN, 0, 1)[: min(n, 3)]                              # (never an empty message buffer)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        mlen = None
    else:
        lens = np.full(n, 32)
        off, mlen = None, 32
    msgs = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    sig = host(engine.ed25519_sign_batch(dev(sk[who]), dev(pk[who]), dev(msgs),
                                         msg_off=None if off is None else dev(off.astype(np.int64)), msg_len=mlen)).copy()
    pubs = pk[who].copy()
    for i in range(n):
        k = i % 8
        if k == 5:
            sig[i, rng.integers(0, 64)] ^= 1 << rng.integers(0, 8)
        elif k == 6:
            pubs[i, rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)
        elif k == 7:
            pubs[i] = rng.integers(0, 256, 32, dtype=np.uint8)
    keys, idx = km.as_keyset(pubs, pk[:nkeys])
    assert np.array_equal(keys[idx], pubs) and np.array_equal(keys[:nkeys], pk[:nkeys])
    want = oracle_verdicts(oracle, sig, pubs, msgs, off, mlen)
    # the off-curve modes agree on this batch: no accepted item has a key that is no curve point (mode 0 rejects those outright)
    assert all(km.decodes(pubs[i].tobytes()) for i in np.nonzero(want)[0])
    if n >= 63:
        assert 0 < want.sum() < n and not all(km.decodes(pubs[i].tobytes()) for i in range(7, n, 8))
    out = (keys, idx, sig, msgs, off, mlen, want)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _MIXED[(n, nkeys, ragged)] = out
    return out


# ---------------------------------------------------------------- 1: parity at small sizes

@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_parity_at_small_sizes(engine, oracle, honest, n, mode):
    """every size at which a block, a wave or a tile ends, key sets of 1, 3 and 300 honest keys (plus the flipped and the random
    entries their items refer to), fixed and ragged messages, both forms, the three off-curve modes"""
    for nkeys in KEYSETS:
        for ragged in (0, 1):
            keys, idx, sig, msgs, off, mlen, want = mixed(engine, oracle, honest, n, nkeys, ragged)
            with engine.keyset_create(dev(keys)) as ks, settings(engine, offcurve=mode):
                assert ks.count == len(keys)
                for form in ("dev", "host"):
                    got = keyed(engine, form, ks, idx, sig, msgs, off, mlen)
                    assert got.dtype == np.uint8 and got.shape == (n,)
                    assert np.array_equal(got, want), (nkeys, ragged, form, bad(got, want))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", ["verify_edges.json", "verify_torsion.json"])
def test_golden_files_as_key_sets(engine, golden, name, mode):
    """entry i = case i's key: idx = arange, then the items shuffled"""
    cases = golden(name)
    sig, keys = pm.arr([pm.H(c["sig"]) for c in cases]), pm.arr([pm.H(c["pub"]) for c in cases])
    want = np.array([c["accept"] for c in cases], np.uint8)
    lens = np.array([len(c["msg"]) // 2 for c in cases])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    msgs = np.frombuffer(b"".join(pm.H(c["msg"]) for c in cases), np.uint8)
    order = np.random.default_rng(5).permutation(len(cases))
    with engine.keyset_create(keys) as ks, settings(engine, offcurve=mode):
        for form in ("dev", "host"):
            got = keyed(engine, form, ks, np.arange(len(cases)), sig, msgs, off)
            assert np.array_equal(got, want), (form, [cases[i]["name"] for i in bad(got, want)])
            o2 = np.concatenate([[0], np.cumsum(lens[order])]).astype(np.uint64)
            m2 = np.frombuffer(b"".join(pm.H(cases[i]["msg"]) for i in order), np.uint8)
            got = keyed(engine, form, ks, order, sig[order], m2, o2)
            assert np.array_equal(got, want[order]), (form, "shuffled", bad(got, want[order]))


# ---------------------------------------------------------------- 2: index patterns

@pytest.fixture(scope="module")
def valid257(engine, honest):
    """257 valid items under five keys, item i under key i % 5"""
    sk, pk = honest
    who = np.arange(257) % 5
    msg = workload.field_bytes(78, 2, workload.F_MSG, 257, 32)
    sig = host(engine.ed25519_sign_batch(dev(sk[who]), dev(pk[who]), dev(msg), msg_len=32))
    return sk, pk[:5].copy(), who.astype(np.uint32), sig, msg


def test_one_key_and_a_permutation(engine, oracle, honest, valid257):
    sk, pk = honest
    _, keys5, who, sig, msg = valid257
    msg1 = workload.field_bytes(79, 2, workload.F_MSG, 257, 32)
    sig1 = host(engine.ed25519_sign_batch(dev(np.repeat(sk[3:4], 257, 0)), dev(np.repeat(pk[3:4], 257, 0)), dev(msg1), msg_len=32)).copy()
    sig1[100, 5] ^= 4
    want1 = oracle.verify_batch(sig1, np.repeat(pk[3:4], 257, 0), msg1, 32)
    assert want1.sum() == 256
    perm = np.random.default_rng(9).permutation(257).astype(np.uint32)
    msgp = workload.field_bytes(80, 2, workload.F_MSG, 257, 32)
    sigp = host(engine.ed25519_sign_batch(dev(sk[perm]), dev(pk[perm]), dev(msgp), msg_len=32))
    assert oracle.verify_batch(sigp, np.ascontiguousarray(pk[perm]), msgp, 32).all()
    with engine.keyset_create(pk[:257]) as ks:
        for form in ("dev", "host"):
            got = keyed(engine, form, ks, np.full(257, 3), sig1, msg1, mlen=32)      # every item refers to the same key
            assert np.array_equal(got, want1), (form, bad(got, want1))
            got = keyed(engine, form, ks, perm, sigp, msgp, mlen=32)                 # a permutation
            assert got.all(), (form, np.nonzero(got == 0)[0][:10])
            # the identity where a permutation is due: only the fixed points verify
            got = keyed(engine, form, ks, np.arange(257), sigp, msgp, mlen=32)
            assert np.array_equal(got, (perm == np.arange(257)).astype(np.uint8)), form


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_out_of_range_indices_reject_their_items_only(engine, oracle, valid257, mode):
    _, keys, who, sig, msg = valid257
    assert oracle.verify_batch(sig, np.ascontiguousarray(keys[who]), msg, 32).all()
    at = (0, 63, 64, 256)
    idx = who.copy()
    for p, v in zip(at, (5, 6, 0xFFFFFFFF, 5)):
        idx[p] = v
    want = np.ones(257, np.uint8)
    want[list(at)] = 0
    with engine.keyset_create(keys) as ks, settings(engine, offcurve=mode):
        for form in ("dev", "host"):
            got = keyed(engine, form, ks, idx, sig, msg, mlen=32)
            assert np.array_equal(got, want), (form, bad(got, want))
            got = keyed(engine, form, ks, who, sig, msg, mlen=32)                      # and nothing sticks
            assert got.all(), form


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("kind", ["valid_for_key_0", "forgery_for_the_zero_key"])
def test_out_of_range_indices_under_the_cofactored_equation(engine, honest, valid257, mode, kind):
    """the cofactored kernels decide every rejected item again from its key bytes: an item without a key must not come back
    accepted - neither with a signature that key 0 made, nor with R = [S]B, which verifies under the all-zero key (a point of
    order 4: [8][t]A vanishes)"""
    sk, keys, who, sig, msg = valid257
    at = (0, 63, 64, 256)
    sig, idx = sig.copy(), who.copy()
    for j, p in enumerate(at):
        idx[p] = (5, 6, 0xFFFFFFFF, 5)[j]
        if kind == "valid_for_key_0":
            sig[p] = host(engine.ed25519_sign_batch(dev(sk[0:1]), dev(keys[0:1]), dev(msg[p:p + 1]), msg_len=32))[0]
            assert cm.accepts(sig[p].tobytes(), keys[0].tobytes(), msg[p].tobytes())
        else:
            s = 12345 + 1000003 * j
            sig[p, :32] = np.frombuffer(cm.encode(cm.pmul(s, cm.B)), np.uint8)
            sig[p, 32:] = np.frombuffer(s.to_bytes(32, "little"), np.uint8)
            assert cm.accepts(sig[p].tobytes(), bytes(32), msg[p].tobytes())          # what a zero key would have let through
        assert not cm.accepts(sig[p].tobytes(), km.NO_KEY, msg[p].tobytes())
    want = np.ones(257, np.uint8)
    want[list(at)] = 0
    assert all(cm.accepts(sig[i].tobytes(), keys[who[i]].tobytes(), msg[i].tobytes()) for i in (1, 62, 65, 255))
    with engine.keyset_create(keys) as ks, settings(engine, offcurve=mode, cofactored=True):
        for form in ("dev", "host"):
            got = keyed(engine, form, ks, idx, sig, msg, mlen=32)
            assert np.array_equal(got, want), (form, bad(got, want))


# ---------------------------------------------------------------- 3: the neutral entry

def _off_curve_keys(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        k = rng.integers(0, 256, 32, dtype=np.uint8)
        if not km.decodes(k.tobytes()):
            out.append(k)
    return np.array(out)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_neutral_entry_is_key_0s_whatever_key_0_is(engine, oracle, valid257, mode):
    """a zero digit reads entry 0 of key 0: (a) key 0 off the curve, the items under on-curve keys; (b) item 0 itself under an
    off-curve key; (c) a key set of off-curve keys only"""
    _, keys5, who, sig, msg = valid257
    off3 = _off_curve_keys(3, 4)
    keys = np.concatenate([off3[:1], keys5])                                          # (a)
    want = oracle.verify_batch(sig, np.ascontiguousarray(keys[who + 1]), msg, 32)
    assert want.all()
    idx_b = (who + 1).copy()
    idx_b[0] = 0                                                                      # (b)
    want_b = oracle.verify_batch(sig, np.ascontiguousarray(keys[idx_b]), msg, 32)
    assert want_b[0] == 0 and want_b[1:].all()
    with engine.keyset_create(keys) as ks, settings(engine, offcurve=mode):
        for form in ("dev", "host"):
            got = keyed(engine, form, ks, who + 1, sig, msg, mlen=32)
            assert np.array_equal(got, want), (form, bad(got, want))
            got = keyed(engine, form, ks, idx_b, sig, msg, mlen=32)
            assert np.array_equal(got, want_b), (form, bad(got, want_b))
    idx_c = (who % 3).astype(np.uint32)                                               # (c)
    want_c = oracle.verify_batch(sig, np.ascontiguousarray(off3[idx_c]), msg, 32)
    with engine.keyset_create(off3) as ks, settings(engine, offcurve=mode):
        for form in ("dev", "host"):
            got = keyed(engine, form, ks, idx_c, sig, msg, mlen=32)
            assert np.array_equal(got, want_c), (form, bad(got, want_c))


# ---------------------------------------------------------------- 4: items without a short pair

N4, K4, SEED4 = (1 << 19) + 77, 1000, 20261019
# on-curve items of the batch below for which keyed_model.short_pair finds no pair below 2^134 (found with the oracle's
# signatures on a CPU; the test holds every one of them against the model again - the list only spares it the other 524 000)
NO_PAIR = (2915, 14301, 31638, 32915, 42369, 52121, 69442, 82263, 82829, 95179, 101811, 114760, 146426, 176271, 177962, 184993, 205807,
           215692, 219894, 236943, 267812, 285197, 288094, 292924, 297178, 307104, 309251, 315227, 321913, 322118, 332695, 336856,
           339170, 340767, 360947, 372668, 395029, 407211, 410912, 412485, 425923, 427481, 444192, 464426, 476376, 477366, 498709,
           500326, 507165, 507947, 512478, 514117, 514212, 516648, 518557, 521833, 522505)   # 57: DESIGN's 8.5 in 10^5 expects 44


def test_items_without_a_short_pair_get_a_copy_of_their_keys_table(engine, oracle):
    """n = 2^19 + 77 takes the narrow search (pairs below 2^134, 8.5 give-ups in 10^5): k_verify_halve_keyed hands those items to
    the exact path, which reads the item's own table - the copy of the key's nine entries.  About 1000 signing keys, the
    config-2 corruption (its flipped and replaced keys become further entries of the key set)."""
    sk = workload.field_bytes(SEED4, 2, workload.F_SK, K4, 32)
    msg = workload.field_bytes(SEED4, 2, workload.F_MSG, N4, 32)
    who = np.arange(N4, dtype=np.int64) * 7919 % K4
    pk = host(engine.ed25519_genpub_batch(dev(sk)))
    sig = host(engine.ed25519_sign_batch(dev(sk[who]), dev(pk[who]), dev(msg), msg_len=32)).copy()
    pubs = np.ascontiguousarray(pk[who])
    expect = workload.corrupt_for_verify(sig, pubs, msg, seed=SEED4, config=2)
    keys, idx = km.as_keyset(pubs, pk)
    want = oracle.verify_batch(sig, pubs, msg, 32)
    assert np.array_equal(want, expect)
    none = [i for i in NO_PAIR if km.decodes(pubs[i].tobytes()) and km.short_pair(km.challenge(sig[i], pubs[i], msg[i])) is None]
    assert len(none) >= 10 and want[none].sum() >= 5, (len(none), int(want[none].sum()))
    with engine.keyset_create(dev(keys)) as ks:
        got = keyed(engine, "dev", ks, idx, sig, msg, mlen=32)
    assert np.array_equal(got, want), bad(got, want)
    assert np.array_equal(got[none], want[none])


# ---------------------------------------------------------------- 5: settings

@pytest.fixture(scope="module")
def policy_items(oracle):
    sig, pk, msg, want = pm.policy_batch(oracle, 600)
    keys, idx = km.as_keyset(pk)
    return sig, pk, msg, want, keys, idx


@pytest.mark.parametrize("policy", pm.BITS + (pm.STRICT,))
def test_each_policy_bit(engine, policy_items, policy):
    sig, pk, msg, want, keys, idx = policy_items
    expect = want & pm.holds_batch(policy, sig, pk)
    assert (expect != want).any()
    with engine.keyset_create(keys) as ks:
        for mode in (0, 1):
            with settings(engine, offcurve=mode, policy=policy):
                for form in ("dev", "host"):
                    got = keyed(engine, form, ks, idx, sig, msg, mlen=pm.MLEN)
                    assert np.array_equal(got, expect), (mode, form, bad(got, expect))
        got = keyed(engine, "dev", ks, idx, sig, msg, mlen=pm.MLEN)                    # the settings are back: the reference's verdicts
        assert np.array_equal(got, want)


@pytest.mark.parametrize("policy", [0, pm.STRICT])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_cofactored_equation_over_its_vectors(engine, golden, mode, policy):
    sig, pk, msg, accept = cm.arrays(cm.from_json(golden("verify_cofactored.json")))
    expect = accept & pm.holds_batch(policy, sig, pk)
    assert 0 < expect.sum() < len(expect)
    order = np.random.default_rng(6).permutation(len(sig))
    with engine.keyset_create(pk) as ks, settings(engine, offcurve=mode, policy=policy, cofactored=True):
        for form in ("dev", "host"):
            got = keyed(engine, form, ks, np.arange(len(sig)), sig, msg, mlen=32)
            assert np.array_equal(got, expect), (form, bad(got, expect))
            got = keyed(engine, form, ks, order, sig[order], msg[order], mlen=32)
            assert np.array_equal(got, expect[order]), (form, "shuffled", bad(got, expect[order]))


# ---------------------------------------------------------------- 6: workspace reuse

@pytest.mark.parametrize("mode", [0, 1])
def test_keyed_and_unkeyed_passes_share_workspaces(engine, oracle, honest, mode):
    """on one stream: keyed, unkeyed, keyed with another key set - and the reverse; neither may depend on what the other left in
    the tables, the flags or the key-bytes area.  Two key sets alive at once; one is destroyed, the other used again"""
    a = mixed(engine, oracle, honest, 4099, 300, 0)
    b = mixed(engine, oracle, honest, 4099, 3, 0)
    ka, kb = engine.keyset_create(dev(a[0])), engine.keyset_create(b[0])               # create_dev and create
    try:
        with settings(engine, offcurve=mode):
            def run_keyed(ks, x):
                got = keyed(engine, "dev", ks, x[1], x[2], x[3], mlen=32)
                assert np.array_equal(got, x[6]), bad(got, x[6])

            def run_unkeyed(x):
                got = host(engine.ed25519_verify_batch(dev(x[2]), dev(x[0][x[1]]), dev(x[3]), msg_len=32))
                assert np.array_equal(got, x[6]), bad(got, x[6])
            for step in ("ka", "ub", "kb", "ua", "ka", "kb", "ka", "ub", "kb"):
                run_keyed(ka if step == "ka" else kb, a if step == "ka" else b) if step[0] == "k" else run_unkeyed(a if step == "ua" else b)
            ka.close()
            run_keyed(kb, b)
            engine.shutdown()                                                         # a key set survives the engines
            engine.init(0)
            run_keyed(kb, b)
    finally:
        ka.close()
        kb.close()


def test_create_and_create_dev_give_the_same_key_set(engine, oracle, honest):
    keys, idx, sig, msgs, off, mlen, want = mixed(engine, oracle, honest, 257, 300, 1)
    with engine.keyset_create(keys) as k1, engine.keyset_create(dev(keys)) as k2:
        assert k1.count == k2.count == len(keys) and k1.device == k2.device == 0
        for ks in (k1, k2):
            for form in ("dev", "host"):
                got = keyed(engine, form, ks, idx, sig, msgs, off, mlen)
                assert np.array_equal(got, want), bad(got, want)
    with pytest.raises(ValueError):
        k1.count


# ---------------------------------------------------------------- 7: chunks

def test_two_passes_of_the_device_form(engine, oracle):
    """n = 2^20 + 513: two workspace passes; the second pass's indices must be the second pass's"""
    n, nk = (1 << 20) + 513, 1024
    sk = workload.field_bytes(91, 2, workload.F_SK, nk, 32)
    msg = workload.field_bytes(91, 2, workload.F_MSG, n, 32)
    who = (np.arange(n, dtype=np.int64) * 613 + 7) % nk
    pk = host(engine.ed25519_genpub_batch(dev(sk)))
    sig = host(engine.ed25519_sign_batch(dev(sk[who]), dev(pk[who]), dev(msg), msg_len=32)).copy()
    sig[5::16, 40] ^= 2
    idx = who.astype(np.uint32)
    idx[9::16] = (idx[9::16] + 1) % nk                                                # the wrong key
    want = oracle.verify_batch(sig, np.ascontiguousarray(pk[idx]), msg, 32)
    assert want[(1 << 20):].sum() not in (0, 513) and want.sum() == n - len(want[5::16]) - len(want[9::16])
    with engine.keyset_create(pk) as ks:
        got = keyed(engine, "dev", ks, idx, sig, msg, mlen=32)
    assert np.array_equal(got, want), bad(got, want)


def test_chunks_of_the_host_form(engine, oracle, honest):
    """the host pipeline forced to chunks of 4096 at n = 3 * 4096 + 77: every chunk uploads its own slice of the indices"""
    sk, pk = honest
    n = 3 * 4096 + 77
    msg = workload.field_bytes(92, 2, workload.F_MSG, n, 32)
    who = (np.arange(n, dtype=np.int64) * 101 + 3) % 300
    sig = host(engine.ed25519_sign_batch(dev(sk[who]), dev(pk[who]), dev(msg), msg_len=32)).copy()
    sig[5::16, 3] ^= 1
    idx = who.astype(np.uint32)
    idx[9::16] = (idx[9::16] + 1) % 300
    want = oracle.verify_batch(sig, np.ascontiguousarray(pk[idx]), msg, 32)
    assert all(0 < want[lo:lo + 4096].sum() < len(want[lo:lo + 4096]) for lo in range(0, n, 4096))
    lib = engine.library()
    with engine.keyset_create(pk) as ks:
        try:
            lib.eddsa_amd_set_pipeline(ctypes.c_size_t(4096), ctypes.c_size_t(4096))
            got = keyed(engine, "host", ks, idx, sig, msg, mlen=32)
        finally:
            lib.eddsa_amd_set_pipeline(ctypes.c_size_t(0), ctypes.c_size_t(0))
    assert np.array_equal(got, want), bad(got, want)


# ---------------------------------------------------------------- 8: the shipped library, from C

def test_c_program_against_the_shipped_library(engine, oracle, honest, tmp_path):
    """tests/c/verify_keyed.c: plain C against eddsa_amd.h, linked against libeddsa_amd.so (which exports no hook)"""
    keys, idx, sig, msgs, off, mlen, want = mixed(engine, oracle, honest, 257, 300, 0)
    idx = idx.copy()
    want = want.copy()
    idx[0], idx[256] = len(keys), 0xFFFFFFFF
    want[0] = want[256] = 0
    exe = build_c_program(tmp_path, "verify_keyed.c", libs=("eddsa_amd",), wall=True)
    files = []
    for name, a in (("keys", keys), ("idx", idx.astype(np.uint32)), ("sigs", sig), ("msgs", msgs), ("want", want)):
        files.append(str(tmp_path / (name + ".bin")))
        np.ascontiguousarray(a).tofile(files[-1])
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify_keyed: ok (257 items" in r.stdout
