"""GPU tests of comb key sets (include/eddsa_amd.h: eddsa_amd_keyset_create_comb[_dev]; keyed_kernels.h: k_keyset_comb_build,
k_verify_main_comb_keyed): the comb each key gets, read back against the integer model (tests/keyed_comb_model.py), and the
verdicts of ed25519_verify_keyed[_rlc] over a comb key set.  Expected verdicts are the oracle's on (sig, keys[idx], msg), the
recorded ones of the golden files, or - under a policy or the cofactored equation - those of tests/policy_model.py and
tests/cofactored_model.py; never the plain keyed form alone.  Every test puts the settings back."""
import ctypes

import numpy as np
import pytest

import cofactored_model as cfm
import keyed_comb_model as cm
import keyed_model as km
import policy_model as pm
import workload  # tools/ is on sys.path (conftest)
from gpu_kit import bad, dev, dev_idx, host, settings
from test_gpu_keyed import honest, keyed, mixed, valid257, _off_curve_keys  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
KEYSETS = (1, 2, 257)
PLAIN_BYTES = 32 + 1 + 9 * 128                       # per key: the bytes, the flag, the nine-entry table
COMB_BYTES = 704 * 128


def comb_set(engine, keys):
    ks = engine.keyset_create(keys, comb=True)
    assert ks.comb and ks.count == len(keys) and ks.nbytes == len(keys) * (PLAIN_BYTES + COMB_BYTES)
    return ks


def comb_of(engine, ks, key):
    words = np.zeros(cm.ENTRIES * cm.ENTRY_WORDS, np.uint32)
    rc = engine.library().eddsa_amd_debug_keyset_comb_read(ks._handle(), ctypes.c_size_t(key), words.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, rc
    return words.reshape(cm.ENTRIES, cm.ENTRY_WORDS)


# ---------------------------------------------------------------- 1: the comb itself

def test_comb_read_back_against_the_integer_model(engine, honest):
    """a 257-key set: the first and the last key, a small-order key and an off-curve key (readable, nothing more) in between;
    entries (0, 1), (0, 32), (21, 1), (21, 32) and one in the middle"""
    _, pk = honest
    keys = pk[:257].copy()
    keys[100] = 0                                                                     # (sqrt(-1), 0): order 4
    keys[200] = _off_curve_keys(1, 8)[0]
    with comb_set(engine, keys) as ks:
        for k in (0, 256, 100):
            neg_a = cm.decode_neg(keys[k].tobytes())
            assert neg_a is not None
            comb = comb_of(engine, ks, k)
            for row, m in ((0, 1), (0, 32), (21, 1), (21, 32), (9, 20)):
                assert cm.entry_point(comb[32 * row + m - 1]) == cm.entry(neg_a, row, m), (k, row, m)
        order4 = comb_of(engine, ks, 100)
        assert cm.entry_point(order4[3]) == cm.NEUTRAL and cm.entry_point(order4[32 * 21]) == cm.NEUTRAL   # 4 (-A) and 4096^21 (-A)
        assert comb_of(engine, ks, 200).shape == (704, 32)                            # off the curve: readable, no fault
        lib = engine.library()
        words = np.zeros(704 * 32, np.uint32)
        assert lib.eddsa_amd_debug_keyset_comb_read(ks._handle(), ctypes.c_size_t(257), words.ctypes.data_as(ctypes.c_void_p)) < 0
    with engine.keyset_create(keys[:2]) as plain:
        assert not plain.comb and plain.nbytes == 2 * PLAIN_BYTES
        assert engine.library().eddsa_amd_debug_keyset_comb_read(plain._handle(), ctypes.c_size_t(0), words.ctypes.data_as(ctypes.c_void_p)) < 0


# ---------------------------------------------------------------- 2: parity

@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_parity_at_small_sizes(engine, oracle, honest, n, mode):
    """every size at which a block, a wave or a tile ends, key sets of 1, 2 and 257 honest keys (plus the flipped and the random
    entries the corrupted items refer to), both forms, the three off-curve modes; ragged messages at the odd key count"""
    for nkeys in KEYSETS:
        ragged = int(nkeys == 2)
        keys, idx, sig, msgs, off, mlen, want = mixed(engine, oracle, honest, n, nkeys, ragged)
        with comb_set(engine, dev(keys)) as ks, settings(engine, offcurve=mode):
            for form in ("dev", "host"):
                got = keyed(engine, form, ks, idx, sig, msgs, off, mlen)
                assert got.dtype == np.uint8 and got.shape == (n,)
                assert np.array_equal(got, want), (nkeys, form, bad(got, want))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", ["verify_edges.json", "verify_torsion.json"])
def test_golden_files_as_a_comb_key_set(engine, golden, name, mode):
    """entry i = case i's key (S + k l, S = 2^256 - 1, small-order keys, non-canonical encodings): idx = arange, then shuffled"""
    cases = golden(name)
    sig, keys = pm.arr([pm.H(c["sig"]) for c in cases]), pm.arr([pm.H(c["pub"]) for c in cases])
    want = np.array([c["accept"] for c in cases], np.uint8)
    lens = np.array([len(c["msg"]) // 2 for c in cases])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    msgs = np.frombuffer(b"".join(pm.H(c["msg"]) for c in cases), np.uint8)
    order = np.random.default_rng(5).permutation(len(cases))
    with comb_set(engine, keys) as ks, settings(engine, offcurve=mode):
        got = keyed(engine, "dev", ks, np.arange(len(cases)), sig, msgs, off)
        assert np.array_equal(got, want), [cases[i]["name"] for i in bad(got, want)]
        o2 = np.concatenate([[0], np.cumsum(lens[order])]).astype(np.uint64)
        m2 = np.frombuffer(b"".join(pm.H(cases[i]["msg"]) for i in order), np.uint8)
        got = keyed(engine, "host", ks, order, sig[order], m2, o2)
        assert np.array_equal(got, want[order]), ("shuffled", bad(got, want[order]))


# ---------------------------------------------------------------- 3: settings

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
    with comb_set(engine, keys) as ks:
        for mode in (0, 1):
            with settings(engine, offcurve=mode, policy=policy):
                got = keyed(engine, "dev", ks, idx, sig, msg, mlen=pm.MLEN)
                assert np.array_equal(got, expect), (mode, bad(got, expect))
        got = keyed(engine, "dev", ks, idx, sig, msg, mlen=pm.MLEN)                    # the settings are back: the reference's verdicts
        assert np.array_equal(got, want)


@pytest.mark.parametrize("policy", [0, pm.STRICT])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_cofactored_equation_over_its_vectors(engine, golden, mode, policy):
    sig, pk, msg, accept = cfm.arrays(cfm.from_json(golden("verify_cofactored.json")))
    expect = accept & pm.holds_batch(policy, sig, pk)
    assert 0 < expect.sum() < len(expect)
    order = np.random.default_rng(6).permutation(len(sig))
    with comb_set(engine, pk) as ks, settings(engine, offcurve=mode, policy=policy, cofactored=True):
        got = keyed(engine, "dev", ks, np.arange(len(sig)), sig, msg, mlen=32)
        assert np.array_equal(got, expect), bad(got, expect)
        got = keyed(engine, "host", ks, order, sig[order], msg[order], mlen=32)
        assert np.array_equal(got, expect[order]), ("shuffled", bad(got, expect[order]))


# ---------------------------------------------------------------- 4: indices

@pytest.mark.parametrize("cofactored", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_out_of_range_indices_reject_their_items_only(engine, oracle, valid257, mode, cofactored):
    """under both equations; the items carry signatures that are valid for key 0, which idle slots walk"""
    sk, keys, who, sig, msg = valid257
    assert oracle.verify_batch(sig, np.ascontiguousarray(keys[who]), msg, 32).all()
    at = (0, 63, 64, 256)
    sig, idx = sig.copy(), who.copy()
    for p, v in zip(at, (5, 6, 0xFFFFFFFF, 5)):
        idx[p] = v
        sig[p] = host(engine.ed25519_sign_batch(dev(sk[0:1]), dev(keys[0:1]), dev(msg[p:p + 1]), msg_len=32))[0]
        assert oracle.verify(sig[p].tobytes(), keys[0].tobytes(), msg[p].tobytes())
        assert not cfm.accepts(sig[p].tobytes(), km.NO_KEY, msg[p].tobytes())
    want = np.ones(257, np.uint8)
    want[list(at)] = 0
    with comb_set(engine, keys) as ks, settings(engine, offcurve=mode, cofactored=cofactored):
        for form in ("dev", "host"):
            got = keyed(engine, form, ks, idx, sig, msg, mlen=32)
            assert np.array_equal(got, want), (form, bad(got, want))
        got = keyed(engine, "dev", ks, who, valid257[3], msg, mlen=32)                 # and nothing sticks
        assert got.all()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_key_0_off_the_curve_changes_nothing_for_the_neighbours(engine, oracle, valid257, mode):
    """a zero digit reads entry 0 of the item's OWN key's table, idle slots walk key 0's comb: (a) key 0 off the curve, the items
    under on-curve keys; (b) item 0 itself under the off-curve key"""
    _, keys5, who, sig, msg = valid257
    keys = np.concatenate([_off_curve_keys(1, 4), keys5])
    want = oracle.verify_batch(sig, np.ascontiguousarray(keys[who + 1]), msg, 32)
    assert want.all()
    idx_b = (who + 1).copy()
    idx_b[0] = 0
    want_b = oracle.verify_batch(sig, np.ascontiguousarray(keys[idx_b]), msg, 32)
    assert want_b[0] == 0 and want_b[1:].all()
    with comb_set(engine, keys) as ks, settings(engine, offcurve=mode):
        got = keyed(engine, "dev", ks, who + 1, sig, msg, mlen=32)
        assert np.array_equal(got, want), bad(got, want)
        got = keyed(engine, "dev", ks, idx_b, sig, msg, mlen=32)
        assert np.array_equal(got, want_b), bad(got, want_b)


# ---------------------------------------------------------------- 5: larger passes, workspaces, forms

N5, K5, SEED5 = (1 << 14) + 333, 500, 20261020


@pytest.fixture(scope="module")
def fuzz(engine, oracle):
    """2^14 + 333 items under about 500 signing keys with the config-2 corruption (its flipped and replaced keys become further
    entries of the key set) -> (keys, idx, sig, msg, the oracle's verdicts)"""
    sk = workload.field_bytes(SEED5, 2, workload.F_SK, K5, 32)
    msg = workload.field_bytes(SEED5, 2, workload.F_MSG, N5, 32)
    who = np.arange(N5, dtype=np.int64) * 7919 % K5
    pk = host(engine.ed25519_genpub_batch(dev(sk)))
    sig = host(engine.ed25519_sign_batch(dev(sk[who]), dev(pk[who]), dev(msg), msg_len=32)).copy()
    pubs = np.ascontiguousarray(pk[who])
    workload.corrupt_for_verify(sig, pubs, msg, seed=SEED5, config=2)
    keys, idx = km.as_keyset(pubs, pk)
    want = oracle.verify_batch(sig, pubs, msg, 32)
    assert 0 < want.sum() < N5 and not all(km.decodes(k.tobytes()) for k in keys)
    return keys, idx, sig, msg, want


def test_one_fuzz_pass_in_mode_1(engine, fuzz):
    keys, idx, sig, msg, want = fuzz
    with comb_set(engine, dev(keys)) as ks, settings(engine, offcurve=1):
        got = keyed(engine, "dev", ks, idx, sig, msg, mlen=32)
    assert np.array_equal(got, want), bad(got, want)


def test_create_comb_and_create_comb_dev_give_the_same_key_set(engine, oracle, honest):
    keys, idx, sig, msgs, off, mlen, want = mixed(engine, oracle, honest, 257, 257, 0)
    with comb_set(engine, keys) as k1, comb_set(engine, dev(keys)) as k2:
        assert k1.nbytes == k2.nbytes and k1.device == k2.device == 0
        assert np.array_equal(comb_of(engine, k1, 256), comb_of(engine, k2, 256))
        for ks in (k1, k2):
            got = keyed(engine, "dev", ks, idx, sig, msgs, off, mlen)
            assert np.array_equal(got, want), bad(got, want)
    with pytest.raises(ValueError):
        k1.comb


@pytest.mark.parametrize("mode", [0, 1])
def test_a_comb_set_and_a_plain_set_alternate_on_one_workspace(engine, oracle, honest, mode):
    """neither route may depend on what the other left in the tables, the flags or the point workspace; the comb set survives
    the engines like a plain one"""
    a = mixed(engine, oracle, honest, 1000, 257, 0)
    b = mixed(engine, oracle, honest, 1000, 2, 1)
    ca, pb, cb = comb_set(engine, dev(a[0])), engine.keyset_create(b[0]), comb_set(engine, b[0])
    try:
        with settings(engine, offcurve=mode):
            for ks, x in ((ca, a), (pb, b), (cb, b), (pb, b), (ca, a), (cb, b)):
                got = keyed(engine, "dev", ks, x[1], x[2], x[3], x[4], x[5])
                assert np.array_equal(got, x[6]), (ks.comb, bad(got, x[6]))
            engine.shutdown()
            engine.init(0)
            got = keyed(engine, "dev", ca, a[1], a[2], a[3], a[4], a[5])
            assert np.array_equal(got, a[6]), bad(got, a[6])
    finally:
        for ks in (ca, pb, cb):
            ks.close()


def test_the_host_form_across_a_chunk_boundary(engine, fuzz):
    """the host pipeline forced to chunks of 4096: every chunk uploads its own slice of the indices"""
    keys, idx, sig, msg, want = fuzz
    n = 2 * 4096 + 77
    assert all(0 < want[lo:min(lo + 4096, n)].sum() < min(4096, n - lo) for lo in range(0, n, 4096))
    lib = engine.library()
    with comb_set(engine, keys) as ks:
        try:
            lib.eddsa_amd_set_pipeline(ctypes.c_size_t(4096), ctypes.c_size_t(4096))
            got = keyed(engine, "host", ks, idx[:n], sig[:n], msg[:n], mlen=32)
        finally:
            lib.eddsa_amd_set_pipeline(ctypes.c_size_t(0), ctypes.c_size_t(0))
    assert np.array_equal(got, want[:n]), bad(got, want[:n])


# ---------------------------------------------------------------- 6: the keyed combination over a comb set

def test_keyed_rlc_over_a_comb_set(engine, oracle, honest):
    """n = 8192 + 1 with one corrupted item, every call combined: the group of the corrupted item is decided per item - by the
    comb route - and the statistics say so"""
    sk, pk = honest
    n = 8192 + 1
    msg = workload.field_bytes(93, 2, workload.F_MSG, n, 32)
    who = (np.arange(n, dtype=np.int64) * 101 + 3) % 257
    sig = host(engine.ed25519_sign_batch(dev(sk[who]), dev(pk[who]), dev(msg), msg_len=32)).copy()
    sig[4000, 7] ^= 16
    want = oracle.verify_batch(sig, np.ascontiguousarray(pk[who]), msg, 32)
    assert want.sum() == n - 1 and want[4000] == 0
    try:
        engine.set_rlc_min_items(0)
        with comb_set(engine, pk[:257]) as ks:
            ok, stats = engine.ed25519_verify_keyed_rlc(dev(sig), ks, dev_idx(who.astype(np.uint32)), dev(msg), msg_len=32, return_stats=True)
            assert np.array_equal(host(ok), want), bad(ok, want)
            assert tuple(int(s) for s in stats) == (1, 8192, 1, 1)                     # combined, per item, groups failed, groups passed
            ok, stats = engine.ed25519_verify_keyed_rlc(sig, ks, who.astype(np.uint32), msg, msg_len=32, return_stats=True)
            assert np.array_equal(ok, want) and tuple(int(s) for s in stats) == (1, 8192, 1, 1)
    finally:
        engine.set_rlc_min_items(engine.RLC_MIN_ITEMS_DEFAULT)
