"""GPU tests of signer sets (include/eddsa_amd.h: eddsa_amd_signer_*, ed25519_sign_keyed and its ctx / ph forms, host- and
device-pointer forms).  Seed sets are held, byte for byte, to the unkeyed calls over the gathered keys (ed25519_sign_batch,
ed25519ctx_sign_batch, ed25519ph_sign_batch - each of which has its own tests against the oracle and the models); expanded keys
to the model (tests/sign_keyed_model.py: hashlib, Python integers, the oracle's base-point multiplication)."""
import ctypes
import threading

import numpy as np
import pytest

import dom2_model as dm
import sign_keyed_model as sm
from gen_golden import golden_msg  # tools/ is on sys.path (conftest)
from gpu_kit import dev

pytestmark = pytest.mark.gpu
L = sm.L
INVALID_VALUE = -1                                  # -hipErrorInvalidValue
SET_SIZES = (1, 2, 1000, 1 << 16)
# the shape boundaries of the point kernel and the finish kernel (kernels.hip: point_shape_of, finish_shape_of): four lanes per
# item up to 2^14, blocks of 128 | 256 | 512 lanes up to 2^15 | 2^16 | beyond, K = 1 | 2 | 4 | 8 items per lane of the finish kernel,
# and one size past POINT_MAX_BLOCKS * POINT_BLOCK = 131 072 items: the persistent shape
SIZES = (1, 63, 64, 65, 255, 256, 257, 1 << 14, (1 << 14) + 1, (1 << 15) + 1, (1 << 16) + 1, 17229, 65536 + 2 * 256 + 77,
         131072 + 256 + 77, 262144 + 2 * 256 + 77, 131072 + 512 + 77)


def idx_dev(idx):
    return dev(np.asarray(idx, np.uint32).view(np.int32))


def ragged(rng, n, longest=300):
    lens = rng.integers(0, longest + 1, n)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return rng.integers(0, 256, int(off[-1]), dtype=np.uint8), off


@pytest.fixture(scope="module")
def keys(engine):
    """2^16 seeds with their public keys (ed25519_genpub_batch has its own tests against the oracle); read-only"""
    secs = np.random.default_rng(65536).integers(0, 256, (1 << 16, 32), dtype=np.uint8)
    pubs = engine.ed25519_genpub_batch(dev(secs)).cpu().numpy()
    secs.setflags(write=False); pubs.setflags(write=False)
    return secs, pubs


@pytest.fixture(scope="module")
def signers(engine, keys):
    """count -> the signer set over the first `count` seeds, created once"""
    made = {}

    def get(count):
        if count not in made:
            made[count] = engine.signer_create(secs=keys[0][:count])
        return made[count]
    yield get
    for s in made.values():
        s.close()


def indices(rng, n, count):
    idx = rng.integers(0, count, n, dtype=np.uint32)
    idx[0], idx[-1] = count - 1, 0                  # the ends of the set occur
    return idx


# ---------------------------------------------------------------- seed sets: byte parity with ed25519_sign_batch

@pytest.mark.parametrize("n", SIZES)
def test_parity_with_sign_batch_over_fixed_messages(engine, keys, signers, n):
    secs, pubs = keys
    rng = np.random.default_rng(n)
    count = SET_SIZES[SIZES.index(n) % len(SET_SIZES)]
    signer = signers(count)
    assert signer.count == count and signer.device == 0
    idx = indices(rng, n, count)
    msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    want = engine.ed25519_sign_batch(dev(secs[idx]), dev(pubs[idx]), dev(msgs)).cpu().numpy()
    got = engine.ed25519_sign_keyed(signer, idx_dev(idx), dev(msgs)).cpu().numpy()
    assert got.shape == (n, 64) and np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0][:8]
    got = engine.ed25519_sign_keyed(signer, idx, msgs)
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0][:8]


@pytest.mark.parametrize("count", SET_SIZES)
def test_every_set_size_at_one_call_size(engine, keys, signers, count):
    secs, pubs = keys
    n = 4099
    rng = np.random.default_rng(count)
    idx = indices(rng, n, count)                    # (a wide set: keys from all over it, in random order)
    msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    want = engine.ed25519_sign_batch(dev(secs[idx]), dev(pubs[idx]), dev(msgs)).cpu().numpy()
    assert np.array_equal(engine.ed25519_sign_keyed(signers(count), idx_dev(idx), dev(msgs)).cpu().numpy(), want)
    assert np.array_equal(engine.ed25519_sign_keyed(signers(count), idx, msgs), want)


# 257: below MSG_ORDER_MIN_N, the items in their own order; the other two: the hashing kernels walk the length permutation
@pytest.mark.parametrize("n", [257, (1 << 14) + 1, 65536 + 2 * 256 + 77])
def test_parity_over_ragged_messages(engine, keys, signers, n):
    secs, pubs = keys
    rng = np.random.default_rng(3 * n)
    idx = indices(rng, n, 1000)
    blob, off = ragged(rng, n)
    want = engine.ed25519_sign_batch(dev(secs[idx]), dev(pubs[idx]), dev(blob), msg_off=dev(off.astype(np.int64))).cpu().numpy()
    got = engine.ed25519_sign_keyed(signers(1000), idx_dev(idx), dev(blob), msg_off=dev(off.astype(np.int64))).cpu().numpy()
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0][:8]
    assert np.array_equal(engine.ed25519_sign_keyed(signers(1000), idx, blob, msg_off=off), want)


def test_the_golden_table_through_a_signer_set(engine, golden):
    """tests/golden/ed25519_table.bin: 1024 (seed, public key, signature) rows, entry i over a message of i bytes"""
    raw = np.frombuffer(golden("ed25519_table.bin"), np.uint8).reshape(1024, 128)
    sk, pk, sig = raw[:, :32].copy(), raw[:, 32:64].copy(), raw[:, 64:].copy()
    msgs = [golden_msg(i) for i in range(1024)]
    off = np.zeros(1025, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    blob = np.frombuffer(b"".join(msgs), np.uint8).copy()
    order = np.random.default_rng(1024).permutation(1024).astype(np.uint32)
    with engine.signer_create(secs=sk[order]) as signer:       # key k of the set is row order[k]
        assert np.array_equal(signer.pubs(), pk[order])
        idx = np.argsort(order).astype(np.uint32)              # item i signs with row i
        assert np.array_equal(engine.ed25519_sign_keyed(signer, idx, blob, msg_off=off), sig)
        got = engine.ed25519_sign_keyed(signer, idx_dev(idx), dev(blob), msg_off=dev(off.astype(np.int64))).cpu().numpy()
        assert np.array_equal(got, sig)


# ---------------------------------------------------------------- ctx / ph

@pytest.mark.parametrize("n", [1, 257, (1 << 14) + 1])
def test_ctx_and_ph_parity(engine, keys, signers, n):
    secs, pubs = keys
    rng = np.random.default_rng(5 * n)
    count = 1 if n == 1 else 1000
    signer = signers(count)
    idx = indices(rng, n, count)
    msgs, pre = rng.integers(0, 256, (n, 45), dtype=np.uint8), rng.integers(0, 256, (n, 64), dtype=np.uint8)
    for clen in (0, 3, 255):
        context = bytes(rng.integers(0, 256, clen, dtype=np.uint8))
        want = engine.ed25519ctx_sign_batch(dev(secs[idx]), dev(pubs[idx]), dev(msgs), context).cpu().numpy()
        assert np.array_equal(engine.ed25519ctx_sign_keyed(signer, idx_dev(idx), dev(msgs), context).cpu().numpy(), want), clen
        assert np.array_equal(engine.ed25519ctx_sign_keyed(signer, idx, msgs, context), want), clen
        want = engine.ed25519ph_sign_batch(dev(secs[idx]), dev(pubs[idx]), dev(pre), context).cpu().numpy()
        assert np.array_equal(engine.ed25519ph_sign_keyed(signer, idx_dev(idx), dev(pre), context).cpu().numpy(), want), clen
        assert np.array_equal(engine.ed25519ph_sign_keyed(signer, idx, pre, context), want), clen
    if n == 257:                                    # ragged messages under a context
        blob, off = ragged(rng, n)
        want = engine.ed25519ctx_sign_batch(dev(secs[idx]), dev(pubs[idx]), dev(blob), b"ragged", msg_off=dev(off.astype(np.int64))).cpu().numpy()
        assert np.array_equal(engine.ed25519ctx_sign_keyed(signer, idx, blob, b"ragged", msg_off=off), want)
        got = engine.ed25519ctx_sign_keyed(signer, idx_dev(idx), dev(blob), b"ragged", msg_off=dev(off.astype(np.int64))).cpu().numpy()
        assert np.array_equal(got, want)


def test_rfc8032_dom2_vectors_through_a_one_key_set(engine):
    zero = np.zeros(1, np.uint32)
    for v in dm.rfc_vectors():
        fn = engine.ed25519ph_sign_keyed if v["flag"] == dm.PH else engine.ed25519ctx_sign_keyed
        m = np.frombuffer(v["mprime"], np.uint8).copy()
        with engine.signer_create(secs=np.frombuffer(v["sk"], np.uint8)) as signer:
            assert signer.pubs().tobytes() == v["pk"]
            assert fn(signer, zero, m, v["context"]).tobytes() == v["sig"], v["name"]
            assert fn(signer, idx_dev(zero), dev(m), v["context"]).cpu().numpy().tobytes() == v["sig"], v["name"]


# ---------------------------------------------------------------- expanded keys

@pytest.fixture(scope="module")
def edge_set(engine, oracle):
    keys = sm.edge_keys(48, seed=48)
    signer = engine.signer_create(expanded=keys)
    yield keys, signer
    signer.close()


def test_expanded_keys_against_the_model(engine, oracle, edge_set):
    """300 items over the edge scalars 0, 1, l - 1, l, l + 1, 2^255 - 1, 2^255, 2^256 - 1 and random unclamped ones: exact bytes"""
    orc = oracle.lib
    keys, signer = edge_set
    pubs = signer.pubs()
    for k in range(48):
        assert pubs[k].tobytes() == sm.pub(orc, keys[k].tobytes()), k
    assert pubs[0].tobytes() == pubs[3].tobytes() == sm.NEUTRAL
    rng = np.random.default_rng(300)
    idx = (np.arange(300) % 48).astype(np.uint32)
    msgs, pre = rng.integers(0, 256, (300, 40), dtype=np.uint8), rng.integers(0, 256, (300, 64), dtype=np.uint8)
    runs = ((sm.PLAIN, b"", msgs, engine.ed25519_sign_keyed(signer, idx_dev(idx), dev(msgs)).cpu().numpy()),
            (sm.PLAIN, b"", msgs, engine.ed25519_sign_keyed(signer, idx, msgs)),
            (sm.CTX, b"expanded", msgs, engine.ed25519ctx_sign_keyed(signer, idx, msgs, b"expanded")),
            (sm.PH, b"", pre, engine.ed25519ph_sign_keyed(signer, idx_dev(idx), dev(pre), b"").cpu().numpy()))
    for flag, context, rows, got in runs:
        for i in range(300):
            k = int(idx[i])
            assert got[i].tobytes() == sm.sign(orc, keys[k].tobytes(), rows[i].tobytes(), flag, context, a_bytes=pubs[k].tobytes()), (flag, i)


def test_expanded_keys_in_a_large_pass(engine, edge_set):
    """2^14 + 1 items: S == (r + t a) mod l in integers for every item, and ed25519_verify_batch accepts every signature under
    signer.pubs() (which pins R = r B)"""
    keys, signer = edge_set
    pubs = signer.pubs()
    n = (1 << 14) + 1
    rng = np.random.default_rng(n)
    idx = rng.integers(0, 48, n, dtype=np.uint32)
    idx[:48] = np.arange(48, dtype=np.uint32)
    msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sig = engine.ed25519_sign_keyed(signer, idx_dev(idx), dev(msgs)).cpu().numpy()
    bad = [i for i in range(n)
           if not sm.response_ok(sig[i].tobytes(), keys[idx[i]].tobytes(), pubs[idx[i]].tobytes(), msgs[i].tobytes())]
    assert not bad, bad[:8]
    ok = engine.ed25519_verify_batch(dev(sig), dev(pubs[idx]), dev(msgs)).cpu().numpy()
    assert ok.all(), np.nonzero(ok == 0)[0][:8]


def test_a_set_from_seeds_and_a_set_from_their_expansions_agree(engine, keys, signers):
    secs, pubs = keys
    exp = np.frombuffer(b"".join(sm.expand(secs[k].tobytes()) for k in range(1000)), np.uint8).reshape(1000, 64)
    rng = np.random.default_rng(77)
    idx = indices(rng, 3000, 1000)
    msgs = rng.integers(0, 256, (3000, 32), dtype=np.uint8)
    with engine.signer_create(expanded=exp) as other:
        assert np.array_equal(other.pubs(), signers(1000).pubs())
        assert np.array_equal(engine.ed25519_sign_keyed(other, idx, msgs), engine.ed25519_sign_keyed(signers(1000), idx, msgs))
        assert np.array_equal(engine.ed25519ph_sign_keyed(other, idx_dev(idx[:64]), dev(np.tile(msgs[:64], 2)), b"c").cpu().numpy(),
                              engine.ed25519ph_sign_keyed(signers(1000), idx_dev(idx[:64]), dev(np.tile(msgs[:64], 2)), b"c").cpu().numpy())


# ---------------------------------------------------------------- pubs, round trip

@pytest.mark.parametrize("count", SET_SIZES)
def test_pubs_equal_genpub(keys, signers, count):
    assert np.array_equal(signers(count).pubs(), keys[1][:count])


def test_round_trip_through_a_key_set(engine, signers):
    signer = signers(1000)
    n = 5000
    rng = np.random.default_rng(n)
    idx = indices(rng, n, 1000)
    msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sig = engine.ed25519_sign_keyed(signer, idx, msgs)
    with engine.keyset_create(signer.pubs()) as ks:
        assert engine.ed25519_verify_keyed(sig, ks, idx, msgs).all()
        msgs[1234, 7] ^= 0x20
        want = np.ones(n, np.uint8); want[1234] = 0
        assert np.array_equal(engine.ed25519_verify_keyed(sig, ks, idx, msgs), want)
        assert np.array_equal(engine.ed25519_verify_keyed(dev(sig), ks, idx_dev(idx), dev(msgs)).cpu().numpy(), want)


# ---------------------------------------------------------------- indices

@pytest.mark.parametrize("n", [257, (1 << 14) + 1])
def test_indices_outside_the_set(engine, signers, n):
    import torch
    count = 1000
    signer = signers(count)
    rng = np.random.default_rng(11 * n)
    idx = indices(rng, n, count)
    msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pre = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    valid = engine.ed25519_sign_keyed(signer, idx_dev(idx), dev(msgs)).cpu().numpy()
    valid_ph = engine.ed25519ph_sign_keyed(signer, idx_dev(idx), dev(pre), b"idx").cpu().numpy()
    assert valid.any(axis=1).all()
    lib = engine.library()
    for bad_value in (count, count + 1, 0xFFFFFFFF):
        for at in (0, n // 2, n - 1):
            bad = idx.copy()
            bad[at] = bad_value
            want = valid.copy(); want[at] = 0
            got = engine.ed25519_sign_keyed(signer, idx_dev(bad), dev(msgs)).cpu().numpy()
            assert np.array_equal(got, want), (bad_value, at)
            if at == n // 2:
                want_ph = valid_ph.copy(); want_ph[at] = 0
                assert np.array_equal(engine.ed25519ph_sign_keyed(signer, idx_dev(bad), dev(pre), b"idx").cpu().numpy(), want_ph)
            # the host form refuses the call and writes nothing
            out = np.full((n, 64), 0xAA, np.uint8)
            rc = lib.ed25519_sign_keyed(out.ctypes.data_as(ctypes.c_void_p), signer._handle(), bad.ctypes.data_as(ctypes.c_void_p),
                                        msgs.ctypes.data_as(ctypes.c_void_p), None, ctypes.c_size_t(32), ctypes.c_size_t(n))
            assert rc == INVALID_VALUE and (out == 0xAA).all(), (bad_value, at)
    with pytest.raises(engine.EddsaAmdError):
        engine.ed25519ctx_sign_keyed(signer, np.full(3, count, np.uint32), msgs[:3], b"")
    torch.cuda.synchronize()


# ---------------------------------------------------------------- secrets, lifetime

def test_secrets_do_not_outlive_the_keyed_sign_calls(engine, keys):
    import torch
    secs, pubs = keys
    n = 20000
    rng = np.random.default_rng(n)
    idx = indices(rng, n, 1000)
    msgs, pre = rng.integers(0, 256, (n, 40), dtype=np.uint8), rng.integers(0, 256, (n, 64), dtype=np.uint8)
    want = engine.ed25519_sign_batch(dev(secs[idx]), dev(pubs[idx]), dev(msgs)).cpu().numpy()
    try:
        first = engine.signer_create(secs=secs[:1000])
        engine.shutdown()                           # fresh workspaces and staging buffers; the set survives
        assert np.array_equal(engine.ed25519_sign_keyed(first, idx, msgs), want)
        engine.ed25519ctx_sign_keyed(first, idx, msgs, b"secrets")
        engine.ed25519ph_sign_keyed(first, idx[:1], pre[:1], b"secrets")
        assert engine.secret_residue() == (0, 0, 0, 0)
        engine.shutdown()
        assert np.array_equal(engine.ed25519_sign_keyed(first, idx_dev(idx), dev(msgs)).cpu().numpy(), want)
        engine.ed25519ph_sign_keyed(first, idx_dev(idx), dev(pre), b"secrets")
        engine.ed25519ctx_sign_keyed(first, idx_dev(idx[:1]), dev(msgs[:1]), b"secrets")
        torch.cuda.synchronize()
        assert engine.secret_residue() == (0, 0, 0, 0)
        first.close()
        with pytest.raises(ValueError):
            first.count
        with engine.signer_create(secs=secs[:1000]) as second:     # a second set after the first was destroyed
            assert np.array_equal(engine.ed25519_sign_keyed(second, idx, msgs), want)
    finally:
        engine.init(0)


def test_a_host_pointer_where_a_device_pointer_belongs_is_refused(engine, signers):
    """what is left of the argument checks once a device exists: `sigs` that is no device memory"""
    out = np.zeros((4, 64), np.uint8)
    idx, msgs = idx_dev(np.zeros(4, np.uint32)), dev(np.zeros((4, 32), np.uint8))
    rc = engine.library().ed25519_sign_keyed_dev(out.ctypes.data_as(ctypes.c_void_p), signers(1)._handle(), ctypes.c_void_p(idx.data_ptr()),
                                                 ctypes.c_void_p(msgs.data_ptr()), None, ctypes.c_size_t(32), ctypes.c_size_t(4), None)
    assert rc != 0 and not out.any()


# ---------------------------------------------------------------- sharing

def test_a_keyed_and_an_unkeyed_call_on_two_streams(engine, keys, signers):
    import torch
    secs, pubs = keys
    n = 30000
    rng = np.random.default_rng(n)
    signer = signers(1000)
    idx = indices(rng, n, 1000)
    msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d_idx, d_msgs, d_sk, d_pk = idx_dev(idx), dev(msgs), dev(secs[idx]), dev(pubs[idx])
    want = engine.ed25519_sign_batch(d_sk, d_pk, d_msgs).cpu().numpy()
    torch.cuda.synchronize()
    results, errors = {}, []

    def worker(name, fn):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                outs = [fn() for _ in range(4)]
            st.synchronize()
            results[name] = [o.cpu().numpy() for o in outs]
        except Exception as e:                      # noqa: BLE001
            errors.append((name, e))
    threads = [threading.Thread(target=worker, args=("keyed", lambda: engine.ed25519_sign_keyed(signer, d_idx, d_msgs))),
               threading.Thread(target=worker, args=("unkeyed", lambda: engine.ed25519_sign_batch(d_sk, d_pk, d_msgs)))]
    for t in threads: t.start()
    for t in threads: t.join()
    assert not errors, errors
    for name in ("keyed", "unkeyed"):
        assert len(results[name]) == 4 and all(np.array_equal(r, want) for r in results[name]), name
