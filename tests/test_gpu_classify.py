"""GPU tests of point classification (include/eddsa_amd.h: ed25519_point_classify_batch[_dev], eddsa_amd_keyset_classify;
classify_kernels.h): the class byte of every string is the model's (tests/classify_model.py: decode_reference, decode_strict, [8]P
and [l]P in Python integers), never the engine's own answer by another route.  Every test puts the settings back."""
import ctypes
import threading

import numpy as np
import pytest

import classify_model as cm
import policy_model as pm
from gpu_kit import bad, dev, dev_idx, host, settings

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
BIG = (1 << 20) + 257


@pytest.fixture(scope="module")
def vec():
    return cm.vectors()


@pytest.fixture(scope="module")
def big(vec):
    """2^20 + 257 items: the vectors tiled by a fixed permutation, so that the expectation is a lookup"""
    names, strings, classes = vec
    idx = (np.arange(BIG, dtype=np.int64) * 389 + 17) % len(names)
    s, c = strings[idx], classes[idx]
    s.setflags(write=False)
    c.setflags(write=False)
    return s, c


def windows(count, n):
    """index windows of n items that together visit every vector, each window rotated to its own start"""
    return [(start + np.arange(n)) % count for start in range(0, count, n)]


# ---------------------------------------------------------------- 1: the device form at small sizes

@pytest.mark.parametrize("n", SIZES)
def test_the_device_form_equals_the_model(engine, vec, n):
    """every size at which a wave or a block ends; over the windows of one size every vector is classified, at changing lanes"""
    names, strings, classes = vec
    shifts = (0,) if n < 255 else (0, 1, 37)
    for shift in shifts:
        for idx in windows(len(names), n):
            idx = (idx + shift) % len(names)
            got = engine.point_classify_batch(dev(strings[idx]))
            assert tuple(got.shape) == (n,)
            got = host(got)
            assert got.dtype == np.uint8
            assert np.array_equal(got, classes[idx]), (n, shift, cm.mismatches(got, classes[idx], [names[i] for i in idx]))


def test_points_and_classes_offset_by_one_byte(engine, vec):
    import torch
    names, strings, classes = vec
    n = len(names)
    lib = engine.library()
    points = torch.empty(32 * n + 1, dtype=torch.uint8, device="cuda")
    points[1:] = torch.from_numpy(strings.reshape(-1).copy()).cuda()
    cls = torch.full((n + 2,), 0xEE, dtype=torch.uint8, device="cuda")
    assert (points.data_ptr() + 1) % 2 == 1 and (cls.data_ptr() + 1) % 2 == 1
    rc = lib.ed25519_point_classify_batch_dev(ctypes.c_void_p(cls.data_ptr() + 1), ctypes.c_void_p(points.data_ptr() + 1), ctypes.c_size_t(n),
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    out = cls.cpu().numpy()
    assert out[0] == 0xEE and out[-1] == 0xEE                                   # the neighbours of the class bytes stand
    assert np.array_equal(out[1:-1], classes), cm.mismatches(out[1:-1], classes, names)


# ---------------------------------------------------------------- 2: one large call, both forms, ordinary and page-locked memory

def test_one_call_of_2_20_plus_257_items_in_both_forms(engine, big):
    strings, classes = big
    got = host(engine.point_classify_batch(dev(strings)))
    assert got.shape == (BIG,) and np.array_equal(got, classes), bad(got, classes)
    ordinary = engine.point_classify_batch(strings)
    assert ordinary.dtype == np.uint8 and ordinary.shape == (BIG,)
    assert np.array_equal(ordinary, classes), bad(ordinary, classes)
    pinned = engine.host_array(strings.shape)
    try:
        pinned[...] = strings
        locked = engine.point_classify_batch(pinned)
        assert locked.tobytes() == ordinary.tobytes()
    finally:
        engine.host_free(pinned)
    assert engine.point_classify_batch(b"").shape == (0,)


# ---------------------------------------------------------------- 3: key sets

def golden_items(golden, names):
    """the cases of the two golden files as keyed items over the vectors: (idx, sig, msgs, off, the reference's verdicts)"""
    cases = golden("verify_edges.json") + golden("verify_torsion.json")
    strings = cm.vectors()[1]
    at = {strings[i].tobytes(): i for i in range(len(names) - 1, -1, -1)}       # (the first vector with those bytes)
    idx = np.array([at[pm.H(c["pub"])] for c in cases], np.uint32)
    sig = pm.arr([pm.H(c["sig"]) for c in cases])
    lens = np.array([len(c["msg"]) // 2 for c in cases])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    msgs = np.frombuffer(b"".join(pm.H(c["msg"]) for c in cases), np.uint8)
    return idx, sig, msgs, off, np.array([c["accept"] for c in cases], np.uint8)


@pytest.mark.parametrize("comb", [False, True])
def test_a_key_set_classifies_its_own_keys(engine, golden, vec, comb):
    """plain and comb sets of ALL the vectors, the strings off the curve included: the set's answer is the batch call's on the same
    bytes and the model's, also after eddsa_amd_shutdown; the keyed verdicts over the set are the same before and after"""
    names, strings, classes = vec
    idx, sig, msgs, off, accept = golden_items(golden, names)
    batch = engine.point_classify_batch(strings)
    assert np.array_equal(batch, classes), cm.mismatches(batch, classes, names)
    ks = engine.keyset_create(strings, comb=comb)
    try:
        assert ks.comb == comb and ks.count == len(names)
        nbytes = ks.nbytes
        verdicts = lambda: host(engine.ed25519_verify_keyed(dev(sig), ks, dev_idx(idx), dev(msgs), msg_off=dev(off.astype(np.int64))))   # noqa: E731
        before = verdicts()
        assert np.array_equal(before, accept), bad(before, accept)
        got = ks.classify()
        assert got.dtype == np.uint8 and got.shape == (len(names),)
        assert got.tobytes() == batch.tobytes(), cm.mismatches(got, batch, names)
        assert ks.nbytes == nbytes and ks.count == len(names)
        after = verdicts()
        assert np.array_equal(after, before), bad(after, before)
        engine.shutdown()                                                         # a key set survives the engines; no table is needed
        try:
            again = ks.classify()
        finally:
            engine.init(0)
        assert again.tobytes() == batch.tobytes(), cm.mismatches(again, batch, names)
        assert np.array_equal(verdicts(), before)
    finally:
        ks.close()
    with pytest.raises(ValueError):
        ks.classify()


# ---------------------------------------------------------------- 4: the process-wide switches play no part

@pytest.mark.parametrize("offcurve", [0, 1, 2])
def test_the_classes_are_unchanged_under_the_verify_settings(engine, vec, offcurve):
    names, strings, classes = vec
    with settings(engine, offcurve=offcurve, policy=engine.VERIFY_STRICT, cofactored=True):
        got = host(engine.point_classify_batch(dev(strings)))
        assert np.array_equal(got, classes), cm.mismatches(got, classes, names)
        got = engine.point_classify_batch(strings)
        assert np.array_equal(got, classes), cm.mismatches(got, classes, names)
    got = host(engine.point_classify_batch(dev(strings)))
    assert np.array_equal(got, classes), cm.mismatches(got, classes, names)


# ---------------------------------------------------------------- 5: beside a verify pass on another stream

def test_a_call_on_a_second_stream_beside_a_verify_pass(engine, golden, vec):
    import torch
    names, strings, classes = vec
    cases = golden("verify_edges.json") + golden("verify_torsion.json")
    reps = 40
    sig = np.tile(pm.arr([pm.H(c["sig"]) for c in cases]), (reps, 1))
    pub = np.tile(pm.arr([pm.H(c["pub"]) for c in cases]), (reps, 1))
    lens = np.tile(np.array([len(c["msg"]) // 2 for c in cases]), reps)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    msgs = np.tile(np.frombuffer(b"".join(pm.H(c["msg"]) for c in cases), np.uint8), reps)
    accept = np.tile(np.array([c["accept"] for c in cases], np.uint8), reps)
    tiled = np.tile(strings, (30, 1))
    want = np.tile(classes, 30)
    d_sig, d_pub, d_msgs, d_off, d_points = dev(sig), dev(pub), dev(msgs), dev(off), dev(tiled)
    torch.cuda.synchronize()
    results, errors = {}, []

    def worker(name, fn):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                outs = [fn() for _ in range(3)]
            st.synchronize()
            results[name] = [o.cpu().numpy() for o in outs]
        except Exception as e:                      # noqa: BLE001
            errors.append((name, e))
    threads = [threading.Thread(target=worker, args=("verify", lambda: engine.ed25519_verify_batch(d_sig, d_pub, d_msgs, msg_off=d_off))),
               threading.Thread(target=worker, args=("classify", lambda: engine.point_classify_batch(d_points)))]
    for t in threads: t.start()
    for t in threads: t.join()
    assert not errors, errors
    assert len(results["verify"]) == 3 and all(np.array_equal(r, accept) for r in results["verify"])
    assert len(results["classify"]) == 3 and all(np.array_equal(r, want) for r in results["classify"])
