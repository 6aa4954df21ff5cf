"""GPU tests of [m]P + [a]B (include/eddsa_amd.h: ed25519_point_muladd_batch[_dev]; muladd_kernels.h around k_verify_main): every
output is the model's (tests/point_muladd_model.py: decode_reference, pmul, padd and encode in Python integers, nothing reduced),
and, independently of the model, what ed25519_genpub_batch and the signer sets derive.  Every comparison is byte-exact.  Every test
puts the settings back."""
import ctypes
import subprocess
import threading

import numpy as np
import pytest

import ed_model as em
import point_muladd_model as mm
import policy_model as pm
from gpu_kit import bad, dev, dev_idx, host, settings
from hostlib import build_c_program

pytestmark = pytest.mark.gpu
BLOCK, FINISH_K = 256, 8                             # kernels.hip: a block is a tile of 256 items; eight tiles share an inversion
SIZES = (1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, FINISH_K * BLOCK - 1, FINISH_K * BLOCK, FINISH_K * BLOCK + 1, 4 * BLOCK + 1)
BIG = (1 << 20) + 257
COMBOS = [(True, True), (True, False), (False, True), (False, False)]


@pytest.fixture(scope="module")
def vec():
    return mm.vectors()


@pytest.fixture(scope="module")
def want(vec):
    """the model's bytes for the four ways to call, computed once: want[with_mul, with_add] (n, 32), read-only"""
    names, points, mul, add, out = vec
    table = {(True, True): out}
    for with_mul, with_add in COMBOS[1:]:
        table[with_mul, with_add] = mm.expected(points, mul if with_mul else None, add if with_add else None)
        table[with_mul, with_add].setflags(write=False)
    return table


def opt(a, given, to=dev):
    return to(a) if given else None


def tiled(count, n, shift=0):
    """n indices into the vectors by a fixed permutation: every vector comes up, at changing lanes"""
    return ((np.arange(n, dtype=np.int64) + shift) * 389 + 17) % count


# ---------------------------------------------------------------- 1: every vector against the model

@pytest.mark.parametrize("with_mul, with_add", COMBOS)
def test_every_vector_in_both_forms(engine, vec, want, with_mul, with_add):
    names, points, mul, add, _ = vec
    w = want[with_mul, with_add]
    got = engine.point_muladd_batch(dev(points), opt(mul, with_mul), opt(add, with_add))
    assert tuple(got.shape) == (len(names), 32)
    got = host(got)
    assert got.dtype == np.uint8 and np.array_equal(got, w), mm.mismatches(got, w, names)
    same = lambda a: np.array(a)                     # noqa: E731  (a writable copy: the fixtures are read-only)
    got = engine.point_muladd_batch(same(points), opt(mul, with_mul, same), opt(add, with_add, same))
    assert got.dtype == np.uint8 and np.array_equal(got, w), mm.mismatches(got, w, names)
    assert engine.point_muladd_batch(b"").shape == (0, 32)


@pytest.mark.parametrize("n", SIZES)
def test_the_shape_boundaries(engine, vec, want, n):
    """every size at which a wave, a block or a finish block ends; over the shifts every vector is computed at changing lanes"""
    names, points, mul, add, out = vec
    for shift in (0, 101) if n < BLOCK - 1 else (0,):
        idx = tiled(len(names), n, shift)
        got = host(engine.point_muladd_batch(dev(points[idx]), dev(mul[idx]), dev(add[idx])))
        assert got.shape == (n, 32) and np.array_equal(got, out[idx]), (n, mm.mismatches(got, out[idx], [names[i] for i in idx]))
    idx = tiled(len(names), n, 7)
    got = host(engine.point_muladd_batch(dev(points[idx]), None, dev(add[idx])))
    assert np.array_equal(got, want[False, True][idx]), (n, mm.mismatches(got, want[False, True][idx], [names[i] for i in idx]))


@pytest.mark.parametrize("n, k", [(4 * BLOCK + 1, 1), ((1 << 16) + BLOCK + 1, 2), ((1 << 17) + 2 * BLOCK + 1, 4), ((1 << 18) + FINISH_K * BLOCK + 1, 8)])
def test_strings_off_the_curve_at_every_position_of_a_shared_inversion(engine, vec, n, k):
    """a finish lane inverts the product of the Z of `k` items, BLOCK apart (kernels.hip: finish_shape_of); a string that is no
    curve point puts 1 in its place.  Such strings at every position of a group among valid items, a group of nothing else, a group
    with one valid item, in the first, a middle and the last (partial) finish block: they get the no-point string and their
    neighbours their own bytes"""
    names, points, mul, add, out = vec
    count = len(names)
    on = np.array([i for i in range(count) if out[i].tobytes() != mm.NO_POINT])
    idx = on[tiled(len(on), n)]
    p, m, a, w = points[idx], mul[idx], add[idx], out[idx].copy()
    off_strings = points[[i for i in range(count) if out[i].tobytes() == mm.NO_POINT]]
    group = k * BLOCK
    spots = []
    for g0 in sorted({0, (n // group // 2) * group, (n - 1) // group * group}):
        for pos in range(k):
            spots.append(g0 + pos * BLOCK + 3 + 9 * pos)                     # one per position, each in a lane of its own
        spots += [g0 + pos * BLOCK + 70 for pos in range(k)]                  # lane 70: the whole group
        spots += [g0 + pos * BLOCK + 200 for pos in range(k) if pos != k // 2]   # lane 200: all but one
    spots = np.array(sorted({s for s in spots if s < n}))
    assert len(spots) > 2 * k
    p[spots] = off_strings[np.arange(len(spots)) % len(off_strings)]
    w[spots] = np.frombuffer(mm.NO_POINT, np.uint8)
    got = host(engine.point_muladd_batch(dev(p), dev(m), dev(a)))
    assert np.array_equal(got, w), (n, k, mm.mismatches(got, w))
    got = host(engine.point_muladd_batch(dev(p), dev(m), None))
    keep = np.ones(n, bool); keep[spots] = False
    assert (got[spots] == w[spots]).all() and not (got[keep] == w[spots][0]).all(axis=1).any()


# ---------------------------------------------------------------- 2: buffers

def test_buffers_offset_by_one_byte(engine, vec):
    import torch
    names, points, mul, add, out = vec
    n = len(names)
    lib = engine.library()
    bufs = []
    for a in (points, mul, add):
        t = torch.empty(32 * n + 1, dtype=torch.uint8, device="cuda")
        t[1:] = torch.from_numpy(a.reshape(-1).copy()).cuda()
        bufs.append(t)
    res = torch.full((32 * n + 2,), 0xEE, dtype=torch.uint8, device="cuda")
    assert all((t.data_ptr() + 1) % 2 == 1 for t in bufs + [res])
    rc = lib.ed25519_point_muladd_batch_dev(ctypes.c_void_p(res.data_ptr() + 1), *[ctypes.c_void_p(t.data_ptr() + 1) for t in bufs],
                                            ctypes.c_size_t(n), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    got = res.cpu().numpy()
    assert got[0] == 0xEE and got[-1] == 0xEE        # the neighbours of the output stand
    assert np.array_equal(got[1:-1].reshape(n, 32), out), mm.mismatches(got[1:-1], out, names)


@pytest.mark.parametrize("n", [300, (3 << 16) + 300])
def test_out_may_be_points(engine, vec, n):
    """in-place derivation, device and host form (the larger size: two chunks of the staging pipeline, whose first holds 2^17 items)"""
    names, points, mul, add, out = vec
    idx = tiled(len(names), n)
    d = dev(points[idx])
    back = engine.point_muladd_batch(d, dev(mul[idx]), dev(add[idx]), out=d)
    assert back.data_ptr() == d.data_ptr()
    assert np.array_equal(host(d), out[idx]), mm.mismatches(host(d), out[idx])
    h = np.array(points[idx])
    back = engine.point_muladd_batch(h, np.array(mul[idx]), np.array(add[idx]), out=h)
    assert np.shares_memory(back, h) and np.array_equal(h, out[idx]), mm.mismatches(h, out[idx])


# ---------------------------------------------------------------- 3: above CHUNK_MAX

def test_one_call_of_2_20_plus_257_items_in_both_forms(engine, vec):
    """two passes through the workspace; the vectors tiled, the model run on the distinct items only"""
    names, points, mul, add, out = vec
    idx = tiled(len(names), BIG)
    p, m, a, w = points[idx], mul[idx], add[idx], out[idx]
    got = host(engine.point_muladd_batch(dev(p), dev(m), dev(a)))
    assert got.shape == (BIG, 32) and np.array_equal(got, w), mm.mismatches(got, w)
    got = engine.point_muladd_batch(p, m, a)
    assert got.shape == (BIG, 32) and np.array_equal(got, w), mm.mismatches(got, w)


# ---------------------------------------------------------------- 4: independent of the model

@pytest.fixture(scope="module")
def seeds():
    s = np.random.default_rng(1024).integers(0, 256, (1024, 32), dtype=np.uint8)
    s.setflags(write=False)
    return s


def test_the_base_point_term_is_genpub(engine, seeds):
    """[0]P + [a]B and P = the neutral element with m absent, a = the clamped scalars of 1024 seeds: ed25519_genpub_batch of the seeds"""
    pubs = host(engine.ed25519_genpub_batch(dev(seeds)))
    a = em.arr([em.le(em.clamped(s.tobytes())) for s in seeds], 32)
    got = host(engine.point_muladd_batch(dev(pubs[::-1]), dev(np.zeros((1024, 32), np.uint8)), dev(a)))
    assert np.array_equal(got, pubs), mm.mismatches(got, pubs)
    neutral = np.tile(np.frombuffer(mm.NEUTRAL, np.uint8), (1024, 1))
    got = host(engine.point_muladd_batch(dev(neutral), None, dev(a)))
    assert np.array_equal(got, pubs)
    assert np.array_equal(engine.point_muladd_batch(neutral, None, a), pubs)


def test_derived_keys_end_to_end(engine, seeds):
    """the use case: parent keys from seeds, A + [z]B and [h]A on the device against the signer sets over (a + z mod l, prefix) and
    (h a mod l, prefix); the device output registered as a key set without a trip to the host; every signature of the derived
    secret keys verifies under the derived public keys; an entry that is the no-point string rejects its items"""
    n_keys, n = 512, 4096
    rng = np.random.default_rng(512)
    parents = engine.ed25519_genpub_batch(dev(seeds[:n_keys]))
    z = rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
    h = rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
    digests = [em.sha(s.tobytes()) for s in seeds[:n_keys]]
    a = [em.clamped(s.tobytes()) for s in seeds[:n_keys]]
    soft_keys = em.arr([em.le((a[k] + em.num(z[k].tobytes())) % em.L) + digests[k][32:] for k in range(n_keys)], 64)
    blind_keys = em.arr([em.le(a[k] * em.num(h[k].tobytes()) % em.L) + digests[k][32:] for k in range(n_keys)], 64)
    idx = rng.integers(0, n_keys, n).astype(np.uint32)
    msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for keys, mul, add in ((soft_keys, None, dev(z)), (blind_keys, dev(h), None)):
        derived = engine.point_muladd_batch(parents, mul, add)               # stays on the device
        with engine.signer_create(expanded=keys) as signer:
            assert np.array_equal(host(derived), signer.pubs())
            sig = engine.ed25519_sign_keyed(signer, dev_idx(idx), dev(msgs))
        with engine.keyset_create(derived) as ks:
            assert ks.count == n_keys
            assert host(engine.ed25519_verify_keyed(sig, ks, dev_idx(idx), dev(msgs))).all()
        # one parent that is no curve point: its derived key is the no-point string, and the set rejects that entry's items
        broken = parents.clone()
        broken[7] = dev(np.frombuffer(em.le(2 | 1 << 255), np.uint8))          # y = 2 under the other sign bit: on no curve point
        derived = engine.point_muladd_batch(broken, mul, add)
        assert host(derived)[7].tobytes() == engine.NO_POINT
        expect = (idx != 7).astype(np.uint8)
        assert 0 < expect.sum() < n
        with engine.keyset_create(derived) as ks:
            for how in (dict(offcurve=0), dict(cofactored=True), dict(offcurve=0, cofactored=True)):
                with settings(engine, **how):
                    got = host(engine.ed25519_verify_keyed(sig, ks, dev_idx(idx), dev(msgs)))
                assert np.array_equal(got, expect), (how, bad(got, expect))


# ---------------------------------------------------------------- 5: the process-wide switches play no part

@pytest.mark.parametrize("offcurve", [0, 1, 2])
def test_the_outputs_are_unchanged_under_the_verify_settings(engine, vec, offcurve):
    names, points, mul, add, out = vec
    with settings(engine, offcurve=offcurve, policy=engine.VERIFY_STRICT, cofactored=True):
        got = host(engine.point_muladd_batch(dev(points), dev(mul), dev(add)))
        assert np.array_equal(got, out), mm.mismatches(got, out, names)
        got = engine.point_muladd_batch(np.array(points), np.array(mul), np.array(add))
        assert np.array_equal(got, out), mm.mismatches(got, out, names)
    got = host(engine.point_muladd_batch(dev(points), dev(mul), dev(add)))
    assert np.array_equal(got, out), mm.mismatches(got, out, names)


# ---------------------------------------------------------------- 6: one workspace pool, three kinds of pass

def test_verify_muladd_and_keyed_passes_share_the_workspaces(engine, golden, vec):
    """a verify pass, a muladd pass and a keyed pass alternating on one stream, then each kind on a stream of its own: every result
    is the one the call gives alone"""
    import torch
    names, points, mul, add, out = vec
    cases = golden("verify_edges.json") + golden("verify_torsion.json")
    reps = 40
    sig = np.tile(pm.arr([pm.H(c["sig"]) for c in cases]), (reps, 1))
    pub = np.tile(pm.arr([pm.H(c["pub"]) for c in cases]), (reps, 1))
    lens = np.tile(np.array([len(c["msg"]) // 2 for c in cases]), reps)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    msgs = np.tile(np.frombuffer(b"".join(pm.H(c["msg"]) for c in cases), np.uint8), reps)
    idx = tiled(len(names), 30 * len(names))
    d_sig, d_pub, d_msgs, d_off = dev(sig), dev(pub), dev(msgs), dev(off)
    d_p, d_m, d_a = dev(points[idx]), dev(mul[idx]), dev(add[idx])
    keys = np.unique(pub, axis=0)
    at = {k.tobytes(): i for i, k in enumerate(keys)}
    d_idx = dev_idx(np.array([at[p.tobytes()] for p in pub], np.uint32))
    with engine.keyset_create(keys) as ks:
        calls = {"verify": lambda: engine.ed25519_verify_batch(d_sig, d_pub, d_msgs, msg_off=d_off),
                 "muladd": lambda: engine.point_muladd_batch(d_p, d_m, d_a),
                 "keyed": lambda: engine.ed25519_verify_keyed(d_sig, ks, d_idx, d_msgs, msg_off=d_off)}
        solo = {}
        for name, fn in calls.items():
            solo[name] = host(fn())
            torch.cuda.synchronize()
        assert np.array_equal(solo["muladd"], out[idx]) and np.array_equal(solo["verify"], solo["keyed"])
        assert np.array_equal(solo["verify"], np.tile(np.array([c["accept"] for c in cases], np.uint8), reps))
        outs = [(name, fn()) for _ in range(3) for name, fn in calls.items()]          # one stream, alternating
        torch.cuda.synchronize()
        for name, o in outs:
            assert np.array_equal(host(o), solo[name]), name
        results, errors = {}, []

        def worker(name, fn):
            try:
                st = torch.cuda.Stream()
                with torch.cuda.stream(st):
                    mine = [fn() for _ in range(3)]
                st.synchronize()
                results[name] = [o.cpu().numpy() for o in mine]
            except Exception as e:                  # noqa: BLE001
                errors.append((name, e))
        for group in (("verify", "muladd"), ("muladd", "keyed")):
            threads = [threading.Thread(target=worker, args=(name, calls[name])) for name in group]
            for t in threads: t.start()
            for t in threads: t.join()
            assert not errors, errors
            for name in group:
                assert len(results[name]) == 3 and all(np.array_equal(r, solo[name]) for r in results[name]), (group, name)


# ---------------------------------------------------------------- 7: the shipped library from plain C

def test_a_c_program_against_the_shipped_library(engine, vec, want, tmp_path):
    """tests/c/point_muladd.c: plain C against eddsa_amd.h, linked against libeddsa_amd.so - the four ways to call, an odd output
    address, in place"""
    names, points, mul, add, out = vec
    exe = build_c_program(tmp_path, "point_muladd.c", libs=("eddsa_amd",), wall=True)
    files = []
    for name, a in (("points", points), ("mul", mul), ("add", add), ("want", out), ("want_mul", want[True, False]),
                    ("want_add", want[False, True]), ("want_points", want[False, False])):
        files.append(str(tmp_path / (name + ".bin")))
        np.ascontiguousarray(a).tofile(files[-1])
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "point_muladd: ok (%d items)" % len(names) in r.stdout
