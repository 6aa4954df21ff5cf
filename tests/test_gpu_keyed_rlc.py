"""GPU tests of the batch verification over a key set (include/eddsa_amd.h: ed25519_verify_keyed_rlc[_dev]; rlc_keyed.h): ok[i] is
what ed25519_verify_batch_rlc returns for (sigs[i], keys[key_idx[i]], message i), an index outside the key set rejects its item
and nothing else.  Expected verdicts are the oracle's on (sig, keys[idx], msg) - under a policy or the cofactored equation those
of tests/policy_model.py and tests/cofactored_model.py; the digit rows, window points and group verdicts of a pass are held
against the integer model of tests/test_gpu_rlc_stages.py with the key terms collected per key.  Every test puts the settings
back."""
import ctypes
import subprocess

import numpy as np
import pytest

import cofactored_model as cm
import keyed_model as km
import policy_model as pm
import test_gpu_rlc_stages as st
from gpu_kit import always_combine, bad, dev, dev_idx, host, settings  # noqa: F401  (always_combine: a fixture)
from hostlib import build_c_program

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("always_combine")]
G = st.G
L = st.L
NMAX = 2 * G + 300
SIZES = (1, 2, 255, 257, 8191, 8192, 8193, NMAX)
KEYSETS = (1, 3, 300, 8191, 8192)
OFF_CURVE = km.NO_KEY                                       # y = 2: no curve point (keyed_model.NO_KEY)
ORDER_2 = (st.P - 1).to_bytes(32, "little")                                  # (0, -1)


def krlc(engine, form, ks, idx, sig, msgs, off=None, mlen=None):
    """-> (verdicts, statistics); form "dev": every array in HBM; "host": numpy arrays"""
    if form == "dev":
        ok, stats = engine.ed25519_verify_keyed_rlc(dev(sig), ks, dev_idx(idx), dev(msgs),
                                                    msg_off=None if off is None else dev(off.astype(np.int64)), msg_len=mlen,
                                                    return_stats=True)
        return host(ok), tuple(stats)
    ok, stats = engine.ed25519_verify_keyed_rlc(sig, ks, np.ascontiguousarray(idx, dtype=np.uint32), msgs, msg_off=off, msg_len=mlen,
                                                return_stats=True)
    return ok, tuple(stats)


def expected_stats(n, failed_groups=()):
    """the four counters of a pass of n items in which exactly `failed_groups` went to the per-item kernels"""
    groups = (n + G - 1) // G
    size = lambda g: min(G, n - g * G)  # noqa: E731
    per_item = sum(size(g) for g in failed_groups)
    return (n - per_item, per_item, len(failed_groups), groups - len(failed_groups))


# ---------------------------------------------------------------- shared inputs: built once, never modified

@pytest.fixture(scope="module")
def keys(engine):
    """8193 secret keys and their public keys"""
    sk = np.random.default_rng(2001).integers(0, 256, (G + 1, 32), dtype=np.uint8)
    pk = host(engine.ed25519_genpub_batch(dev(sk)))
    sk.setflags(write=False); pk.setflags(write=False)
    return sk, pk


_TRAFFIC = {}


def traffic(engine, oracle, keys, nkeys, ragged=False):
    """2 * 8192 + 300 valid items under the first `nkeys` keys, item i under key (7919 i + 3) mod nkeys - every prefix is a batch
    of its own.  -> (idx, sig, msgs, off, mlen); the oracle accepts every item"""
    if (nkeys, ragged) in _TRAFFIC:
        return _TRAFFIC[(nkeys, ragged)]
    sk, pk = keys
    rng = np.random.default_rng(2002 + 10 * nkeys + ragged)
    idx = ((np.arange(NMAX, dtype=np.int64) * 7919 + 3) % nkeys).astype(np.uint32)
    if ragged:
        lens = rng.integers(0, 101, NMAX)
        lens[:3] = (100, 0, 1)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        mlen = None
    else:
        lens = np.full(NMAX, 32)
        off, mlen = None, 32
    msgs = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    sig = host(engine.ed25519_sign_batch(dev(sk[idx]), dev(pk[idx]), dev(msgs), msg_off=None if off is None else dev(off.astype(np.int64)),
                                         msg_len=mlen))
    if ragged:
        flat = msgs.tobytes()
        want = np.array([oracle.verify(sig[i].tobytes(), pk[idx[i]].tobytes(), flat[int(off[i]):int(off[i + 1])]) for i in range(NMAX)], np.uint8)
    else:
        want = oracle.verify_batch(np.ascontiguousarray(sig), np.ascontiguousarray(pk[idx]), msgs, 32)
    assert want.all()
    out = (idx, sig, msgs, off, mlen)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _TRAFFIC[(nkeys, ragged)] = out
    return out


def prefix(t, n):
    idx, sig, msgs, off, mlen = t
    if off is None:
        return idx[:n], sig[:n], msgs[:n * 32], None, mlen
    return idx[:n], sig[:n], msgs[:int(off[n])], off[:n + 1], None


_KEYSETS = {}


@pytest.fixture(scope="module")
def keyset_of(engine, keys):
    """nkeys -> the key set of the first nkeys keys, created once per module"""
    def get(nkeys):
        if nkeys not in _KEYSETS:
            _KEYSETS[nkeys] = engine.keyset_create(dev(keys[1][:nkeys]))
        return _KEYSETS[nkeys]
    yield get
    for ks in _KEYSETS.values():
        ks.close()
    _KEYSETS.clear()


# ---------------------------------------------------------------- 1: parity

@pytest.mark.parametrize("n", SIZES)
def test_parity_of_both_forms(engine, oracle, keys, keyset_of, n):
    """all-valid batches are decided by the combination; with one S corrupted at 0, 8191, 8192 and n - 1 (where the batch has
    such an item) the verdicts are the oracle's and exactly the groups that hold a corrupted item go to the per-item kernels"""
    sk, pk = keys
    for nkeys in KEYSETS:
        ks = keyset_of(nkeys)
        assert ks.count == nkeys
        for ragged in (False, True):
            idx, sig, msgs, off, mlen = prefix(traffic(engine, oracle, keys, nkeys, ragged), n)
            for form in ("dev", "host"):
                ok, stats = krlc(engine, form, ks, idx, sig, msgs, off, mlen)
                assert ok.dtype == np.uint8 and ok.shape == (n,)
                assert ok.all() and stats == expected_stats(n), (nkeys, ragged, form, stats, bad(ok, 1))
            for rows in ([0], [8191], [8192], [n - 1], [0, 8191, 8192, n - 1]):
                rows = sorted({r for r in rows if r < n})
                if not rows:
                    continue
                s2 = sig.copy()
                s2[rows, 32 + 7] ^= 0x10
                want = np.ones(n, np.uint8)
                for r in rows:
                    m = msgs[32 * r:32 * r + 32] if off is None else msgs[int(off[r]):int(off[r + 1])]
                    want[r] = oracle.verify(s2[r].tobytes(), pk[idx[r]].tobytes(), m.tobytes())
                assert not want[rows].any()
                form = "dev" if len(rows) == 1 else "host"
                ok, stats = krlc(engine, form, ks, idx, s2, msgs, off, mlen)
                assert np.array_equal(ok, want), (nkeys, ragged, rows, bad(ok, want))
                assert stats == expected_stats(n, sorted({r // G for r in rows})), (nkeys, ragged, rows, stats)


# ---------------------------------------------------------------- 2: the stages of a pass

def centred(v):
    v %= 8 * L
    return v - 8 * L if v >= 4 * L else v


def check_keyed_stages(engine, m, key_bytes, idx, which_r):
    """the last pass against the model m (tests/test_gpu_rlc_stages.py: Model over the items' own key bytes) with the key terms
    collected per key: t, S, flags, the -R rows and the base-point digits as in an unkeyed pass; the -A rows indexed by KEY; every
    -A window point, the -R window points `which_r` = [(group, entry)], and the group verdicts"""
    n, count = m.n, len(key_bytes)
    assert engine.debug_rlc_snapshot("info")[:2] == (n, m.groups)
    assert engine.debug_rlc_snapshot("seed") == m.seed
    ts = engine.debug_rlc_snapshot("ts")
    assert [st.LE(ts[i, 0].tobytes()) for i in range(n)] == m.t and [st.LE(ts[i, 1].tobytes()) for i in range(n)] == m.s
    assert engine.debug_rlc_snapshot("flags").tolist() == m.flags and not any(f & 2 for f in m.flags)
    dig = engine.debug_rlc_snapshot("dig")
    assert dig.shape == (m.groups, 48, G) and dig.dtype == np.int8
    assert np.array_equal(dig[:, 32:], m.dig[:, 32:])                                 # the digits of z: per item, as ever
    sums = {}
    for i in range(n):
        if m.flags[i] & 1:
            sums[(i // G, int(idx[i]))] = sums.get((i // G, int(idx[i])), 0) + m.z[i] * m.t[i]
    want = np.zeros((m.groups, 32, G), np.int8)
    for (g, k), v in sums.items():
        want[g, :, k] = st.signed_digits(centred(v), 32)
    assert not dig[:, :32, count:].any()                                              # k >= count
    unused = [(g, k) for g in range(m.groups) for k in range(count) if (g, k) not in sums]
    assert all(not dig[g, :32, k].any() for g, k in unused)
    assert np.array_equal(dig[:, :32], want)
    bdig = engine.debug_rlc_snapshot("bdig")
    assert np.array_equal(bdig, m.bdig)
    # window points: the key points taken once per key
    key_pts = []
    for kb in key_bytes:
        on, x, y = st.decode(kb)
        assert on
        key_pts.append(st.neg(st.ext((x, y))))
    seg = engine.debug_rlc_snapshot("seg")
    gok = engine.debug_rlc_snapshot("gok")
    assert seg.shape == (m.groups, 48, 4, 32)
    points = [[st.entry_point(seg[g, s]) for s in range(48)] for g in range(m.groups)]
    for g in range(m.groups):
        for s in range(32):
            w = 31 - s
            digits = np.append(want[g, w, :count].astype(np.int64), int(m.bdig[g, w]))
            assert st.affine(points[g][s]) == st.affine(st.weighted_sum(digits, key_pts + [st.BASE])), (g, s)
    for g, s in which_r:
        assert st.affine(points[g][s]) == st.affine(m.window_point(g, s)), (g, s)
    assert not engine.debug_rlc_snapshot("gflags").any()
    for g in range(m.groups):
        assert st.is_neutral(st.horner(points[g])) == (gok[g] == 1), g
    return unused, gok


@pytest.mark.parametrize("n", [700, G + 300])
def test_digit_rows_window_points_and_group_verdicts(engine, oracle, keys, n):
    """n = 700: every key used once, two keys of the set unused.  n = 8192 + 300: key 0 carries all 8192 items of group 0 (the
    longest sum, the most contended accumulator), keys 1..300 one item each and in group 1 only, key 301 unused"""
    sk, pk = keys
    if n == 700:
        idx, count = np.arange(n, dtype=np.uint32), 702
    else:
        idx, count = np.concatenate([np.zeros(G, np.uint32), 1 + np.arange(300, dtype=np.uint32)]), 302
    msg = np.random.default_rng(2003 + n).integers(0, 256, (n, 32), dtype=np.uint8)
    sig = host(engine.ed25519_sign_batch(dev(sk[idx]), dev(pk[idx]), dev(msg), msg_len=32))
    assert oracle.verify_batch(sig, np.ascontiguousarray(pk[idx]), msg, 32).all()
    with engine.keyset_create(pk[:count]) as ks:
        ok, stats = krlc(engine, "dev", ks, idx, sig, msg, mlen=32)
        assert ok.all() and stats == expected_stats(n)
        m = st.Model(sig, pk[idx], msg)
        key_bytes = [pk[k].tobytes() for k in range(count)]
        groups = (n + G - 1) // G
        which_r = [(0, 32 + 15 - w) for w in (0, 15)] + [(groups - 1, s) for s in range(32, 48)]
        unused, gok = check_keyed_stages(engine, m, key_bytes, idx, which_r)
        assert gok.tolist() == [1] * groups
        if n == 700:
            assert unused == [(0, 700), (0, 701)]
        else:
            assert (0, 1) in unused and (1, 0) in unused and (1, 301) in unused and (0, 0) not in unused and (1, 300) not in unused
        # one S corrupted: the window points are still the model's, the total is not neutral, the group goes per item
        s2 = sig.copy(); s2[n - 1, 32 + 9] ^= 0x20
        ok, stats = krlc(engine, "dev", ks, idx, s2, msg, mlen=32)
        want = np.ones(n, np.uint8); want[n - 1] = 0
        assert np.array_equal(ok, want) and stats == expected_stats(n, [groups - 1])
        _, gok = check_keyed_stages(engine, st.Model(s2, pk[idx], msg), key_bytes, idx, [(groups - 1, 47)])
        assert gok.tolist() == [1] * (groups - 1) + [0]


# ---------------------------------------------------------------- 3: indices outside the key set

@pytest.mark.parametrize("cofactored", [False, True])
def test_bad_indices_reject_their_items_and_nothing_else(engine, oracle, keys, keyset_of, cofactored):
    n = G + 300
    idx, sig, msgs, off, mlen = prefix(traffic(engine, oracle, keys, 300), n)
    at = (0, 63, 64, 8191, 8192)
    idx = idx.copy()
    for p, v in zip(at, (300, 301, 0xFFFFFFFF, 1 << 20, 300)):
        idx[p] = v
    want = np.ones(n, np.uint8)
    want[list(at)] = 0
    ks = keyset_of(300)
    with settings(engine, cofactored=cofactored):
        for form in ("dev", "host"):
            ok, stats = krlc(engine, form, ks, idx, sig, msgs, off, mlen)
            assert np.array_equal(ok, want), (form, bad(ok, want))
            assert stats == expected_stats(n), (form, stats)                          # both groups are still combined
        flags = engine.debug_rlc_snapshot("flags")
        assert [int(flags[p]) for p in at] == [0] * 5 and not engine.debug_rlc_snapshot("gflags").any()
        dig = engine.debug_rlc_snapshot("dig")
        assert not dig[0, 32:, [0, 63, 64, 8191]].any() and not dig[1, 32:, 0].any()  # no digit of z: the item is in no sum
        assert not dig[:, :32, 300:].any()                                            # and no row of a key that does not exist
        ok, stats = krlc(engine, "dev", ks, traffic(engine, oracle, keys, 300)[0][:n], sig, msgs, off, mlen)   # and nothing sticks
        assert ok.all() and stats == expected_stats(n)


# ---------------------------------------------------------------- 4: keys in the set that cannot be combined

@pytest.mark.parametrize("cofactored", [False, True])
def test_bad_keys_in_the_set_route_only_the_groups_that_use_them(engine, oracle, keys, cofactored):
    sk, pk = keys
    n = NMAX
    idx, sig, msgs, off, mlen = traffic(engine, oracle, keys, 300)
    keyset = np.concatenate([pk[:300], np.frombuffer(OFF_CURVE + ORDER_2, np.uint8).reshape(2, 32)])
    assert not km.decodes(OFF_CURVE) and km.decodes(ORDER_2)
    idx = idx.copy()
    idx[G + 5], idx[2 * G + 7] = 300, 301
    want = np.ones(n, np.uint8)
    for r in (G + 5, 2 * G + 7):
        args = (sig[r].tobytes(), keyset[idx[r]].tobytes(), msgs[32 * r:32 * r + 32].tobytes())
        want[r] = cm.accepts(*args) if cofactored else oracle.verify(*args)
    assert not want[G + 5]
    with engine.keyset_create(keyset) as ks, settings(engine, cofactored=cofactored):
        for form in ("dev", "host"):
            ok, stats = krlc(engine, form, ks, idx, sig, msgs, off, mlen)
            assert np.array_equal(ok, want), (form, bad(ok, want))
            assert stats == expected_stats(n, [1, 2]), (form, stats)                  # group 0 refers to neither: combined
        assert [int(x != 0) for x in engine.debug_rlc_snapshot("gflags")] == [0, 1, 1]
        # the set still holds both keys; no item refers to them: every group is combined
        ok, stats = krlc(engine, "dev", ks, traffic(engine, oracle, keys, 300)[0], sig, msgs, off, mlen)
        assert ok.all() and stats == expected_stats(n)


# ---------------------------------------------------------------- 5: settings

@pytest.fixture(scope="module")
def policy_items(oracle):
    sig, pk, msg, want = pm.policy_batch(oracle, 600)
    keyset, idx = km.as_keyset(pk)
    return sig, pk, msg, want, keyset, idx


@pytest.mark.parametrize("policy", pm.BITS + (pm.STRICT,))
def test_each_policy_bit(engine, oracle, keys, keyset_of, policy_items, policy):
    sig, pk, msg, want, keyset, idx = policy_items
    expect = want & pm.holds_batch(policy, sig, pk)
    assert (expect != want).any()
    with engine.keyset_create(keyset) as ks:
        for mode in (0, 1):
            with settings(engine, offcurve=mode, policy=policy):
                keyed = engine.ed25519_verify_keyed(sig, ks, idx, msg, msg_len=pm.MLEN)
                assert np.array_equal(keyed, expect)
                for form in ("dev", "host"):
                    ok, _ = krlc(engine, form, ks, idx, sig, msg, mlen=pm.MLEN)
                    assert np.array_equal(ok, keyed), (mode, form, bad(ok, keyed))
    # a group that IS combined: 300 valid items and one with S + l, which only S < l rejects - the strict rules read the items'
    # key bytes where the keyed pass left them
    n = 301
    idx, sig, msgs, off, mlen = prefix(traffic(engine, oracle, keys, 300), n)
    sig = sig.copy()
    sig[17, 32:] = np.frombuffer((int.from_bytes(sig[17, 32:].tobytes(), "little") + L).to_bytes(32, "little"), np.uint8)
    pubs = np.ascontiguousarray(keys[1][idx])
    assert oracle.verify_batch(sig, pubs, msgs, 32).all()
    expect = pm.holds_batch(policy, sig, pubs)
    assert expect.sum() == (n - 1 if policy & pm.S_BELOW_L else n)
    ks = keyset_of(300)
    with settings(engine, policy=policy):
        assert np.array_equal(engine.ed25519_verify_keyed(sig, ks, idx, msgs, msg_len=32), expect)
        for form in ("dev", "host"):
            ok, stats = krlc(engine, form, ks, idx, sig, msgs, mlen=32)
            assert np.array_equal(ok, expect) and stats == expected_stats(n), (form, stats, bad(ok, expect))


@pytest.mark.parametrize("policy", [0, pm.STRICT])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_cofactored_equation_over_its_vectors(engine, golden, mode, policy):
    sig, pk, msg, accept = cm.arrays(cm.from_json(golden("verify_cofactored.json")))
    expect = accept & pm.holds_batch(policy, sig, pk)
    assert 0 < expect.sum() < len(expect)
    order = np.random.default_rng(6).permutation(len(sig))
    with engine.keyset_create(pk) as ks, settings(engine, offcurve=mode, policy=policy, cofactored=True):
        keyed = engine.ed25519_verify_keyed(sig, ks, np.arange(len(sig), dtype=np.uint32), msg, msg_len=32)
        assert np.array_equal(keyed, expect)
        for form in ("dev", "host"):
            ok, _ = krlc(engine, form, ks, np.arange(len(sig)), sig, msg, mlen=32)
            assert np.array_equal(ok, keyed), (form, bad(ok, keyed))
            ok, _ = krlc(engine, form, ks, order, sig[order], msg[order], mlen=32)
            assert np.array_equal(ok, keyed[order]), (form, "shuffled", bad(ok, keyed[order]))


# ---------------------------------------------------------------- 6: a key set wider than a group

def test_a_key_set_of_8193_keys_is_decided_per_item(engine, oracle, keys):
    sk, pk = keys
    n = G + 300
    idx = ((np.arange(n, dtype=np.int64) * 5 + 8192) % (G + 1)).astype(np.uint32)     # item 0 under key 8192
    msg = np.random.default_rng(2006).integers(0, 256, (n, 32), dtype=np.uint8)
    sig = host(engine.ed25519_sign_batch(dev(sk[idx]), dev(pk[idx]), dev(msg), msg_len=32)).copy()
    sig[[0, 4000, n - 1], 32 + 3] ^= 2
    want = oracle.verify_batch(sig, np.ascontiguousarray(pk[idx]), msg, 32)
    assert want.sum() == n - 3
    with engine.keyset_create(pk) as ks:
        assert ks.count == G + 1
        keyed = engine.ed25519_verify_keyed(sig, ks, idx, msg, msg_len=32)
        assert np.array_equal(keyed, want)
        for form in ("dev", "host"):
            ok, stats = krlc(engine, form, ks, idx, sig, msg, mlen=32)
            assert np.array_equal(ok, keyed), (form, bad(ok, keyed))
            assert stats == (0, n, 2, 0), (form, stats)


# ---------------------------------------------------------------- 7: one workspace, four kinds of pass

def test_keyed_and_unkeyed_passes_share_one_workspace(engine, oracle, keys, keyset_of):
    """keyed _rlc, unkeyed _rlc, keyed per item and keyed _rlc again, in turn on one stream, each with inputs of its own and one
    corrupted item: none may depend on what another left in the digit rows, the point areas, the key-bytes area or the
    accumulators"""
    sk, pk = keys

    def case(nkeys, n, row):
        idx, sig, msgs, off, mlen = prefix(traffic(engine, oracle, keys, nkeys), n)
        sig = sig.copy(); sig[row, 32 + 1] ^= 8
        want = np.ones(n, np.uint8); want[row] = 0
        assert not oracle.verify(sig[row].tobytes(), pk[idx[row]].tobytes(), msgs[32 * row:32 * row + 32].tobytes())
        return idx, sig, msgs, want

    a, b, c, d = case(300, G + 300, G + 1), case(8192, NMAX, 5), case(3, 4099, 4098), case(8191, G + 7, 100)
    for _ in range(2):
        ok, stats = krlc(engine, "dev", keyset_of(300), a[0], a[1], a[2], mlen=32)
        assert np.array_equal(ok, a[3]) and stats == expected_stats(G + 300, [1]), stats
        ok, stats = engine.ed25519_verify_batch_rlc(dev(b[1]), dev(pk[b[0]]), dev(b[2]), msg_len=32, return_stats=True)
        assert np.array_equal(host(ok), b[3]) and tuple(stats) == expected_stats(NMAX, [0]), stats
        ok = host(engine.ed25519_verify_keyed(dev(c[1]), keyset_of(3), dev_idx(c[0]), dev(c[2]), msg_len=32))
        assert np.array_equal(ok, c[3])
        ok, stats = krlc(engine, "dev", keyset_of(8191), d[0], d[1], d[2], mlen=32)
        assert np.array_equal(ok, d[3]) and stats == expected_stats(G + 7, [0]), stats


# ---------------------------------------------------------------- 8: the device form, the host form

def test_two_passes_of_the_device_form_on_one_stream(engine, oracle, keys, keyset_of):
    """two calls queued back to back, nothing read in between; each synchronises the stream once for its group verdicts"""
    import torch
    x = prefix(traffic(engine, oracle, keys, 300), NMAX)
    y = prefix(traffic(engine, oracle, keys, 3), G + 300)
    sy = y[1].copy(); sy[G + 299, 32] ^= 1
    args = [(dev(x[1]), keyset_of(300), dev_idx(x[0]), dev(x[2])), (dev(sy), keyset_of(3), dev_idx(y[0]), dev(y[2]))]
    torch.cuda.synchronize()
    out = [engine.ed25519_verify_keyed_rlc(*a, msg_len=32, return_stats=True) for a in args]
    assert host(out[0][0]).all() and tuple(out[0][1]) == expected_stats(NMAX)
    want = np.ones(G + 300, np.uint8); want[G + 299] = 0
    assert np.array_equal(host(out[1][0]), want) and tuple(out[1][1]) == expected_stats(G + 300, [1])


def test_the_host_form_under_the_pipeline_hook(engine, oracle, keys, keyset_of):
    """eddsa_amd_set_pipeline(4096, 4096), the hook of test_gpu_keyed.py's chunk test: a call of the batch verification keeps its
    one combination per 2^20 items (host_pipe.c: a call with statistics is not tunable), so the groups are the call's and every
    chunk-sized slice of the indices is the right one"""
    n = NMAX
    idx, sig, msgs, off, mlen = traffic(engine, oracle, keys, 300)
    sig = sig.copy(); sig[3 * 4096 + 5, 32 + 2] ^= 1
    want = np.ones(n, np.uint8); want[3 * 4096 + 5] = 0
    lib = engine.library()
    try:
        lib.eddsa_amd_set_pipeline(ctypes.c_size_t(4096), ctypes.c_size_t(4096))
        ok, stats = krlc(engine, "host", keyset_of(300), idx, sig, msgs, mlen=32)
    finally:
        lib.eddsa_amd_set_pipeline(ctypes.c_size_t(0), ctypes.c_size_t(0))
    assert np.array_equal(ok, want), bad(ok, want)
    assert stats == expected_stats(n, [1])


def test_small_calls_go_to_the_keyed_per_item_kernels(engine, oracle, keys, keyset_of):
    """one knob for the keyed and the unkeyed form"""
    n = 700
    idx, sig, msgs, off, mlen = prefix(traffic(engine, oracle, keys, 300), n)
    engine.set_rlc_min_items(n + 1)
    for form in ("dev", "host"):
        ok, stats = krlc(engine, form, keyset_of(300), idx, sig, msgs, mlen=32)
        assert ok.all() and stats == (0, n, 1, 0), (form, stats)
    engine.set_rlc_min_items(n)
    ok, stats = krlc(engine, "dev", keyset_of(300), idx, sig, msgs, mlen=32)
    assert ok.all() and stats == (n, 0, 0, 1)


# ---------------------------------------------------------------- 9: the shipped library, from C

def test_c_program_against_the_shipped_library(engine, oracle, keys, tmp_path):
    """tests/c/verify_keyed_rlc.c: plain C against eddsa_amd.h, linked against libeddsa_amd.so (which exports no hook)"""
    sk, pk = keys
    n = G + 300
    idx, sig, msgs, off, mlen = prefix(traffic(engine, oracle, keys, 300), n)
    idx, sig = idx.copy(), sig.copy()
    idx[0], idx[256] = 300, 0xFFFFFFFF
    sig[G + 9, 32 + 4] ^= 1
    want = np.ones(n, np.uint8)
    want[[0, 256, G + 9]] = 0
    exe = build_c_program(tmp_path, "verify_keyed_rlc.c", libs=("eddsa_amd",), wall=True)
    files = []
    for name, a in (("keys", pk[:300]), ("idx", idx.astype(np.uint32)), ("sigs", sig), ("msgs", msgs), ("want", want)):
        files.append(str(tmp_path / (name + ".bin")))
        np.ascontiguousarray(a).tofile(files[-1])
    r = subprocess.run([str(exe)] + files + [str(G)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify_keyed_rlc: ok (%d items, 300 keys, %d combined)" % (n, G) in r.stdout
