"""GPU tests of the digest, Ed25519ctx and Ed25519ph forms of key-set verification (include/eddsa_amd.h:
ed25519_verify_keyed_digests[_rlc], ed25519ctx_verify_keyed, ed25519ph_verify_keyed; keyed_kernels.h, rlc_keyed.h): ok[i] is what
the unkeyed form of the same name returns for (sigs[i], keys[key_idx[i]], digest / message / prehash i), an index outside the key
set rejects its item.  Expected verdicts are the oracle's on (sig, keys[idx], msg) with the digests computed by hashlib, and
tests/dom2_model.py's for ctx / ph; the unkeyed form of the same name over keys[idx] is held against them too.  Every test puts the
settings back."""
import ctypes
import hashlib

import numpy as np
import pytest

import dom2_model as dm
import keyed_model as km
import policy_model as pm
from ed_model import arr
from gpu_kit import always_combine, bad, dev, dev_idx, host, settings  # noqa: F401  (always_combine: a fixture)
from test_gpu_keyed import honest, keyed, mixed  # noqa: F401 (fixtures)
from test_gpu_keyed_comb import comb_set
from test_gpu_keyed_rlc import expected_stats

pytestmark = pytest.mark.gpu
G = 8192
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 4099)
KEYSETS = (1, 3, 300)
CONTEXTS = (b"", b"ctx", bytes(range(255)))
NO_IDX = 0xFFFFFFFF


def u32(idx):
    return np.ascontiguousarray(idx, dtype=np.uint32)


def make_set(engine, keys, comb):
    return comb_set(engine, keys) if comb else engine.keyset_create(dev(keys))


def rows_of(msgs, off, mlen, n):
    """the items' messages as a list of bytes"""
    flat = msgs.tobytes()
    if off is None:
        return [flat[mlen * i:mlen * i + mlen] for i in range(n)]
    return [flat[int(off[i]):int(off[i + 1])] for i in range(n)]


def digests_of(sig, pubs, rows):
    """SHA-512(R || A || M) per item, as the caller of the digest forms computes it"""
    return arr([hashlib.sha512(sig[i, :32].tobytes() + pubs[i].tobytes() + rows[i]).digest() for i in range(len(sig))])


def with_bad_indices(idx, want, count):
    """an index equal to `count` and 0xFFFFFFFF put over two items (one item: over it) -> (idx, want with those items 0, their
    positions); the items' other inputs stay what they were"""
    idx, want = u32(idx).copy(), want.copy()
    at = sorted({len(idx) // 2, len(idx) - 1})
    for p, v in zip(at, (count, NO_IDX) if len(at) == 2 else (NO_IDX,)):
        idx[p], want[p] = v, 0
    return idx, want, at


def expanded(keys, idx):
    """keys[idx] for the unkeyed call; an index outside the set stands for key 0 (its verdict is forced to 0 by the caller)"""
    idx = np.asarray(idx, dtype=np.int64)
    return np.ascontiguousarray(keys[np.where(idx < len(keys), idx, 0)])


def kdigests(engine, form, ks, idx, sig, dig):
    if form == "dev":
        return host(engine.ed25519_verify_keyed_digests(dev(sig), ks, dev_idx(idx), dev(dig)))
    return engine.ed25519_verify_keyed_digests(sig, ks, u32(idx), dig)


def kdom(engine, form, flag, ks, idx, sig, msgs, off, mlen, context):
    """ed25519ctx_verify_keyed (flag 0: msgs / off / mlen as in ed25519_verify_keyed) or ed25519ph_verify_keyed (flag 1: msgs holds
    the prehashes)"""
    put, pidx = (dev, dev_idx) if form == "dev" else ((lambda a: a), u32)
    if flag == dm.PH:
        return host(engine.ed25519ph_verify_keyed(put(sig), ks, pidx(idx), put(msgs), context))
    o = None if off is None else (dev(off.astype(np.int64)) if form == "dev" else off)
    return host(engine.ed25519ctx_verify_keyed(put(sig), ks, pidx(idx), put(msgs), context, msg_off=o, msg_len=mlen))


def udom(engine, flag, sig, pubs, msgs, off, mlen, context):
    """the unkeyed form of the same name, device pointers"""
    if flag == dm.PH:
        return host(engine.ed25519ph_verify_batch(dev(sig), dev(pubs), dev(msgs), context))
    return host(engine.ed25519ctx_verify_batch(dev(sig), dev(pubs), dev(msgs), context,
                                               msg_off=None if off is None else dev(off.astype(np.int64)), msg_len=mlen))


# ---------------------------------------------------------------- shared inputs: built once, never modified

_DOM = {}


def dom_mixed(engine, oracle, honest, n, nkeys, flag, ragged, context):
    """test_gpu_keyed.mixed for the context variants: n items signed by the engine's own ed25519ctx_sign_batch / ed25519ph_sign_batch
    under `nkeys` honest keys and `context`, then mixed by item index mod 8 - 0..4: untouched; 5: one bit of the signature flipped;
    6: its key with one bit flipped; 7: a random 32-byte key.  ph: the "messages" are 64 random bytes per item, the prehashes.
    -> (keys, idx, sig, msgs, off, mlen, dom2_model's verdicts on (sig, keys[idx], message))"""
    key = (n, nkeys, flag, ragged, context)
    if key in _DOM:
        return _DOM[key]
    sk, pk = honest
    rng = np.random.default_rng(7000 * n + 70 * nkeys + 7 * flag + ragged + len(context))
    who = rng.integers(0, nkeys, n)
    if ragged:
        lens = rng.integers(0, 151, n)
        lens[: min(n, 3)] = (150, 0, 1)[: min(n, 3)]
        off, mlen = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), None
    else:
        lens = np.full(n, 64 if flag == dm.PH else 32)
        off, mlen = None, int(lens[0])
    msgs = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    if flag == dm.PH:
        sig = host(engine.ed25519ph_sign_batch(dev(sk[who]), dev(pk[who]), dev(msgs), context)).copy()
    else:
        sig = host(engine.ed25519ctx_sign_batch(dev(sk[who]), dev(pk[who]), dev(msgs), context,
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
    rows = rows_of(msgs, off, mlen, n)
    want = np.array([dm.verify(oracle.lib, sig[i].tobytes(), pubs[i].tobytes(), rows[i], flag, context) for i in range(n)], np.uint8)
    assert all(want[i] for i in range(n) if i % 8 < 5)
    assert all(km.decodes(pubs[i].tobytes()) for i in np.nonzero(want)[0])               # the off-curve modes agree on this batch
    out = (keys, idx, sig, msgs, off, mlen, want)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _DOM[key] = out
    return out


# ---------------------------------------------------------------- 1: parity at every boundary

@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_digests_parity_at_every_boundary(engine, oracle, honest, n, mode):
    """the mixed workload of test_gpu_keyed.py with its digests computed by hashlib, an index equal to `count` and 0xFFFFFFFF on top:
    plain and comb sets, both forms, the three off-curve modes; fixed and ragged messages differ only in what was hashed"""
    for nkeys in KEYSETS:
        for ragged in (0, 1):
            keys, idx, sig, msgs, off, mlen, want = mixed(engine, oracle, honest, n, nkeys, ragged)
            dig = digests_of(sig, keys[idx], rows_of(msgs, off, mlen, n))
            idx, want, at = with_bad_indices(idx, want, len(keys))
            pubs = expanded(keys, idx)
            for comb in (False, True):
                with make_set(engine, keys, comb) as ks, settings(engine, offcurve=mode):
                    unkeyed = host(engine.ed25519_verify_digests(dev(sig), dev(pubs), dev(dig)))
                    unkeyed[at] = 0
                    for form in ("dev", "host"):
                        got = kdigests(engine, form, ks, idx, sig, dig)
                        assert got.dtype == np.uint8 and got.shape == (n,)
                        assert np.array_equal(got, want), (nkeys, ragged, comb, form, bad(got, want))
                        assert np.array_equal(got, unkeyed), (nkeys, ragged, comb, form, bad(got, unkeyed))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_ctx_and_ph_parity_at_every_boundary(engine, oracle, honest, n, mode):
    """ctx over fixed and ragged messages and ph, each under contexts of 0, 3 and 255 bytes - the context goes round with the key
    set's size, so that each form meets each length"""
    for j, nkeys in enumerate(KEYSETS):
        for v, (flag, ragged) in enumerate(((dm.CTX, 0), (dm.CTX, 1), (dm.PH, 0))):
            context = CONTEXTS[(j + v) % 3]
            keys, idx, sig, msgs, off, mlen, want = dom_mixed(engine, oracle, honest, n, nkeys, flag, ragged, context)
            idx, want, at = with_bad_indices(idx, want, len(keys))
            pubs = expanded(keys, idx)
            for comb in (False, True):
                with make_set(engine, keys, comb) as ks, settings(engine, offcurve=mode):
                    unkeyed = udom(engine, flag, sig, pubs, msgs, off, mlen, context)
                    unkeyed[at] = 0
                    for form in ("dev", "host"):
                        got = kdom(engine, form, flag, ks, idx, sig, msgs, off, mlen, context)
                        assert got.dtype == np.uint8 and got.shape == (n,)
                        assert np.array_equal(got, want), (nkeys, flag, ragged, len(context), comb, form, bad(got, want))
                        assert np.array_equal(got, unkeyed), (nkeys, flag, ragged, len(context), comb, form, bad(got, unkeyed))


# ---------------------------------------------------------------- 2: the edge and torsion vectors

@pytest.fixture(scope="module")
def vectors(golden, oracle):
    """the 273 + 192 recorded vectors as one key set (entry i = case i's key), shuffled: sig, keys, idx, the messages, their
    digests, the recorded verdicts, and dom2_model's verdicts for the same (R, S, A, M) read as ctx and as ph signatures"""
    cases = golden("verify_edges.json") + golden("verify_torsion.json")
    assert len(cases) == 273 + 192
    order = np.random.default_rng(15).permutation(len(cases))
    sig, keys = pm.arr([pm.H(cases[i]["sig"]) for i in order]), pm.arr([pm.H(c["pub"]) for c in cases])
    rows = [pm.H(cases[i]["msg"]) for i in order]
    want = np.array([cases[i]["accept"] for i in order], np.uint8)
    pubs = keys[order]
    pre = [hashlib.sha512(r).digest() for r in rows]                                   # ph: the prehashes of the same messages
    context = b"vectors"
    dom_want = {dm.CTX: np.array([dm.verify(oracle.lib, sig[i].tobytes(), pubs[i].tobytes(), rows[i], dm.CTX, context) for i in range(len(rows))], np.uint8),
                dm.PH: np.array([dm.verify(oracle.lib, sig[i].tobytes(), pubs[i].tobytes(), pre[i], dm.PH, context) for i in range(len(rows))], np.uint8)}
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    return dict(sig=sig, keys=keys, idx=u32(order), pubs=pubs, msgs=np.frombuffer(b"".join(rows), np.uint8), off=off,
                pre=arr(pre), dig=digests_of(sig, pubs, rows), want=want, dom_want=dom_want, context=context)


@pytest.mark.parametrize("cofactored", [False, True])
@pytest.mark.parametrize("policy", [0, pm.STRICT])
@pytest.mark.parametrize("comb", [False, True])
def test_edge_and_torsion_vectors(engine, vectors, comb, policy, cofactored):
    """through the three per-item keyed forms.  Under the reference's equation the digest form is held against the recorded verdicts
    and ctx / ph against dom2_model (the vectors' R, S and A under another challenge), each cut down by policy_model's rules; under
    every setting - the cofactored equation included - each is held against the unkeyed form of the same name"""
    v = vectors
    holds = pm.holds_batch(policy, v["sig"], v["pubs"])
    with make_set(engine, v["keys"], comb) as ks, settings(engine, policy=policy, cofactored=cofactored):
        runs = [("digests", lambda form: kdigests(engine, form, ks, v["idx"], v["sig"], v["dig"]),
                 host(engine.ed25519_verify_digests(dev(v["sig"]), dev(v["pubs"]), dev(v["dig"]))), v["want"]),
                ("ctx", lambda form: kdom(engine, form, dm.CTX, ks, v["idx"], v["sig"], v["msgs"], v["off"], None, v["context"]),
                 udom(engine, dm.CTX, v["sig"], v["pubs"], v["msgs"], v["off"], None, v["context"]), v["dom_want"][dm.CTX]),
                ("ph", lambda form: kdom(engine, form, dm.PH, ks, v["idx"], v["sig"], v["pre"], None, 64, v["context"]),
                 udom(engine, dm.PH, v["sig"], v["pubs"], v["pre"], None, 64, v["context"]), v["dom_want"][dm.PH])]
        for name, run, unkeyed, recorded in runs:
            for form in ("dev", "host"):
                got = run(form)
                assert np.array_equal(got, unkeyed), (name, form, bad(got, unkeyed))
                if not cofactored:
                    assert np.array_equal(got, recorded & holds), (name, form, bad(got, recorded & holds))
    assert 0 < v["want"].sum() < len(v["want"])


# ---------------------------------------------------------------- 3: the variants keep apart; a digest over other bytes

def test_cross_variant_separation(engine, oracle, honest):
    """a plain Ed25519 signature is rejected by the ctx and ph keyed forms, a ctx signature by ph and ph by ctx; each is accepted by
    its own form (the signatures are the library's own)"""
    sk, pk = honest
    n = 300
    who = np.arange(n) % 7
    pre = np.random.default_rng(31).integers(0, 256, (n, 64), dtype=np.uint8)          # 64-byte messages: a prehash, or a message
    context = b"separate"
    plain = host(engine.ed25519_sign_batch(dev(sk[who]), dev(pk[who]), dev(pre), msg_len=64))
    ctx = host(engine.ed25519ctx_sign_batch(dev(sk[who]), dev(pk[who]), dev(pre), context, msg_len=64))
    ph = host(engine.ed25519ph_sign_batch(dev(sk[who]), dev(pk[who]), dev(pre), context))
    assert oracle.verify_batch(plain, np.ascontiguousarray(pk[who]), pre, 64).all()
    for comb in (False, True):
        with make_set(engine, pk[:7], comb) as ks:
            for form in ("dev", "host"):
                for sig, accepts in ((plain, None), (ctx, dm.CTX), (ph, dm.PH)):
                    for flag in (dm.CTX, dm.PH):
                        got = kdom(engine, form, flag, ks, who, sig, pre.reshape(-1), None, 64, context)
                        assert got.all() if flag == accepts else not got.any(), (comb, form, accepts, flag)
                # ... and another context is another domain
                assert not kdom(engine, form, dm.CTX, ks, who, ctx, pre.reshape(-1), None, 64, b"separatf").any()
                # the plain signatures through the digest form, for completeness: accepted
                assert kdigests(engine, form, ks, who, plain, digests_of(plain, pk[who], [r.tobytes() for r in pre])).all()


def test_a_digest_over_another_key_is_rejected(engine, honest, oracle):
    """the caller vouches for the key bytes in the digest: one computed with another key than keys[key_idx[i]] is verified as the
    challenge it is - the item is rejected, its neighbours are not affected"""
    keys, idx, sig, msgs, off, mlen, want = mixed(engine, oracle, honest, 257, 3, 0)
    rows = rows_of(msgs, off, mlen, 257)
    dig = digests_of(sig, keys[idx], rows)
    at = [i for i in (0, 64, 128, 256) if want[i]]
    assert len(at) >= 3
    other = keys[idx].copy()
    other[at] = keys[(idx[at] + 1) % 3]
    assert not any(np.array_equal(other[p], keys[idx[p]]) for p in at)
    dig2 = dig.copy()
    dig2[at] = digests_of(sig[at], other[at], [rows[p] for p in at])
    expect = want.copy()
    expect[at] = 0
    for comb in (False, True):
        with make_set(engine, keys, comb) as ks:
            for form in ("dev", "host"):
                got = kdigests(engine, form, ks, idx, sig, dig2)
                assert np.array_equal(got, expect), (comb, form, bad(got, expect))
                assert np.array_equal(kdigests(engine, form, ks, idx, sig, dig), want)


# ---------------------------------------------------------------- 4: the combination over digests

NMAX = 2 * G + 5


@pytest.fixture(scope="module")
def many_keys(engine):
    """8193 secret keys and their public keys"""
    sk = np.random.default_rng(3001).integers(0, 256, (G + 1, 32), dtype=np.uint8)
    pk = host(engine.ed25519_genpub_batch(dev(sk)))
    sk.setflags(write=False); pk.setflags(write=False)
    return sk, pk


_TRAFFIC = {}


def traffic(engine, oracle, many_keys, nkeys):
    """2 * 8192 + 5 valid items under the first `nkeys` keys, item i under key (7919 i + 3) mod nkeys: every prefix is a batch of
    its own -> (idx, sig, digests, msgs); the oracle accepts every item"""
    if nkeys not in _TRAFFIC:
        sk, pk = many_keys
        idx = ((np.arange(NMAX, dtype=np.int64) * 7919 + 3) % nkeys).astype(np.uint32)
        msg = np.random.default_rng(3002 + nkeys).integers(0, 256, (NMAX, 32), dtype=np.uint8)
        sig = host(engine.ed25519_sign_batch(dev(sk[idx]), dev(pk[idx]), dev(msg), msg_len=32))
        assert oracle.verify_batch(np.ascontiguousarray(sig), np.ascontiguousarray(pk[idx]), msg, 32).all()
        dig = digests_of(sig, pk[idx], [m.tobytes() for m in msg])
        for a in (idx, sig, dig, msg):
            a.setflags(write=False)
        _TRAFFIC[nkeys] = (idx, sig, dig, msg)
    return _TRAFFIC[nkeys]


def kdrlc(engine, form, ks, idx, sig, dig):
    """-> (verdicts, statistics)"""
    if form == "dev":
        ok, stats = engine.ed25519_verify_keyed_digests_rlc(dev(sig), ks, dev_idx(idx), dev(dig), return_stats=True)
        return host(ok), tuple(stats)
    ok, stats = engine.ed25519_verify_keyed_digests_rlc(sig, ks, u32(idx), dig, return_stats=True)
    return ok, tuple(stats)


@pytest.mark.parametrize("cofactored", [False, True])
@pytest.mark.parametrize("nkeys", [1, 300, G])
def test_rlc_groups_and_fallback(engine, oracle, many_keys, always_combine, nkeys, cofactored):
    """n on both sides of a group's end and 2 * 8192 + 5: all valid - every group combined; one corrupted item at 0, 8191, 8192 and
    n - 1 - exactly those groups go to the per-item kernels; one out-of-range index in an otherwise valid group - still combined,
    that item 0.  Verdicts against the oracle (every other item is valid) and the unkeyed digests _rlc over the expanded keys"""
    sk, pk = many_keys
    idx, sig, dig, msg = traffic(engine, oracle, many_keys, nkeys)
    with engine.keyset_create(dev(pk[:nkeys])) as ks, settings(engine, cofactored=cofactored):
        for n in (G - 1, G, G + 1, NMAX):
            for form in ("dev", "host") if n in (G + 1, NMAX) else ("dev",):
                ok, stats = kdrlc(engine, form, ks, idx[:n], sig[:n], dig[:n])
                assert ok.all() and stats == expected_stats(n), (n, form, stats)
            rows = sorted({p for p in (0, G - 1, G, n - 1) if p < n})
            s2 = sig[:n].copy()
            s2[rows, 32 + 2] ^= 4
            want = np.ones(n, np.uint8); want[rows] = 0
            assert not oracle.verify_batch(np.ascontiguousarray(s2[rows]), np.ascontiguousarray(pk[idx[rows]]), np.ascontiguousarray(msg[rows]), 32).any()
            ok, stats = kdrlc(engine, "dev", ks, idx[:n], s2, dig[:n])
            assert np.array_equal(ok, want), (n, bad(ok, want))
            assert stats == expected_stats(n, sorted({p // G for p in rows})), (n, stats)
            unkeyed, ustats = engine.ed25519_verify_digests_rlc(dev(s2), dev(pk[idx[:n]]), dev(dig[:n]), return_stats=True)
            assert np.array_equal(host(unkeyed), ok) and tuple(ustats) == stats
            i2 = idx[:n].copy()
            i2[n // 2] = nkeys if n & 1 else NO_IDX
            want = np.ones(n, np.uint8); want[n // 2] = 0
            ok, stats = kdrlc(engine, "dev", ks, i2, sig[:n], dig[:n])
            assert np.array_equal(ok, want) and stats == expected_stats(n), (n, stats, bad(ok, want))


def test_rlc_over_8193_keys_runs_per_item(engine, oracle, many_keys, always_combine):
    sk, pk = many_keys
    n = G + 300
    idx = ((np.arange(n, dtype=np.int64) * 5 + 8192) % (G + 1)).astype(np.uint32)     # item 0 under key 8192
    msg = np.random.default_rng(3006).integers(0, 256, (n, 32), dtype=np.uint8)
    sig = host(engine.ed25519_sign_batch(dev(sk[idx]), dev(pk[idx]), dev(msg), msg_len=32)).copy()
    sig[[0, 4000, n - 1], 32 + 3] ^= 2
    want = oracle.verify_batch(sig, np.ascontiguousarray(pk[idx]), msg, 32)
    assert want.sum() == n - 3
    dig = digests_of(sig, pk[idx], [m.tobytes() for m in msg])
    with engine.keyset_create(pk) as ks:
        assert ks.count == G + 1
        for form in ("dev", "host"):
            ok, stats = kdrlc(engine, form, ks, idx, sig, dig)
            assert np.array_equal(ok, want), (form, bad(ok, want))
            assert stats == (0, n, 2, 0), (form, stats)


def test_rlc_over_a_comb_set_falls_back_to_the_comb_route(engine, oracle, many_keys, always_combine):
    """the combination does not use the comb; the group with a corrupted item is decided by the comb route's kernels"""
    sk, pk = many_keys
    n = G + 300
    idx, sig, dig, msg = traffic(engine, oracle, many_keys, 300)
    s2 = sig[:n].copy()
    s2[G + 7, 32 + 3] ^= 1                                                            # (in S: an R that decodes to no point is rejected without a fallback)
    want = np.ones(n, np.uint8); want[G + 7] = 0
    assert not oracle.verify(s2[G + 7].tobytes(), pk[idx[G + 7]].tobytes(), msg[G + 7].tobytes())
    with comb_set(engine, pk[:300]) as ks:
        assert ks.comb
        for form in ("dev", "host"):
            ok, stats = kdrlc(engine, form, ks, idx[:n], s2, dig[:n])
            assert np.array_equal(ok, want), (form, bad(ok, want))
            assert stats == expected_stats(n, [1]), (form, stats)


def test_rlc_seed_equals_the_unkeyed_digest_pass(engine, oracle, many_keys, always_combine):
    """the leaves are formed from the same bytes: seed (and with it every coefficient z_i) and leaves of a keyed digest pass equal
    those of ed25519_verify_digests_rlc over the expanded keys"""
    sk, pk = many_keys
    n = G + 300
    idx, sig, dig, msg = traffic(engine, oracle, many_keys, 300)
    with engine.keyset_create(pk[:300]) as ks:
        ok = engine.ed25519_verify_keyed_digests_rlc(dev(sig[:n]), ks, dev_idx(idx[:n]), dev(dig[:n]))
        assert host(ok).all() and engine.debug_rlc_snapshot("info")[:2] == (n, 2)
        seed, leaf = engine.debug_rlc_snapshot("seed"), engine.debug_rlc_snapshot("leaf").copy()
    ok = engine.ed25519_verify_digests_rlc(dev(sig[:n]), dev(pk[idx[:n]]), dev(dig[:n]))
    assert host(ok).all() and engine.debug_rlc_snapshot("info")[:2] == (n, 2)
    assert engine.debug_rlc_snapshot("seed") == seed and np.array_equal(engine.debug_rlc_snapshot("leaf"), leaf)
    assert leaf[5].tobytes() == hashlib.sha512(dig[5].tobytes() + sig[5, 32:].tobytes()).digest()[:32]


# ---------------------------------------------------------------- 5: chunks; one workspace

def test_chunks_of_the_host_form(engine, oracle, honest):
    """eddsa_amd_set_pipeline(4096, 4096), the hook of test_gpu_keyed.py's chunk test, at n = 3 * 4096 + 77: every chunk uploads its
    own slice of the indices and of the digests"""
    sk, pk = honest
    n = 3 * 4096 + 77
    msg = np.random.default_rng(92).integers(0, 256, (n, 32), dtype=np.uint8)
    who = (np.arange(n, dtype=np.int64) * 101 + 3) % 300
    sig = host(engine.ed25519_sign_batch(dev(sk[who]), dev(pk[who]), dev(msg), msg_len=32)).copy()
    sig[5::16, 3] ^= 1
    idx = who.astype(np.uint32)
    idx[9::16] = (idx[9::16] + 1) % 300                                               # the wrong key: the digest is over its bytes
    want = oracle.verify_batch(sig, np.ascontiguousarray(pk[idx]), msg, 32)
    assert all(0 < want[lo:lo + 4096].sum() < len(want[lo:lo + 4096]) for lo in range(0, n, 4096))
    assert all(len(set(idx[lo - 8:lo + 8])) > 8 for lo in range(4096, n, 4096))          # the indices differ across the boundaries
    dig = digests_of(sig, pk[idx], [m.tobytes() for m in msg])
    pre = np.random.default_rng(93).integers(0, 256, (n, 64), dtype=np.uint8)
    sig_ph = host(engine.ed25519ph_sign_batch(dev(sk[who]), dev(pk[who]), dev(pre), b"chunks"))
    want_ph = (idx == who).astype(np.uint8)
    lib = engine.library()
    with engine.keyset_create(pk) as ks:
        try:
            lib.eddsa_amd_set_pipeline(ctypes.c_size_t(4096), ctypes.c_size_t(4096))
            got = kdigests(engine, "host", ks, idx, sig, dig)
            got_ph = kdom(engine, "host", dm.PH, ks, idx, sig_ph, pre.reshape(-1), None, 64, b"chunks")
        finally:
            lib.eddsa_amd_set_pipeline(ctypes.c_size_t(0), ctypes.c_size_t(0))
    assert np.array_equal(got, want), bad(got, want)
    assert np.array_equal(got_ph, want_ph), bad(got_ph, want_ph)


@pytest.mark.parametrize("comb", [False, True])
def test_passes_of_four_kinds_share_one_workspace(engine, oracle, honest, comb):
    """on one stream, back to back: a keyed message pass, a keyed digest pass, an unkeyed ctx pass and a keyed ctx pass, each over
    inputs of its own - the key-bytes area and the ctx digests' area are written by one pass and read by the next one's kernels
    only behind it"""
    a = mixed(engine, oracle, honest, 4099, 300, 0)
    b = mixed(engine, oracle, honest, 1000, 3, 1)
    dig_b = digests_of(b[2], b[0][b[1]], rows_of(b[3], b[4], b[5], 1000))
    c = dom_mixed(engine, oracle, honest, 4099, 3, dm.CTX, 1, CONTEXTS[1])
    d = dom_mixed(engine, oracle, honest, 1000, 300, dm.CTX, 0, CONTEXTS[2])
    with make_set(engine, a[0], comb) as ka, make_set(engine, b[0], comb) as kb, make_set(engine, d[0], comb) as kd:
        dev_args = dict(a=(dev(a[2]), ka, dev_idx(a[1]), dev(a[3])), b=(dev(b[2]), kb, dev_idx(b[1]), dev(dig_b)),
                        c=(dev(c[2]), dev(c[0][c[1]]), dev(c[3])), d=(dev(d[2]), kd, dev_idx(d[1]), dev(d[3])))
        import torch
        torch.cuda.synchronize()
        for _ in range(3):
            outs = [engine.ed25519_verify_keyed(*dev_args["a"], msg_len=32),
                    engine.ed25519_verify_keyed_digests(*dev_args["b"]),
                    engine.ed25519ctx_verify_batch(*dev_args["c"], CONTEXTS[1], msg_off=dev(c[4].astype(np.int64))),
                    engine.ed25519ctx_verify_keyed(*dev_args["d"], CONTEXTS[2], msg_len=32)]
            for got, x in zip(outs, (a, b, c, d)):                                    # nothing was read in between
                assert np.array_equal(host(got), x[6]), bad(got, x[6])
