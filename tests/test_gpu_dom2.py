"""GPU tests of Ed25519ctx and Ed25519ph (include/eddsa_amd.h: ed25519ctx_*, ed25519ph_*, host- and device-pointer forms).
Expected signatures come from the model (tests/dom2_model.py: hashlib, Python integers, the oracle's curve operations) and from
RFC 8032's vectors; expected verdicts from ed25519_verify_digests on hashlib's SHA-512(dom2 || R || A || M') - never from the
forms under test."""
import ctypes

import numpy as np
import pytest

import dom2_model as dm
from ed_model import arr
from gpu_kit import dev, host

pytestmark = pytest.mark.gpu
L = dm.L
CTX, PH = dm.CTX, dm.PH
INVALID_VALUE = -1                                  # -hipErrorInvalidValue


def run(engine, what, flag, device, first, pk, rows, context, ragged=False):
    """one call of the form (what: "sign" | "verify", flag, host or device pointers) over the messages / prehashes `rows` (a list
    of bytes; ragged: packed back to back behind an offset table, else all of one length) -> the result as a numpy array"""
    put = dev if device else (lambda a: a)
    fn = getattr(engine, f"ed25519{'ph' if flag == PH else 'ctx'}_{what}_batch")
    if flag == PH:
        assert not ragged
        return host(fn(put(first), put(pk), put(arr(rows, 64)), context))
    blob = np.frombuffer(b"".join(bytes(r) for r in rows), np.uint8).copy()
    if ragged:
        off = np.zeros(len(rows) + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in rows])
        return host(fn(put(first), put(pk), put(blob), context, msg_off=put(off) if device else off.astype(np.uint64)))
    assert len({len(r) for r in rows}) == 1
    return host(fn(put(first), put(pk), put(blob), context, msg_len=len(rows[0])))


def digests(sig, pk, rows, flag, context):
    return arr([dm.challenge_digest(sig[i].tobytes(), pk[i].tobytes(), bytes(rows[i]), flag, context) for i in range(len(rows))])


def check_signatures(engine, orc, sig, sk, pk, rows, flag, context, modelled=200):
    """every item: S == (r + t a) mod l with t from the returned R, and the signature is accepted by ed25519_verify_digests on
    hashlib's digest (which pins R = r B); the first `modelled` items and the last tile: the model's signature, byte for byte"""
    n = len(rows)
    assert sig.shape == (n, 64) and sig.dtype == np.uint8
    dom, bad, dig = dm.dom2(flag, context), [], []
    sigb, skb, pkb = sig.tobytes(), sk.tobytes(), pk.tobytes()
    for i in range(n):                              # (dm.response_ok, with each hash of the item computed once)
        s, p, m = sigb[64 * i:64 * i + 64], pkb[32 * i:32 * i + 32], bytes(rows[i])
        a, prefix = dm.secret_scalar(skb[32 * i:32 * i + 32])
        dig.append(dm.sha(dom, s[:32], p, m))
        if dm.num(s[32:]) != (dm.num(dm.sha(dom, prefix, m)) + dm.num(dig[-1]) * a) % L:
            bad.append(i)
    assert not bad, bad[:8]
    ok = engine.ed25519_verify_digests(dev(sig), dev(pk), dev(arr(dig))).cpu().numpy()
    assert ok.all(), np.nonzero(ok == 0)[0][:8]
    for i in sorted(set(range(min(n, modelled))) | set(range(max(0, n - 256), n))):
        assert sig[i].tobytes() == dm.sign(orc, sk[i].tobytes(), pk[i].tobytes(), bytes(rows[i]), flag, context), i


def corrupt(sig, pk, rows, seed):
    """one item in eight: a bit of R, of S, of A or of M' in turn (an empty message: of R) -> copies"""
    rng = np.random.default_rng(seed)
    sig, pk, rows = sig.copy(), pk.copy(), [bytearray(r) for r in rows]
    for i in range(3, len(rows), 8):
        k = (i // 8) % 4
        bit = 1 << int(rng.integers(0, 8))
        if k == 0 or (k == 3 and not rows[i]): sig[i, rng.integers(0, 32)] ^= bit
        elif k == 1: sig[i, 32 + rng.integers(0, 32)] ^= bit
        elif k == 2: pk[i, rng.integers(0, 32)] ^= bit
        else: rows[i][int(rng.integers(0, len(rows[i])))] ^= bit
    return sig, pk, [bytes(r) for r in rows]


def check_verdicts(engine, got, sig, pk, rows, flag, context, some_rejects=True):
    want = engine.ed25519_verify_digests(dev(sig), dev(pk), dev(digests(sig, pk, rows, flag, context))).cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    untouched = np.ones(len(rows), bool); untouched[3::8] = False
    assert want[untouched].all() and (not some_rejects or len(rows) < 4 or not want[3::8].all())


def rows_of(rng, n, length):
    data = rng.integers(0, 256, (n, length), dtype=np.uint8)
    return [data[i].tobytes() for i in range(n)]


# ---------------------------------------------------------------- RFC 8032's vectors through the eight entry points

def test_rfc8032_vectors_through_all_eight_entry_points(engine, oracle):
    orc = oracle.lib
    flip = lambda b, at: b[:at] + bytes([b[at] ^ 0x10]) + b[at + 1:]                     # noqa: E731
    for v in dm.rfc_vectors():
        sk, pk, m, c, f, sig = (v[k] for k in ("sk", "pk", "mprime", "context", "flag", "sig"))
        one = lambda b: arr([b])                                                         # noqa: E731
        for device in (False, True):
            assert run(engine, "sign", f, device, one(sk), one(pk), [m], c).tobytes() == sig, (v["name"], device)
            accepts = lambda s, p, mm, cc, ff=f: bool(run(engine, "verify", ff, device, one(s), one(p), [mm], cc)[0])   # noqa: E731
            assert accepts(sig, pk, m, c), (v["name"], device)
            for other in (b"fo", b"foo"[:len(c)] + b"o", b"", b"fooo", b"x" * 255):
                assert accepts(sig, pk, m, other) == (other == c), (v["name"], device, other)
            assert not accepts(flip(sig, 5), pk, m, c) and not accepts(flip(sig, 37), pk, m, c)
            assert not accepts(sig, flip(pk, 9), m, c) and not accepts(sig, pk, flip(m, len(m) - 1), c)
            # the flag: a 64-byte M' is a message to one form and a prehash to the other; neither accepts the other's signature
            m64 = dm.sha(b"either a message or a prehash")
            for ff in (CTX, PH):
                s64 = run(engine, "sign", ff, device, one(sk), one(pk), [m64], c).tobytes()
                assert s64 == dm.sign(orc, sk, pk, m64, ff, c)
                assert accepts(s64, pk, m64, c, ff) and not accepts(s64, pk, m64, c, 1 - ff)
            # plain Ed25519 against Ed25519ctx, both ways (dom2(0, "") is still a prefix)
            plain = oracle.sign(sk, pk, m64)
            assert oracle.verify(plain, pk, m64) and bool(engine.ed25519_verify_batch(one(plain), one(pk), one(m64))[0])
            ctx_sig = run(engine, "sign", CTX, device, one(sk), one(pk), [m64], b"").tobytes()
            for cc in (b"", c, b"foo"):
                assert not accepts(plain, pk, m64, cc, CTX) and not accepts(plain, pk, m64, cc, PH)
            assert accepts(ctx_sig, pk, m64, b"", CTX)
            assert not bool(engine.ed25519_verify_batch(one(ctx_sig), one(pk), one(m64))[0])
            assert not bool(engine.ed25519_verify_batch(dev(one(ctx_sig)), dev(one(pk)), dev(one(m64))).cpu().numpy()[0])


# ---------------------------------------------------------------- sign against the model

# 1, 65: four lanes per item with a partial tile; 16 384 | 16 385: POINT_SPLIT_MAX_N; the last: more tiles than resident blocks,
# the persistent shape (POINT_MAX_BLOCKS * POINT_BLOCK = 131 072)
@pytest.mark.parametrize("n", [1, 65, 16384, 16385, 131072 + 512 + 77])
def test_sign_against_the_model(engine, oracle, n):
    orc = oracle.lib
    rng = np.random.default_rng(n)
    sk, pk = dm.keys(orc, n, seed=n + 1)
    context = bytes(rng.integers(0, 256, int(rng.integers(1, 256)), dtype=np.uint8))
    for flag in (CTX, PH) if n < 100000 else (CTX,):   # (the persistent shape: one call)
        rows = rows_of(rng, n, 64 if flag == PH else 45)
        device = n > 100 or flag == PH                 # the small ctx calls through the staging pipeline, everything else in HBM
        sig = run(engine, "sign", flag, device, sk, pk, rows, context)
        check_signatures(engine, orc, sig, sk, pk, rows, flag, context)
    if n <= 65:
        for flag, device in ((CTX, True), (PH, False)):
            rows = rows_of(rng, n, 64)
            check_signatures(engine, orc, run(engine, "sign", flag, device, sk, pk, rows, context), sk, pk, rows, flag, context)


# ---------------------------------------------------------------- contexts and lengths

@pytest.fixture(scope="module")
def sweep_keys(oracle):
    sk, pk = dm.keys(oracle.lib, 310, seed=310)
    sk.setflags(write=False); pk.setflags(write=False)
    return sk, pk


@pytest.mark.parametrize("clen", [0, 1, 2, 3, 30, 94, 95, 222, 255])
def test_context_and_length_sweep(engine, oracle, sweep_keys, clen):
    """per context length: 310 ragged items of 0..309 bytes packed back to back (every alignment of the item pointer), and fixed
    lengths 0 and 32; sign checked against the model, verify against ed25519_verify_digests, one item in eight corrupted.  The
    host and the device forms take turns over the contexts; each context runs both in one of the two operations."""
    orc = oracle.lib
    sk, pk = sweep_keys
    rng = np.random.default_rng(1000 + clen)
    context = bytes(rng.integers(0, 256, clen, dtype=np.uint8))
    sign_on_device = clen % 2 == 0
    blob = rng.integers(0, 256, 310 * 309 // 2, dtype=np.uint8).tobytes()
    ragged = [blob[i * (i - 1) // 2:i * (i + 1) // 2] for i in range(310)]
    assert [len(r) for r in ragged] == list(range(310))
    for rows, is_ragged in ((ragged, True), ([b""] * 310, False), (rows_of(rng, 310, 32), False)):
        sig = run(engine, "sign", CTX, sign_on_device, sk, pk, rows, context, ragged=is_ragged)
        check_signatures(engine, orc, sig, sk, pk, rows, CTX, context, modelled=310 if is_ragged else 20)
        bsig, bpk, brows = corrupt(sig, pk, rows, seed=clen)
        got = run(engine, "verify", CTX, not sign_on_device, bsig, bpk, brows, context, ragged=is_ragged)
        check_verdicts(engine, got, bsig, bpk, brows, CTX, context)
    rows = rows_of(rng, 310, 64)
    sig = run(engine, "sign", PH, not sign_on_device, sk, pk, rows, context)
    check_signatures(engine, orc, sig, sk, pk, rows, PH, context, modelled=20)
    bsig, bpk, brows = corrupt(sig, pk, rows, seed=clen + 1)
    check_verdicts(engine, run(engine, "verify", PH, sign_on_device, bsig, bpk, brows, context), bsig, bpk, brows, PH, context)


# ---------------------------------------------------------------- verify call sizes

# 63 | 64 | 65 and 257: a wave and a tile, one more; 4099 ragged: MSG_ORDER_MIN_N, the hash kernel runs over the length permutation;
# 24 576 + 333: the four-lane preparation gives way to the one-lane one
@pytest.mark.parametrize("n,ragged", [(1, False), (63, False), (64, False), (65, False), (257, False), (4099, True), (24576 + 333, False)])
def test_verify_call_sizes(engine, oracle, n, ragged):
    rng = np.random.default_rng(7 * n)
    sk, pk = dm.keys(oracle.lib, n, seed=n + 3)
    context = b"size " + str(n).encode()
    if ragged:
        lens = rng.integers(0, 700, n)
        blob = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8).tobytes()
        ends = np.cumsum(lens)
        rows = [blob[int(e - k):int(e)] for e, k in zip(ends, lens)]
    else:
        rows = rows_of(rng, n, 32)
    sig = run(engine, "sign", CTX, True, sk, pk, rows, context, ragged=ragged)
    bsig, bpk, brows = corrupt(sig, pk, rows, seed=n)
    for device in (True, False):
        got = run(engine, "verify", CTX, device, bsig, bpk, brows, context, ragged=ragged)
        check_verdicts(engine, got, bsig, bpk, brows, CTX, context)
    pre = rows_of(rng, n, 64)
    psig = run(engine, "sign", PH, True, sk, pk, pre, context)
    bsig, bpk, bpre = corrupt(psig, pk, pre, seed=n + 1)
    check_verdicts(engine, run(engine, "verify", PH, True, bsig, bpk, bpre, context), bsig, bpk, bpre, PH, context)


# ---------------------------------------------------------------- long items

def test_long_items_behind_an_unaligned_prefix(engine, oracle):
    """lengths 8191, 8192 and 65 553 among short ones in one ragged call: the blocks wholly inside such a message take the
    full-block path from a pointer that the prefix (34 + 3 bytes here, then 34 + 94) and the neighbours leave at any alignment"""
    orc = oracle.lib
    lens = [5, 8191, 0, 8192, 3, 65553, 1, 127, 128, 129, 8191, 2, 8192] + list(range(60))
    n = len(lens)
    rng = np.random.default_rng(65553)
    sk, pk = dm.keys(orc, n, seed=65553)
    rows = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in lens]
    for context, device in ((b"foo", True), (bytes(range(94)), False)):
        sig = run(engine, "sign", CTX, device, sk, pk, rows, context, ragged=True)
        check_signatures(engine, orc, sig, sk, pk, rows, CTX, context, modelled=n)
        bsig, bpk, brows = corrupt(sig, pk, rows, seed=n)
        got = run(engine, "verify", CTX, device, bsig, bpk, brows, context, ragged=True)
        check_verdicts(engine, got, bsig, bpk, brows, CTX, context)


# ---------------------------------------------------------------- the strict rules

def test_the_verify_policy_applies(engine, oracle):
    orc = oracle.lib
    sk, pk = dm.keys(orc, 9, seed=99)
    rows = rows_of(np.random.default_rng(5), 9, 20)
    sig = run(engine, "sign", CTX, True, sk, pk, rows, b"policy")
    for i in (2, 7):                                # S + l: a second encoding of the same signature
        s = dm.num(sig[i, 32:].tobytes()) + L
        assert s < 2**256
        sig[i, 32:] = np.frombuffer(dm.le(s), np.uint8)
    strict = np.ones(9, np.uint8); strict[[2, 7]] = 0
    try:
        for device in (False, True):
            engine.set_verify_policy(0)
            assert run(engine, "verify", CTX, device, sig, pk, rows, b"policy").all()
            engine.set_verify_policy(engine.VERIFY_STRICT)
            assert np.array_equal(run(engine, "verify", CTX, device, sig, pk, rows, b"policy"), strict)
    finally:
        engine.set_verify_policy(0)


# ---------------------------------------------------------------- secrets

def test_secrets_do_not_outlive_the_sign_calls(engine, oracle):
    """after host- and device-pointer ctx and ph sign calls - one item, and a batch of the one-lane shape - the scalar workspace
    (a, r between the three kernels) and the staging copies of the secret keys read zero, as after ed25519_sign_batch
    (tests/test_gpu_multi.py)"""
    import torch
    sk, pk = dm.keys(oracle.lib, 20000, seed=4)
    rng = np.random.default_rng(4)
    rows, pre = rows_of(rng, 20000, 40), rows_of(rng, 20000, 64)
    try:
        for n in (1, 20000):
            engine.shutdown()
            run(engine, "sign", CTX, False, sk[:n], pk[:n], rows[:n], b"secrets")
            run(engine, "sign", PH, False, sk[:n], pk[:n], pre[:n], b"secrets")
            aux, acc, stage_in, stage_out = engine.secret_residue()
            assert aux == 0 and stage_in == 0, (n, aux, stage_in)
            engine.shutdown()
            run(engine, "sign", CTX, True, sk[:n], pk[:n], rows[:n], b"secrets")
            run(engine, "sign", PH, True, sk[:n], pk[:n], pre[:n], b"secrets")
            torch.cuda.synchronize()
            aux, acc, stage_in, stage_out = engine.secret_residue()
            assert aux == 0 and stage_in == 0, (n, aux, stage_in)
    finally:
        engine.init(0)


# ---------------------------------------------------------------- errors

def test_a_long_context_is_refused_and_an_empty_batch_is_done(engine, oracle):
    """context_len 256: -hipErrorInvalidValue from all eight entry points, outputs untouched; n = 0: 0"""
    import torch
    lib = engine.library()
    sk, pk = dm.keys(oracle.lib, 4, seed=256)
    msg, pre = arr(rows_of(np.random.default_rng(1), 4, 32)), arr(rows_of(np.random.default_rng(2), 4, 64))
    context = ctypes.c_char_p(b"c" * 256)
    size = ctypes.c_size_t
    for n, clen, want in ((4, 256, INVALID_VALUE), (0, 3, 0), (0, 0, 0)):
        for name, first_w, out_w in (("ed25519ctx_sign_batch", 32, 64), ("ed25519ctx_verify_batch", 64, 1),
                                     ("ed25519ph_sign_batch", 32, 64), ("ed25519ph_verify_batch", 64, 1)):
            first = sk if first_w == 32 else np.zeros((4, 64), np.uint8)
            body = [msg, None, size(32)] if "ctx" in name else [pre]
            out = np.full((4, out_w), 0xAA, np.uint8)
            ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p) if isinstance(a, np.ndarray) else a   # noqa: E731
            rc = getattr(lib, name)(ptr(out), ptr(first), ptr(pk), *[ptr(b) for b in body], size(n), context, size(clen))
            assert rc == want and (out == 0xAA).all(), (name, n, clen, rc)
            dout, dfirst, dpk = dev(out), dev(first), dev(pk)
            dbody = [dev(b) if isinstance(b, np.ndarray) else b for b in body]
            dptr = lambda t: ctypes.c_void_p(t.data_ptr()) if isinstance(t, torch.Tensor) else t   # noqa: E731
            rc = getattr(lib, name + "_dev")(dptr(dout), dptr(dfirst), dptr(dpk), *[dptr(b) for b in dbody], size(n), context, size(clen), None)
            torch.cuda.synchronize()
            assert rc == want and bool((dout == 0xAA).all()), (name + "_dev", n, clen, rc)
    # NULL is a context of length 0
    one = lambda a: a[:1].copy()                                                          # noqa: E731
    out = np.zeros((1, 64), np.uint8)
    rc = lib.ed25519ctx_sign_batch(out.ctypes.data_as(ctypes.c_void_p), one(sk).ctypes.data_as(ctypes.c_void_p), one(pk).ctypes.data_as(ctypes.c_void_p),
                                   one(msg).ctypes.data_as(ctypes.c_void_p), None, size(32), size(1), None, size(0))
    assert rc == 0 and out.tobytes() == dm.sign(oracle.lib, sk[0].tobytes(), pk[0].tobytes(), msg[0].tobytes(), CTX, b"")
