"""GPU parity tests: every entry point of the C-ABI (through the ctypes mirror) against the
committed golden vectors and against the oracle on seeded random batches.  Bit-exact."""
import hashlib
import os

import numpy as np
import pytest

from ed_model import D, H, L, P, arr, inv, le
from gen_golden import golden_msg  # tools/ is on sys.path (conftest)
from gpu_kit import dev
from hostlib import ROOT, build_c_program

pytestmark = pytest.mark.gpu


def ragged(msgs):
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    blob = np.frombuffer(b"".join(msgs), np.uint8).copy() if off[-1] else np.zeros(0, np.uint8)
    return blob, off


# ---------------------------------------------------------------- golden vectors

def test_x25519_reference_table(engine, golden):
    raw = np.frombuffer(golden("x25519_table.bin"), np.uint8).reshape(1024, 96)
    pt, sc, res = raw[:, :32].copy(), raw[:, 32:64].copy(), raw[:, 64:].copy()
    assert np.array_equal(engine.x25519_batch(sc, pt), res)                    # host-pointer path
    assert np.array_equal(engine.x25519_batch(dev(sc), dev(pt)).cpu().numpy(), res)   # device-pointer path
    for i in (0, 1, 2, 500, 1023):                                             # eddsa.h surface
        assert engine.x25519(sc[i].tobytes(), pt[i].tobytes()) == res[i].tobytes()
        assert engine.DH(sc[i].tobytes(), pt[i].tobytes()) == res[i].tobytes()


def test_ed25519_table(engine, golden):
    raw = np.frombuffer(golden("ed25519_table.bin"), np.uint8).reshape(1024, 128)
    sk, pk, sig = raw[:, :32].copy(), raw[:, 32:64].copy(), raw[:, 64:].copy()
    msgs = [golden_msg(i) for i in range(1024)]          # entry i signs a message of i bytes
    blob, off = ragged(msgs)
    assert np.array_equal(engine.ed25519_genpub_batch(sk), pk)
    assert np.array_equal(engine.ed25519_sign_batch(sk, pk, blob, msg_off=off), sig)
    assert engine.ed25519_verify_batch(sig, pk, blob, msg_off=off).all()
    import torch
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    assert np.array_equal(engine.ed25519_sign_batch(dev(sk), dev(pk), dev(blob), msg_off=d_off).cpu().numpy(), sig)
    assert engine.ed25519_verify_batch(dev(sig), dev(pk), dev(blob), msg_off=d_off).all()
    for i in (0, 1, 47, 48, 111, 112, 1023):
        s, p_, g = sk[i].tobytes(), pk[i].tobytes(), sig[i].tobytes()
        assert engine.ed25519_genpub(s) == p_ and engine.eddsa_genpub(s) == p_
        assert engine.ed25519_sign(s, p_, msgs[i]) == g and engine.eddsa_sign(s, p_, msgs[i]) == g
        assert engine.ed25519_verify(g, p_, msgs[i]) and engine.eddsa_verify(g, p_, msgs[i])
        assert not engine.ed25519_verify(g, p_, msgs[i] + b"x")


def test_verify_edge_cases(engine, golden):
    cases = golden("verify_edges.json")
    blob, off = ragged([H(c["msg"]) for c in cases])
    got = engine.ed25519_verify_batch(arr([H(c["sig"]) for c in cases]), arr([H(c["pub"]) for c in cases]),
                                      blob, msg_off=off)
    want = np.array([c["accept"] for c in cases], np.uint8)
    bad = [cases[i]["name"] for i in np.nonzero(got != want)[0]]
    assert not bad, bad
    assert want.sum() >= 30 and (1 - want).sum() >= 100


def test_layer_kats_through_the_abi(engine, golden):
    k = golden("layer_kats.json")
    for name, fn in (("pk_to_x", engine.pk_ed25519_to_x25519_batch), ("sk_to_x", engine.sk_ed25519_to_x25519_batch),
                     ("x25519_base", engine.x25519_base_batch)):
        ins, outs = arr([H(a) for a, _ in k[name]]), arr([H(r) for _, r in k[name]])
        assert np.array_equal(fn(ins), outs), name
        assert np.array_equal(fn(dev(ins)).cpu().numpy(), outs), name
    a, r = k["pk_to_x"][5]
    assert engine.pk_ed25519_to_x25519(H(a)) == H(r) and engine.eddsa_pk_eddsa_to_dh(H(a)) == H(r)
    a, r = k["sk_to_x"][5]
    assert engine.sk_ed25519_to_x25519(H(a)) == H(r) and engine.eddsa_sk_eddsa_to_dh(H(a)) == H(r)
    a, r = k["x25519_base"][5]
    assert engine.x25519_base(H(a)) == H(r)


def test_device_tables_equal_the_reference_table(engine, oracle, golden):
    """the tables generated on the device: comb[i][k] = (k+1) * 4096^i * B (row 0 = the first row of the
    reference's lib/ed_lookup64.h, every entry against the oracle's k * B) and base16[k] = k * B"""
    import ctypes
    base16 = np.zeros((32769, 32), np.uint32); comb = np.zeros((704, 32), np.uint32)
    rc = engine.library().eddsa_amd_dump_tables(base16.ctypes.data_as(ctypes.c_void_p), comb.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    pos = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]

    def val(limbs):
        return sum(int(v) << s for v, s in zip(limbs, pos))

    def enc(entry):
        ymx, ypx = val(entry[0:10]), val(entry[10:20])
        y, x = (ypx + ymx) * inv(2) % P, (ypx - ymx) * inv(2) % P
        assert val(entry[20:30]) == 2 * D * x * y % P
        return le(y | (x & 1) << 255)

    pts = golden("comb_points.bin")
    out = ctypes.create_string_buffer(32)
    for e in range(704):
        oracle.lib.orc_ed_scale_base(out, int((e % 32 + 1) * 4096 ** (e // 32) % L).to_bytes(32, "little"))
        assert enc(comb[e]) == out.raw, e
    for k in range(1, 9):                                  # base16[k] = k*B = comb row 0 = the reference's row 0
        assert enc(comb[k - 1]) == pts[32 * (k - 1):32 * k]
        assert enc(base16[k]) == pts[32 * (k - 1):32 * k]
    assert val(base16[0][0:10]) == 1 and val(base16[0][10:20]) == 1 and val(base16[0][20:30]) == 0
    out = ctypes.create_string_buffer(32)                  # every 97th entry and the last against the oracle's k*B
    for k in list(range(9, 32769, 97)) + [256, 32767, 32768]:
        oracle.lib.orc_ed_scale_base(out, int(k).to_bytes(32, "little"))
        assert enc(base16[k]) == out.raw, k


# ---------------------------------------------------------------- seeded random batches vs the oracle

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 5000])
def test_x25519_random(engine, oracle, n):
    rng = np.random.default_rng(100 + n)
    sc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pt = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for i, v in enumerate([0, 1, 9, P - 1, P, P + 1, 2**255 - 1, 2**255, 2**256 - 1,
                           325606250916557431795983626356110631294008115727848805560023387167927233504,  # order 8
                           39382357235489614581723060781553021112529911719440698176882885853963445705823][:n]):
        pt[i] = np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)
    want = oracle.x25519_batch(sc, pt)
    assert np.array_equal(engine.x25519_batch(sc, pt), want)
    assert np.array_equal(engine.x25519_batch(dev(sc), dev(pt)).cpu().numpy(), want)


@pytest.mark.parametrize("mlen", [0, 1, 31, 32, 47, 48, 63, 64, 111, 112, 175, 176, 300])
def test_sign_verify_random_fixed_length(engine, oracle, mlen):
    n = 700
    rng = np.random.default_rng(200 + mlen)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (n, max(mlen, 1)), dtype=np.uint8)[:, :mlen].copy()
    pk = oracle.genpub_batch(sk)
    assert np.array_equal(engine.ed25519_genpub_batch(sk), pk)
    sig = oracle.sign_batch(sk, pk, msg, mlen)
    assert np.array_equal(engine.ed25519_sign_batch(sk, pk, msg, msg_len=mlen), sig)
    assert np.array_equal(engine.ed25519_sign_batch(dev(sk), dev(pk), dev(msg), msg_len=mlen).cpu().numpy(), sig)
    # corrupt a third of the items in assorted places, add garbage and S + l
    s2, p2, m2 = sig.copy(), pk.copy(), msg.copy()
    for i in range(n):
        k = i % 9
        if k == 1: s2[i, rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)
        elif k == 2: s2[i, 32 + rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)
        elif k == 3: p2[i, rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)
        elif k == 4 and mlen: m2[i, rng.integers(0, mlen)] ^= 1 << rng.integers(0, 8)
        elif k == 5: s2[i] = rng.integers(0, 256, 64); p2[i] = rng.integers(0, 256, 32)
        elif k == 6:
            s = int.from_bytes(s2[i, 32:].tobytes(), "little") + L * int(rng.integers(1, 15))
            if s < 2**256: s2[i, 32:] = np.frombuffer(s.to_bytes(32, "little"), np.uint8)
    want = oracle.verify_batch(s2, p2, m2, mlen)
    assert np.array_equal(engine.ed25519_verify_batch(s2, p2, m2, msg_len=mlen), want)
    assert np.array_equal(engine.ed25519_verify_batch(dev(s2), dev(p2), dev(m2), msg_len=mlen).cpu().numpy(), want)
    assert 0 < want.sum() < n


def test_off_curve_keys_take_the_exact_path(engine, oracle):
    """public keys that do not decode to curve points (about half of random 32-byte strings) are
    evaluated by k_verify_exact in the reference's own operation order; verdicts equal the oracle's,
    which reproduces the reference's chain byte for byte on such inputs"""
    n = 6000
    rng = np.random.default_rng(4242)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (n, 40), dtype=np.uint8)
    pk = oracle.genpub_batch(sk)
    sig = oracle.sign_batch(sk, pk, msg, 40)
    pk[::2] = rng.integers(0, 256, (n // 2, 32), dtype=np.uint8)        # garbage keys under genuine signatures
    sig[1::4, :32] = 0                                                   # R = 32 zero bytes ...
    sig[1::4, 32:] = rng.integers(0, 256, (len(sig[1::4]), 32), dtype=np.uint8)
    pk[1::4] = rng.integers(0, 256, (len(pk[1::4]), 32), dtype=np.uint8)  # ... under garbage keys (the Z = 0 corner)
    want = oracle.verify_batch(sig, pk, msg, 40)
    assert np.array_equal(engine.ed25519_verify_batch(sig, pk, msg, msg_len=40), want)
    assert np.array_equal(engine.ed25519_verify_batch(dev(sig), dev(pk), dev(msg), msg_len=40).cpu().numpy(), want)
    assert want[3::4].all() and not want[::2].any()
    # reject mode: the same verdicts (the two modes can differ only on a SHA-512 fixed point)
    engine.set_offcurve_mode(False)
    try:
        assert np.array_equal(engine.ed25519_verify_batch(sig, pk, msg, msg_len=40), want)
    finally:
        engine.set_offcurve_mode(True)


@pytest.mark.parametrize("n", [1 << 16, (1 << 18) + 77])
def test_both_forms_of_the_exact_path_around_their_threshold(engine, oracle, n):
    """Which form replays the reference's chain for the keys that are no curve points is decided on the device by the length of
    the work list: below 8192 entries the four-lane chain (k_verify_exact_quad), from there on one lane per item
    (k_verify_exact_lane_setup / _chain; csrc/kernels.hip: EXACT_LANE_MIN_LISTED).  Passes with exactly 8191, 8192 and 8193 such
    keys - and none, and one - on both routes that have the choice (2^16 items: three-lane preparation; 2^18 + 77: one lane per
    item), genuine signatures and R = 0 under the bad keys: every verdict as the oracle's"""
    rng = np.random.default_rng(n)
    m = 4096
    sk = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    pk = oracle.genpub_batch(sk)
    sig = oracle.sign_batch(sk, pk, msg, 32)
    reps = (n + m - 1) // m
    sig_n, pk_n, msg_n = (np.tile(a, (reps, 1))[:n].copy() for a in (sig, pk, msg))
    # 8200 distinct strings that are no curve points (the probe library's ed_import reports the flag)
    engine.debug_init(0, True)
    try:
        cand = rng.integers(0, 256, (20000, 32), dtype=np.uint8)
        flags = engine.debug_layer("ed_import_export", [bytes(r) for r in cand], 33)
    finally:
        engine.debug_init(0, False)
    off = cand[np.array([f[32] == 0 for f in flags])][:8200]
    assert len(off) == 8200
    spots = rng.permutation(n)[:8200]
    for k in (0, 1, 8191, 8192, 8193):
        keys, s2 = pk_n.copy(), sig_n.copy()
        keys[spots[:k]] = off[:k]
        s2[spots[:k:5], :32] = 0                     # R = 0 under some of them (the Z = 0 corner of the chain)
        want = oracle.verify_batch(s2, keys, msg_n, 32)
        assert want.sum() == n - k
        assert np.array_equal(engine.ed25519_verify_batch(dev(s2), dev(keys), dev(msg_n), msg_len=32).cpu().numpy(), want), k


def test_every_route_with_two_thirds_of_the_keys_random(engine, oracle):
    """a pass of 2^17 items whose work list is long (a third of the keys are no curve points: the two-items-per-lane chain) on every
    evaluation the library has - the default arrangement of that size, full-length windows (whose main kernel runs over the whole
    pass beside the chain), half-length with one lane per item, the mid-size arrangement: the same verdict bytes, and the oracle's"""
    import workload
    n = 1 << 17
    sk, msg = workload.sign_inputs(n, seed=5, config=2)
    pk = engine.ed25519_genpub_batch(dev(sk))
    sig = engine.ed25519_sign_batch(dev(sk), pk, dev(msg))
    rng = np.random.default_rng(17)
    keys = pk.cpu().numpy().copy()
    sel = rng.permutation(n)[: n * 2 // 3]
    keys[sel] = rng.integers(0, 256, (len(sel), 32), dtype=np.uint8)
    want = oracle.verify_batch(sig.cpu().numpy(), keys, msg, 32)
    assert 0 < want.sum() < n
    try:
        for algo in (0, 1, 2, 3):
            engine.set_verify_algo(algo)
            assert np.array_equal(engine.ed25519_verify_batch(sig, dev(keys), dev(msg), msg_len=32).cpu().numpy(), want), algo
    finally:
        engine.set_verify_algo(0)


def test_a_lost_hand_off_between_the_chain_s_waves_is_an_error_not_a_hang(engine, oracle):
    """The waves of k_verify_exact_lane_chain hand a tile's accumulators to one another through memory, and a wave that drew
    stretch s waits for stretch s - 1.  The wait is bounded: with the test hook withholding the first hand-off of tile 0, the
    wave that waits for it gives up after its bound (seconds), the launch drains, and the pass comes back as
    EDDSA_AMD_STALLED - through the host-pointer call that ran it, and through the NEXT device-pointer call after one whose
    kernels stalled (that call had returned before its kernels ran).  Afterwards the engine serves the same pass correctly."""
    import torch
    import workload
    n = 1 << 16
    sk, msg = workload.sign_inputs(n, seed=21, config=2)
    pk = engine.ed25519_genpub_batch(dev(sk))
    sig = engine.ed25519_sign_batch(dev(sk), pk, dev(msg)).cpu().numpy()
    keys = pk.cpu().numpy().copy()
    keys[::2] = np.random.default_rng(21).integers(0, 256, (n // 2, 32), dtype=np.uint8)     # ~15 000 keys off the curve: the one-lane form
    want = oracle.verify_batch(sig, keys, msg, 32)
    assert np.array_equal(engine.ed25519_verify_batch(dev(sig), dev(keys), dev(msg)).cpu().numpy(), want)   # (allocates the workspace)
    assert engine.debug_withhold_handoff(1) == engine.HOOKS_OFF                                # inert until armed
    engine.debug_init(0, True)
    try:
        assert engine.debug_withhold_handoff(1) >= 0
        with pytest.raises(engine.EddsaAmdError) as err:
            engine.ed25519_verify_batch(sig, keys, msg)                                          # host pointers: this call reports it
        assert f"rc={engine.STALLED}" in str(err.value)
        engine.ed25519_verify_batch(dev(sig), dev(keys), dev(msg))                              # device pointers: returns before its kernels give up
        torch.cuda.synchronize()
        assert engine.debug_withhold_handoff(0) >= 0
        with pytest.raises(engine.EddsaAmdError) as err:
            engine.ed25519_verify_batch(dev(sig), dev(keys), dev(msg))                          # ... so the next call carries the report
        assert f"rc={engine.STALLED}" in str(err.value)
    finally:
        engine.debug_withhold_handoff(0)
        engine.debug_init(0, False)
    assert np.array_equal(engine.ed25519_verify_batch(dev(sig), dev(keys), dev(msg)).cpu().numpy(), want)
    assert np.array_equal(engine.ed25519_verify_batch(sig, keys, msg), want)


def test_the_hand_off_under_concurrency(engine, oracle):
    """a short run of tools/exact_soak.py inside the suite: the passes "every second key random" and "just above the
    threshold of the one-lane form" from two host threads on two streams at once, 12 times each - every verdict vector
    equal to the oracle's"""
    import threading
    import torch
    import workload
    n = 1 << 18
    sk, msg = workload.sign_inputs(n, seed=22, config=2)
    pk = engine.ed25519_genpub_batch(dev(sk))
    sig = engine.ed25519_sign_batch(dev(sk), pk, dev(msg))
    dm = dev(msg)
    garbage = np.random.default_rng(22).integers(0, 256, (n, 32), dtype=np.uint8)
    cases = {}
    for tag, sel in (("every second", slice(0, n, 2)), ("just above the threshold", slice(0, 20000))):
        keys = pk.cpu().numpy().copy()
        keys[sel] = garbage[sel]
        cases[tag] = (dev(keys), torch.from_numpy(oracle.verify_batch(sig.cpu().numpy(), keys, msg, 32)).cuda())
    errs = []

    def worker(tag):
        keys, want = cases[tag]
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            for r in range(12):
                ok = engine.ed25519_verify_batch(sig, keys, dm)
                s.synchronize()
                if not torch.equal(ok, want):
                    errs.append((tag, r, int((ok != want).sum())))
    ts = [threading.Thread(target=worker, args=(t,)) for t in cases]
    for t in ts: t.start()
    for t in ts: t.join()
    assert not errs, errs[:5]


def test_every_item_through_the_reference_order_kernels(engine):
    """self-check mode 2: all 70 000 items (more than the 65 536 the setup/chain kernels take, so the
    strided k_verify_exact runs too) are decided by the replay of the reference's JSF/Shamir chain;
    genuine and corrupted signatures get the verdicts the windowed kernels give them"""
    import workload
    n = 70000
    sk, msg = workload.sign_inputs(n, seed=11, config=2)
    pk = engine.ed25519_genpub_batch(dev(sk))
    sig = engine.ed25519_sign_batch(dev(sk), pk, dev(msg)).cpu().numpy()
    pk = pk.cpu().numpy()
    expect = workload.corrupt_for_verify(sig, pk, msg)
    windowed = engine.ed25519_verify_batch(dev(sig), dev(pk), dev(msg), msg_len=32).cpu().numpy()
    assert np.array_equal(windowed, expect) and 0 < expect.sum() < n
    engine.set_offcurve_mode(2)
    try:
        replay = engine.ed25519_verify_batch(dev(sig), dev(pk), dev(msg), msg_len=32).cpu().numpy()
    finally:
        engine.set_offcurve_mode(True)
    assert np.array_equal(replay, expect)


@pytest.mark.parametrize("stride,sig_off,pub_off,msg_off,mlen", [(128, 0, 64, 96, 32), (137, 41, 5, 105, 32),
                                                                 (160, 96, 64, 0, 61), (96, 0, 64, 96, 0)])
def test_verify_records(engine, oracle, stride, sig_off, pub_off, msg_off, mlen):
    """fixed-size (sig, pub, msg) records: same verdicts as the packed arrays and as the oracle, on the
    host path and on the device path, aligned and unaligned layouts, empty messages"""
    import workload
    n = 3000
    rng = np.random.default_rng(stride)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (n, mlen), dtype=np.uint8)
    pk = oracle.genpub_batch(sk)
    sig = oracle.sign_batch(sk, pk, msg, mlen)
    sig[::7, 3] ^= 1; pk[3::11, 9] ^= 0x40                       # some corrupt signatures and keys (off-curve ones too)
    if mlen:
        msg[5::13, 0] ^= 2
    rec = rng.integers(0, 256, (n, stride), dtype=np.uint8)      # garbage between the fields
    rec[:, sig_off:sig_off + 64] = sig
    rec[:, pub_off:pub_off + 32] = pk
    rec[:, msg_off:msg_off + mlen] = msg
    want = oracle.verify_batch(sig, pk, msg, mlen)
    assert 0 < want.sum() < n
    assert np.array_equal(engine.ed25519_verify_records(rec, sig_off, pub_off, msg_off, mlen), want)
    assert np.array_equal(engine.ed25519_verify_records(dev(rec), sig_off, pub_off, msg_off, mlen).cpu().numpy(), want)


def test_route_boundaries_agree(engine, oracle):
    """the same items as a pass of 2^14 items and as one of 2^14 + 1 get the same verdicts, equal to the oracle's; keys on and
    off the curve.  (2^14 is the boundary between four lanes and one lane per item of the FULL-LENGTH route only - algo 1 and
    reject mode; the default route takes both passes through the same half-length four-lane kernels, and its own boundaries
    are those of test_small_route_edges_agree_with_the_oracle below and of tests/test_gpu_fuzz.py)"""
    n = (1 << 14) + 1
    rng = np.random.default_rng(99)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pk = engine.ed25519_genpub_batch(sk)
    sig = engine.ed25519_sign_batch(sk, pk, msg)
    sig[::5, 40] ^= 8
    pk[2::9] = rng.integers(0, 256, (len(pk[2::9]), 32), dtype=np.uint8)       # garbage keys: half are off the curve
    want = oracle.verify_batch(sig, pk, msg, 32)
    big = engine.ed25519_verify_batch(dev(sig), dev(pk), dev(msg), msg_len=32).cpu().numpy()
    small = engine.ed25519_verify_batch(dev(sig[:-1]), dev(pk[:-1]), dev(msg[:-1]), msg_len=32).cpu().numpy()
    assert np.array_equal(big, want) and np.array_equal(small, want[:-1]) and 0 < want.sum() < n


@pytest.fixture(scope="module")
def route_edge_items(engine, oracle):
    """2^18 items signed on the device, one signature in five corrupt and one key in nine random bytes (half of those are no
    curve points), with the oracle's verdicts - computed once: a pass of n items takes the first n"""
    n = 1 << 18
    rng = np.random.default_rng(2718)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pk = engine.ed25519_genpub_batch(dev(sk))
    sig = engine.ed25519_sign_batch(dev(sk), pk, dev(msg)).cpu().numpy()
    pk = pk.cpu().numpy()
    sig[::5, 40] ^= 8
    pk[2::9] = rng.integers(0, 256, (len(pk[2::9]), 32), dtype=np.uint8)
    return sig, pk, msg, oracle.verify_batch(sig, pk, msg, 32)


@pytest.mark.parametrize("algo,n", [(0, 256), (0, 257), (0, 2048), (0, 2049), (0, 24576), (0, 24577), (1, 16384), (1, 16385),
                                    (3, 262144)])
def test_small_route_edges_agree_with_the_oracle(engine, route_edge_items, algo, n):
    """both sides of every boundary below 2^18 items of the table in csrc/kernels.hip: verify_route_of - the default route's
    256 | 257 (pairs up to 2^134 | 2^138), 2048 | 2049 (window sums | the four-lane half-length evaluation), 24 576 | 24 577
    (four lanes | the mid-size arrangement); the full-length route's 2^14 | 2^14 + 1 (four lanes | one); and algo 3 at 2^18
    items, where the mid-size arrangement ends and the pass takes the full-length route: every verdict as the oracle's"""
    sig, pk, msg, want = (a[:n] for a in route_edge_items)
    assert 0 < want.sum() < n
    engine.set_verify_algo(algo)
    try:
        got = engine.ed25519_verify_batch(dev(sig), dev(pk), dev(msg), msg_len=32).cpu().numpy()
    finally:
        engine.set_verify_algo(0)
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def fixed_base_in_small_passes(engine):
    """2^18 + 1 secret keys, 32-byte messages and X25519 scalars, and what the three fixed-base operations give for them in
    device passes of 4096 items (four lanes per item, one block per 64 items) - computed once: a pass of n items takes the first n"""
    import torch
    n, step = (1 << 18) + 1, 4096
    rng = np.random.default_rng(3141)
    sk, msg, sc = (rng.integers(0, 256, (n, 32), dtype=np.uint8) for _ in range(3))
    d_sk, d_msg, d_sc = dev(sk), dev(msg), dev(sc)
    cuts = [slice(at, min(at + step, n)) for at in range(0, n, step)]
    pk = torch.cat([engine.ed25519_genpub_batch(d_sk[c]) for c in cuts])
    sig = torch.cat([engine.ed25519_sign_batch(d_sk[c], pk[c], d_msg[c]) for c in cuts])
    xb = torch.cat([engine.x25519_base_batch(d_sc[c]) for c in cuts])
    return sk, msg, sc, pk.cpu().numpy(), sig.cpu().numpy(), xb.cpu().numpy()


@pytest.mark.parametrize("n", [16384, 16385, 32769, 65537, 131072, 131073, 262145])
def test_fixed_base_launch_shapes(engine, oracle, fixed_base_in_small_passes, n):
    """ed25519_genpub_batch, ed25519_sign_batch and x25519_base_batch as ONE device pass of n items, on both sides of every
    change of the launch shape (csrc/kernels.hip: point_shape_of, finish_shape_of): 2^14 | 2^14 + 1 four lanes per item | one, in
    blocks of 128 lanes; 2^15 + 1 blocks of 256; 2^16 + 1 blocks of 512 and two items per lane in the finish kernels; 2^17 |
    2^17 + 1 a block per tile | persistent blocks that draw their tiles, and four items per lane; 2^18 + 1 eight.  Every byte as
    in passes of 4096 items, and the first and last 256 items as the oracle's"""
    sk, msg, sc, pk_small, sig_small, xb_small = (a[:n] for a in fixed_base_in_small_passes)
    pk = engine.ed25519_genpub_batch(dev(sk))
    sig = engine.ed25519_sign_batch(dev(sk), pk, dev(msg)).cpu().numpy()
    pk = pk.cpu().numpy()
    xb = engine.x25519_base_batch(dev(sc)).cpu().numpy()
    assert np.array_equal(pk, pk_small) and np.array_equal(sig, sig_small) and np.array_equal(xb, xb_small)
    for ends in (slice(0, 256), slice(n - 256, n)):
        e_sk, e_msg = np.ascontiguousarray(sk[ends]), np.ascontiguousarray(msg[ends])
        e_pk = oracle.genpub_batch(e_sk)
        assert np.array_equal(pk[ends], e_pk)
        assert np.array_equal(sig[ends], oracle.sign_batch(e_sk, e_pk, e_msg, 32))
        assert [bytes(r) for r in xb[ends]] == [oracle.x25519_base(bytes(s)) for s in sc[ends]]


def test_unaligned_device_buffers(engine, oracle):
    """device pointers that are not 16-byte aligned take the byte-wise load/store path"""
    import torch
    n = 300
    rng = np.random.default_rng(77)
    sc = rng.integers(0, 256, (n, 32), dtype=np.uint8); pt = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    want = oracle.x25519_batch(sc, pt)
    for shift in (1, 3, 4, 8):
        bs = torch.zeros(n * 32 + 16, dtype=torch.uint8, device="cuda"); bp = torch.zeros_like(bs)
        s = bs[shift:shift + n * 32]; p_ = bp[shift:shift + n * 32]
        s.copy_(dev(sc).view(-1)); p_.copy_(dev(pt).view(-1))
        assert np.array_equal(engine.x25519_batch(s, p_).cpu().numpy(), want), shift
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8); msg = rng.integers(0, 256, (n, 33), dtype=np.uint8)
    pk = oracle.genpub_batch(sk); sig = oracle.sign_batch(sk, pk, msg, 33)     # 33-byte stride: unaligned msgs
    assert np.array_equal(engine.ed25519_sign_batch(dev(sk), dev(pk), dev(msg), msg_len=33).cpu().numpy(), sig)
    assert engine.ed25519_verify_batch(dev(sig), dev(pk), dev(msg), msg_len=33).all()


def test_device_calls_on_several_streams(engine, oracle):
    """host threads that each own a stream use different workspaces of the pool and overlap on the
    GPU: six threads (more than the pool has slots), mixed operations and sizes, all results right"""
    import threading
    import torch
    rng = np.random.default_rng(31)
    jobs = []
    for k in range(6):
        n = int(rng.choice([300, 5000, 20000, 70000]))
        sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        msg = rng.integers(0, 256, (n, 24), dtype=np.uint8)
        pk = oracle.genpub_batch(sk)
        sig = oracle.sign_batch(sk, pk, msg, 24)
        sig[::3, 1] ^= 1
        jobs.append((dev(sk), dev(pk), dev(msg), dev(sig), sig.copy(), oracle.verify_batch(sig, pk, msg, 24), pk))
    torch.cuda.synchronize()
    bad = []

    def worker(k):
        d_sk, d_pk, d_msg, d_sig, sig, want, pk = jobs[k]
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            for _ in range(4):
                ok = engine.ed25519_verify_batch(d_sig, d_pk, d_msg, msg_len=24)
                pub = engine.ed25519_genpub_batch(d_sk)
                x = engine.x25519_batch(d_sk, d_pk)
            st.synchronize()
        if not np.array_equal(ok.cpu().numpy(), want) or not np.array_equal(pub.cpu().numpy(), pk) \
                or not np.array_equal(x.cpu().numpy(), oracle.x25519_batch(d_sk.cpu().numpy(), pk)):
            bad.append(k)

    th = [threading.Thread(target=worker, args=(k,)) for k in range(6)]
    for t in th: t.start()
    for t in th: t.join()
    assert not bad


def test_shutdown_and_implicit_reinit(engine, golden):
    """eddsa_amd_shutdown releases everything; the next call builds tables and workspaces again"""
    t = np.frombuffer(golden("x25519_table.bin"), np.uint8).reshape(-1, 96)
    want = t[:64, 64:]
    assert np.array_equal(engine.x25519_batch(t[:64, 32:64].copy(), t[:64, :32].copy()), want)
    engine.shutdown()
    assert np.array_equal(engine.x25519_batch(t[:64, 32:64].copy(), t[:64, :32].copy()), want)
    sk = np.arange(32, dtype=np.uint8).reshape(1, 32)
    pk = engine.ed25519_genpub_batch(sk)
    engine.shutdown()
    sig = engine.ed25519_sign_batch(sk, pk, np.zeros((1, 5), np.uint8))
    assert engine.ed25519_verify_batch(sig, pk, np.zeros((1, 5), np.uint8))[0] == 1
    # every free / destroy / device restore of those teardowns succeeded (they are counted, not ignored)
    assert engine.debug_teardown_errors() == (0, 0)


def test_empty_batches(engine):
    z32, z64 = np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8)
    assert engine.x25519_batch(z32, z32).shape == (0, 32)
    assert engine.ed25519_verify_batch(z64, z32, np.zeros(0, np.uint8)).shape == (0,)
    assert engine.ed25519_sign_batch(z32, z32, np.zeros(0, np.uint8)).shape == (0, 64)
    assert engine.ed25519_genpub_batch(z32).shape == (0, 32)


def test_reference_selftest_consistency(engine):
    """the reference's consistency selftests on the device (test/selftest-x25519_base.c:11-45 and
    test/selftest-convert.c:9-80): x25519_base(x) == x25519(x, 9) and
    x25519_base(sk_to_x(sk)) == pk_to_x(genpub(sk))"""
    n = 1024
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    nine = np.zeros((n, 32), np.uint8); nine[:, 0] = 9
    assert np.array_equal(engine.x25519_base_batch(x), engine.x25519_batch(x, nine))
    lhs = engine.x25519_base_batch(engine.sk_ed25519_to_x25519_batch(x))
    rhs = engine.pk_ed25519_to_x25519_batch(engine.ed25519_genpub_batch(x))
    assert np.array_equal(lhs, rhs)


def test_small_batch_digests(engine, golden):
    import workload
    d = golden("batch_digests.json")
    n = 1 << 14
    sc, pt = workload.x25519_inputs(n)
    assert hashlib.sha512(engine.x25519_batch(sc, pt).tobytes()).hexdigest() == d["x25519_2^14"]
    sk, msg = workload.sign_inputs(n)
    pk = engine.ed25519_genpub_batch(sk)
    assert hashlib.sha512(pk.tobytes()).hexdigest() == d["genpub_2^14"]
    assert hashlib.sha512(engine.ed25519_sign_batch(sk, pk, msg).tobytes()).hexdigest() == d["sign_2^14"]


def test_c_program_against_eddsa_h(engine, golden, tmp_path):
    """a plain C program written against eddsa.h / eddsa_amd.h (tests/c/selftest_dropin.c: the checks
    of the reference's four selftests on the golden tables) linked against libeddsa_amd.so - the SHIPPED library, which
    exports no hook (the two programs below use the measurement surface and link libeddsa_amd_debug.so)"""
    import os
    import subprocess
    exe = build_c_program(tmp_path, "selftest_dropin.c", libs=("eddsa_amd",))
    msgs = tmp_path / "msgs.bin"
    msgs.write_bytes(b"".join(golden_msg(i) for i in range(1024)))
    r = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "x25519_table.bin"),
                        os.path.join(ROOT, "tests", "golden", "ed25519_table.bin"), str(msgs)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "selftest_dropin: ok" in r.stdout


def test_host_side_stress_program_on_the_real_runtime(engine, golden, tmp_path):
    """tests/c/host_side_stress.c - multi-chunk pipelines on small batches (ragged verify, the opt-in batch verification,
    sign, x25519), the fault hooks, 16 threads of chunked batches and single-item calls while the pipeline trace is switched on
    and off, two concurrent shutdowns beside callers, no HIP call failed on a clean-up path - against the real library and
    the real runtime, where the ordering between streams is the hardware's (the CPU suite runs the same program against the
    fake runtime under the sanitizers)"""
    import os
    import subprocess
    exe = build_c_program(tmp_path, "host_side_stress.c", libs=("eddsa_amd_debug", "dl"), threads=True)
    msgs = tmp_path / "msgs.bin"
    msgs.write_bytes(b"".join(golden_msg(i) for i in range(1024)))
    r = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "ed25519_table.bin"), str(msgs),
                        os.path.join(ROOT, "tests", "golden", "x25519_table.bin"), "16", "12"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_side_stress: ok (16 threads" in r.stdout


def test_threaded_c_application_on_the_single_item_functions(engine, golden, tmp_path):
    """VERDICT r02 missing #4: tests/c/threaded_callers.c, 64 pthreads looping over ed25519_verify (then a mix of
    verify / sign / x25519 / genpub) through eddsa.h only.  Every result must be the golden table's, and the calls must
    not run one GPU pass each: the combiner (host_pipe.c) merges what is queued for one operation into one launch -
    round 2 gave such a program about 2.4 k verifies/s in total, the reference about 20 k/s per core"""
    import os
    import re
    import subprocess
    exe = build_c_program(tmp_path, "threaded_callers.c", libs=("eddsa_amd_debug",), threads=True)
    msgs = tmp_path / "msgs.bin"
    msgs.write_bytes(b"".join(golden_msg(i) for i in range(1024)))
    r = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "ed25519_table.bin"), str(msgs),
                        os.path.join(ROOT, "tests", "golden", "x25519_table.bin"), "64", "100"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "threaded_callers: ok" in r.stdout
    print(r.stdout)
    rates = [float(x) for x in re.findall(r"= (\d+) calls/s", r.stdout)]
    assert len(rates) == 3
    # one caller is latency-bound (a pass per call); 64 callers must get far more than that in total
    assert rates[1] > 8 * rates[0] and rates[1] > 30000, r.stdout
    launches, calls = [int(x) for x in re.findall(r"(\d+) launches carried (\d+) calls", r.stdout)[-1]]
    assert calls > 4 * launches


def test_page_locked_caller_memory_is_used_in_place(engine, oracle):
    """arrays from eddsa_amd_host_alloc (1 MB and more: the size from which the library asks) are read and written by the
    DMA engines directly, inputs and outputs alike; smaller ones and ordinary memory are staged: same bytes either way"""
    import ctypes
    n = 1 << 16
    rng = np.random.default_rng(5)
    sc = rng.integers(0, 256, (n, 32), dtype=np.uint8); pt = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    want = engine.x25519_batch(sc, pt)                             # ordinary memory, staged
    assert np.array_equal(want[:500], oracle.x25519_batch(sc[:500], pt[:500]))
    hs, hp, ho = engine.host_array((n, 32)), engine.host_array((n, 32)), engine.host_array((n, 32))
    hs[...] = sc; hp[...] = pt; ho[...] = 0xEE
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib = engine.library()
    assert lib.x25519_batch(P(ho), P(hs), P(hp), ctypes.c_size_t(n)) == 0          # all three page-locked
    assert np.array_equal(ho, want)
    out = np.zeros((n, 32), np.uint8)
    assert lib.x25519_batch(P(out), P(hs), P(pt), ctypes.c_size_t(n)) == 0         # mixed: one input page-locked, the rest staged
    assert np.array_equal(out, want)
    ho[...] = 0
    assert lib.x25519_batch(P(ho), P(hs), P(hp), ctypes.c_size_t(100)) == 0        # a small call from the same buffers: staged
    assert np.array_equal(ho[:100], want[:100]) and not ho[100:].any()
    # verify with a page-locked verdict array
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8); msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pk = engine.ed25519_genpub_batch(sk); sig = engine.ed25519_sign_batch(sk, pk, msg); sig[::7, 50] ^= 2
    hsig, hok = engine.host_array((n, 64)), engine.host_array((1 << 20,))
    hsig[...] = sig
    assert lib.ed25519_verify_batch(P(hok), P(hsig), P(pk), P(msg), None, ctypes.c_size_t(32), ctypes.c_size_t(n)) == 0
    assert np.array_equal(hok[:n], (np.arange(n) % 7 != 0).astype(np.uint8))
    for a in (hs, hp, ho, hsig, hok):
        engine.host_free(a)


def test_combined_small_calls_of_many_threads(engine, oracle):
    """the combiner (host_pipe.c) under a mixed load: 24 Python threads (ctypes releases the GIL) issue host-pointer calls of
    1..64 items - verify with message lengths that differ from call to call (the combined batch becomes ragged), sign,
    x25519, genpub - while another thread runs large batches through the same pipeline; every caller gets its own results"""
    import threading
    rng = np.random.default_rng(123)
    N = 4096
    sk = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    pk = oracle.genpub_batch(sk)
    pt = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    want_x = oracle.x25519_batch(sk, pt)
    msgs = {L: rng.integers(0, 256, (N, L), dtype=np.uint8) for L in (0, 1, 31, 32, 100, 300)}
    sigs = {L: oracle.sign_batch(sk, pk, m, L) if L else np.stack([np.frombuffer(oracle.sign(sk[i].tobytes(), pk[i].tobytes(), b""), np.uint8) for i in range(N)]) for L, m in msgs.items()}
    before = engine.combiner_stats()
    errors = []

    def small(tid):
        r = np.random.default_rng(1000 + tid)
        try:
            for it in range(40):
                n = int(r.choice([1, 1, 1, 2, 5, 17, 64]))
                lo = int(r.integers(0, N - n))
                L = int(r.choice(list(msgs)))
                kind = (tid + it) % 4
                if kind == 0:
                    bad = sigs[L][lo:lo + n].copy()
                    flip = r.integers(0, 2, n).astype(bool)
                    bad[flip, 37] ^= 4
                    ok = engine.ed25519_verify_batch(bad, pk[lo:lo + n], msgs[L][lo:lo + n], msg_len=L)
                    assert np.array_equal(ok, (~flip).astype(np.uint8)), ("verify", tid, it)
                elif kind == 1:
                    got = engine.ed25519_sign_batch(sk[lo:lo + n], pk[lo:lo + n], msgs[L][lo:lo + n], msg_len=L)
                    assert np.array_equal(got, sigs[L][lo:lo + n]), ("sign", tid, it)
                elif kind == 2:
                    assert np.array_equal(engine.x25519_batch(sk[lo:lo + n], pt[lo:lo + n]), want_x[lo:lo + n]), ("x25519", tid, it)
                else:
                    assert np.array_equal(engine.ed25519_genpub_batch(sk[lo:lo + n]), pk[lo:lo + n]), ("genpub", tid, it)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    def big():
        try:
            for _ in range(6):
                assert np.array_equal(engine.x25519_batch(sk, pt), want_x)
                assert bool(engine.ed25519_verify_batch(sigs[32], pk, msgs[32], msg_len=32).all())
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=small, args=(t,)) for t in range(24)] + [threading.Thread(target=big)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]
    after = engine.combiner_stats()
    calls, launches = after[1] - before[1], after[0] - before[0]
    assert calls == 24 * 40 and launches < calls          # some calls did travel together
    # the packed copies of secret keys and shared secrets do not outlive their launch: a fresh engine, secret-key calls only
    engine.shutdown()

    def secret_only(tid):
        try:
            for it in range(10):
                lo = 50 * tid + it
                assert np.array_equal(engine.x25519_batch(sk[lo:lo + 3], pt[lo:lo + 3]), want_x[lo:lo + 3])
                assert np.array_equal(engine.ed25519_sign_batch(sk[lo:lo + 2], pk[lo:lo + 2], msgs[32][lo:lo + 2], msg_len=32), sigs[32][lo:lo + 2])
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=secret_only, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]
    res = engine.secret_residue()
    assert res[0] == 0 and res[2] == 0, res               # scalar workspace, input staging (HBM, pinned, the combiner's)


def test_edge_and_torsion_vectors_as_concurrent_single_item_calls(engine, golden):
    """the 273 edge cases and the 192 mixed-order vectors, every one as its own ed25519_verify call, issued by 16 threads
    at once: the combiner packs whatever meets into ragged batches (off-curve keys, non-canonical encodings, messages of
    0..1023 bytes side by side) and every caller must get the reference's verdict for ITS item"""
    import threading
    cases = golden("verify_edges.json") + golden("verify_torsion.json")
    items = [(bytes.fromhex(c["sig"]), bytes.fromhex(c["pub"]), bytes.fromhex(c["msg"]), bool(c["accept"]), c["name"]) for c in cases]
    wrong, before = [], engine.combiner_stats()

    def worker(t):
        for k in range(t, len(items), 16):
            sig, pub, msg, want, name = items[k]
            if engine.ed25519_verify(sig, pub, msg) != want:
                wrong.append(name)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not wrong, wrong[:5]
    after = engine.combiner_stats()
    assert after[1] - before[1] == len(items) and after[0] - before[0] < len(items)


def test_concurrent_host_threads(engine, oracle):
    """several host threads issue batched calls at once (host-pointer pipeline and device-pointer
    entry points on different torch streams): calls serialise on the engine's workspaces and every
    result is still bit-exact"""
    import threading
    import torch
    n = 3000
    rng = np.random.default_rng(99)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (n, 24), dtype=np.uint8)
    pk = oracle.genpub_batch(sk)
    sig = oracle.sign_batch(sk, pk, msg, 24)
    bad = sig.copy(); bad[::3, 40] ^= 1
    want = oracle.verify_batch(bad, pk, msg, 24)
    sc = rng.integers(0, 256, (n, 32), dtype=np.uint8); pt = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    want_x = oracle.x25519_batch(sc, pt)
    errors = []

    def host_worker():
        try:
            for _ in range(4):
                assert np.array_equal(engine.ed25519_verify_batch(bad, pk, msg, msg_len=24), want)
                assert np.array_equal(engine.ed25519_sign_batch(sk, pk, msg, msg_len=24), sig)
                assert np.array_equal(engine.x25519_batch(sc, pt), want_x)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    def dev_worker():
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                d = [dev(a) for a in (bad, pk, msg, sk, sc, pt)]
                for _ in range(4):
                    ok = engine.ed25519_verify_batch(d[0], d[1], d[2], msg_len=24)
                    sg = engine.ed25519_sign_batch(d[3], d[1], d[2], msg_len=24)
                    xo = engine.x25519_batch(d[4], d[5])
                    st.synchronize()
                    assert np.array_equal(ok.cpu().numpy(), want)
                    assert np.array_equal(sg.cpu().numpy(), sig)
                    assert np.array_equal(xo.cpu().numpy(), want_x)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=host_worker) for _ in range(2)] + [threading.Thread(target=dev_worker) for _ in range(2)]
    for t in threads: t.start()
    for t in threads: t.join()
    assert not errors, errors


def _bench_line(args, env_extra=None, launcher=None):
    import json, socket, subprocess, sys
    env = dict(os.environ, **(env_extra or {}))
    cmd = [sys.executable]
    if launcher:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(launcher),
                "--master-addr", "127.0.0.1", "--master-port", str(port)]
    out = subprocess.run(cmd + [os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout                   # ONE JSON line, from rank 0 only
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["verify", "x25519", "sign"])
def test_bench_contract_single_gpu(engine, op):
    """bench.py's line carries the driver's keys plus roofline and cpu_baseline, and checks its outputs"""
    d = _bench_line(["--op", op, "--steps", "2", "--warmup", "1", "--log2n", "14", "--cpu-sample", "2048", "--full"])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["outputs_correct"] is True and d["vs_baseline"] is None
    assert d["cpu_baseline"]["kind"] in ("reference", "port") and d["cpu_baseline"]["gpu_matches_cpu_on_sample"]
    assert 0 < d["roofline"]["frac"] < 1.5 and "workload" in d["config"]


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["verify", "x25519", "sign"])
def test_bench_plain_line_and_dumped_outputs(engine, oracle, op, tmp_path):
    """a plain run (no --full): the headline keys only, exactly --steps timed steps, and --dump-outputs writes what the last
    step returned - the oracle's bytes on the same seeded inputs"""
    import workload
    n = 1 << 14
    d = _bench_line(["--op", op, "--steps", "3", "--warmup", "1", "--log2n", "14", "--dump-outputs", str(tmp_path)])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert not {"roofline", "cpu_baseline", "verdicts", "secondary"} & set(d)
    assert d["steps"] == 3 and d["outputs_correct"] is (True if op == "verify" else None)
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - n) < 1e-6 * n            # value = items / (ms_per_step)
    if op == "verify":
        sk, msg = workload.sign_inputs(n, seed=1, config=2)
        pk = oracle.genpub_batch(sk)
        want = workload.corrupt_for_verify(oracle.sign_batch(sk, pk, msg, 32), pk, msg)
        name = "verdicts"
    elif op == "x25519":
        want, name = oracle.x25519_batch(*workload.x25519_inputs(n)), "x25519_outputs"
    else:
        sk, msg = workload.sign_inputs(n)
        want, name = oracle.sign_batch(sk, oracle.genpub_batch(sk), msg, 32), "signatures"
    got = np.load(tmp_path / (name + ".npy"))
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))


@pytest.mark.gpu
def test_bench_two_ranks_on_one_gpu(engine):
    """the N > 1 path of bench.py (shards, gather, max-over-ranks timing) launched exactly as the driver
    launches it, with the two ranks sharing the box's single GPU and gloo standing in for RCCL"""
    d = _bench_line(["--gpus", "2", "--steps", "2", "--warmup", "1", "--log2n", "14", "--full"],
                    {"EDDSA_BENCH_SHARE_GPU": "1", "EDDSA_BENCH_BACKEND": "gloo"}, launcher=2)
    assert d["n_gpus"] == 2 and d["outputs_correct"] is True and d["scaling"] == "weak"
    assert d["config"]["parallelism"] == "shard2+allgather"
    assert d["cpu_baseline"]["gpu_matches_cpu_on_sample"] is True       # rank 0 times it; the other rank sleeps in a host barrier
    assert d["value"] > 0 and len(d["per_rank"]["ranks"]) == 2
    for op in ("x25519", "sign"):
        assert len(d["secondary"][op]["per_rank"]["ranks"]) == 2 and d["secondary"][op]["cpu_baseline"] is not None
    # SCALE readiness: what the gather ran over, a device per rank (here: the test hook says they share one),
    # and every rank's clock / power sample
    r = d["rccl"]
    assert r["world"] == 2 and r["backend"] == "gloo" and r["is_rccl"] is False and r["shared_gpu_test_hook"] is True
    assert len(r["devices"]) == 2 and r["devices_distinct"] is False
    for row in d["per_rank"]["ranks"]:
        assert {"rank", "device", "kernel_ms", "gather_ms", "wall_ms_per_step", "power_w", "sclk_mhz"} <= set(row)
