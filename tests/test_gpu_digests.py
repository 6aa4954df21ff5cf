"""GPU tests of verification from caller-supplied digests (include/eddsa_amd.h: ed25519_verify_digests, _rlc, _multi and the
device-pointer forms): item i is accepted exactly when the reference's ed25519_verify accepts (sigs[i], pubs[i], M) for an M
with SHA-512(R_i || A_i || M) = digests[i].  Digests come from hashlib, expected verdicts from the oracle or from the committed
vectors' accept fields - never from the engine's own message form."""
import hashlib
import subprocess

import numpy as np
import pytest

from ed_model import H, L, arr
from gen_golden import golden_msg  # tools/ is on sys.path (conftest)
from gpu_kit import dev
from hostlib import build_c_program

pytestmark = pytest.mark.gpu
G = 8192                                            # items per group of the batch verification


def digests_of(sig, pk, msgs):
    """SHA-512(R || A || M) per item, as the caller of the digest forms computes it; msgs: an (n, len) array or a list of bytes"""
    return arr([hashlib.sha512(sig[i, :32].tobytes() + pk[i].tobytes() + bytes(msgs[i])).digest() for i in range(len(sig))])


def both_forms(engine, sig, pk, dig):
    """(host-pointer verdicts, device-pointer verdicts)"""
    return engine.ed25519_verify_digests(sig, pk, dig), engine.ed25519_verify_digests(dev(sig), dev(pk), dev(dig)).cpu().numpy()


# ---------------------------------------------------------------- 1, 2: the committed vectors

def test_golden_table(engine, golden):
    """the 1024 entries of ed25519_table.bin (messages of 0 .. 1023 bytes): all accepted; with the digests rotated by one item, none"""
    raw = np.frombuffer(golden("ed25519_table.bin"), np.uint8).reshape(1024, 128)
    pk, sig = raw[:, 32:64].copy(), raw[:, 64:].copy()
    dig = digests_of(sig, pk, [golden_msg(i) for i in range(1024)])
    for got in both_forms(engine, sig, pk, dig):
        assert got.shape == (1024,) and got.dtype == np.uint8 and got.all()
    for got in both_forms(engine, sig, pk, np.roll(dig, 1, axis=0)):
        assert not got.any()


def test_edge_and_torsion_vectors(engine, golden):
    """verify_edges.json + verify_torsion.json (S out of range, non-canonical and small-order A and R, keys off the curve, mixed
    torsion) through the host form, the device form and the batch verification: the accept fields"""
    cases = golden("verify_edges.json") + golden("verify_torsion.json")
    sig, pk = arr([H(c["sig"]) for c in cases]), arr([H(c["pub"]) for c in cases])
    dig = digests_of(sig, pk, [H(c["msg"]) for c in cases])
    want = np.array([c["accept"] for c in cases], np.uint8)
    assert 0 < want.sum() < len(cases)
    for form, got in zip(("host", "device"), both_forms(engine, sig, pk, dig)):
        assert not [cases[i]["name"] for i in np.nonzero(got != want)[0]], form
    engine.set_rlc_min_items(0)
    try:
        got = engine.ed25519_verify_digests_rlc(sig, pk, dig)
        assert not [cases[i]["name"] for i in np.nonzero(got != want)[0]], "rlc, host"
        got = engine.ed25519_verify_digests_rlc(dev(sig), dev(pk), dev(dig)).cpu().numpy()
        assert not [cases[i]["name"] for i in np.nonzero(got != want)[0]], "rlc, device"
    finally:
        engine.set_rlc_min_items(engine.RLC_MIN_ITEMS_DEFAULT)


# ---------------------------------------------------------------- 3: every hashing kernel

MLEN = 40


@pytest.fixture(scope="module")
def signed(oracle):
    """2049 valid signatures over 40-byte messages, made with the oracle; shared, never modified"""
    rng = np.random.default_rng(31337)
    sk = rng.integers(0, 256, (2049, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (2049, MLEN), dtype=np.uint8)
    pk = oracle.genpub_batch(sk)
    sig = oracle.sign_batch(sk, pk, msg, MLEN)
    for a in (sig, pk, msg):
        a.setflags(write=False)
    return sig, pk, msg


def corrupted(oracle, signed, n):
    """the first n items, corrupted by item index mod 12 -> (sig, pk, digests, expected verdicts).  1: R; 2: S; 3: the key; 4: S + k l;
    5: random signature and key (digests of 1 - 5: the true ones of the corrupted item: the oracle decides); 6: a digest bit in
    byte 0; 7: in byte 63; 8: the digest swapped with the next item's (both are then wrong); 10: digest +- k l as a 512-bit integer,
    whichever stays in range (the same t: the oracle decides); 0, 11 (and 9 where there is no item 8 before it): untouched"""
    rng = np.random.default_rng(n)
    sig, pk, msg = (a[:n].copy() for a in signed)
    for i in range(n):
        k = i % 12
        if k == 1: sig[i, rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)
        elif k == 2: sig[i, 32 + rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)
        elif k == 3: pk[i, rng.integers(0, 32)] ^= 1 << rng.integers(0, 8)
        elif k == 4:
            s = int.from_bytes(sig[i, 32:].tobytes(), "little") + L * int(rng.integers(1, 15))
            assert s < 2**256                      # (S < l < 2^253)
            sig[i, 32:] = np.frombuffer(s.to_bytes(32, "little"), np.uint8)
        elif k == 5: sig[i] = rng.integers(0, 256, 64); pk[i] = rng.integers(0, 256, 32)
    want = oracle.verify_batch(sig, pk, msg, MLEN)
    dig = digests_of(sig, pk, msg)
    for i in range(n):
        k = i % 12
        if k == 6: dig[i, 0] ^= 1 << rng.integers(0, 8); want[i] = 0
        elif k == 7: dig[i, 63] ^= 1 << rng.integers(0, 8); want[i] = 0
        elif k == 8 and i + 1 < n:
            dig[[i, i + 1]] = dig[[i + 1, i]]; want[i] = want[i + 1] = 0
        elif k == 10:
            d, kl = int.from_bytes(dig[i].tobytes(), "little"), L * int(rng.integers(1, 1 << 62))
            d = d + kl if d + kl < 2**512 else d - kl
            assert 0 <= d < 2**512
            dig[i] = np.frombuffer(d.to_bytes(64, "little"), np.uint8)
    return sig, pk, dig, want


@pytest.mark.parametrize("algo,n", [(0, 1), (0, 64), (0, 65), (0, 200), (0, 300), (0, 2049), (1, 300), (2, 300), (3, 300)])
def test_every_hashing_kernel_at_the_smallest_pass_that_reaches_it(engine, oracle, signed, algo, n):
    """algo 0: the three-lane preparation with pairs up to 2^134 (window sums up to 2048 items, beyond them the four-lane
    evaluation) ; 1 and 2: the one-lane preparation (full-length / half-length evaluation); 3: the three-lane preparation with pairs
    up to 2^138 - each in its digest form, host and device"""
    sig, pk, dig, want = corrupted(oracle, signed, n)
    if n >= 12:
        assert 0 < want.sum() < n
    else:
        assert want.all()
    engine.set_verify_algo(algo)
    try:
        host, device = both_forms(engine, sig, pk, dig)
    finally:
        engine.set_verify_algo(0)
    assert np.array_equal(host, want), np.nonzero(host != want)[0][:10]
    assert np.array_equal(device, want), np.nonzero(device != want)[0][:10]


# ---------------------------------------------------------------- 4: keys off the curve

def test_off_curve_keys(engine, oracle):
    """the batch of test_off_curve_keys_take_the_exact_path (garbage keys under genuine signatures, R = 0 under garbage keys):
    the exact path reads t from the workspace and does not know where it came from.  Modes 1 (replay), 0 (reject), 2 (replay all)"""
    n = 6000
    rng = np.random.default_rng(4242)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (n, 40), dtype=np.uint8)
    pk = oracle.genpub_batch(sk)
    sig = oracle.sign_batch(sk, pk, msg, 40)
    pk[::2] = rng.integers(0, 256, (n // 2, 32), dtype=np.uint8)
    sig[1::4, :32] = 0
    sig[1::4, 32:] = rng.integers(0, 256, (len(sig[1::4]), 32), dtype=np.uint8)
    pk[1::4] = rng.integers(0, 256, (len(pk[1::4]), 32), dtype=np.uint8)
    want = oracle.verify_batch(sig, pk, msg, 40)
    assert want[3::4].all() and not want[::2].any()
    dig = digests_of(sig, pk, msg)
    for got in both_forms(engine, sig, pk, dig):
        assert np.array_equal(got, want)
    try:
        engine.set_offcurve_mode(False)
        for got in both_forms(engine, sig, pk, dig):
            assert np.array_equal(got, want)
        engine.set_offcurve_mode(2)
        for got in both_forms(engine, sig[:300], pk[:300], dig[:300]):
            assert np.array_equal(got, want[:300])
    finally:
        engine.set_offcurve_mode(True)


# ---------------------------------------------------------------- 5: the batch verification

def test_rlc_groups_and_fallback(engine, oracle):
    """one full group and a partial one, all valid: both decided by the combination; then one digest bit in the partial group: that
    group goes to the per-item kernels, which reject the one item"""
    n = G + 5
    rng = np.random.default_rng(55)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pk = oracle.genpub_batch(sk)
    sig = oracle.sign_batch(sk, pk, msg, 32)
    dig = digests_of(sig, pk, msg)
    bad = dig.copy(); bad[G + 2, 17] ^= 0x20
    want = np.ones(n, np.uint8); want[G + 2] = 0
    engine.set_rlc_min_items(0)
    try:
        for put in (lambda a: a, dev):
            ok, st = engine.ed25519_verify_digests_rlc(put(sig), put(pk), put(dig), return_stats=True)
            assert bool(ok.all()) and len(ok) == n and st == (n, 0, 0, 2)
            ok, st = engine.ed25519_verify_digests_rlc(put(sig), put(pk), put(bad), return_stats=True)
            ok = ok if isinstance(ok, np.ndarray) else ok.cpu().numpy()
            assert np.array_equal(ok, want) and st == (G, 5, 1, 1)
    finally:
        engine.set_rlc_min_items(engine.RLC_MIN_ITEMS_DEFAULT)


# ---------------------------------------------------------------- 6: host chunking and memory kinds

def test_host_chunks_and_memory_kinds(engine, oracle, signed):
    """2^16 + 300 items - past the first chunk of a verify call - with every 7th corrupted (signature, key or digest in turn): from
    ordinary numpy memory (staged by the copier threads), from page-locked arrays (read in place), and on the device form with
    sigs, pubs and digests each starting at an odd address"""
    import torch
    n = (1 << 16) + 300
    rng = np.random.default_rng(66)
    reps = (n + 2048) // 2049
    sig, pk, msg = (np.tile(a, (reps, 1))[:n].copy() for a in signed)
    hit = np.arange(0, n, 7)
    sig[hit[0::3], 5] ^= 4
    pk[hit[1::3], 9] ^= 8
    want = oracle.verify_batch(sig, pk, msg, MLEN)
    dig = digests_of(sig, pk, msg)
    dig[hit[2::3], rng.integers(0, 64, len(hit[2::3]))] ^= 1
    want[hit[2::3]] = 0
    assert n - len(hit) <= want.sum() < n
    assert np.array_equal(engine.ed25519_verify_digests(sig, pk, dig), want)
    pinned = [engine.host_array(a.shape) for a in (sig, pk, dig)]
    try:
        for p, a in zip(pinned, (sig, pk, dig)):
            p[...] = a
        assert np.array_equal(engine.ed25519_verify_digests(*pinned), want)
    finally:
        for p in pinned:
            engine.host_free(p)
    odd = []
    for a in (sig, pk, dig):
        t = torch.empty(a.size + 1, dtype=torch.uint8, device="cuda")
        t[1:] = torch.from_numpy(a.reshape(-1)).cuda()
        odd.append(t[1:])
        assert odd[-1].data_ptr() % 2 == 1 and odd[-1].is_contiguous()
    assert np.array_equal(engine.ed25519_verify_digests(*odd).cpu().numpy(), want)


# ---------------------------------------------------------------- 7: the multi-device host form, empty batches

def test_multi_device_form_and_empty_batches(engine, oracle, signed):
    assert engine.init_devices([0]) == 1
    n = 5000
    reps = (n + 2048) // 2049
    sig, pk, msg = (np.tile(a, (reps, 1))[:n].copy() for a in signed)
    sig[::5, 40] ^= 2
    want = oracle.verify_batch(sig, pk, msg, MLEN)
    assert 0 < want.sum() < n
    dig = digests_of(sig, pk, msg)
    assert np.array_equal(engine.ed25519_verify_digests_multi(sig, pk, dig), want)
    for fn in (engine.ed25519_verify_digests, engine.ed25519_verify_digests_rlc, engine.ed25519_verify_digests_multi):
        got = fn(sig[:0], pk[:0], dig[:0])
        assert got.shape == (0,) and got.dtype == np.uint8


# ---------------------------------------------------------------- 8: the shipped library, from C

def test_c_program_against_the_shipped_library(engine, oracle, signed, tmp_path):
    """tests/c/verify_digests.c: plain C against eddsa_amd.h, linked against libeddsa_amd.so (which exports no hook), on the
    (0, 300) batch of the kernel test: ed25519_verify_digests and ed25519_verify_digests_rlc return the oracle's verdicts"""
    sig, pk, dig, want = corrupted(oracle, signed, 300)
    exe = build_c_program(tmp_path, "verify_digests.c", libs=("eddsa_amd",), wall=True)
    files = []
    for name, a in (("sigs", sig), ("pubs", pk), ("digests", dig), ("want", want)):
        files.append(str(tmp_path / (name + ".bin")))
        a.tofile(files[-1])
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify_digests: ok (300 items)" in r.stdout
