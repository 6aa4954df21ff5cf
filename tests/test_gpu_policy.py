"""GPU tests of the opt-in strict rules of verification (include/eddsa_amd.h: EDDSA_AMD_VERIFY_*; kernels.hip: k_verify_policy):
under policy P item i is accepted exactly when the reference accepts it AND every predicate of P holds for its bytes.  Expected
verdicts are (the oracle's, or the committed vectors' accept fields) AND the Python model of tests/policy_model.py - never the
engine's.  Every test puts the mode word back."""
import hashlib

import numpy as np
import pytest

import policy_model as pm
from gpu_kit import dev, host, settings
from policy_model import BITS, MLEN, POLICIES, STRICT

pytestmark = pytest.mark.gpu
G = 8192                                            # items per group of the batch verification
BLOCK = 256                                         # lanes per block of k_verify_policy (kernels.hip)


@pytest.fixture(scope="module")
def batch(oracle):
    """the policy batch at its largest size (tests/policy_model.py: policy_batch; an item's class is its index mod 8, so every
    prefix is a batch of the same kind); shared, never modified"""
    return pm.policy_batch(oracle, 2049)


def ragged(msgs):
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b"".join(msgs) or b"\0", np.uint8).copy(), off


# ---------------------------------------------------------------- 1: the committed vectors, every form

def test_vector_files_through_every_form(engine, golden):
    """verify_edges.json + verify_torsion.json under policy 0, each bit alone and all four: the host form, the device form, the
    digest form, the records form (one call per message length) and the single-item ed25519_verify"""
    cases, sig, pk, accept = pm.vector_cases(golden)
    msgs = [pm.H(c["msg"]) for c in cases]
    flat, off = ragged(msgs)
    dig = pm.arr([hashlib.sha512(sig[i, :32].tobytes() + pk[i].tobytes() + msgs[i]).digest() for i in range(len(cases))])
    by_len = {}
    for i, m in enumerate(msgs):
        by_len.setdefault(len(m), []).append(i)
    records = {mlen: (np.array(idx), np.concatenate([sig[idx], pk[idx], pm.arr([msgs[i] for i in idx]).reshape(len(idx), mlen)], axis=1))
               for mlen, idx in by_len.items()}

    def names(got, want):
        return [cases[i]["name"] for i in np.nonzero(np.asarray(got) != want)[0]]

    for policy in POLICIES:
        want = accept & pm.holds_batch(policy, sig, pk)
        with settings(engine, policy=policy):
            assert not names(engine.ed25519_verify_batch(sig, pk, flat, msg_off=off), want), (hex(policy), "host")
            got = engine.ed25519_verify_batch(dev(sig), dev(pk), dev(flat), msg_off=dev(off.astype(np.int64)))
            assert not names(host(got), want), (hex(policy), "device")
            assert not names(engine.ed25519_verify_digests(sig, pk, dig), want), (hex(policy), "digests, host")
            assert not names(host(engine.ed25519_verify_digests(dev(sig), dev(pk), dev(dig))), want), (hex(policy), "digests, device")
            got_h, got_d = np.zeros(len(cases), np.uint8), np.zeros(len(cases), np.uint8)
            for mlen, (idx, rec) in records.items():
                got_h[idx] = engine.ed25519_verify_records(rec, 0, 64, 96, mlen)
                got_d[idx] = host(engine.ed25519_verify_records(dev(rec), 0, 64, 96, mlen))
            assert not names(got_h, want), (hex(policy), "records, host")
            assert not names(got_d, want), (hex(policy), "records, device")
            single = [engine.ed25519_verify(sig[i].tobytes(), pk[i].tobytes(), msgs[i]) for i in range(len(cases))]
            assert not names(np.array(single, np.uint8), want), (hex(policy), "ed25519_verify")
    # (the numbers the CPU suite pinned: this test does reject something under every bit)
    assert [int((accept & ~pm.holds_batch(bit, sig, pk) & 1).sum()) for bit in BITS] == [13, 2, 17, 17]


# ---------------------------------------------------------------- 2: the policy batch at every size and route

SIZES = [(0, 1), (0, 64), (0, 65), (0, BLOCK - 1), (0, BLOCK), (0, BLOCK + 1), (0, 300), (0, 2049), (1, 300), (2, 300), (3, 300)]


@pytest.mark.parametrize("case,algo,n", [(j, a, n) for j, (a, n) in enumerate(SIZES)])
def test_policy_batch_at_the_smallest_pass_that_reaches_each_writer_of_ok(engine, batch, case, algo, n):
    """algo 0: window sums up to 2048 items, beyond them the four-lane half-length evaluation; 1: the full-length evaluation and
    k_verify_finish; 2: k_verify_halve + k_verify_main_half; 3: the mid-size arrangement - and the grid of k_verify_policy with one
    lane, one lane short of a block, a whole block, a block and a lane, and nine blocks.  Host and device forms, under all four
    bits and under one bit (each bit in turn over the cases)"""
    sig, pk, msg, oracle_ok = (a[:n] for a in batch)
    for policy in (STRICT, BITS[case % 4]):
        want = oracle_ok & pm.holds_batch(policy, sig, pk)
        with settings(engine, policy=policy, algo=algo):
            got_h = engine.ed25519_verify_batch(sig, pk, msg, msg_len=MLEN)
            got_d = host(engine.ed25519_verify_batch(dev(sig), dev(pk), dev(msg), msg_len=MLEN))
        assert np.array_equal(got_h, want), (hex(policy), "host", np.nonzero(got_h != want)[0][:10])
        assert np.array_equal(got_d, want), (hex(policy), "device", np.nonzero(got_d != want)[0][:10])
        if n >= 64:
            assert 0 < want.sum() < oracle_ok.sum()


def test_policy_batch_when_every_verdict_comes_from_the_side_stream(engine, batch):
    """set_offcurve_mode(2): k_verify_exact_quad on the side stream writes every verdict and the windowed kernels' are ignored;
    k_verify_policy runs behind the join.  Set in both orders: neither Python setter clears the other's half of the word"""
    sig, pk, msg, oracle_ok = (a[:300] for a in batch)
    for policy, policy_first in ((STRICT, False), (BITS[0], True)):
        want = oracle_ok & pm.holds_batch(policy, sig, pk)
        try:
            if policy_first:
                engine.set_verify_policy(policy); engine.set_offcurve_mode(2)
            else:
                engine.set_offcurve_mode(2); engine.set_verify_policy(policy)
            got_h = engine.ed25519_verify_batch(sig, pk, msg, msg_len=MLEN)
            got_d = host(engine.ed25519_verify_batch(dev(sig), dev(pk), dev(msg), msg_len=MLEN))
        finally:
            engine.set_verify_policy(0)
            engine.set_offcurve_mode(True)
        assert np.array_equal(got_h, want) and np.array_equal(got_d, want), hex(policy)
        assert 0 < want.sum() < oracle_ok.sum()
    # back at policy 0 and the default mode: the oracle's verdicts
    assert np.array_equal(engine.ed25519_verify_batch(sig, pk, msg, msg_len=MLEN), oracle_ok)


# ---------------------------------------------------------------- 3: the batch verification

def test_batch_verification_applies_the_policy_and_routes_as_before(engine, oracle, batch):
    """8192 + 5 valid items plus four items only a policy rejects, inserted among them (S + k l, an identity key and an identity R
    in the full group, S + k l in the partial group, which then holds 9 items): right verdicts under all four bits and under one,
    and the statistics policy 0 reports for the same input - the policy changes no routing"""
    rng = np.random.default_rng(77)
    sk = rng.integers(0, 256, (G + 5, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (G + 5, MLEN), dtype=np.uint8)
    pk = oracle.genpub_batch(sk)
    sig = oracle.sign_batch(sk, pk, msg, MLEN)
    bsig, bpk, bmsg, _ = batch
    for at, src in ((7, 1), (4000, 2), (8000, 3), (G + 6, 9)):          # (ascending: `at` is the item's final index; classes 1, 2, 3, 1)
        sig, pk, msg = (np.insert(a, at, b[src], axis=0) for a, b in ((sig, bsig), (pk, bpk), (msg, bmsg)))
    n = G + 9
    assert len(sig) == len(pk) == len(msg) == n and np.array_equal(sig[G + 6], bsig[9]) and np.array_equal(pk[4000], bpk[2])
    oracle_ok = oracle.verify_batch(sig, pk, msg, MLEN)
    assert oracle_ok.all()
    for put in (lambda a: a, dev):
        with settings(engine, policy=0, rlc_min=0):
            ok, base = engine.ed25519_verify_batch_rlc(put(sig), put(pk), put(msg), msg_len=MLEN, return_stats=True)
        assert host(ok).all() and sum(base[:2]) == n
        for policy in (STRICT, BITS[0]):
            want = pm.holds_batch(policy, sig, pk)
            with settings(engine, policy=policy, rlc_min=0):
                ok, st = engine.ed25519_verify_batch_rlc(put(sig), put(pk), put(msg), msg_len=MLEN, return_stats=True)
            assert np.array_equal(host(ok), want), (hex(policy), np.nonzero(host(ok) != want)[0])
            assert st == base, (hex(policy), st, base)
            assert n - int(want.sum()) == (4 if policy == STRICT else 2)


# ---------------------------------------------------------------- 4: host chunking

def test_host_chunks_from_ordinary_memory(engine, oracle, batch):
    """2^16 + 300 items - past the first chunk of a verify call - from ordinary numpy memory under all four bits: the valid items
    of the policy batch over and over, every 7th item one of its classes 1 - 3"""
    bsig, bpk, bmsg, bok = batch
    n = (1 << 16) + 300
    k = np.arange(len(bsig)) % 8
    valid, odd = np.nonzero(np.isin(k, (0, 7)))[0], np.nonzero(np.isin(k, (1, 2, 3)))[0]
    pick = valid[np.arange(n) % len(valid)]
    hit = np.arange(0, n, 7)
    pick[hit] = odd[np.arange(len(hit)) % len(odd)]
    sig, pk, msg = bsig[pick], bpk[pick], bmsg[pick]
    oracle_ok = oracle.verify_batch(sig, pk, msg, MLEN)
    assert oracle_ok.all()
    want = pm.holds_batch(STRICT, bsig, bpk)[pick]
    assert np.array_equal(np.nonzero(want == 0)[0], hit)
    with settings(engine, policy=STRICT):
        got = engine.ed25519_verify_batch(sig, pk, msg, msg_len=MLEN)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]


# ---------------------------------------------------------------- 5: the multi-device host form, empty batches

def test_multi_device_form_and_empty_batches(engine, batch):
    assert engine.init_devices([0]) == 1
    n = 5000
    pick = np.arange(n) % len(batch[0])
    sig, pk, msg, oracle_ok = (a[pick] for a in batch)
    want = oracle_ok & pm.holds_batch(STRICT, batch[0], batch[1])[pick]
    assert 0 < want.sum() < oracle_ok.sum()
    with settings(engine, policy=STRICT, rlc_min=0):
        assert np.array_equal(engine.ed25519_verify_batch_multi(sig, pk, msg, msg_len=MLEN), want)
        for fn in (engine.ed25519_verify_batch, engine.ed25519_verify_batch_rlc, engine.ed25519_verify_batch_multi):
            got = fn(sig[:0], pk[:0], msg[:0], msg_len=MLEN)
            assert got.shape == (0,) and got.dtype == np.uint8
        got = engine.ed25519_verify_batch(dev(sig[:0]), dev(pk[:0]), dev(msg[:0]), msg_len=MLEN)
        assert tuple(got.shape) == (0,)
