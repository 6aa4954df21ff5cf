"""GPU tests of the arrangement of full-size verify passes - k_verify_halve with the balanced pair search (libeddsa_amd/csrc/
halve.h: halve_balanced_lane, both |u| and v at most B33) and k_verify_main_half over 33 windows - forced at small sizes through
set_verify_algo(4): the oracle's verdict bytes on the recorded edge and mixed-order vectors and on passes of 1, 63, 64, 65 and
300 items, two thirds of them under random keys, with signatures whose t has no balanced pair among them; and the device's
pairs against the host build of the same source and the integer model.  (Passes of 2^19 items and more take this arrangement by
themselves: tests/test_gpu_torsion.py, test_gpu_fuzz.py and bench.py's reference digest hold it there.)"""
import hashlib

import numpy as np
import pytest

import balanced_model as bm
from balanced_model import B33, CRAFTED, L, N8L, lane_pairs
from ed_model import H, arr
from gpu_kit import bad, dev, host, settings
from hostlib import build_check

pytestmark = pytest.mark.gpu
BALANCED = 4                  # set_verify_algo: the arrangement of passes of 2^19 items and more, at any size


def test_edge_and_torsion_vectors_through_33_windows(engine, golden):
    cases = golden("verify_edges.json") + golden("verify_torsion.json")
    msgs = [H(c["msg"]) for c in cases]
    off = np.zeros(len(msgs) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    blob = np.frombuffer(b"".join(msgs), np.uint8).copy()
    sig, pub = arr([H(c["sig"]) for c in cases]), arr([H(c["pub"]) for c in cases])
    want = np.array([c["accept"] for c in cases], np.uint8)
    with settings(engine, algo=BALANCED):
        got = engine.ed25519_verify_batch(sig, pub, blob, msg_off=off)
        assert not [cases[i]["name"] for i in bad(got, want)]
        got = engine.ed25519_verify_batch(dev(sig), dev(pub), dev(blob), msg_off=dev(off.astype(np.int64)))
        assert np.array_equal(host(got), want)
    assert engine.halve_rejected() == 0


@pytest.fixture(scope="module")
def batch(oracle):
    """300 items with 40-byte messages and the oracle's verdicts: item i with i % 3 != 0 stands under a random key (half of those
    are no curve points: the exact path), the others under their signer's key, every fourth of them corrupted; items 0, 62, 64
    and 299 carry a t without a balanced pair (searched with the model over one key's signatures), the one at 62 with a wrong S"""
    n, rng = 300, np.random.default_rng(33)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (n, 40), dtype=np.uint8)
    pk = oracle.genpub_batch(sk)
    slots, i = [0, 62, 64, 299], 0
    for slot in slots:
        while True:
            msg[slot, :8] = np.frombuffer(i.to_bytes(8, "little"), np.uint8)
            i += 1
            s = oracle.sign(sk[slot].tobytes(), pk[slot].tobytes(), msg[slot].tobytes())
            t = int.from_bytes(hashlib.sha512(s[:32] + pk[slot].tobytes() + msg[slot].tobytes()).digest(), "little") % L
            if not bm.balanced_pair(t)[0]:
                break
    sig = oracle.sign_batch(sk, pk, msg, 40)
    for k in range(n):
        if k in slots:
            continue
        if k % 3:
            pk[k] = rng.integers(0, 256, 32, dtype=np.uint8)
        elif k % 12 == 0:
            sig[k, rng.integers(0, 64)] ^= 1 << rng.integers(0, 8)
    sig[62, 40] ^= 1
    want = oracle.verify_batch(sig, pk, msg, 40)
    assert want[0] == 1 and want[62] == 0 and want[64] == 1 and want[299] == 1 and 60 <= want.sum() <= 90
    for a in (sig, pk, msg, want):
        a.setflags(write=False)
    return sig, pk, msg, want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_small_passes_through_the_balanced_arrangement(engine, batch, n):
    """the first n and the last n items of the batch, from host and from device memory: byte for byte the oracle's verdicts - a
    genuine signature without a balanced pair is accepted only if the exact path decided it (33 windows cannot hold its t)"""
    sig, pk, msg, want = batch
    with settings(engine, algo=BALANCED):
        for lo in sorted({0, len(want) - n}):
            part = [a[lo:lo + n].copy() for a in (sig, pk, msg)]
            got = engine.ed25519_verify_batch(*part, msg_len=40)
            assert np.array_equal(got, want[lo:lo + n]), (lo, bad(got, want[lo:lo + n]))
            got = engine.ed25519_verify_batch(*(dev(a) for a in part), msg_len=40)
            assert np.array_equal(host(got), want[lo:lo + n]), (lo, bad(got, want[lo:lo + n]))
    assert engine.halve_rejected() == 0


def test_device_pairs_against_the_host_lane_and_the_model(engine, tmp_path_factory):
    """the search as the DEVICE runs it (reciprocals by Newton steps where the host build divides) on the crafted scalars and on
    20 000 random ones: the same found / not found and the same pair as the host build of the source, item by item, and as the
    integer model; every pair holds u t = v (mod 8 l) with u odd and both values at most B33"""
    rng = np.random.default_rng(133)
    ts = [t for t, _ in CRAFTED] + [N8L // k % L for k in (3, 5, 7, 9, 1000003, (1 << 61) - 1, (1 << 100) + 277, (1 << 125) + 1, (1 << 128) + 51)]
    ts += [int.from_bytes(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), "little") % L for _ in range(20000)]
    on_host = lane_pairs(build_check(tmp_path_factory, "balanced"), ts)
    on_device = engine.debug_halve(ts, wide=2)
    given_up = 0
    for t, h, d in zip(ts, on_host, on_device):
        assert h[0] == d[0], hex(t)
        found, u, v, way, big = bm.balanced_trace(t)
        if big < 1 << 24:
            assert d[0] == found, hex(t)
        if d[0]:
            assert d == h and d[1:] == (u, v) and (u * t - v) % N8L == 0 and u & 1 and abs(u) <= B33 and 0 <= v <= B33, hex(t)
        else:
            given_up += 1
    assert given_up <= 8 + 0.0025 * len(ts) + 4 * (0.0025 * len(ts)) ** 0.5       # the crafted ones, the cap and four deviations of a count
    for (t, way), d in zip(CRAFTED, on_device):
        if way:
            assert d[0] == (way != "none"), hex(t)
