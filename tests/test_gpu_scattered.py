"""GPU tests of ed25519_verify_scattered (include/eddsa_amd.h): items given by byte offsets into one buffer, device and host form.
Every check is exact equality of verdict bytes.  Expected verdicts are the oracle's over the spans gathered in numpy, or the committed
vectors' accept fields; ed25519_verify_batch of the same library over the gathered arrays is heard as a second witness."""
import ctypes
import subprocess

import numpy as np
import pytest

import cofactored_model as cm
import policy_model as pm
from ed_model import H
from gpu_kit import bad, dev, dev_idx, host, settings
from hostlib import build_c_program
from policy_model import POLICIES, STRICT

pytestmark = pytest.mark.gpu

LENGTHS = (0, 47, 48, 63, 64, 175, 176, 303, 304, 1000)   # with R || A in front: the last lengths of 1, 2, 3 blocks and the first beyond
SIZES = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 1 << 14, (1 << 14) + 1)   # wave, block, length order, four-lane route
SZ = ctypes.c_size_t
INVALID_VALUE = 1


class Spans:
    """a buffer and the four index arrays of a call; shared fixtures are read-only"""

    def __init__(self, data, so, po, mo, ml):
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.idx = [np.ascontiguousarray(a, dtype=np.uint32) for a in (so, po, mo, ml)]
        self.n = len(self.idx[0])

    def take(self, pick):
        return Spans(self.data, *(a[pick] for a in self.idx))

    def triples(self):
        b = self.data.tobytes()
        return [(b[s:s + 64], b[p:p + 32], b[m:m + l]) for s, p, m, l in zip(*(a.tolist() for a in self.idx))]

    def gathered(self):
        """-> sig (n, 64), pk (n, 32), the messages end to end, their n + 1 offsets"""
        t = self.triples()
        off = np.concatenate([[0], np.cumsum([len(m) for _, _, m in t])]).astype(np.uint64)
        return pm.arr([s for s, _, _ in t], 64), pm.arr([p for _, p, _ in t], 32), np.frombuffer(b"".join(m for _, _, m in t), np.uint8), off

    def on_device(self, engine, data=None):
        return host(engine.ed25519_verify_scattered(dev(self.data) if data is None else data, *(dev_idx(a) for a in self.idx)))

    def on_host(self, engine):
        return engine.ed25519_verify_scattered(self.data, *self.idx)


def lay_out(triples):
    """every (sig, pub, msg) as a packet of its own, end to end: packet i's three spans start at i, i + 5 and i + 11 mod 16, so a
    few dozen packets give each offset every residue; the last message ends with the buffer"""
    buf, cols = bytearray(), ([], [], [], [])
    for i, (s, p, m) in enumerate(triples):
        for part, col, r in ((s, cols[0], i), (p, cols[1], i + 5), (m, cols[2], i + 11)):
            buf += b"\xc3" * ((r - len(buf)) % 16)
            col.append(len(buf))
            buf += part
        cols[3].append(len(m))
    return Spans(np.frombuffer(bytes(buf), np.uint8), *cols)


def oracle_verdicts(oracle, sp):
    return np.array([oracle.verify(s, p, m) for s, p, m in sp.triples()], np.uint8)


def witness(engine, sp):
    """ed25519_verify_batch of the same library over the gathered arrays, under the settings in force"""
    sig, pk, flat, off = sp.gathered()
    return host(engine.ed25519_verify_batch(dev(sig), dev(pk), dev(flat if flat.size else np.zeros(1, np.uint8)), msg_off=dev(off.astype(np.int64))))


@pytest.fixture(scope="module")
def base(oracle):
    """48 signed packets, every length of LENGTHS at several alignments, and a corrupted copy of each (a bit of R, of S, of the key
    or of the message in turn) -> (the 96 items, the oracle's verdicts); shared, never modified"""
    rng = np.random.default_rng(20261021)
    triples = []
    for i in range(48):
        sk = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        m = rng.integers(0, 256, LENGTHS[i % len(LENGTHS)], dtype=np.uint8).tobytes()
        pk = oracle.genpub(sk)
        triples.append((oracle.sign(sk, pk, m), pk, m))
    for i in range(48):
        s, p, m = (bytearray(x) for x in triples[i])
        part = (s, s, p, m)[i % 4] if m or i % 4 != 3 else s
        at = int(rng.integers(0, 32)) + (32 if i % 4 == 1 else 0) if part is not m else int(rng.integers(0, len(m)))
        part[at] ^= 1 << int(rng.integers(0, 8))
        triples.append((bytes(s), bytes(p), bytes(m)))
    sp = lay_out(triples)
    want = oracle_verdicts(oracle, sp)
    assert want[:48].all() and not want[48:].any()
    for col in sp.idx[:3]:
        assert set((col % 16).tolist()) == set(range(16))
    assert sp.idx[2][-1] + sp.idx[3][-1] == sp.data.size
    for a in (sp.data, want, *sp.idx):
        a.setflags(write=False)
    return sp, want


def replicated(base, n, stride=37):
    """n items: the base items through the offsets, valid and corrupted mixed (37 and 96 are coprime)"""
    sp, want = base
    pick = (np.arange(n) * stride + 5) % sp.n
    return sp.take(pick), want[pick]


# ---------------------------------------------------------------- every size, both forms

@pytest.mark.parametrize("n", SIZES)
def test_every_size_in_both_forms(engine, base, n):
    sp, want = replicated(base, n)
    assert n < 12 or 0 < want.sum() < n
    got = sp.on_device(engine)
    assert got.dtype == np.uint8 and got.shape == (n,) and not len(bad(got, want)), bad(got, want)
    assert not len(bad(sp.on_host(engine), want))
    if n <= 4097:
        assert not len(bad(witness(engine, sp), want))


# ---------------------------------------------------------------- shared and overlapping spans

def test_shared_and_overlapping_spans(engine, oracle):
    """one packet: a 1000-byte message, eight (signature, key) pairs behind it - the third signer's signature spoilt -, two items
    with the same signature and key, and an item whose message span contains its own signature"""
    rng = np.random.default_rng(8)
    m = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
    buf, so, po = bytearray(b"\x11" * 3) + m, [], []
    for k in range(8):
        sk = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        pk = oracle.genpub(sk)
        sig = bytearray(oracle.sign(sk, pk, m))
        if k == 2:
            sig[40] ^= 0x10
        buf += b"\x22" * (k % 3)
        so.append(len(buf)); buf += sig
        po.append(len(buf)); buf += pk
    items = [(so[k], po[k], 3, 1000) for k in range(8)]
    items += [items[0], items[0]]                                     # the same signature and key twice
    items += [(so[1], po[1], 3, len(buf) - 3), (so[1], po[1], so[1] - 10, 100)]   # the message holds the item's own signature
    items += [(so[4], po[4], 3, 999), (so[4], po[4], 4, 1000)]        # a neighbour's message, one byte off
    sp = Spans(np.frombuffer(bytes(buf), np.uint8), *zip(*items))
    want = oracle_verdicts(oracle, sp)
    assert want.tolist() == [1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0]
    assert not len(bad(sp.on_device(engine), want)) and not len(bad(sp.on_host(engine), want))
    assert not len(bad(witness(engine, sp), want))


# ---------------------------------------------------------------- spans that leave the buffer

def outside_cases(data_len):
    """(field, offset, msg_len or None): for each field a span that starts one byte too late, at data_len and at 2^32 - 1; for
    the message also msg_off = 1 with msg_len = 2^32 - 1"""
    cases = [(f, off, None) for f, w in ((0, 64), (1, 32)) for off in (data_len - w + 1, data_len, 2**32 - 1)]
    cases += [(2, data_len - 9, 10), (2, data_len, 1), (2, 2**32 - 1, 1), (2, 1, 2**32 - 1)]
    return cases


def with_outside(sp, case, at):
    field, off, ml = case
    idx = [a.copy() for a in sp.idx]
    idx[field][at] = off
    if ml is not None:
        idx[3][at] = ml
    return Spans(sp.data, *idx)


SETTINGS = (dict(offcurve=True), dict(offcurve=False), dict(offcurve=2), dict(policy=STRICT), dict(cofactored=True), dict(algo=1))


@pytest.mark.parametrize("how", SETTINGS, ids=lambda h: "-".join(f"{k}={v}" for k, v in h.items()))
def test_items_outside_the_buffer_get_zero_on_the_device(engine, base, how):
    """positions 0, 63, 64, 255, 256 and n - 1 among valid and corrupted items: ok is 0 there and what it was elsewhere.  The valid
    items are honest signatures: 1 under every setting; the corrupted ones are the witness's under the same setting"""
    import torch
    n = 300
    sp, want = replicated(base, n)
    at = np.array([0, 63, 64, 255, 256, n - 1])
    framed = []
    for fill in (0x00, 0xFF):                         # the same buffer inside a larger tensor, at an odd address
        big = torch.full((sp.data.size + 2 * 4099,), fill, dtype=torch.uint8, device="cuda")
        big[4099:4099 + sp.data.size] = torch.from_numpy(sp.data.copy()).cuda()
        framed.append(big[4099:4099 + sp.data.size])
        assert framed[-1].data_ptr() % 2 == 1
    with settings(engine, **how):
        plain = witness(engine, sp)
        assert np.array_equal(plain[want == 1], want[want == 1])
        assert not len(bad(sp.on_device(engine), plain))
        for case in outside_cases(sp.data.size):
            cut = with_outside(sp, case, at)
            expect = plain.copy()
            expect[at] = 0
            got = cut.on_device(engine)
            assert not len(bad(got, expect)), (case, bad(got, expect))
            for data in framed:
                assert np.array_equal(cut.on_device(engine, data), got), case
    assert plain[at].any()                            # (some of the six were accepted before)


def test_the_host_form_refuses_items_outside_the_buffer(engine, base):
    sp, _ = replicated(base, 300)
    lib = engine.library()
    for case in outside_cases(sp.data.size):
        for at in (0, 63, 64, 255, 256, 299):
            cut = with_outside(sp, case, at)
            ok = np.full(300, 0xEE, np.uint8)
            rc = lib.ed25519_verify_scattered(ok.ctypes.data_as(ctypes.c_void_p), cut.data.ctypes.data_as(ctypes.c_void_p), SZ(cut.data.size),
                                              *(a.ctypes.data_as(ctypes.c_void_p) for a in cut.idx), SZ(300))
            assert rc == -INVALID_VALUE and (ok == 0xEE).all(), (case, at)


# ---------------------------------------------------------------- the recorded vectors

def test_recorded_edge_and_torsion_vectors(engine, golden):
    """verify_edges.json + verify_torsion.json in the three off-curve modes and under every policy: the accept fields and the
    policy model, as tests/test_gpu_policy.py holds the other forms against them"""
    cases, sig, pk, accept = pm.vector_cases(golden)
    sp = lay_out([(sig[i].tobytes(), pk[i].tobytes(), H(c["msg"])) for i, c in enumerate(cases)])
    names = lambda got, want: [cases[i]["name"] for i in bad(got, want)]   # noqa: E731
    for offcurve in (True, False, 2):
        for policy in POLICIES if offcurve is True else (0, STRICT):
            want = accept & pm.holds_batch(policy, sig, pk)
            with settings(engine, offcurve=offcurve, policy=policy):
                assert not names(sp.on_device(engine), want), (offcurve, hex(policy), "device")
                assert not names(sp.on_host(engine), want), (offcurve, hex(policy), "host")


def test_recorded_cofactored_vectors(engine, golden):
    """verify_cofactored.json under the cofactored equation (the vectors' accept fields, as tests/test_gpu_cofactored.py) and
    under the reference's (the oracle)"""
    sig, pk, msg, want = cm.arrays(cm.from_json(golden("verify_cofactored.json")))
    sp = lay_out([(sig[i].tobytes(), pk[i].tobytes(), msg[i].tobytes()) for i in range(len(sig))])
    for offcurve in (True, False, 2):
        with settings(engine, cofactored=True, offcurve=offcurve):
            assert not len(bad(sp.on_device(engine), want)), offcurve
            assert not len(bad(sp.on_host(engine), want)), offcurve
    with settings(engine, cofactored=True, policy=STRICT):
        strict = want & pm.holds_batch(STRICT, sig, pk)
        assert not len(bad(sp.on_device(engine), strict))


def test_recorded_cofactored_vectors_under_the_cofactorless_equation(engine, golden, oracle):
    sig, pk, msg, want = cm.arrays(cm.from_json(golden("verify_cofactored.json")))
    sp = lay_out([(sig[i].tobytes(), pk[i].tobytes(), msg[i].tobytes()) for i in range(len(sig))])
    less = oracle.verify_batch(sig, pk, msg, msg.shape[1])
    assert (less != want).any()
    assert not len(bad(sp.on_device(engine), less)) and not len(bad(sp.on_host(engine), less))


# ---------------------------------------------------------------- more than one pass

def test_a_call_of_more_than_one_pass(engine, base):
    """2^20 + 257 items over 64 distinct packets cross the size of a workspace pass; the buffer stays a few KiB"""
    sp, want = base
    n = (1 << 20) + 257
    pick = (np.arange(n) * 37 + 5) % 64 + 16                 # 64 of the 96 items: 32 valid, 32 corrupted
    assert len(set(pick.tolist())) == 64
    many, expect = sp.take(pick), want[pick]
    assert 0 < expect.sum() < n
    assert not len(bad(many.on_device(engine), expect))
    assert not len(bad(many.on_host(engine), expect))


# ---------------------------------------------------------------- the shared workspace areas

def test_scattered_ctx_and_keyed_passes_share_a_workspace(engine, oracle, base):
    """on one stream: scattered, Ed25519ctx, keyed over a plain set, scattered again - domdig and keybytes serve all three kinds"""
    n = 300
    sp, want = replicated(base, n)
    other, other_want = replicated(base, n, stride=41)
    rng = np.random.default_rng(77)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msg = rng.integers(0, 256, (n, 40), dtype=np.uint8)
    pk = oracle.genpub_batch(sk)
    sig = oracle.sign_batch(sk, pk, msg, 40)
    sig[::7, 3] ^= 2
    keyed_want = oracle.verify_batch(sig, pk, msg, 40)
    assert 0 < keyed_want.sum() < n
    ctx_sig = engine.ed25519ctx_sign_batch(sk, pk, msg, b"scattered", msg_len=40)
    ctx_msg = msg.copy()
    ctx_msg[::5, 7] ^= 1
    ctx_want = np.ones(n, np.uint8)
    ctx_want[::5] = 0                                   # a signature over another message; the others are the signer's own
    ks = engine.keyset_create(dev(pk[:50]))
    try:
        idx = np.arange(n, dtype=np.uint32) % 50
        kw = oracle.verify_batch(sig, pk[idx], msg, 40)
        assert 0 < kw.sum() < n
        d_data, d_idx = dev(sp.data), [dev_idx(a) for a in sp.idx]
        o_idx = [dev_idx(a) for a in other.idx]
        d_sig, d_pk, d_msg, d_csig, d_cmsg, d_kidx = dev(sig), dev(pk), dev(msg), dev(ctx_sig), dev(ctx_msg), dev_idx(idx)
        a = engine.ed25519_verify_scattered(d_data, *d_idx)
        b = engine.ed25519ctx_verify_batch(d_csig, d_pk, d_cmsg, b"scattered", msg_len=40)
        c = engine.ed25519_verify_keyed(d_sig, ks, d_kidx, d_msg, msg_len=40)
        d = engine.ed25519_verify_scattered(d_data, *o_idx)
        assert not len(bad(a, want)) and not len(bad(b, ctx_want)) and not len(bad(c, kw)) and not len(bad(d, other_want))
    finally:
        ks.close()


def test_two_streams_at_once(engine, base):
    import torch
    runs = [replicated(base, 5000, stride=s) for s in (37, 41)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    args = [(dev(sp.data), [dev_idx(a) for a in sp.idx]) for sp, _ in runs]
    torch.cuda.synchronize()
    got = []
    for _ in range(3):
        for st, (data, idx) in zip(streams, args):
            with torch.cuda.stream(st):
                got.append(engine.ed25519_verify_scattered(data, *idx))
    torch.cuda.synchronize()
    for k, g in enumerate(got):
        assert not len(bad(g, runs[k % 2][1])), k


# ---------------------------------------------------------------- arguments

def test_arguments(engine, base):
    import torch
    sp, want = replicated(base, 10)
    empty = np.zeros(0, np.uint32)
    got = engine.ed25519_verify_scattered(sp.data, empty, empty, empty, empty)
    assert got.shape == (0,) and got.dtype == np.uint8
    got = engine.ed25519_verify_scattered(dev(sp.data), *(dev_idx(empty) for _ in range(4)))
    assert tuple(got.shape) == (0,)
    lib = engine.library()
    ok = torch.full((10,), 0xEE, dtype=torch.uint8, device="cuda")
    ptrs = [ctypes.c_void_p(ok.data_ptr()), ctypes.c_void_p(dev(sp.data).data_ptr())]
    tensors = [dev_idx(a) for a in sp.idx]
    idx = [ctypes.c_void_p(t.data_ptr()) for t in tensors]
    for hole in range(6):
        args = [ptrs[0], ptrs[1], SZ(sp.data.size), *idx, SZ(10), None]
        args[hole if hole < 2 else hole + 1] = None
        assert lib.ed25519_verify_scattered_dev(*args) == -INVALID_VALUE, hole
    assert lib.ed25519_verify_scattered_dev(ptrs[0], ptrs[1], SZ(2**32), *idx, SZ(10), None) == -INVALID_VALUE
    torch.cuda.synchronize()
    assert (ok.cpu().numpy() == 0xEE).all()
    with pytest.raises(ValueError):
        engine.ed25519_verify_scattered(dev(sp.data), *(dev(a.view(np.uint8)) for a in sp.idx))


def test_ok_on_another_device_than_data(engine, base):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    sp, _ = replicated(base, 10)
    lib = engine.library()
    ok = torch.zeros(10, dtype=torch.uint8, device="cuda:1")
    data, idx = dev(sp.data), [dev_idx(a) for a in sp.idx]
    rc = lib.ed25519_verify_scattered_dev(ctypes.c_void_p(ok.data_ptr()), ctypes.c_void_p(data.data_ptr()), SZ(sp.data.size),
                                          *(ctypes.c_void_p(t.data_ptr()) for t in idx), SZ(10), None)
    assert rc == -INVALID_VALUE


# ---------------------------------------------------------------- the shipped library, from C

def test_c_program_against_the_shipped_library(engine, base, tmp_path):
    """tests/c/verify_scattered.c: plain C against eddsa_amd.h, linked against libeddsa_amd.so (which exports no hook)"""
    sp, want = replicated(base, 300)
    exe = build_c_program(tmp_path, "verify_scattered.c", libs=("eddsa_amd",), wall=True)
    files = []
    for name, a in (("data", sp.data), ("sig_off", sp.idx[0]), ("pub_off", sp.idx[1]), ("msg_off", sp.idx[2]), ("msg_len", sp.idx[3]),
                    ("want", want)):
        files.append(str(tmp_path / (name + ".bin")))
        a.tofile(files[-1])
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify_scattered: ok (300 items)" in r.stdout
