"""The opt-in strict rules of verification (include/eddsa_amd.h: EDDSA_AMD_VERIFY_*), the part that needs no GPU: the lane
function of k_verify_policy (libeddsa_amd/csrc/policy_lanes.h: verify_policy_lane) compiled for the host with every bound
asserted (tests/host_check/policy_check.cpp) against Python integers (tests/policy_model.py), what the rules do to the committed
vectors and to the batch the GPU tests use, the Python setters, and the header."""
import ctypes
import itertools
import os
import random
import re

import numpy as np
import pytest

import policy_model as pm
from hostlib import ROOT, build_check, declared_names, header_text
from policy_model import BITS, L, P, POLICIES, STRICT

MACROS = {"EDDSA_AMD_VERIFY_S_BELOW_L": 0x100, "EDDSA_AMD_VERIFY_A_CANONICAL": 0x200, "EDDSA_AMD_VERIFY_A_NOT_SMALL": 0x400,
          "EDDSA_AMD_VERIFY_R_NOT_SMALL": 0x800, "EDDSA_AMD_VERIFY_STRICT": 0xF00, "EDDSA_AMD_VERIFY_POLICY_MASK": 0xF00}


@pytest.fixture(scope="module")
def policycheck(tmp_path_factory):
    """tests/host_check/policy_check.cpp built with the flags of the hostcheck fixture (conftest.py), outside the tree"""
    h = build_check(tmp_path_factory, "policy")
    h.pc_violations.restype = ctypes.c_long
    return h


def lane(h, policy, sig, pk):
    sig, pk = np.ascontiguousarray(sig), np.ascontiguousarray(pk)
    out = np.full(len(sig), 7, np.uint8)
    h.pc_policy(out.ctypes.data_as(ctypes.c_void_p), sig.ctypes.data_as(ctypes.c_void_p), pk.ctypes.data_as(ctypes.c_void_p),
                ctypes.c_size_t(len(sig)), ctypes.c_uint(policy))
    return out


def enc(v):
    return v.to_bytes(32, "little")


def test_the_model_finds_the_eight_points_and_their_five_ys():
    """l times a curve point is a point of order dividing 8; the eight of them have five values of y, all on the curve"""
    pts, ys = pm.torsion_points(), pm.small_order_ys()
    assert len(pts) == 8 and (0, 1) in pts and (0, P - 1) in pts
    assert sorted(min(k for k in (1, 2, 4, 8) if pm.mul(k, pt) == (0, 1)) for pt in pts) == [1, 2, 4, 4, 8, 8, 8, 8]
    assert all(pm.is_square(pm.x_squared(y)) for y in ys)
    assert sum(pm.canonical(e) for e in pm.torsion_encodings()) == 8      # one canonical encoding per point


def test_verify_policy_lane_against_python_integers(policycheck):
    """S at the edges of [0, l) and of 256 bits, A and R with y at the edges of [0, p) and of 255 bits under both sign bits (all
    2048 combinations), the eight points of order dividing 8 in every encoding as A and as R, and 2000 seeded random triples;
    each bit alone, all four, none"""
    s_edges = [enc(v) for v in (0, 1, L - 1, L, L + 1, 1 << 252, (1 << 253) - 1, (1 << 256) - 1)]
    y_edges = [enc(y | sign << 255) for y in (0, 1, 2, P - 1, P, P + 1, P + 18, (1 << 255) - 1) for sign in (0, 1)]
    assert P + 18 == (1 << 255) - 1                 # (the largest y a key can carry is the last one >= p: listed once, run twice)
    tors = pm.torsion_encodings()
    rng = random.Random(20261019)
    items = [(r + s, a) for s, a, r in itertools.product(s_edges, y_edges, y_edges)]
    items += [(r + s, a) for a, r in itertools.product(tors, tors) for s in (enc(L - 1), enc(L))]
    items += [(rng.randbytes(64), rng.randbytes(32)) for _ in range(2000)]
    sig, pk = pm.arr([s for s, _ in items]), pm.arr([a for _, a in items])
    for policy in POLICIES:
        got, want = lane(policycheck, policy, sig, pk), pm.holds_batch(policy, sig, pk)
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (hex(policy), [(items[i][0].hex(), items[i][1].hex(), int(got[i])) for i in bad[:3]])
        if policy:                                  # (the check checks: every policy rejects and accepts some of these)
            assert 0 < want.sum() < len(items)
        else:
            assert want.all()
    # the random keys are on the curve about half of the time, so the square test saw both answers
    on = sum(pm.canonical(a) for _, a in items[-2000:])
    assert 800 < on < 1200
    assert policycheck.pc_violations() == 0


def test_the_vector_files_under_the_model(policycheck, golden):
    """what the GPU test will expect of verify_edges.json + verify_torsion.json, known before a GPU visit: of the 67 accepted cases
    the four bits reject 13, 2, 17 and 17; 37 survive all four.  The lane agrees with the model on all 465"""
    cases, sig, pk, accept = pm.vector_cases(golden)
    assert (len(cases), int(accept.sum())) == (273 + 192, 40 + 27)
    rejected = [int((accept & ~pm.holds_batch(bit, sig, pk) & 1).sum()) for bit in BITS]
    assert rejected == [13, 2, 17, 17]
    assert int((accept & pm.holds_batch(STRICT, sig, pk)).sum()) == 37
    for policy in POLICIES:
        assert np.array_equal(lane(policycheck, policy, sig, pk), pm.holds_batch(policy, sig, pk)), hex(policy)
    assert policycheck.pc_violations() == 0


def test_the_policy_batch_has_what_the_gpu_test_needs(policycheck, oracle):
    """the batch of tests/test_gpu_policy.py at n = 2049: every single bit flips at least n / 16 items the oracle accepts, at
    least n / 4 survive all four, and the items built by hand (identity keys, identity R, S + k l) are accepted by the oracle"""
    n = 2049
    sig, pk, msg, want = pm.policy_batch(oracle, n)
    k = np.arange(n) % 8
    assert want[np.isin(k, (0, 1, 2, 3, 6, 7))].all() and not want[np.isin(k, (4, 5))].any()
    for bit in BITS:
        holds = pm.holds_batch(bit, sig, pk)
        assert int((want & ~holds & 1).sum()) >= n / 16, hex(bit)
        assert np.array_equal(lane(policycheck, bit, sig, pk), holds), hex(bit)
    strict = pm.holds_batch(STRICT, sig, pk)
    assert int((want & strict).sum()) >= n / 4
    assert np.array_equal(lane(policycheck, STRICT, sig, pk), strict)
    assert np.array_equal(np.nonzero(want & strict)[0], np.nonzero(np.isin(k, (0, 7)))[0])
    assert policycheck.pc_violations() == 0


class StubLibrary:
    """stands in for the loaded library: records the words eddsa_amd_set_offcurve_mode receives"""

    def __init__(self):
        self.words = []

    def eddsa_amd_set_offcurve_mode(self, word):
        self.words.append(word)


@pytest.fixture
def stub(monkeypatch):
    from libeddsa_amd import api
    s = StubLibrary()
    monkeypatch.setattr(api, "_LIB", s)
    monkeypatch.setattr(api, "_offcurve_mode", 1)
    monkeypatch.setattr(api, "_verify_policy", 0)
    return s


def test_set_verify_policy_rejects_other_bits_before_the_c_call(stub):
    import libeddsa_amd as ed
    for bad in (1, 2, 0x80, 0x1000, 0xF01, -1, 1 << 31):
        with pytest.raises(ValueError):
            ed.set_verify_policy(bad)
    assert stub.words == []
    ed.set_verify_policy(ed.VERIFY_STRICT)
    assert stub.words == [1 | 0xF00]


def test_the_two_setters_compose(stub):
    """each setter remembers its half of the word and sends both: changing one never clears the other"""
    import libeddsa_amd as ed
    assert (ed.VERIFY_S_BELOW_L, ed.VERIFY_A_CANONICAL, ed.VERIFY_A_NOT_SMALL, ed.VERIFY_R_NOT_SMALL, ed.VERIFY_STRICT) == BITS + (STRICT,)
    ed.set_verify_policy(ed.VERIFY_S_BELOW_L | ed.VERIFY_R_NOT_SMALL)
    ed.set_offcurve_mode(2)
    ed.set_offcurve_mode(False)
    ed.set_verify_policy(ed.VERIFY_A_CANONICAL)
    ed.set_offcurve_mode(True)
    ed.set_verify_policy(0)
    ed.set_offcurve_mode(7)                         # any other true value is "exact", as before
    assert stub.words == [1 | 0x900, 2 | 0x900, 0 | 0x900, 0 | 0x200, 1 | 0x200, 1, 1]


def test_the_header_defines_the_six_macros_and_declares_no_new_function():
    text, code = header_text(), header_text(strip_comments=True)
    defined = {name: int(value, 0) for name, value in re.findall(r"#define\s+(EDDSA_AMD_VERIFY_\w+)\s+(\w+)", code)}
    assert defined == MACROS
    assert STRICT == sum(BITS) == MACROS["EDDSA_AMD_VERIFY_POLICY_MASK"]
    declared = declared_names(code, r"EDDSA_AMD_DECL")
    assert len(declared) == 39 and not [name for name in declared if "policy" in name.lower() or "strict" in name.lower()]
    kernels = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "libeddsa_amd", "csrc", "eddsa_kernels.h")).read(), flags=re.S)
    edk = set(re.findall(r"\b(edk_\w+)\s*\(", kernels))
    # the 17 functions of before, which tests/fake_hip stands in for, and edk_rlc_region (the debug build's snapshot of a batch-verification
    # pass), which it does not: eddsa_amd.c refers to that one weakly
    assert len(edk) == 18 and "edk_rlc_region" in edk and not [name for name in edk if "policy" in name]
    # the changed meaning of values with bits 8-11, the missing R bit and the batch verification's caveat are stated
    flat = " ".join(text.split())
    for words in ("used to mean", "There is no R_CANONICAL bit", "keeps its documented caveat under every policy"):
        assert words in flat, words
