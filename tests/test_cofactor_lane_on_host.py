"""The opt-in cofactored equation of verification (include/eddsa_amd.h: eddsa_amd_set_verify_equation), the part that needs no
GPU: the Python model (tests/cofactored_model.py) against the affine group law and the oracle, the committed vectors against the
model that generates them, the lane steps of k_cofactor_points / k_cofactor_eval (libeddsa_amd/csrc/cofactor_lanes.h) compiled
for the host with every bound asserted (tests/host_check/cofactor_check.cpp) against the model, the setters and the header."""
import collections
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest

import cofactored_model as cm
import policy_model as pm
from ed_model import L, P, arr, le, num, sha
from hostlib import ROOT, build_check, exported_names, header_text

GOLDEN = "verify_cofactored.json"
COUNTS = {"a_torsion": 196, "b_honest": 16, "c_mixed": 49, "d_s_plus_kl": 16, "e_bit_flip": 16, "f_off_curve": 8, "g_mixed_s_plus_l": 49}
ACCEPTED = ("a_torsion", "b_honest", "c_mixed")


@pytest.fixture(scope="module")
def vecs():
    return cm.vectors()


@pytest.fixture(scope="module")
def cofactorcheck(tmp_path_factory):
    """tests/host_check/cofactor_check.cpp built with the flags of the hostcheck fixture (conftest.py), outside the tree"""
    h = build_check(tmp_path_factory, "cofactor")
    h.cc_violations.restype = ctypes.c_long
    return h


def lane(h, sig, pk, dig):
    sig, pk, dig = (np.ascontiguousarray(a) for a in (sig, pk, dig))
    out = np.full(len(sig), 7, np.uint8)
    h.cc_cofactored(out.ctypes.data_as(ctypes.c_void_p), sig.ctypes.data_as(ctypes.c_void_p), pk.ctypes.data_as(ctypes.c_void_p),
                    dig.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(sig)))
    return out


def digests(sig, pk, msg, prefix=b""):
    return arr([sha(prefix, sig[i, :32].tobytes(), pk[i].tobytes(), msg[i].tobytes()) for i in range(len(sig))])


# ---------------------------------------------------------------- the model

def test_the_vectors_have_their_classes_and_verdicts(vecs):
    assert collections.Counter(v["class"] for v in vecs) == COUNTS
    for v in vecs:
        assert v["accept"] == (v["class"] in ACCEPTED), v["class"]
        assert len(v["sig"]) == 64 and len(v["pub"]) == 32 and len(v["msg"]) == 32
    for v in vecs:                                       # the classes are what they say
        s = num(v["sig"][32:])
        if v["class"] in ("d_s_plus_kl", "g_mixed_s_plus_l"):
            assert L <= s < 2**256
        if v["class"] in ("a_torsion",):
            assert s == 0 and pm.small_order(v["pub"]) and pm.small_order(v["sig"][:32])
        if v["class"] == "f_off_curve":
            assert (cm.decode(v["pub"]) is None) != (cm.decode(v["sig"][:32]) is None)
        if v["class"] == "c_mixed":                      # neither point is of small order, neither lies in the prime-order subgroup
            for enc in (v["pub"], v["sig"][:32]):
                assert not pm.small_order(enc) and not cm.is_neutral(cm.pmul(L, cm.decode(enc)))


def test_the_committed_vectors_are_what_the_model_generates(vecs, golden):
    assert golden(GOLDEN) == cm.as_json(vecs)
    assert cm.from_json(json.loads(json.dumps(cm.as_json(vecs)))) == vecs


def test_where_the_two_equations_differ(vecs, oracle):
    """against the oracle's cofactorless verdicts: the equations differ in the torsion, mixed-order and S + k l classes - what
    keeps the GPU tests from passing on the unchanged pass - and never on honest signatures or on their bit flips"""
    differ = collections.Counter()
    for v in vecs:
        differ[v["class"]] += oracle.verify(v["sig"], v["pub"], v["msg"]) != v["accept"]
    assert differ["a_torsion"] >= 1 and differ["c_mixed"] >= 1 and differ["d_s_plus_kl"] >= 1, differ
    assert differ["b_honest"] == 0 and differ["e_bit_flip"] == 0, differ
    assert differ["d_s_plus_kl"] == COUNTS["d_s_plus_kl"]            # the reference does not range-check S
    # more than 64 of the first 257 tiled items are rejected by the pass itself: the list of the GPU test crosses a wave
    sig, pk, msg, accept, pick = cm.tiled(cm.arrays(vecs), 257)
    assert int((oracle.verify_batch(sig, pk, msg, 32) == 0).sum()) > 64


# ---------------------------------------------------------------- the lane on the host

def test_the_lane_against_the_model_on_every_vector(cofactorcheck, vecs):
    sig, pk, msg, accept = cm.arrays(vecs)
    got = lane(cofactorcheck, sig, pk, digests(sig, pk, msg))
    bad = np.nonzero(got != accept)[0]
    assert not len(bad), [(vecs[i]["class"], int(got[i])) for i in bad[:5]]
    assert 0 < accept.sum() < len(vecs)
    assert cofactorcheck.cc_violations() == 0


def test_the_lane_under_a_dom2_prefix_and_with_other_digests(cofactorcheck, vecs):
    """t comes from whatever 64 bytes the prepare kernel was given: vectors made under dom2(1, "ctx") verify with that digest and
    (but for the torsion class, where t does not matter) not with the plain one"""
    prefix = cm.dom2(1, b"ctx")
    dvecs = cm.vectors(prefix, mlen=64)
    sig, pk, msg, accept = cm.arrays(dvecs)
    assert np.array_equal(lane(cofactorcheck, sig, pk, digests(sig, pk, msg, prefix)), accept)
    plain = digests(sig, pk, msg)
    want = np.array([cm.accepts_t(sig[i], pk[i], num(plain[i].tobytes()) % L) for i in range(len(sig))], np.uint8)
    assert np.array_equal(lane(cofactorcheck, sig, pk, plain), want)
    cls = np.array([v["class"] for v in dvecs])
    assert want[cls == "a_torsion"].all() and not want[cls == "b_honest"].any()
    assert cofactorcheck.cc_violations() == 0


def test_the_lane_on_edges_and_random_strings(cofactorcheck, vecs):
    """S at the edges of [0, l) and of 256 bits under an honest key and R, y at the edges of [0, p) and of 255 bits as A and as
    R, and 300 seeded random triples (about a quarter have both encodings on the curve)"""
    rng = random.Random(20261019)
    honest = [v for v in vecs if v["class"] == "b_honest"][0]
    items = [(honest["sig"][:32] + le(s), honest["pub"]) for s in (0, 1, L - 1, L, L + 1, 1 << 252, (1 << 253) - 1, (1 << 256) - 1)]
    y_edges = [le(y | sign << 255) for y in (0, 1, 2, P - 1, P, P + 1, P + 18, (1 << 255) - 1) for sign in (0, 1)]
    items += [(r + bytes(32), a) for a in y_edges for r in y_edges]
    items += [(rng.randbytes(64), rng.randbytes(32)) for _ in range(300)]
    sig, pk = arr([s for s, _ in items]), arr([a for _, a in items])
    dig = arr([rng.randbytes(64) for _ in items])
    want = np.array([cm.accepts_t(s, a, num(dig[i].tobytes()) % L) for i, (s, a) in enumerate(items)], np.uint8)
    got = lane(cofactorcheck, sig, pk, dig)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), [(items[i][0].hex(), items[i][1].hex(), int(got[i])) for i in bad[:3]]
    assert 0 < want.sum() < len(items)
    both = sum(cm.decode(s[:32]) is not None and cm.decode(a) is not None for s, a in items[-300:])
    assert 40 < both < 120
    assert cofactorcheck.cc_violations() == 0


# ---------------------------------------------------------------- the setters and the header

class StubLibrary:
    """stands in for the loaded library: records what the two C setters receive"""

    def __init__(self):
        self.words, self.equations = [], []

    def eddsa_amd_set_offcurve_mode(self, word):
        self.words.append(word)

    def eddsa_amd_set_verify_equation(self, equation):
        self.equations.append(equation.value)
        return 0


def test_the_python_setter_leaves_the_other_two_words_alone(monkeypatch):
    import libeddsa_amd as ed
    from libeddsa_amd import api
    stub = StubLibrary()
    monkeypatch.setattr(api, "_LIB", stub)
    monkeypatch.setattr(api, "_offcurve_mode", 2)
    monkeypatch.setattr(api, "_verify_policy", 0x900)
    assert (ed.EQUATION_COFACTORLESS, ed.EQUATION_COFACTORED) == (0, 1)
    ed.set_verify_equation(True)
    ed.set_verify_equation(ed.EQUATION_COFACTORED)
    ed.set_verify_equation(False)
    ed.set_verify_equation()
    assert stub.equations == [1, 1, 0, 0] and stub.words == []
    assert (api._offcurve_mode, api._verify_policy) == (2, 0x900)
    ed.set_verify_policy(ed.VERIFY_S_BELOW_L)                # ... and the other setters send what they sent before
    assert stub.words == [2 | 0x100] and stub.equations == [1, 1, 0, 0]


def test_the_c_setter_returns_0_or_invalid_value():
    """no device is touched: the call takes the settings lock and stores a word"""
    import libeddsa_amd as ed
    fn = ed.library().eddsa_amd_set_verify_equation
    fn.restype = ctypes.c_int
    invalid = -1                                             # -hipErrorInvalidValue
    try:
        assert fn(ctypes.c_int(1)) == 0 and fn(ctypes.c_int(0)) == 0
        for bad in (2, -1, 0x100, 0x1000, 1 << 30):
            assert fn(ctypes.c_int(bad)) == invalid, bad
        with pytest.raises(ed.EddsaAmdError):
            ed.set_verify_equation(2)
    finally:
        assert fn(ctypes.c_int(0)) == 0


def test_the_header_declares_the_setter_and_its_two_values():
    text, code = header_text(), header_text(strip_comments=True)
    defined = {name: int(value, 0) for name, value in re.findall(r"#define\s+(EDDSA_AMD_EQUATION_\w+)\s+(\w+)", code)}
    assert defined == {"EDDSA_AMD_EQUATION_COFACTORLESS": 0, "EDDSA_AMD_EQUATION_COFACTORED": 1}
    assert re.search(r"#define\s+EDDSA_AMD_VERIFY_POLICY_MASK\s+0xF00\b", code)       # not a bit of the off-curve word
    assert re.findall(r"(\w+_DECL)\s+int\s+eddsa_amd_set_verify_equation\s*\(\s*int\s+equation\s*\)", code) == ["RFC8032_EDDSA_DECL"]
    assert "eddsa_amd_set_verify_equation" in exported_names("libeddsa_amd.so")
    flat = " ".join(text.split())
    for words in ("[8]([S]B - [t]A - R)", "x = 0 with the sign bit set is accepted", "for EVERY input", "nothing is queued",
                  "that caveat does not exist"):
        assert words in flat, words
    # the layer below: the source of a pass carries the equation next to the policy, and the lane's header exists
    kernels = open(os.path.join(ROOT, "libeddsa_amd", "csrc", "eddsa_kernels.h")).read()
    assert re.search(r"int policy;.*?int equation;", kernels, flags=re.S)
    assert os.path.exists(os.path.join(ROOT, "libeddsa_amd", "csrc", "cofactor_lanes.h"))
