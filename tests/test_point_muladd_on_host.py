"""[m]P + [a]B (include/eddsa_amd.h: ed25519_point_muladd_batch, _dev), the part that needs no GPU: the header and the shipped
library's exports, the argument checks that run before any device is touched, the launcher's header, the rows of the host pipeline,
the Python mirror, the host side without the HIP translation unit (tests/c/muladd_without_kernels.c), and the lane sequence of the
pass (libeddsa_amd/csrc/muladd_lanes.h: point_muladd_prepare_lane, then lanes.h: verify_main_lane and encode_lane) compiled for the
host with every bound asserted (tests/host_check/muladd_check.cpp) against the model (tests/point_muladd_model.py: Python integers)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ed_model as em
import point_muladd_model as mm
from hostlib import ROOT, build_check, declared_names, exported_names, header_text

SZ = ctypes.c_size_t
NAMES = ("ed25519_point_muladd_batch", "ed25519_point_muladd_batch_dev")
INVALID_VALUE = 1                                    # hipErrorInvalidValue


# ---------------------------------------------------------------- the interface

def test_the_header_declares_the_two_names_and_the_libraries_export_them():
    text = header_text(strip_comments=True)
    assert set(NAMES) <= declared_names(text, r"RFC8032_EDDSA_DECL")
    assert not set(NAMES) & declared_names(text, r"(?<![0-9A-Z_])EDDSA_AMD_DECL")
    assert set(NAMES) <= exported_names("libeddsa_amd.so") and set(NAMES) <= exported_names("libeddsa_amd_debug.so")
    assert re.search(r"#define EDDSA_AMD_NO_POINT_BYTE0 0x02\b", text)
    one_line = " ".join(text.split())
    assert ("int ed25519_point_muladd_batch (uint8_t *out, const uint8_t *points, const uint8_t *mul, const uint8_t *add, size_t n);"
            in one_line)
    assert ("int ed25519_point_muladd_batch_dev(uint8_t *out, const uint8_t *points, const uint8_t *mul, const uint8_t *add, size_t n, "
            "void *stream);" in one_line)
    # no new debug name: what the debug library exports on top of the shipped one is what its header declares
    debug_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eddsa_amd_debug.h")).read(), flags=re.S)
    extra = exported_names("libeddsa_amd_debug.so") - exported_names("libeddsa_amd.so")
    assert extra <= set(re.findall(r"\b(eddsa_amd_\w+)\s*\(", debug_h)), extra
    assert not [n for n in extra if "muladd" in n]


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*", " ", header_text()).split())
    for phrase in ("NOT FOR SECRETS", "the scalars lie unwiped in the verify workspace",
                   "out[i] is the canonical RFC 8032 encoding of [m_i]P_i + [a_i]B",
                   "read as integers in [0, 2^256): not clamped, not range-checked",
                   "a is reduced mod l (B has order l), m is reduced mod 8 l and never mod l",
                   "mul == NULL means every m_i = 1 (soft derivation, A + [z]B)", "add == NULL means every a_i = 0 (blinding, [h]A)",
                   "with both NULL the call re-encodes P canonically",
                   "y is the low 255 bits mod p, and x = 0 takes either sign bit",
                   "a string that is no curve point gives out[i] = 02 00 .. 00",
                   "Its y = 2 is on no curve point, so it can never be a valid result",
                   "rejects its items in reject mode and under the cofactored equation",
                   "The neighbours of such an item are unaffected",
                   "The off-curve mode, the strict rules and the equation play no part",
                   "`out` may be the very buffer `points` (in-place derivation). Any other overlap is undefined",
                   "a NULL out or points with n > 0 returns -hipErrorInvalidValue before any device is touched",
                   "enqueues on `stream` and returns without synchronising",
                   "never merged by the small-call combiner",
                   "answers -hipErrorNotSupported from both",
                   "Out of scope: constant-time forms; four-lane forms for small passes; _multi and single-item forms; a key-set "
                   "constructor that derives in place", "hashing the derivation scalars, which is the caller's scheme",
                   "profiles/point_muladd.txt"):
        assert phrase in text, phrase


def test_the_calls_check_their_arguments_before_any_device_is_touched():
    """against the shipped library on a machine without a GPU: -hipErrorInvalidValue, or 0 for an empty batch, shows that no device
    was asked"""
    lib = ctypes.CDLL(os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd.so"))
    points, mul, add, out = ((ctypes.c_uint8 * 128)() for _ in range(4))
    ctypes.memset(out, 0xEE, 128)
    for m in (mul, None):
        for a in (add, None):
            assert lib.ed25519_point_muladd_batch(None, points, m, a, SZ(4)) == -INVALID_VALUE
            assert lib.ed25519_point_muladd_batch(out, None, m, a, SZ(4)) == -INVALID_VALUE
            assert lib.ed25519_point_muladd_batch(out, points, m, a, SZ(0)) == 0
            assert lib.ed25519_point_muladd_batch_dev(None, points, m, a, SZ(4), None) == -INVALID_VALUE
            assert lib.ed25519_point_muladd_batch_dev(out, None, m, a, SZ(4), None) == -INVALID_VALUE
            assert lib.ed25519_point_muladd_batch_dev(out, points, m, a, SZ(0), None) == 0
    assert lib.ed25519_point_muladd_batch(None, None, None, None, SZ(0)) == 0
    assert lib.ed25519_point_muladd_batch_dev(None, None, None, None, SZ(0), None) == 0
    assert bytes(out) == b"\xee" * 128


def test_the_launcher_the_pipeline_rows_and_the_python_mirror():
    """the launcher lives in a header of its own, referenced weakly; eddsa_kernels.h keeps its 18 edk_* functions; the chain is
    k_verify_main itself"""
    csrc = os.path.join(ROOT, "libeddsa_amd", "csrc")
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)   # noqa: E731
    kernels_h = open(os.path.join(csrc, "eddsa_kernels.h")).read()
    assert len(set(re.findall(r"\b(edk_\w+)\s*\(", strip(kernels_h)))) == 18
    muladd_h = strip(open(os.path.join(csrc, "edk_muladd.h")).read())
    assert set(re.findall(r"\b(edk_\w+)\s*\(", muladd_h)) == {"edk_point_muladd"}
    host = open(os.path.join(csrc, "eddsa_amd.c")).read()
    assert "extern __typeof__(edk_point_muladd) edk_point_muladd __attribute__((weak));" in host
    assert host.count("if (!edk_point_muladd) return -(int)hipErrorNotSupported;") == 2
    body = host[host.index("int muladd_on("):]
    body = body[:body.index("\n}\n")]
    for part in ("take_async_error(e)", "pass_open(&p, e, n, PASS_WS, st)", "done += CHUNK_MAX", "pass_close(&p, rc)"):
        assert part in body, part
    kernels = open(os.path.join(csrc, "kernels.hip")).read()
    assert '#include "muladd_kernels.h"' in kernels
    launcher = kernels[kernels.index("hipError_t edk_point_muladd("):]
    launcher = launcher[:launcher.index("\n}\n")]
    order = [launcher.index(k) for k in ("EDK_LAUNCH(k_point_muladd_prepare,", "EDK_LAUNCH(k_verify_main,", "EDK_LAUNCH(k_point_muladd_finish,")]
    assert order == sorted(order)
    new = open(os.path.join(csrc, "muladd_lanes.h")).read() + open(os.path.join(csrc, "muladd_kernels.h")).read()
    assert "asm" not in new and "finish_batch8(muladd_finish_policy{" in new and "den_commit(z, good, acc, k, K);" in new
    pipe = open(os.path.join(csrc, "host_pipe.c")).read()
    rows = {name: re.search(r"\[%s\] = \{([^}]*\{[^}]*\}[^}]*)\}" % name, pipe).group(1)
            for name in ("OP_POINT_MULADD", "OP_POINT_MULADD_MUL", "OP_POINT_MULADD_ADD", "OP_POINT_MULADD_POINTS")}
    for name, widths in (("OP_POINT_MULADD", ".n_in = 3, .in_w = { 32, 32, 32 }"), ("OP_POINT_MULADD_MUL", ".n_in = 2, .in_w = { 32, 32, 0 }"),
                         ("OP_POINT_MULADD_ADD", ".n_in = 2, .in_w = { 32, 32, 0 }"), ("OP_POINT_MULADD_POINTS", ".n_in = 1, .in_w = { 32, 0, 0 }")):
        for part in (widths, ".out_w = 32", ".chain = 1", ".kind = KIND_NONE", ".wipe = WIPE_NONE"):
            assert part in rows[name], (name, part)
    import sys
    sys.path.insert(0, ROOT)
    import libeddsa_amd
    assert callable(libeddsa_amd.point_muladd_batch) and libeddsa_amd.NO_POINT == bytes([2]) + bytes(31) == mm.NO_POINT
    for bad in ((bytes(33), None, None), (bytes(64), bytes(32), None), (bytes(64), None, bytes(96)), (bytes(32), bytes(31), None)):
        with pytest.raises(ValueError):
            libeddsa_amd.point_muladd_batch(*bad)
    with pytest.raises(ValueError):
        libeddsa_amd.point_muladd_batch(np.zeros((2, 32), np.uint8), out=np.zeros((2, 32), np.uint8))


def test_without_the_hip_translation_unit_the_pass_is_not_supported(tmp_path):
    """the host side against tests/fake_hip (a fake runtime, CPU launchers without this pass), built here without a sanitizer:
    tests/c/muladd_without_kernels.c, a program of its own"""
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("the HIP headers (types only) are needed to compile the host side")
    csrc, fake = os.path.join(ROOT, "libeddsa_amd", "csrc"), os.path.join(ROOT, "tests", "fake_hip")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I/opt/rocm/include", "-I" + fake]
    objs = []
    for src, cc, flags in ((os.path.join(csrc, "eddsa_amd.c"), "gcc", ["-std=c11", "-DEDDSA_BUILD"]),
                           (os.path.join(csrc, "host_pipe.c"), "gcc", ["-std=c11", "-DEDDSA_BUILD"]),
                           (os.path.join(fake, "fake_hip.c"), "gcc", ["-std=c11"]),
                           (os.path.join(fake, "fake_kernels.cpp"), "g++", ["-std=c++17", "-DED_HOST_CHECK", "-Wno-unknown-pragmas"]),
                           (os.path.join(ROOT, "tests", "c", "muladd_without_kernels.c"), "gcc", ["-std=c11"])):
        objs.append(str(tmp_path / (os.path.basename(src) + ".o")))
        subprocess.check_call([cc, "-O1", "-fPIC", *flags, *inc, "-c", src, "-o", objs[-1]])
    exe = str(tmp_path / "muladd_without_kernels")
    subprocess.check_call(["g++", *objs, "-o", exe, "-lpthread", "-ldl"])
    assert "libamdhip64" not in subprocess.check_output(["ldd", exe], text=True)
    r = subprocess.run([exe], env=dict(os.environ, FAKE_HIP_DEVICES="2"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "muladd_without_kernels ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- the model's vectors

def test_the_vectors_are_what_the_issue_lists():
    names, points, mul, add, out = mm.vectors()
    n = len(names)
    assert points.shape == mul.shape == add.shape == out.shape == (n, 32) and 200 < n < 600
    count = lambda part: sum(part in x for x in names)   # noqa: E731
    assert count(" B + T") >= 5 * 8 * 2 and count("torsion encoding") == 28 and count("neutral,") == 2 and count("y = p + ") == 38
    assert count("sign 1, m = ") == 4 and count("the no-point string") == 2 and count("off the curve") == 12
    scalars = {em.num(r.tobytes()) for r in mul} & {em.num(r.tobytes()) for r in add}
    assert set(mm.SCALARS) <= scalars and len(mm.SCALARS) == 18
    assert sum(em.num(r.tobytes()) >= 2**255 for r in mul) > 20 and sum(em.num(r.tobytes()) >= 2**255 for r in add) > 20
    by = {x: out[i].tobytes() for i, x in enumerate(names)}
    pairs = [x for x in names if x.startswith("pair mod l:") and x.endswith(", m")]
    assert len(pairs) == 4 and all(by[x] != by[x + " + l"] for x in pairs)
    pairs = [x for x in names if x.startswith("pair mod 8l:") and x.endswith(", m")]
    assert len(pairs) == 4 and all(by[x] == by[x + " + 8 l"] for x in pairs)
    assert sum(by[x] == mm.NEUTRAL for x in names if x.endswith("the neutral element")) == 5
    off = [i for i in range(n) if em.decode_reference(points[i].tobytes()) is None]
    assert len(off) >= 14 + 14 and all(out[i].tobytes() == mm.NO_POINT for i in off)
    assert all(em.decode_strict(out[i].tobytes()) is not None for i in range(n) if i not in off)    # every result is canonical
    ys = {em.num(r.tobytes()) & em.MASK255 for r in out}
    assert {0, 1, em.P - 1} <= ys                    # results of order 4 (y = 0), 1 and 2 (x = 0)
    # the model with an array left out is the model with m = 1 / a = 0 spelled out
    ones, zeros = em.arr([em.le(1)] * n, 32), np.zeros((n, 32), np.uint8)
    assert np.array_equal(mm.expected(points, None, add), mm.expected(points, ones, add))
    assert np.array_equal(mm.expected(points, mul, None), mm.expected(points, mul, zeros))


# ---------------------------------------------------------------- the lanes on the host

@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """tests/host_check/muladd_check.cpp built with the flags of the hostcheck fixture (conftest.py), outside the tree"""
    h = build_check(tmp_path_factory, "muladd")
    h.mc_violations.restype = ctypes.c_long
    return h


def lanes(check, points, mul, add):
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    points, mul, add = (None if a is None else np.ascontiguousarray(a) for a in (points, mul, add))
    out, flags = np.zeros_like(points), np.zeros(points.shape[0], np.uint8)
    check.mc_muladd(ptr(out), ptr(flags), ptr(points), ptr(mul), ptr(add), SZ(points.shape[0]))
    return out, flags


@pytest.mark.parametrize("with_mul, with_add", [(True, True), (True, False), (False, True), (False, False)])
def test_the_lane_sequence_gives_every_vector_its_bytes(check, with_mul, with_add):
    names, points, mul, add, out = mm.vectors()
    mul, add = mul if with_mul else None, add if with_add else None
    want = out if with_mul and with_add else mm.expected(points, mul, add)
    got, flags = lanes(check, points, mul, add)
    assert not mm.mismatches(got, want, names)
    on = np.array([em.decode_reference(p.tobytes()) is not None for p in points], np.uint8)
    assert np.array_equal(flags, on)
    assert check.mc_violations() == 0


def test_the_centred_scalar_is_m_mod_8l(check):
    """point_muladd_scalar_lane alone: m' = m (mod 8 l) with |m'| <= 4 l, for the scalar list, its neighbours and random values"""
    rng = np.random.default_rng(8)
    values = list(mm.SCALARS) + [k * em.L + d for k in range(17) for d in (-1, 0, 1) if 0 <= k * em.L + d < 2**256]
    values += [em.num(rng.integers(0, 256, 32, dtype=np.uint8).tobytes()) for _ in range(200)]
    for m in values:
        mag = (ctypes.c_uint8 * 32)()
        neg = check.mc_scalar(mag, em.le(m))
        v = -em.num(bytes(mag)) if neg else em.num(bytes(mag))
        assert (v - m) % (8 * em.L) == 0 and abs(v) <= 4 * em.L and abs(v) < 2**255, hex(m)
        assert not (neg and v == 0), hex(m)
    assert check.mc_violations() == 0
