"""Point classification (include/eddsa_amd.h: ed25519_point_classify_batch, _dev, eddsa_amd_keyset_classify), the part that needs no
GPU: the header and the shipped library's exports, the argument checks that run before any device is touched, the launcher's header,
the Python mirror, the host side without the HIP translation unit (tests/c/classify_without_kernels.c), and the lane of the kernel
(libeddsa_amd/csrc/classify_lanes.h) compiled for the host with every bound asserted (tests/host_check/classify_check.cpp) against
the model (tests/classify_model.py: decode_reference, decode_strict, [8]P and [l]P in Python integers)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import classify_model as cm
import ed_model as em
from hostlib import ROOT, build_check, declared_names, exported_names, header_text

SZ = ctypes.c_size_t
NAMES = ("ed25519_point_classify_batch", "ed25519_point_classify_batch_dev", "eddsa_amd_keyset_classify")
INVALID_VALUE = 1                                    # hipErrorInvalidValue


# ---------------------------------------------------------------- the interface

def test_the_header_declares_the_three_names_and_the_library_exports_them():
    text = header_text(strip_comments=True)
    assert set(NAMES) <= declared_names(text, r"RFC8032_EDDSA_DECL")
    assert not set(NAMES) & declared_names(text, r"(?<![0-9A-Z_])EDDSA_AMD_DECL")
    assert set(NAMES) <= exported_names("libeddsa_amd.so")
    for name, value in (("ON_CURVE", 1), ("CANONICAL", 2), ("SMALL_ORDER", 4), ("PRIME_SUBGROUP", 8)):
        assert re.search(r"#define EDDSA_AMD_POINT_%s\s+0x0%d\n" % (name, value), text), name
    # no new debug name: what the debug library exports on top of the shipped one is what its header declares
    debug_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eddsa_amd_debug.h")).read(), flags=re.S)
    extra = exported_names("libeddsa_amd_debug.so") - exported_names("libeddsa_amd.so")
    assert extra <= set(re.findall(r"\b(eddsa_amd_\w+)\s*\(", debug_h)), extra
    assert not [n for n in extra if "classify" in n]


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*", " ", header_text()).split())
    for phrase in ("y is the low 255 bits mod p, so a y >= p counts, and x = 0 takes either sign bit",
                   "y < p, a root exists, and not x = 0 with the sign bit set. It implies ON_CURVE",
                   "[8]P is the neutral element", "[l]P is the neutral element",
                   "it is the only point with both SMALL_ORDER and PRIME_SUBGROUP",
                   "has ON_CURVE and neither of the two order bits",
                   "A string that is no curve point classifies as 0",
                   "The class depends on the 32 bytes only",
                   "(cls & 0x0F) == (EDDSA_AMD_POINT_ON_CURVE | EDDSA_AMD_POINT_CANONICAL | EDDSA_AMD_POINT_PRIME_SUBGROUP)",
                   "the cofactorless caveat of the _rlc forms is about R alone",
                   "two or more crafted R with small-order components in one group can still cancel",
                   "Under the cofactored equation (eddsa_amd_set_verify_equation) there was no caveat to begin with",
                   "`points` and `cls` may have any alignment",
                   "a NULL cls or points with n > 0 returns -hipErrorInvalidValue before any device is touched",
                   "never merged by the small-call combiner",
                   "It works on plain and on comb sets, and after eddsa_amd_shutdown",
                   "It refuses a NULL ks or cls",
                   "Out of scope: strided input (the R of packed signatures in place); _multi and single-item forms; a strict rule that "
                   "requires the subgroup inside a verify pass; four-lane forms for small batches",
                   "profiles/point_classify.txt"):
        assert phrase in text, phrase


def test_the_calls_check_their_arguments_before_any_device_is_touched():
    """against the shipped library on a machine without a GPU: -hipErrorInvalidValue, or 0 for an empty batch, shows that no device
    was asked"""
    lib = ctypes.CDLL(os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd.so"))
    points, cls = (ctypes.c_uint8 * 128)(), (ctypes.c_uint8 * 4)()
    assert lib.ed25519_point_classify_batch(None, points, SZ(4)) == -INVALID_VALUE
    assert lib.ed25519_point_classify_batch(cls, None, SZ(4)) == -INVALID_VALUE
    assert lib.ed25519_point_classify_batch(cls, points, SZ(0)) == 0
    assert lib.ed25519_point_classify_batch(None, None, SZ(0)) == 0
    assert lib.ed25519_point_classify_batch_dev(None, points, SZ(4), None) == -INVALID_VALUE
    assert lib.ed25519_point_classify_batch_dev(cls, None, SZ(4), None) == -INVALID_VALUE
    assert lib.ed25519_point_classify_batch_dev(cls, points, SZ(0), None) == 0
    assert lib.ed25519_point_classify_batch_dev(None, None, SZ(0), None) == 0
    ks = ctypes.cast((ctypes.c_uint8 * 256)(), ctypes.c_void_p)                          # "a key set": never looked into
    assert lib.eddsa_amd_keyset_classify(None, cls) == -INVALID_VALUE
    assert lib.eddsa_amd_keyset_classify(ks, None) == -INVALID_VALUE
    assert bytes(cls) == bytes(4)


def test_the_launcher_and_the_python_mirror():
    """the launcher lives in a header of its own, referenced weakly; eddsa_kernels.h keeps its 18 edk_* functions"""
    csrc = os.path.join(ROOT, "libeddsa_amd", "csrc")
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)   # noqa: E731
    kernels_h = open(os.path.join(csrc, "eddsa_kernels.h")).read()
    assert len(set(re.findall(r"\b(edk_\w+)\s*\(", strip(kernels_h)))) == 18
    classify_h = strip(open(os.path.join(csrc, "edk_classify.h")).read())
    assert set(re.findall(r"\b(edk_\w+)\s*\(", classify_h)) == {"edk_point_classify"}
    host = open(os.path.join(csrc, "eddsa_amd.c")).read()
    assert "extern __typeof__(edk_point_classify) edk_point_classify __attribute__((weak));" in host
    assert "if (!edk_point_classify) return -(int)hipErrorNotSupported;" in host
    kernels = open(os.path.join(csrc, "kernels.hip")).read()
    assert '#include "classify_kernels.h"' in kernels and "hipLaunchKernelGGL(k_point_classify," in kernels
    assert "asm" not in open(os.path.join(csrc, "classify_lanes.h")).read() + open(os.path.join(csrc, "classify_kernels.h")).read()
    pipe = open(os.path.join(csrc, "host_pipe.c")).read()
    row = re.search(r"\[OP_CLASSIFY\] = \{([^}]*\{[^}]*\}[^}]*)\}", pipe).group(1)
    for part in (".n_in = 1", ".in_w = { 32, 0, 0 }", ".out_w = 1", ".chain = 1", ".kind = KIND_NONE", ".wipe = WIPE_NONE"):
        assert part in row, part
    import sys
    sys.path.insert(0, ROOT)
    import libeddsa_amd
    assert callable(libeddsa_amd.point_classify_batch) and callable(libeddsa_amd.Keyset.classify)
    assert (libeddsa_amd.POINT_ON_CURVE, libeddsa_amd.POINT_CANONICAL, libeddsa_amd.POINT_SMALL_ORDER,
            libeddsa_amd.POINT_PRIME_SUBGROUP) == (1, 2, 4, 8) == (cm.ON_CURVE, cm.CANONICAL, cm.SMALL_ORDER, cm.PRIME_SUBGROUP)
    with pytest.raises(ValueError):
        libeddsa_amd.point_classify_batch(bytes(33))


def test_without_the_hip_translation_unit_classifying_is_not_supported(tmp_path):
    """the host side against tests/fake_hip (a fake runtime, CPU launchers without point classification), built here without a
    sanitizer: tests/c/classify_without_kernels.c, a program of its own"""
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("the HIP headers (types only) are needed to compile the host side")
    csrc, fake = os.path.join(ROOT, "libeddsa_amd", "csrc"), os.path.join(ROOT, "tests", "fake_hip")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I/opt/rocm/include", "-I" + fake]
    objs = []
    for src, cc, flags in ((os.path.join(csrc, "eddsa_amd.c"), "gcc", ["-std=c11", "-DEDDSA_BUILD"]),
                           (os.path.join(csrc, "host_pipe.c"), "gcc", ["-std=c11", "-DEDDSA_BUILD"]),
                           (os.path.join(fake, "fake_hip.c"), "gcc", ["-std=c11"]),
                           (os.path.join(fake, "fake_kernels.cpp"), "g++", ["-std=c++17", "-DED_HOST_CHECK", "-Wno-unknown-pragmas"]),
                           (os.path.join(ROOT, "tests", "c", "classify_without_kernels.c"), "gcc", ["-std=c11"])):
        objs.append(str(tmp_path / (os.path.basename(src) + ".o")))
        subprocess.check_call([cc, "-O1", "-fPIC", *flags, *inc, "-c", src, "-o", objs[-1]])
    exe = str(tmp_path / "classify_without_kernels")
    subprocess.check_call(["g++", *objs, "-o", exe, "-lpthread", "-ldl"])
    assert "libamdhip64" not in subprocess.check_output(["ldd", exe], text=True)
    r = subprocess.run([exe], env=dict(os.environ, FAKE_HIP_DEVICES="2"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "classify_without_kernels ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- the lane on the host

@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """tests/host_check/classify_check.cpp built with the flags of the hostcheck fixture (conftest.py), outside the tree"""
    h = build_check(tmp_path_factory, "classify")
    h.cc_violations.restype = ctypes.c_long
    return h


def lane(check, strings):
    strings = np.ascontiguousarray(strings)
    out = np.zeros(strings.shape[0], np.uint8)
    check.cc_classify(out.ctypes.data_as(ctypes.c_void_p), strings.ctypes.data_as(ctypes.c_void_p), SZ(strings.shape[0]))
    return out


def test_the_vectors_are_what_the_issue_lists():
    names, strings, classes = cm.vectors()
    assert strings.shape == (len(names), 32) and classes.shape == (len(names),) and 300 < len(names) < 800
    count = lambda prefix: sum(n.startswith(prefix) for n in names)   # noqa: E731
    assert count("torsion encoding") == 14 and count("random") == 100 and count("y = p + ") == 38 and count("neutral") == 1
    assert sum(" B + T" in n for n in names) == 19 * 8
    by_name = dict(zip(names, classes.tolist()))
    assert by_name["neutral"] == 0x0F                # the only point with both order bits
    assert sum(1 for c in classes.tolist() if c & cm.SMALL_ORDER and c & cm.PRIME_SUBGROUP) == \
        sum(1 for s in strings if em.decode_reference(s.tobytes()) == (0, 1))
    assert by_name["y = 1, sign 1"] == cm.ON_CURVE | cm.SMALL_ORDER | cm.PRIME_SUBGROUP      # x = 0 with the sign bit: not canonical
    assert by_name["y = -1, sign 0"] == cm.ON_CURVE | cm.CANONICAL | cm.SMALL_ORDER
    assert by_name["y = p + 1, sign 0"] == by_name["y = 1, sign 1"]                           # y >= p counts, mod p
    honest = [c for n, c in by_name.items() if " B + T" in n]
    assert sum(c == cm.REGISTRABLE for c in honest) == 19 and sum(c == (cm.ON_CURVE | cm.CANONICAL) for c in honest) == 19 * 7
    randoms = [c for n, c in by_name.items() if n.startswith("random")]
    # about half are no curve point; of those that are, seven in eight are of mixed order (the group has 8 l elements)
    assert 30 <= sum(c == 0 for c in randoms) <= 70 and all(c in (0, cm.ON_CURVE | cm.CANONICAL, cm.REGISTRABLE) for c in randoms)
    assert sum(c == cm.ON_CURVE | cm.CANONICAL for c in randoms) > 3 * sum(c == cm.REGISTRABLE for c in randoms)
    assert all(c & cm.ON_CURVE for c in classes.tolist() if c) and all(c & cm.ON_CURVE for c in classes.tolist() if c & cm.CANONICAL)


def test_the_lane_gives_every_vector_its_class(check):
    names, strings, classes = cm.vectors()
    got = lane(check, strings)
    assert not cm.mismatches(got, classes, names)
    assert check.cc_violations() == 0


def test_the_chain_alone_against_l_times_the_point(check):
    """ge_mul_l_is_neutral on its own for the decodable vectors - the subgroup bit is the chain's answer and nothing else's"""
    names, strings, classes = cm.vectors()
    for name, s, c in zip(names, strings, classes.tolist()):
        got = check.cc_mul_l_is_neutral(s.tobytes())
        assert got == (-1 if c == 0 else int(bool(c & cm.PRIME_SUBGROUP))), name
    assert check.cc_violations() == 0


def test_the_exported_digits_recompose_to_l(check):
    digits = (ctypes.c_int8 * 256)()
    check.cc_l_digits(digits)
    d = [int(x) for x in digits]
    assert set(d) <= {-1, 0, 1}
    assert sum(x << i for i, x in enumerate(d)) == em.L
    assert all(not (d[i] and d[i + 1]) for i in range(255))                     # non-adjacent: an addition is followed by a doubling
    top = check.cc_l_top()
    assert top == 252 and d[top] == 1 and not any(d[top + 1:]) and d[0] != 0
    assert sum(1 for x in d if x) == 46                                         # the leading digit and 45 additions
