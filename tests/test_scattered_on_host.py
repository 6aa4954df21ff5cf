"""ed25519_verify_scattered (include/eddsa_amd.h), the part that needs no GPU: the header and the shipped library's exports, the
argument checks that run before any device is touched, the launcher's header and the Python mirror, the host side without the HIP
translation unit (tests/c/scattered_without_kernels.c), and the span test and the lane of the front kernel
(libeddsa_amd/csrc/scatter_lanes.h) compiled for the host with every bound asserted (tests/host_check/scatter_check.cpp): the span
test against a three-line model, the lane's digest against hashlib and its gathered bytes against the buffer, and the same cases
once more in a program of its own under AddressSanitizer and UBSan over a buffer allocated at exactly its size."""
import ctypes
import hashlib
import itertools
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from hostlib import CHECK_FLAGS, ROOT, build_check, declared_names, exported_names, header_text

SZ = ctypes.c_size_t
U32, U64 = ctypes.c_uint32, ctypes.c_uint64
NAMES = ("ed25519_verify_scattered", "ed25519_verify_scattered_dev")
INVALID_VALUE = 1                                    # hipErrorInvalidValue
LENGTHS = (0, 47, 48, 63, 64, 175, 176, 303, 304, 1000)   # with R || A in front: the last lengths of 1, 2, 3 blocks and the first beyond
NO_KEY = bytes([2]) + bytes(31)


# ---------------------------------------------------------------- the interface

def test_the_header_declares_the_two_names_and_the_libraries_export_them():
    text = header_text(strip_comments=True)
    assert set(NAMES) <= declared_names(text, r"RFC8032_EDDSA_DECL")
    assert not set(NAMES) & declared_names(text, r"(?<![0-9A-Z_])EDDSA_AMD_DECL")
    assert set(NAMES) <= exported_names("libeddsa_amd.so") and set(NAMES) <= exported_names("libeddsa_amd_debug.so")
    one_line = " ".join(text.split())
    args = ("(uint8_t *ok, const uint8_t *data, size_t data_len, const uint32_t *sig_off, const uint32_t *pub_off, "
            "const uint32_t *msg_off, const uint32_t *msg_len, size_t n")
    assert "int ed25519_verify_scattered " + args + ");" in one_line
    assert "int ed25519_verify_scattered_dev" + args + ", void *stream);" in one_line
    debug_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eddsa_amd_debug.h")).read(), flags=re.S)
    extra = exported_names("libeddsa_amd_debug.so") - exported_names("libeddsa_amd.so")
    assert extra <= set(re.findall(r"\b(eddsa_amd_\w+)\s*\(", debug_h)), extra
    assert not [n for n in extra if "scatter" in n]


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*", " ", header_text()).split())
    for phrase in ("the signature data[sig_off[i] .. +64), the key data[pub_off[i] .. +32) and the message data[msg_off[i] .. +msg_len[i])",
                   "packed uint32, one entry per item: host memory in the first form, HBM in the second, like key_idx",
                   "ok[i] is byte for byte what ed25519_verify_batch returns for those three spans",
                   "several items sharing one message is the point of the call", "`data` is only read. `ok` must not overlap it",
                   "data_len >= 2^32 returns -hipErrorInvalidValue", "both before any device is touched", "n == 0 returns 0",
                   "computed in 64 bits, nothing wraps", "gets ok[i] = 0 under every setting",
                   "no byte of `data` is read for that item, and the verdicts of its neighbours are unaffected",
                   "an item that is not entirely in the buffer is no item",
                   "returns -hipErrorInvalidValue with `ok` untouched, like a bad ragged table",
                   "up to 3 bytes outside [data, data + data_len) lie in the same word as a byte of the buffer",
                   "never merged by the small-call combiner", "answers -hipErrorNotSupported from both",
                   "NOT chunked through the staging pipeline",
                   "Out of scope: _rlc, keyed (key_idx in place of pub_off), digest, ctx / ph and _multi forms of the scattered call; "
                   "64-bit offsets; a streaming host pipeline for the host-pointer form",
                   "profiles/verify_scattered.txt"):
        assert phrase in text, phrase


def test_the_calls_check_their_arguments_before_any_device_is_touched():
    """against the shipped library on a machine without a GPU: -hipErrorInvalidValue, or 0 for an empty batch, shows that no device
    was asked.  The host form also refuses every span that leaves the buffer there, with `ok` untouched"""
    lib = ctypes.CDLL(os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd.so"))
    data, ok = (ctypes.c_uint8 * 512)(), (ctypes.c_uint8 * 4)()
    ctypes.memset(ok, 0xEE, 4)
    idx = [(U32 * 4)(*(128 * i + d for i in range(4))) for d in (0, 64, 96)] + [(U32 * 4)(32, 32, 32, 32)]
    for fn, tail in ((lib.ed25519_verify_scattered, ()), (lib.ed25519_verify_scattered_dev, (None,))):
        for hole in range(6):
            args = [ok, data, SZ(512), *idx, SZ(4)]
            args[hole if hole < 2 else hole + 1] = None
            assert fn(*args, *tail) == -INVALID_VALUE, hole
        assert fn(ok, data, SZ(2**32), *idx, SZ(4), *tail) == -INVALID_VALUE
        assert fn(ok, data, SZ(2**40), *idx, SZ(4), *tail) == -INVALID_VALUE
        assert fn(ok, data, SZ(512), *idx, SZ(0), *tail) == 0
        assert fn(None, None, SZ(0), None, None, None, None, SZ(0), *tail) == 0
    for which, width in enumerate((64, 32, 32)):
        for off in (512 - width + 1, 512, 2**32 - 1):
            bad = [(U32 * 4)(*a) for a in idx]
            bad[which][2] = off
            assert lib.ed25519_verify_scattered(ok, data, SZ(512), *bad, SZ(4)) == -INVALID_VALUE, (which, off)
    bad = [(U32 * 4)(*a) for a in idx]
    bad[2][3], bad[3][3] = 1, 2**32 - 1
    assert lib.ed25519_verify_scattered(ok, data, SZ(512), *bad, SZ(4)) == -INVALID_VALUE
    assert bytes(ok) == b"\xee" * 4


def test_the_launcher_the_source_and_the_python_mirror():
    """the launcher lives in a header of its own, referenced weakly; eddsa_kernels.h keeps its 18 edk_* functions; the source is
    written by a sibling of verify_src; the workspace area is the slot's and freed with it"""
    csrc = os.path.join(ROOT, "libeddsa_amd", "csrc")
    strip = lambda s: re.sub(r"/\*.*?\*/", "", s, flags=re.S)   # noqa: E731
    kernels_h = open(os.path.join(csrc, "eddsa_kernels.h")).read()
    assert len(set(re.findall(r"\b(edk_\w+)\s*\(", strip(kernels_h)))) == 18
    scatter_h = strip(open(os.path.join(csrc, "edk_scatter.h")).read())
    assert set(re.findall(r"\b(edk_\w+)\s*\(", scatter_h)) == {"edk_scatter_challenge", "edk_scatter_spans_inside"}
    host = open(os.path.join(csrc, "eddsa_amd.c")).read()
    assert "extern __typeof__(edk_scatter_challenge) edk_scatter_challenge __attribute__((weak));" in host
    assert "if (v->ws.gsigs) HIP_NOTE(hipFree(v->ws.gsigs));" in host and "v->ws.gsigs = NULL;" in host
    assert "gsigs" not in host[host.index("static int ws_reserve("):host.index("static int rws_reserve(")]   # no other call pays for it
    body = host[host.index("int verify_on("):]
    body = body[:body.index("\n}\n")]
    order = [body.index(part) for part in ("gsigs_reserve(p.v)", "edk_scatter_challenge(src.sc_data", "src.sigs = p.v->ws.gsigs",
                                           "edk_verify(ok + done")]
    assert order == sorted(order)
    engine = open(os.path.join(csrc, "engine.h")).read()
    assert "static inline edk_verify_src verify_src_scattered(" in engine
    assert not re.search(r"\.sc_\w+\s*=", host)                 # the fields are written in one place
    kernels = open(os.path.join(csrc, "kernels.hip")).read()
    assert '#include "scatter_kernels.h"' in kernels
    new = open(os.path.join(csrc, "scatter_lanes.h")).read() + open(os.path.join(csrc, "scatter_kernels.h")).read()
    assert "asm" not in new and "__launch_bounds__(BLOCK, 2)\nk_scatter_challenge(" in new
    assert len(re.findall(r"\(uint64_t\)\w+ \+ \w+ <= data_len", new)) == 3      # the one place that decides
    sys.path.insert(0, ROOT)
    import libeddsa_amd
    assert callable(libeddsa_amd.ed25519_verify_scattered)
    u32 = lambda *v: np.array(v, np.uint32)   # noqa: E731
    for bad in ((np.zeros(128, np.uint16), u32(0), u32(64), u32(96), u32(32)),
                (np.zeros(128, np.uint8), np.array([0], np.int32), u32(64), u32(96), u32(32)),
                (np.zeros(128, np.uint8), u32(0), u32(64), u32(96), np.array([32], np.uint64)),
                (np.zeros(128, np.uint8), u32(0), u32(64, 64), u32(96), u32(32))):
        with pytest.raises((ValueError, TypeError)):
            libeddsa_amd.ed25519_verify_scattered(*bad)


def test_without_the_hip_translation_unit_the_pass_is_not_supported(tmp_path):
    """the host side against tests/fake_hip (a fake runtime, CPU launchers without this pass), built here without a sanitizer:
    tests/c/scattered_without_kernels.c, a program of its own"""
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("the HIP headers (types only) are needed to compile the host side")
    csrc, fake = os.path.join(ROOT, "libeddsa_amd", "csrc"), os.path.join(ROOT, "tests", "fake_hip")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I/opt/rocm/include", "-I" + fake]
    objs = []
    for src, cc, flags in ((os.path.join(csrc, "eddsa_amd.c"), "gcc", ["-std=c11", "-DEDDSA_BUILD"]),
                           (os.path.join(csrc, "host_pipe.c"), "gcc", ["-std=c11", "-DEDDSA_BUILD"]),
                           (os.path.join(fake, "fake_hip.c"), "gcc", ["-std=c11"]),
                           (os.path.join(fake, "fake_kernels.cpp"), "g++", ["-std=c++17", "-DED_HOST_CHECK", "-Wno-unknown-pragmas"]),
                           (os.path.join(ROOT, "tests", "c", "scattered_without_kernels.c"), "gcc", ["-std=c11"])):
        objs.append(str(tmp_path / (os.path.basename(src) + ".o")))
        subprocess.check_call([cc, "-O1", "-fPIC", *flags, *inc, "-c", src, "-o", objs[-1]])
    exe = str(tmp_path / "scattered_without_kernels")
    subprocess.check_call(["g++", *objs, "-o", exe, "-lpthread", "-ldl"])
    assert "libamdhip64" not in subprocess.check_output(["ldd", exe], text=True)
    r = subprocess.run([exe], env=dict(os.environ, FAKE_HIP_DEVICES="2"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "scattered_without_kernels ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- the span test and the lane on the host

@pytest.fixture(scope="module")
def check(tmp_path_factory):
    h = build_check(tmp_path_factory, "scatter")
    h.sc_violations.restype = ctypes.c_long
    h.sc_len.restype = ctypes.c_uint32
    return h


def inside(so, po, mo, ml, data_len):
    """the model: three comparisons over Python integers"""
    return so + 64 <= data_len and po + 32 <= data_len and mo + ml <= data_len


def edge(data_len, w):
    return sorted({v for v in (0, 1, *range(max(0, data_len - w - 1), data_len + 2), 2**32 - 1) if v < 2**32})


def test_the_span_test_is_the_model_on_every_edge(check):
    seen = set()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    for data_len in (0, 1, 31, 32, 33, 63, 64, 65, 96, 97, 200):
        lens = sorted({v for v in (0, 1, 32, data_len - 1, data_len, data_len + 1, 2**32 - 1) if 0 <= v < 2**32})
        msgs = [(mo, ml) for ml in lens for mo in edge(data_len, ml)]
        combos = [(so, po, mo, ml) for so, po, (mo, ml) in itertools.product(edge(data_len, 64), edge(data_len, 32), msgs)]
        want = np.array([inside(*c, data_len) for c in combos], np.uint8)
        cols = [np.ascontiguousarray(c, dtype=np.uint32) for c in zip(*combos)]
        got, got_len = np.full(len(combos), 7, np.uint8), np.zeros(len(combos), np.uint32)
        check.sc_spans(ptr(got), ptr(got_len), *(ptr(c) for c in cols), SZ(len(combos)), U64(data_len))
        assert np.array_equal(got, want), (data_len, [combos[i] for i in np.nonzero(got != want)[0][:5]])
        assert np.array_equal(got_len, np.where(want == 1, cols[3], 0))
        seen |= set(want.tolist())
    assert seen == {0, 1}
    assert not check.sc_inside(U32(0), U32(0), U32(1), U32(2**32 - 1), U64(2**32 - 1))      # 2^32: the sum does not wrap
    assert check.sc_inside(U32(0), U32(0), U32(0), U32(2**32 - 1), U64(2**32 - 1))
    assert not check.sc_inside(U32(2**32 - 1), U32(0), U32(0), U32(0), U64(2**32 - 1))


def lane_cases(data_len):
    """(sig_off, pub_off, msg_off, msg_len): every length with every residue mod 16 of each offset, the three offsets' residues
    all different within a case; shared and overlapping spans; spans that leave the buffer"""
    cases = []
    for k, ml in enumerate(LENGTHS):
        for a in range(16):
            so, po, mo = 1024 + 16 * k + a, 2048 + 16 * k + (a + 5) % 16, 3072 + 16 * k + (a + 11) % 16
            cases.append((so, po, mo, ml))
    cases += [(data_len - 64, data_len - 32, 0, data_len),       # the whole buffer as a message that holds its own signature and key
              (0, 0, 0, 0), (0, 32, 0, 64), (5, 5, 5, 1000),     # overlapping spans
              (data_len - 64, 0, data_len, 0), (7, data_len - 32, data_len - 1, 1)]
    for bad in (data_len - 63, data_len, 2**32 - 1):
        cases += [(bad, 0, 0, 10)]
    for bad in (data_len - 31, data_len, 2**32 - 1):
        cases += [(0, bad, 0, 10)]
    cases += [(0, 64, data_len - 9, 10), (0, 64, data_len, 1), (0, 64, 2**32 - 1, 1), (0, 64, 1, 2**32 - 1)]
    return cases


def lane_data(data_len=5003):
    return np.random.default_rng(20).integers(0, 256, data_len, dtype=np.uint8)


def expected_digest(data, so, po, mo, ml):
    b = data.tobytes()
    return hashlib.sha512(b[so:so + 32] + b[po:po + 32] + b[mo:mo + ml]).digest()


def test_the_lane_gathers_and_hashes_what_hashlib_hashes(check):
    data = lane_data()
    n = data.size
    residues = [set(), set(), set()]
    for so, po, mo, ml in lane_cases(n):
        sig, key, dig = (ctypes.c_uint8 * 64)(), (ctypes.c_uint8 * 32)(), (ctypes.c_uint8 * 64)()
        got = check.sc_lane(sig, key, dig, data.ctypes.data_as(ctypes.c_void_p), U64(n), U32(so), U32(po), U32(mo), U32(ml))
        if inside(so, po, mo, ml, n):
            assert got == 1
            assert bytes(sig) == data[so:so + 64].tobytes() and bytes(key) == data[po:po + 32].tobytes(), (so, po, mo, ml)
            assert bytes(dig) == expected_digest(data, so, po, mo, ml), (so, po, mo, ml)
            for r, v in zip(residues, (so, po, mo)):
                r.add(v % 16)
        else:
            assert got == 0 and bytes(sig) == bytes(64) and bytes(dig) == bytes(64) and bytes(key) == NO_KEY, (so, po, mo, ml)
    assert all(r == set(range(16)) for r in residues)
    assert check.sc_violations() == 0


def test_the_lane_reads_nothing_outside_the_documented_words(tmp_path):
    """scatter_check.cpp as a program of its own under AddressSanitizer and UBSan: the buffer is an allocation of exactly data_len
    rounded up to 4 bytes, so a read beyond the aligned words that hold it ends the program.  data_len takes all four residues
    mod 4, with messages that end at the buffer's last byte"""
    exe = str(tmp_path / "scatter_check")
    flags = [f for f in CHECK_FLAGS if f not in ("-shared", "-fPIC", "-O2")]
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSCATTER_CHECK_MAIN", *flags,
                           os.path.join(ROOT, "tests", "host_check", "scatter_check.cpp"), "-o", exe])
    for data_len in (5000, 5001, 5002, 5003):
        data = lane_data(data_len)
        cases = lane_cases(data_len)
        cases += [(0, 64, data_len - ml, ml) for ml in LENGTHS] + [(data_len - 64 - ml, 64, data_len - ml, ml) for ml in LENGTHS]
        blob = struct.pack("<I", data_len) + data.tobytes() + struct.pack("<I", len(cases))
        for so, po, mo, ml in cases:
            want = expected_digest(data, so, po, mo, ml) if inside(so, po, mo, ml, data_len) else bytes(64)
            blob += struct.pack("<4I", so, po, mo, ml) + want
        path = tmp_path / f"cases{data_len}.bin"
        path.write_bytes(blob)
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"scatter_check: ok ({len(cases)} cases" in r.stdout, r.stdout + r.stderr
