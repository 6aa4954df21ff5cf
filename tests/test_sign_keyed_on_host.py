"""Signer sets (include/eddsa_amd.h: eddsa_amd_signer_*, ed25519_sign_keyed and its ctx / ph forms), the part that needs no GPU:
the header and the shipped library's exports, the argument checks that run before any device is touched, and the lane sequences
of the signer kernels (libeddsa_amd/csrc/signer_lanes.h, signer_kernels.h) compiled for the host with every bound asserted
(tests/host_check/signer_check.cpp) against the model (tests/sign_keyed_model.py: hashlib, Python integers, the oracle's base-point
multiplication) and against the unkeyed sign sequence for the same seeds."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dom2_model as dm
import sign_keyed_model as sm
from hostlib import ROOT, build_check, declared_names, exported_names, header_text

SZ = ctypes.c_size_t
L = sm.L
NAMES = ("eddsa_amd_signer_create", "eddsa_amd_signer_create_expanded", "eddsa_amd_signer_destroy", "eddsa_amd_signer_count",
         "eddsa_amd_signer_device", "eddsa_amd_signer_pubs", "ed25519_sign_keyed", "ed25519_sign_keyed_dev", "ed25519ctx_sign_keyed",
         "ed25519ctx_sign_keyed_dev", "ed25519ph_sign_keyed", "ed25519ph_sign_keyed_dev")
INVALID_VALUE = 1                                    # hipErrorInvalidValue


# ---------------------------------------------------------------- the interface

def test_the_header_declares_the_twelve_names_and_the_library_exports_them():
    assert len(set(NAMES)) == 12
    text = header_text(strip_comments=True)
    declared = declared_names(text, r"RFC8032_EDDSA_DECL")
    assert set(NAMES) <= declared
    assert set(NAMES) <= exported_names("libeddsa_amd.so")
    assert "typedef struct eddsa_amd_signer eddsa_amd_signer;" in text and "#define EDDSA_AMD_SIGNER_MAX_KEYS ((size_t)1 << 20)" in text
    # no new debug name: what the debug library exports on top of the shipped one is what its header declares
    debug_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eddsa_amd_debug.h")).read(), flags=re.S)
    extra = exported_names("libeddsa_amd_debug.so") - exported_names("libeddsa_amd.so")
    assert extra <= set(re.findall(r"\b(eddsa_amd_\w+)\s*\(", debug_h)), extra
    assert not [n for n in extra if "signer" in n or "sign_keyed" in n]


def test_the_header_states_the_contract():
    text = " ".join(re.sub(r"\n \*", " ", header_text()).split())
    for phrase in ("the scalar a mod l (32 bytes), the prefix (32 bytes) and the public key A = (a mod l) B encoded (32 bytes) - 96 bytes per key",
                   "h = SHA-512(seed), a = h[0..32) clamped, prefix = h[32..64)",
                   "sigs[i] is byte for byte what ed25519_sign_batch writes for (secs[key_idx[i]], its public key, message i)",
                   "byte for byte what ed25519ctx_sign_batch / ed25519ph_sign_batch write under the same context",
                   "used mod l and NOT clamped", "S = (r + t a) mod l", "Any 64 bytes are legal input",
                   "a = 0 mod l gives the neutral element as A and is not an error",
                   "are indistinguishable",
                   "write 64 zero bytes for an item with key_idx[i] >= count", "read nothing outside the set for it",
                   "check the whole index array first and return -hipErrorInvalidValue before anything is touched",
                   "*out is left NULL on these and on every other error",
                   "the NULL signer is refused even for n == 0", "context_len > 255",
                   "A device-pointer call whose `sigs` lie on another device returns -hipErrorInvalidValue",
                   "host-pointer calls run on the set's device", "SURVIVES eddsa_amd_shutdown",
                   "a signer set is the one place where secrets stay in HBM by design",
                   "destroy overwrites the scalars and prefixes with zeros on the device and waits for that before it frees",
                   "create zeroes its staging copy before it returns",
                   "never merged by the small-call combiner",
                   "upload 4 bytes of index and the message per item",
                   "Out of scope: creation from device pointers; _multi and single-item forms",
                   "profiles/sign_keyed.txt"):
        assert phrase in text, phrase
    # the paragraph at the top got a sentence appended; the sentence in front of it stands
    assert "zeroed in HBM before a call's stream work completes (the reference wipes its stack after the same operations" in text
    assert "A signer set (eddsa_amd_signer, at the end of this header) is the one exception by design" in text


def test_the_calls_check_their_arguments_before_any_device_is_touched():
    """against the shipped library on a machine without a GPU: -hipErrorInvalidValue shows that no device was asked.  The "signer"
    of the NULL-argument cases is never looked into: the NULL checks come first."""
    lib = ctypes.CDLL(os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd.so"))
    keys = (ctypes.c_uint8 * 128)()
    for name in ("eddsa_amd_signer_create", "eddsa_amd_signer_create_expanded"):
        fn = getattr(lib, name)
        out = ctypes.c_void_p(0xdead)
        assert fn(None, keys, SZ(1)) == -INVALID_VALUE, name
        for args in ((None, SZ(1)), (keys, SZ(0)), (keys, SZ((1 << 20) + 1))):
            out.value = 0xdead
            assert fn(ctypes.byref(out), *args) == -INVALID_VALUE and out.value is None, (name, args)
    assert lib.eddsa_amd_signer_pubs(None, keys) == -INVALID_VALUE
    lib.eddsa_amd_signer_count.restype = ctypes.c_size_t
    assert lib.eddsa_amd_signer_count(None) == 0 and lib.eddsa_amd_signer_device(None) == -1
    lib.eddsa_amd_signer_destroy(None)                                                    # NULL allowed
    sig, idx, msg = (ctypes.c_uint8 * 256)(), (ctypes.c_uint32 * 4)(), (ctypes.c_uint8 * 256)()
    sg = ctypes.cast((ctypes.c_uint8 * 256)(), ctypes.c_void_p)                          # "a signer set"
    ctx = ctypes.c_char_p(b"abc")
    n = SZ(4)
    calls = {                                        # name -> (arguments in front of n, arguments behind n)
        "ed25519_sign_keyed": ([sig, sg, idx, msg, None, SZ(32)], []),
        "ed25519_sign_keyed_dev": ([sig, sg, idx, msg, None, SZ(32)], [None]),
        "ed25519ctx_sign_keyed": ([sig, sg, idx, msg, None, SZ(32)], [ctx, SZ(3)]),
        "ed25519ctx_sign_keyed_dev": ([sig, sg, idx, msg, None, SZ(32)], [ctx, SZ(3), None]),
        "ed25519ph_sign_keyed": ([sig, sg, idx, msg], [ctx, SZ(3)]),
        "ed25519ph_sign_keyed_dev": ([sig, sg, idx, msg], [ctx, SZ(3), None]),
    }
    for name, (front, back) in calls.items():
        fn = getattr(lib, name)
        pointers = [k for k, a in enumerate(front) if a in (sig, sg, idx, msg)]
        assert len(pointers) == 4
        for k in pointers:                           # NULL sigs, signer, key_idx, fixed-length messages / prehashes
            args = list(front)
            args[k] = None
            assert fn(*args, n, *back) == -INVALID_VALUE, (name, k)
        if back:
            tail = back[2:]
            assert fn(*front, n, ctx, SZ(256), *tail) == -INVALID_VALUE, name          # a context of 256 bytes
            assert fn(*front, n, None, SZ(3), *tail) == -INVALID_VALUE, name           # no context where a length is given
        front0 = list(front)
        front0[1] = None
        assert fn(*front0, SZ(0), *back) == -INVALID_VALUE, name                       # a NULL signer with an empty batch
        assert fn(*front, SZ(0), *back) == 0, name                                     # an empty batch is done


def test_the_launchers_and_the_python_mirror():
    """the launchers live in a header of their own, referenced weakly; eddsa_kernels.h keeps its 18 edk_* functions"""
    csrc = os.path.join(ROOT, "libeddsa_amd", "csrc")
    kernels_h = open(os.path.join(csrc, "eddsa_kernels.h")).read()
    assert len(set(re.findall(r"\b(edk_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", kernels_h, flags=re.S)))) == 18
    signer_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(csrc, "edk_signer.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(edk_\w+)\s*\(", signer_h)) == {"edk_signer_build", "edk_sign_keyed"}
    host = open(os.path.join(csrc, "eddsa_amd.c")).read()
    for name in ("edk_signer_build", "edk_sign_keyed"):
        assert f"extern __typeof__({name}) {name} __attribute__((weak));" in host
    kernels = open(os.path.join(csrc, "kernels.hip")).read()
    assert '#include "signer_kernels.h"' in kernels and "k_signer_build<true>" in kernels and "k_sign_keyed_finish<true>" in kernels
    import sys
    sys.path.insert(0, ROOT)
    import libeddsa_amd
    for name in ("Signer", "signer_create", "ed25519_sign_keyed", "ed25519ctx_sign_keyed", "ed25519ph_sign_keyed"):
        assert callable(getattr(libeddsa_amd, name)), name
    for attr in ("count", "device", "pubs", "close"):
        assert hasattr(libeddsa_amd.Signer, attr)
    with pytest.raises(ValueError):
        libeddsa_amd.signer_create()


def test_without_the_hip_translation_unit_creating_a_signer_is_not_supported(tmp_path):
    """the host side against tests/fake_hip (a fake runtime, CPU launchers without signer sets), built here without a sanitizer:
    tests/c/signer_without_kernels.c, a program of its own"""
    if not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("the HIP headers (types only) are needed to compile the host side")
    csrc, fake = os.path.join(ROOT, "libeddsa_amd", "csrc"), os.path.join(ROOT, "tests", "fake_hip")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-I/opt/rocm/include", "-I" + fake]
    objs = []
    for src, cc, flags in ((os.path.join(csrc, "eddsa_amd.c"), "gcc", ["-std=c11", "-DEDDSA_BUILD"]),
                           (os.path.join(csrc, "host_pipe.c"), "gcc", ["-std=c11", "-DEDDSA_BUILD"]),
                           (os.path.join(fake, "fake_hip.c"), "gcc", ["-std=c11"]),
                           (os.path.join(fake, "fake_kernels.cpp"), "g++", ["-std=c++17", "-DED_HOST_CHECK", "-Wno-unknown-pragmas"]),
                           (os.path.join(ROOT, "tests", "c", "signer_without_kernels.c"), "gcc", ["-std=c11"])):
        objs.append(str(tmp_path / (os.path.basename(src) + ".o")))
        subprocess.check_call([cc, "-O1", "-fPIC", *flags, *inc, "-c", src, "-o", objs[-1]])
    exe = str(tmp_path / "signer_without_kernels")
    subprocess.check_call(["g++", *objs, "-o", exe, "-lpthread", "-ldl"])
    assert "libamdhip64" not in subprocess.check_output(["ldd", exe], text=True)
    r = subprocess.run([exe], env=dict(os.environ, FAKE_HIP_DEVICES="2"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "signer_without_kernels ok" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------------------- the lane sequences on the host

@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """tests/host_check/signer_check.cpp built with the flags of the hostcheck fixture (conftest.py), outside the tree"""
    h = build_check(tmp_path_factory, "signer")
    h.sgc_violations.restype = ctypes.c_long
    return h


def build(check, keys, is_expanded):
    keys = np.ascontiguousarray(keys)
    count = keys.shape[0]
    out = ctypes.create_string_buffer(96 * count)
    check.sgc_build(out, keys.ctypes.data_as(ctypes.c_void_p), count, int(is_expanded))
    return [out.raw[96 * k:96 * k + 96] for k in range(count)]


def sign(check, idx, msg, dom=None):
    sig, aux = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    check.sgc_sign(sig, aux, ctypes.c_uint32(idx), msg, SZ(len(msg)), dom, len(dom) if dom else 0)
    return sig.raw, aux.raw


VARIANTS = ((sm.PLAIN, b""), (sm.CTX, b""), (sm.CTX, b"foo"), (sm.PH, bytes(range(255))))


def test_the_scalar_import_reduces_every_256_bit_integer(check):
    """signer_lanes.h claims it for signer_expanded_lane: whatever the 32 bytes, what comes out is the value mod l, below l"""
    rng = np.random.default_rng(256)
    values = list(sm.EDGE_SCALARS) + [2 * L, 2 * L - 1, 15 * L, 15 * L + 1, 2**252, 2**253, 2**256 - L] + \
        [dm.num(rng.integers(0, 256, 32, dtype=np.uint8).tobytes()) for _ in range(2000)]
    for x in values:
        out = ctypes.create_string_buffer(32)
        check.sgc_reduce256(out, dm.le(x))
        assert dm.num(out.raw) == x % L and dm.num(out.raw) < L, hex(x)
    assert check.sgc_violations() == 0


def test_seed_sets_against_the_model_and_the_unkeyed_sequence(check, oracle):
    orc = oracle.lib
    secs, pubs = dm.keys(orc, 24, seed=24)
    rows = build(check, secs, False)
    rng = np.random.default_rng(24)
    for k, row in enumerate(rows):
        exp = sm.expand(secs[k].tobytes())
        assert row[:32] == dm.le(sm.scalar(exp)) and row[32:64] == exp[32:] and row[64:] == pubs[k].tobytes() == sm.pub(orc, exp), k
    # a set from the expansions of the same seeds is the same set
    assert build(check, np.frombuffer(b"".join(sm.expand(s.tobytes()) for s in secs), np.uint8).reshape(24, 64), True) == rows
    build(check, secs, False)
    for i in range(96):
        k = int(rng.integers(0, 24))
        msg = rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes()
        got, aux = sign(check, k, msg)
        ref, ref_aux = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        check.sgc_sign_unkeyed(ref, ref_aux, secs[k].tobytes(), pubs[k].tobytes(), msg, SZ(len(msg)))
        assert got == ref.raw == oracle.sign(secs[k].tobytes(), pubs[k].tobytes(), msg), i
        assert aux == ref_aux.raw                    # a | r: the layout and the values k_sign_point leaves
        assert got == sm.sign(orc, sm.expand(secs[k].tobytes()), msg)
    for flag, context in VARIANTS[1:]:
        for i in range(12):
            k = int(rng.integers(0, 24))
            msg = rng.integers(0, 256, 64 if flag == sm.PH else int(rng.integers(0, 200)), dtype=np.uint8).tobytes()
            got, _ = sign(check, k, msg, dm.dom2(flag, context))
            assert got == dm.sign(orc, secs[k].tobytes(), pubs[k].tobytes(), msg, flag, context), (flag, len(context), i)
    assert check.sgc_violations() == 0


def test_expanded_sets_against_the_model(check, oracle):
    """the edge scalars 0, 1, l - 1, l, l + 1, 2^255 - 1, 2^255, 2^256 - 1 and random unclamped ones"""
    orc = oracle.lib
    keys = sm.edge_keys(40, seed=40)
    rows = build(check, keys, True)
    for k, row in enumerate(rows):
        exp = keys[k].tobytes()
        a = sm.scalar(exp)
        assert dm.num(row[:32]) == a < L and row[32:64] == exp[32:] and row[64:] == sm.pub(orc, exp), k
    assert rows[0][64:] == rows[3][64:] == sm.NEUTRAL and rows[1][64:] == rows[4][64:] == dm.scale_base(orc, 1)   # a = 0, l | 1, l + 1
    assert any(dm.num(keys[k, :32].tobytes()) >= 2**255 for k in range(8, 40))                # unclamped: the top bit occurs
    rng = np.random.default_rng(41)
    for flag, context in VARIANTS:
        dom = None if flag is sm.PLAIN else dm.dom2(flag, context)
        for k in range(40):
            msg = rng.integers(0, 256, 64 if flag == sm.PH else (k * 7) % 150, dtype=np.uint8).tobytes()
            got, aux = sign(check, k, msg, dom)
            exp = keys[k].tobytes()
            assert got == sm.sign(orc, exp, msg, flag, context, a_bytes=rows[k][64:]), (flag, k)
            assert aux == dm.le(sm.scalar(exp)) + dm.le(sm.nonce(exp, msg, flag, context))
            assert sm.response_ok(got, exp, rows[k][64:], msg, flag, context)
    assert check.sgc_violations() == 0


def test_an_index_outside_the_set_leaves_zeros(check):
    keys = sm.edge_keys(9, seed=9)
    build(check, keys, True)
    for idx in (9, 10, 0xFFFFFFFF):
        for dom in (None, dm.dom2(sm.CTX, b"x")):
            got, aux = sign(check, idx, b"some message", dom)
            assert got == bytes(64) and aux == bytes(64), idx
    assert sign(check, 8, b"some message")[0] != bytes(64)
    assert check.sgc_violations() == 0
