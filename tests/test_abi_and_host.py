"""CPU-side checks of the product: the C-ABI library loads and exports every symbol the public
headers declare, fails loudly without a GPU (no CPU fallback), and the host-side logic (argument
checks, sharding, workload generator, multi-rank gather over gloo) behaves."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from hostlib import ROOT, declared_names, exported_names, header_text


def _lib_path(name="libeddsa_amd.so"):
    path = os.path.join(ROOT, "libeddsa_amd", name)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", ROOT, "libeddsa_amd/" + name])
    return path


def _declared(header):
    return declared_names(header_text(strip_comments=True, name=header), r"EDDSA(?:_AMD)?_DECL")


def test_library_exports_every_declared_symbol():
    """The shipped library exports the reference's 13 names (default visibility on the public names only:
    /root/reference/lib/eddsa.h:12-28) and the batched set of include/eddsa_amd.h - and NOTHING else: the test and measurement
    hooks of include/eddsa_amd_debug.h exist only in libeddsa_amd_debug.so, the same object files plus those functions
    (VERDICT r05 #5), which is what the tests, bench.py and tools/ load."""
    lib = ctypes.CDLL(_lib_path())
    product = _declared("eddsa.h") | _declared("eddsa_amd.h")
    debug = _declared("eddsa_amd_debug.h")
    assert {"ed25519_genpub", "ed25519_sign", "ed25519_verify", "x25519_base", "x25519", "pk_ed25519_to_x25519",
            "sk_ed25519_to_x25519", "eddsa_genpub", "eddsa_sign", "eddsa_verify", "DH", "eddsa_pk_eddsa_to_dh",
            "eddsa_sk_eddsa_to_dh"} <= product                    # the reference's 13 (lib/eddsa.h:44-113)
    assert len(product) >= 13 + 14 + 5 and len(debug) >= 10 and not (product & debug)
    for n in product:
        assert hasattr(lib, n), n
    assert exported_names(_lib_path()) == product, exported_names(_lib_path()) ^ product                     # nothing else leaks out
    dbg = _lib_path("libeddsa_amd_debug.so")
    assert exported_names(dbg) == product | debug, exported_names(dbg) ^ (product | debug)
    # the debug build is the product's objects plus the hooks: the same kernels (one compilation of each .hip file serves both)
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(DEBUGLIB): $(BUILD)/kernels.o $(BUILD)/rlc.o $(BUILD)/eddsa_amd.dbg.o $(BUILD)/host_pipe.dbg.o" in mk
    assert "$(LIB): $(BUILD)/kernels.o $(BUILD)/rlc.o $(BUILD)/eddsa_amd.o $(BUILD)/host_pipe.o" in mk


def test_the_wave_share_constants_match_the_committed_counters():
    """k_verify_exact_lane_chain takes its share of the wave slots from three cost constants (executed instructions per item, in
    thousands: its own, k_verify_main_half's, k_verify_main's; csrc/kernels.hip).  They drift when the kernels change: held
    against the counters committed with the profile of the same sources (profiles/pmc_summary.json: SQ_INSTS_VALU counts wave
    instructions; the chain's row comes from self-check mode 2, 2^20 items alone on the chip; the main kernel's from config 2)"""
    import json
    src = open(os.path.join(ROOT, "libeddsa_amd", "csrc", "kernels.hip")).read()
    chain = int(re.search(r"EXACT_CHAIN_COST = (\d+);", src).group(1))
    half, full = (int(x) for x in re.search(r"half_main \? (\d+)u : (\d+)u", src).groups())
    pmc = json.load(open(os.path.join(ROOT, "profiles", "pmc_summary.json")))
    per_item = lambda k: pmc[k]["SQ_INSTS_VALU"] * 64 / (1 << 20) / 1000          # noqa: E731
    assert abs(per_item("ed::k_verify_exact_lane_chain") - chain) < 0.03 * chain
    assert abs(per_item("ed::k_verify_main_half") - half) < 0.03 * half              # (over the on-curve list: 0.8 % fewer items than 2^20)
    if pmc.get("ed::k_verify_main", {}).get("SQ_INSTS_VALU"):
        assert abs(per_item("ed::k_verify_main") - full) < 0.05 * full
    assert 1.3 < full / half < 1.6                                                    # 252 doublings against 132, both with their additions


def test_the_product_header_holds_no_test_hooks():
    """include/eddsa_amd.h lists what a caller binds (the shape of the reference's lib/eddsa.h:44-113:
    nothing but the functions); fault injectors, route selection, probes and traces live in eddsa_amd_debug.h"""
    product = _declared("eddsa_amd.h")
    assert not [n for n in product if "debug" in n or n in (
        "eddsa_amd_set_verify_algo", "eddsa_amd_set_pipeline", "eddsa_amd_set_pipeline_chain", "eddsa_amd_secret_residue",
        "eddsa_amd_halve_rejected", "eddsa_amd_set_profiling", "eddsa_amd_verify_phase_ms", "eddsa_amd_combiner_stats",
        "eddsa_amd_dump_tables")]
    text = open(os.path.join(ROOT, "include", "eddsa_amd.h")).read()
    assert "eddsa_amd_debug.h" in text and "#include \"eddsa_amd_debug.h\"" not in text    # mentioned, not pulled in


def test_the_reference_selftests_compile_against_our_header():
    """the reference's runnable selftests (test/selftest-x25519.c, -convert.c, -x25519_base.c) compile unchanged against
    include/eddsa.h: the header IS the reference's contract (lib/eddsa.h:44-113).  The oracle's recipe compiles them where
    the reference's sources lie (nothing is copied) into oracle/_ref/ at build time; this test reads what it left.  The
    x25519 one links and passes against the GPU library through tests/c/selftest_dropin.c, which drives the same table.
    Each object must have been compiled against include/eddsa.h AS IT IS NOW: the recipe records the header's sha256 beside
    the object (file times say when a checkout or a copy wrote a file, not whether its content changed)."""
    import hashlib
    ref = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(ref, "libeddsa_ref.so")):
        pytest.skip("oracle/_ref not built: no reference checkout where the project was built")
    header = hashlib.sha256(open(os.path.join(ROOT, "include", "eddsa.h"), "rb").read()).hexdigest()
    for name in ("selftest-x25519", "selftest-convert", "selftest-x25519_base"):
        obj, log, stamp = (os.path.join(ref, name + ext) for ext in (".o", ".log", ".header"))
        assert os.path.exists(obj), name + ": " + (open(log).read() if os.path.exists(log) else "not compiled: rebuild oracle/_ref")
        assert os.path.exists(stamp), name + ": no record of the header it was compiled against: rebuild oracle/_ref"
        assert open(stamp).read().split()[0] == header, name + ": compiled before include/eddsa.h changed: rebuild oracle/_ref"


def test_the_hooks_are_inert_until_armed():
    """the fault injectors answer EDDSA_AMD_HOOKS_OFF and do nothing when nobody called eddsa_amd_debug_init(..,
    EDDSA_AMD_TEST_HOOKS) (no GPU needed: they are refused before any device work)"""
    lib = ctypes.CDLL(_lib_path("libeddsa_amd_debug.so"))
    off = -100002
    assert lib.eddsa_amd_debug_fail_next_host_call() == off
    assert lib.eddsa_amd_debug_fail_hip_call(3) == off
    lib.eddsa_amd_strerror.restype = ctypes.c_char_p
    assert b"hooks not armed" in lib.eddsa_amd_strerror(off)      # (not whatever HIP calls error 100002)


def test_the_layer_probes_are_a_library_of_their_own():
    """the probe kernels (k_debug_layer spilled 107 registers) and their entry points used to ship inside
    libeddsa_amd.so.  Now: libeddsa_amd_probe.so exports exactly what include/eddsa_amd_probe.h declares, the product
    exports nothing of the kind, its device code holds no probe kernel, and no product kernel spills a vector register
    or uses scratch memory (code-object metadata of the shipped library)"""
    probe = os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd_probe.so")
    if not os.path.exists(probe):
        subprocess.check_call(["make", "-C", ROOT, "probe"])
    declared = declared_names(header_text(strip_comments=True, name="eddsa_amd_probe.h"), r"EDDSA_PROBE_DECL")
    assert declared == {"eddsa_amd_probe_layer", "eddsa_amd_probe_halve"}
    assert exported_names(probe) == declared
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib_path()], text=True)
    assert not [l for l in out.splitlines() if "probe" in l or "debug_layer" in l or "debug_halve" in l]
    ldd = subprocess.check_output(["ldd", probe], text=True)
    assert "libeddsa" not in ldd and "oracle" not in ldd             # self-contained: HIP and libc only
    # the product's code objects (one per .hip file, bundled in .hip_fatbin): kernel names and resources from their metadata
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-readelf")):
        pytest.skip("no ROCm LLVM tools here")
    import struct
    import tempfile
    notes = ""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, _lib_path(), os.path.join(d, "scratch.so")])
        blob = open(fat, "rb").read()
        magic = b"__CLANG_OFFLOAD_BUNDLE__"
        starts = [m.start() for m in re.finditer(magic, blob)]
        assert len(starts) == 2                                       # kernels.hip and rlc.hip
        for k, at in enumerate(starts):
            (count,) = struct.unpack_from("<Q", blob, at + len(magic))
            pos = at + len(magic) + 8
            for _ in range(count):
                off, size, tlen = struct.unpack_from("<QQQ", blob, pos)
                triple = blob[pos + 24:pos + 24 + tlen].decode()
                pos += 24 + tlen
                if "gfx950" in triple:
                    co = os.path.join(d, f"co{k}")
                    open(co, "wb").write(blob[at + off:at + off + size])
                    notes += subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], text=True)
    names = re.findall(r"\.name:\s+(\S+)", notes)
    assert len(names) > 30 and not [n for n in names if "debug" in n or "probe" in n], [n for n in names if "debug" in n]
    assert all(int(v) == 0 for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", notes))
    assert all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes))


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import libeddsa_amd as ed
    with pytest.raises(ed.EddsaAmdError):
        ed.x25519_batch(np.zeros((4, 32), np.uint8), np.zeros((4, 32), np.uint8))
    with pytest.raises(ed.EddsaAmdError):
        ed.ed25519_verify_batch(np.zeros((1, 64), np.uint8), np.zeros((1, 32), np.uint8), np.zeros((1, 8), np.uint8))
    # the eddsa.h single-item functions have no error channel: they abort the process
    code = ("import libeddsa_amd as ed; ed.x25519(bytes(32), bytes(32))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr


def test_product_does_not_reference_the_oracle():
    """no file of the product imports, links or loads anything under oracle/"""
    for base, _, files in os.walk(os.path.join(ROOT, "libeddsa_amd")):
        for f in files:
            if f.endswith((".py", ".c", ".h", ".hip")):
                text = open(os.path.join(base, f)).read()
                assert "liboracle" not in text and "orc_" not in text and "_ref" not in text, f
    out = subprocess.check_output(["ldd", _lib_path()], text=True)
    assert "oracle" not in out


def test_device_code_has_no_folded_dpp_operations(tmp_path):
    """hipcc's DPP combiner can emit v_subrev_u32_dpp, which this hardware executes as dpp(src1) - src0 instead of
    src1 - dpp(src0) (tools/microbench/dpp_subrev.hip).  The product is built with the combiner off: in the
    device code of the shipped library every DPP instruction is a plain v_mov_b32_dpp"""
    import shutil
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump in this image")
    so = tmp_path / "lib.so"
    shutil.copy(_lib_path(), so)
    subprocess.run([objdump, "--offloading", str(so)], check=True, capture_output=True)     # writes the bundles next to the input
    objs = [f for f in os.listdir(tmp_path) if "amdgcn" in f]
    assert objs, os.listdir(tmp_path)
    dpp = []
    for f in objs:
        dis = subprocess.run([objdump, "-d", str(tmp_path / f)], check=True, capture_output=True, text=True).stdout
        dpp += [ln.split()[0] for ln in dis.splitlines() if "_dpp" in ln and ln.strip().startswith("v_")]
    assert len(dpp) > 500 and set(dpp) == {"v_mov_b32_dpp"}, sorted(set(dpp))


def test_argument_validation():
    import libeddsa_amd as ed
    with pytest.raises(ValueError):
        ed.x25519_batch(np.zeros(33, np.uint8), np.zeros(33, np.uint8))
    with pytest.raises(ValueError):
        ed.x25519_batch(np.zeros((2, 32), np.uint8), np.zeros((3, 32), np.uint8))
    with pytest.raises(TypeError):
        ed.ed25519_genpub_batch(np.zeros((2, 32), np.int32))
    with pytest.raises(ValueError):
        ed.ed25519_verify_batch(np.zeros((2, 64), np.uint8), np.zeros((2, 32), np.uint8), np.zeros(5, np.uint8))
    with pytest.raises(ValueError):
        ed.ed25519_verify_batch(np.zeros((2, 64), np.uint8), np.zeros((2, 32), np.uint8), np.zeros(5, np.uint8),
                                msg_off=[0, 3, 9])
    with pytest.raises(ValueError):
        ed.ed25519_sign(bytes(31), bytes(32), b"")
    # records: every field must lie inside the record (checked in C, before any device work)
    with pytest.raises(ed.EddsaAmdError):
        ed.ed25519_verify_records(np.zeros((2, 100), np.uint8), 40, 0, 0, 32)      # signature sticks out
    with pytest.raises(ed.EddsaAmdError):
        ed.ed25519_verify_records(np.zeros((2, 128), np.uint8), 0, 64, 100, 32)    # message sticks out
    with pytest.raises(ValueError):
        ed.ed25519_verify_records(np.zeros(128, np.uint8), 0, 64, 96, 32)
    # the five calls that carry messages share one driver: each refuses the same bad inputs, in the words it always used
    for fn, first, w in ((ed.ed25519_verify_batch, "sigs", 64), (ed.ed25519_verify_batch_rlc, "sigs", 64),
                         (ed.ed25519_sign_batch, "secs", 32), (ed.ed25519_verify_batch_multi, "sigs", 64),
                         (ed.ed25519_sign_batch_multi, "secs", 32)):
        a, p, m = np.zeros((2, w), np.uint8), np.zeros((2, 32), np.uint8), np.zeros(6, np.uint8)
        for args, kw, exc, text in (
                ((a, np.zeros((3, 32), np.uint8), m), {}, ValueError, f"{fn.__name__}: {first} and pubs disagree on the batch size"),
                ((a, p, np.zeros(5, np.uint8)), {}, ValueError, "msgs: size is not a multiple of the batch size; pass msg_len or msg_off"),
                ((a, p, m), {"msg_off": [0, 3]}, ValueError, "msg_off: expected n+1 offsets within msgs"),              # wrong length
                ((a, p, m), {"msg_off": [0, 3, 9]}, ValueError, "msg_off: expected n+1 offsets within msgs"),           # runs past msgs
                ((a.astype(np.int32), p, m), {}, TypeError, f"{first}: expected uint8 data"),
                ((a, p.astype(np.int32), m), {}, TypeError, "pubs: expected uint8 data"),
                ((a, p, m.astype(np.int32)), {}, TypeError, "msgs: expected uint8 data"),
                ((np.zeros(2 * w + 1, np.uint8), p, m), {}, ValueError, f"{first}: size {2 * w + 1} is not a multiple of {w}")):
            with pytest.raises(exc) as e:
                fn(*args, **kw)
            assert type(e.value) is exc and str(e.value) == text, (fn.__name__, text, e.value)
        # a doubly wrong call: the plain and the sign form look at msgs first, the other three at the batch sizes
        msgs_first = fn in (ed.ed25519_verify_batch, ed.ed25519_sign_batch)
        with pytest.raises(TypeError if msgs_first else ValueError) as e:
            fn(a, np.zeros((3, 32), np.uint8), m.astype(np.int32))
        assert str(e.value) == ("msgs: expected uint8 data" if msgs_first else f"{fn.__name__}: {first} and pubs disagree on the batch size")
    # the thirteen eddsa.h names: every fixed-width argument of each, one byte short (refused before the C function is called)
    sec, pub, sig = ("sec", 32), ("pub", 32), ("sig", 64)
    singles = {"ed25519_genpub": (sec,), "ed25519_sign": (sec, pub, b""), "ed25519_verify": (sig, pub, b""),
               "x25519_base": (("scalar", 32),), "x25519": (("scalar", 32), ("point", 32)), "pk_ed25519_to_x25519": (pub,),
               "sk_ed25519_to_x25519": (sec,), "eddsa_genpub": (sec,), "eddsa_sign": (sec, pub, b""), "eddsa_verify": (sig, pub, b""),
               "DH": (sec, ("point", 32)), "eddsa_pk_eddsa_to_dh": (pub,), "eddsa_sk_eddsa_to_dh": (sec,)}
    assert len(singles) == 13
    for name, params in singles.items():
        fixed = [x for x in params if x != b""]
        for short in range(len(fixed)):
            args = [bytes(wd - (k == short)) for k, (_, wd) in enumerate(fixed)] + [b""] * (len(params) - len(fixed))
            with pytest.raises(ValueError) as e:
                getattr(ed, name)(*args)
            assert str(e.value) == f"{fixed[short][0]}: expected {fixed[short][1]} bytes, got {fixed[short][1] - 1}", name
        # by keyword as well; too few, too many, unknown and doubled arguments are a TypeError
        good = {nm: bytes(wd) for nm, wd in fixed}
        good.update({"data": b""} if len(params) > len(fixed) else {})
        with pytest.raises(ValueError) as e:
            getattr(ed, name)(**dict(good, **{fixed[0][0]: bytes(fixed[0][1] + 1)}))
        assert str(e.value) == f"{fixed[0][0]}: expected {fixed[0][1]} bytes, got {fixed[0][1] + 1}", name
        for args, kw in (((), {}), (tuple(good.values()) + (b"",), {}), ((), dict(good, other=b"")), (tuple(good.values()), {fixed[0][0]: b""})):
            with pytest.raises(TypeError):
                getattr(ed, name)(*args, **kw)


def test_bench_insists_on_a_device_per_rank():
    """SCALE readiness: two ranks on one device are an error, not a scaling point"""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.devices_distinct([0, 1, 2, 3], 4, False) is True
    assert bench.devices_distinct([0, 0], 2, True) is False          # the one-GPU test hook: allowed, and said so in the line
    with pytest.raises(SystemExit):
        bench.devices_distinct([0, 0], 2, False)
    with pytest.raises(SystemExit):
        bench.devices_distinct([0, 1, 1, 3], 4, False)


def test_shard_bounds_partition():
    from libeddsa_amd import shard_bounds
    for n in (0, 1, 7, 8, 1000, 1 << 24):
        for world in (1, 2, 3, 8):
            spans = [shard_bounds(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1
    assert shard_bounds(1 << 24, 3, 8) == (3 << 21, 4 << 21)       # config 4: 2^21 per GPU
    with pytest.raises(ValueError):
        shard_bounds(10, 2, 2)


def test_workload_is_deterministic_and_shardable():
    import workload
    a, b = workload.x25519_inputs(1000)
    a2, b2 = workload.x25519_inputs(300, first=500)
    assert np.array_equal(a[500:800], a2) and np.array_equal(b[500:800], b2)
    assert a[0, :4].tolist() == [23, 167, 82, 220]                 # pinned first bytes of the stream
    sig = np.zeros((64, 64), np.uint8); pub = np.zeros((64, 32), np.uint8); msg = np.zeros((64, 32), np.uint8)
    exp = workload.corrupt_for_verify(sig, pub, msg, edges=False)   # (the edge splice: see the test further down)
    assert exp.sum() == 60 and [i for i in range(64) if not exp[i]] == [5, 21, 37, 53]
    flipped = [int(np.count_nonzero(x)) for x in (sig[:, :32], sig[:, 32:], pub, msg)]
    assert flipped == [1, 1, 1, 1]                                  # R, S, A, msg round-robin


_WORKER = r'''
import os, sys, ctypes
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, os.environ["REPO"]); sys.path.insert(0, os.path.join(os.environ["REPO"], "tools"))
import workload
from libeddsa_amd import shard_bounds, gather_bytes
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
n = 1003                                   # ragged: shards of 502 and 501
lo, hi = shard_bounds(n, rank, world)
sc, pt = workload.x25519_inputs(hi - lo, first=lo)
orc = ctypes.CDLL(os.path.join(os.environ["REPO"], "oracle", "liboracle.so"))
out = np.zeros((hi - lo, 32), np.uint8)
P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
orc.orc_x25519_batch(P(out), P(sc), P(pt), ctypes.c_size_t(hi - lo), 2)   # stand-in for the GPU shard
full = gather_bytes(torch.from_numpy(out), n)
sc_all, pt_all = workload.x25519_inputs(n)
want = np.zeros((n, 32), np.uint8)
orc.orc_x25519_batch(P(want), P(sc_all), P(pt_all), ctypes.c_size_t(n), 2)
assert full.shape == (n, 32) and np.array_equal(full.numpy(), want), "gathered batch differs"
ok = torch.from_numpy((np.arange(lo, hi) % 16 != 5).astype(np.uint8))
allok = gather_bytes(ok, n)
assert allok.shape == (n,) and int(allok.sum()) == int((np.arange(n) % 16 != 5).sum())
dist.destroy_process_group()
open(os.path.join(os.environ["OUT_DIR"], f"rank{rank}.ok"), "w").write("ok")
'''


_BENCH_WORKER = r'''
import os, sys, time
import torch, torch.distributed as dist
sys.path.insert(0, os.environ["REPO"])
import bench
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
calls = []
def step():
    calls.append(1)
    time.sleep(0.05 * (rank + 1))                       # rank 1 is the slow one
    out = torch.full((1000,), rank + 1, dtype=torch.uint8)
    full = bench.gather_results(out, world)
    assert full.shape == (world, 1000) and [int(full[r, 0]) for r in range(world)] == [1, 2]
    return out
elapsed, out = bench.timed_region(step, 4, world, lambda: None, torch.device("cpu"))
assert len(calls) == 4                                   # exactly K steps
assert 0.39 < elapsed < 1.5, elapsed                     # the MAX over ranks (4 x 0.1 s), on every rank
# the per-rank breakdown and the host-side barrier of the N > 1 line (a second, gloo group beside the RCCL one)
bench.HOST_GROUP[0] = dist.new_group(backend="gloo")
pr = bench.per_rank_breakdown(world, rank, 4, 10.0 * (rank + 1), 1.0 + rank)
assert [r["rank"] for r in pr["ranks"]] == [0, 1] and pr["slowest_rank"] == 1, pr
assert pr["kernel_ms_min_max"] == [10.0, 20.0] and pr["gather_ms_max"] == 2.0
assert abs(pr["ranks"][rank]["wall_ms_per_step"] - bench.LOCAL_ELAPSED[0] / 4 * 1e3) < 1e-6
# SCALE readiness: every rank's row names its device and carries a clock / power sample (None without a GPU); the line
# states what the gather ran over, with world == N, and two ranks on one device are refused unless the test hook says so
assert all({"device", "power_w", "sclk_mhz"} <= set(r) for r in pr["ranks"])
facts = bench.collective_facts(world, "gloo", True)
assert facts["world"] == world == 2 and facts["backend"] == "gloo" and facts["version"] is None and facts["is_rccl"] is False
assert facts["devices"] == [-1, -1] and facts["devices_distinct"] is False and facts["shared_gpu_test_hook"] is True
try:
    bench.collective_facts(world, "gloo", False)
    raise AssertionError("two ranks on one device were accepted")
except SystemExit:
    pass
t0 = time.perf_counter()
if rank == 0:
    time.sleep(0.3)                                      # rank 0 "times the CPU baseline"; rank 1 sleeps in the barrier
bench.host_barrier()
assert time.perf_counter() - t0 > 0.25
dist.destroy_process_group()
open(os.path.join(os.environ["OUT_DIR"], f"rank{rank}.ok"), "w").write("ok")
'''


def _torchrun(script, env):
    import socket
    with socket.socket() as sk:                 # a free rendezvous port (avoids TIME_WAIT collisions)
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    return subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                           "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)],
                          env=env, capture_output=True, text=True, timeout=300)


def test_bench_timing_and_gather_helpers_over_gloo(tmp_path):
    """bench.py's N > 1 plumbing (barrier-bracketed region, max over ranks, result all-gather)"""
    script = tmp_path / "bench_worker.py"
    script.write_text(_BENCH_WORKER)
    env = dict(os.environ, REPO=ROOT, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", OUT_DIR=str(tmp_path))
    r = _torchrun(script, env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "rank0.ok").exists() and (tmp_path / "rank1.ok").exists()


def test_two_rank_shard_and_gather_over_gloo(oracle, tmp_path):
    """N > 1 path: contiguous shards, independent compute, one all-gather of the result bytes."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, REPO=ROOT, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", OUT_DIR=str(tmp_path))
    r = _torchrun(script, env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "rank0.ok").exists() and (tmp_path / "rank1.ok").exists()


def test_bench_helpers_without_gpu(tmp_path, monkeypatch):
    """bench.py's host-side helpers: cgroup-aware core count, PMC traffic lookup (sums the kernels of
    a multi-kernel pass, applies the gfx950 FETCH_SIZE x2 rule), canonical work figures"""
    import json
    import bench
    assert 1 <= bench.usable_cores() <= (os.cpu_count() or 1)
    assert bench.MUL32_VERIFY == 2291 * 100 + 1514 * 55 == 312370            # BASELINE.md "Work per item"
    assert bench.MUL32_X25519 == 1292 * 100 + 1278 * 55 + 256 * 10 == 202050
    assert bench.MUL32_SIGN == 506 * 100 + 254 * 55 == 64570
    assert abs(bench.PEAK_TMUL32 - 39.3216) < 1e-9
    import source_hash
    here = source_hash.device_source_hash()
    assert len(here) == 64 and "kernels.hip" in source_hash.device_source_files() and "probe.hip" not in source_hash.device_source_files()
    summary = {"ed::k_a": {"FETCH_SIZE": 1000.0, "WRITE_SIZE": 10.0, "SQ_INSTS_VALU": 512.0, "GRBM_GUI_ACTIVE": 32.0},
               "ed::k_b": {"FETCH_SIZE": 24.0, "WRITE_SIZE": 6.0}, "_source": {"sha256": here}}
    path = tmp_path / "pmc_summary.json"
    path.write_text(json.dumps(summary))
    monkeypatch.setattr(bench, "PMC_PATH", str(path))
    bench._PMC_CACHE.clear()
    t = bench.pmc_traffic("k_a + k_b")
    assert t["bytes"] == (2 * 1024.0 + 16.0) * 1024.0 and t["fetch_size_kb_raw"] == 1024.0
    assert bench.pmc_traffic("k_missing") is None
    assert bench.pmc_valu_busy("k_a")["value"] == 4.0 * 512 / (1024 * 32 / 8) and bench.pmc_note() is None
    # counters recorded from OTHER kernel sources are not printed - one changed hex digit of the recorded
    # hash (as after any edit of csrc/ without a new tools/profile.sh run), or a summary without a hash at all
    for broken in ({**summary, "_source": {"sha256": ("0" if here[0] != "0" else "1") + here[1:]}},
                   {k: v for k, v in summary.items() if k != "_source"}):
        path.write_text(json.dumps(broken))
        bench._PMC_CACHE.clear()
        assert bench.pmc_traffic("k_a + k_b") is None and bench.pmc_valu_busy("k_a") is None and bench.pmc_executed("k_a", 64) is None
        assert "other kernel sources" in bench.pmc_note()
    bench._PMC_CACHE.clear()


def test_bench_dump_outputs_without_gpu(tmp_path, monkeypatch):
    """--dump-outputs: the last step's bytes as float32 .npy; an output above the size cap becomes a fixed sample of
    whole items (the same items on every run), here of signatures gathered over two ranks"""
    import torch
    import bench
    v = (torch.arange(1000) % 3 == 0).to(torch.uint8)
    bench.dump_outputs(str(tmp_path / "v"), "verify", v)
    got = np.load(tmp_path / "v" / "verdicts.npy")
    assert got.dtype == np.float32 and np.array_equal(got, v.numpy())
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100 * 64 * 4)
    s = torch.randint(0, 256, (2, 500, 64), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), "sign", s)
    a, b = np.load(tmp_path / "a" / "signatures.npy"), np.load(tmp_path / "b" / "signatures.npy")
    assert a.shape == (100, 64) and a.dtype == np.float32 and np.array_equal(a, b)
    rows = {r.tobytes() for r in s.reshape(-1, 64).numpy().astype(np.float32)}
    assert all(r.tobytes() in rows for r in a)


def test_c_shard_bounds_match_the_python_sharder():
    """eddsa_amd_shard_bounds (the C multi-device entry points) and libeddsa_amd.shard_bounds (the
    one-process-per-GPU path) cut a batch identically: contiguous, balanced, covering"""
    import libeddsa_amd as ed
    lib = ctypes.CDLL(_lib_path())
    lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
    for n in (0, 1, 7, 8, 1003, 1 << 24, (1 << 24) + 5):
        for world in (1, 2, 3, 8):
            end = 0
            for r in range(world):
                lib.eddsa_amd_shard_bounds(ctypes.c_size_t(n), r, world, ctypes.byref(lo), ctypes.byref(hi))
                assert (lo.value, hi.value) == ed.shard_bounds(n, r, world) and lo.value == end
                end = hi.value
            assert end == n
    assert ed.shard_bounds(1 << 24, 3, 8) == (3 << 21, 4 << 21)              # config 4: 2^21 per GPU


def test_multi_device_calls_need_a_bound_device_set():
    import libeddsa_amd as ed
    assert ed.device_count() == 0
    with pytest.raises(ed.EddsaAmdError):
        ed.ed25519_verify_batch_multi(np.zeros((2, 64), np.uint8), np.zeros((2, 32), np.uint8), np.zeros((2, 8), np.uint8))


def test_bench_spawns_ranks_and_checks_the_launcher(tmp_path):
    """`python bench.py --gpus 2` with no launcher environment starts two ranks as a CHILD process (here
    both stop at the missing GPU, loudly); a launcher whose world size differs from --gpus is refused"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: covered by tests/test_gpu_multi.py")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], env=env,
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    # (the launcher stops the second rank as soon as the first has failed, so one message may be all there is)
    assert r.returncode != 0 and "needs an MI355X" in r.stderr and "nproc_per_node" not in r.stderr[:0], r.stderr[-2000:]
    assert "ChildFailedError" in r.stderr or "local_rank" in r.stderr, r.stderr[-2000:]   # it WAS the child launcher
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], env=dict(env, WORLD_SIZE="2", RANK="0"),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "--gpus 4 but the launcher started 2" in r.stderr


def test_workload_edge_vectors_against_the_oracle(oracle):
    """tools/workload.py: the spliced edge vectors sit where documented, never on a corrupted item, and the
    expected verdicts (derived from the reference's semantics) are the oracle's on two full blocks"""
    import workload
    n = 2 * workload.EDGE_BLOCK
    sk, msg = workload.sign_inputs(n, seed=1, config=2)
    pk = oracle.genpub_batch(sk)
    sig = oracle.sign_batch(sk, pk, msg, 32)
    plain = workload.corrupt_for_verify(sig.copy(), pk.copy(), msg.copy(), edges=False)
    s2, p2, m2 = sig.copy(), pk.copy(), msg.copy()
    expect = workload.corrupt_for_verify(s2, p2, m2)
    pos = [workload.edge_position(m, e) for m in range(2) for e in range(workload.EDGE_KINDS)]
    assert all(p % 16 == 9 for p in pos) and len(set(pos)) == 128 and max(pos) < n
    assert np.array_equal(oracle.verify_batch(s2, p2, m2, 32), expect)
    untouched = np.ones(n, bool); untouched[pos] = False
    assert np.array_equal(expect[untouched], plain[untouched])
    first = [int(expect[workload.edge_position(0, e)]) for e in range(12)]
    assert first == [1, 1, 1, 1, 0, 0, 0, 0, 1, 0, 1, 1]        # S + k l accepted; S = 0, l, 2^256-1 not; identity cases
    # a shard that starts in the middle of the stream sees the same bytes
    lo = workload.EDGE_BLOCK - 100
    sk3, msg3 = workload.sign_inputs(300, seed=1, config=2, first=lo)
    pk3 = oracle.genpub_batch(sk3); sig3 = oracle.sign_batch(sk3, pk3, msg3, 32)
    e3 = workload.corrupt_for_verify(sig3, pk3, msg3, first=lo)
    assert np.array_equal(sig3, s2[lo:lo + 300]) and np.array_equal(pk3, p2[lo:lo + 300]) and np.array_equal(e3, expect[lo:lo + 300])
