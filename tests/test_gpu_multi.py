"""GPU tests of the rows VERDICT r01 listed as missing: BASELINE config 4 (2^24 verifies, one GPU and
sharded), the single-process multi-device C entry points with their RCCL gather, bench.py's own rank
spawning, and the secret hygiene of the HBM buffers.  Everything goes through the C-ABI."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_kit import dev
from hostlib import ROOT, build_c_program

pytestmark = pytest.mark.gpu


def golden_msg(i):
    out, c = b"", 0
    while len(out) < i:
        out += hashlib.sha512(b"libeddsa-amd golden msg" + i.to_bytes(4, "little") + c.to_bytes(4, "little")).digest()
        c += 1
    return out[:i]


def _config4_batch(engine, n, first=0):
    import workload
    sk, msg = workload.sign_inputs(n, seed=3, config=4, first=first)
    pk = engine.ed25519_genpub_batch(dev(sk))
    sig = engine.ed25519_sign_batch(dev(sk), pk, dev(msg)).cpu().numpy()
    pk = pk.cpu().numpy()
    expect = workload.corrupt_for_verify(sig, pk, msg, seed=3, config=4, first=first)
    return sig, pk, msg, expect


def test_config4_full_2_24_on_one_gpu(engine, golden):
    """BASELINE config 4's batch (2^24 items, seed 3) through ONE GPU: sixteen workspace passes; inputs and
    verdicts hash to what the compiled reference produced (tests/golden/batch_digests.json, verify_2^24),
    and each eighth of the verdict vector to the per-shard digests"""
    import torch
    v = golden("batch_digests.json")["verify_2^24"]
    n = 1 << 24
    sig, pk, msg, expect = _config4_batch(engine, n)
    h = hashlib.sha512()
    for a in (sig, pk, msg):
        h.update(a.tobytes())
    assert h.hexdigest() == v["inputs_sha512"]
    ok = engine.ed25519_verify_batch(dev(sig), dev(pk), dev(msg), msg_len=32).cpu().numpy()
    torch.cuda.empty_cache()
    assert np.array_equal(ok, expect) and int(ok.sum()) == v["accepted"]
    assert hashlib.sha512(ok.tobytes()).hexdigest() == v["verdicts_sha512"]
    for k in range(8):
        assert hashlib.sha512(ok[k * (n // 8):(k + 1) * (n // 8)].tobytes()).hexdigest() == v["shard8_verdicts_sha512"][k]
    # the record form and the host-pointer pipeline on one 2^21 shard (config 4's per-GPU share)
    lo, hi = 3 * (n // 8), 4 * (n // 8)
    assert np.array_equal(engine.ed25519_verify_batch(sig[lo:hi], pk[lo:hi], msg[lo:hi], msg_len=32), expect[lo:hi])
    # every pair of the half-length route passed its exact integer check (lanes.h: verify_half_scalars_lane)
    assert engine.halve_rejected() == 0
    # SURVEY 8(e) as the C-ABI does it: one process, EVERY visible device, shard d resident on device d, one RCCL
    # all-gather of the verdict bytes (grouped broadcasts when the shards differ in length).  One device on the
    # round's box (world size 1); on a multi-GPU node the same assertions cover the real gather: the reference's
    # digest in EVERY device's buffer, once with even shards (2^24) and once with uneven ones (2^24 - 3).
    g = engine.init_devices()
    assert g == torch.cuda.device_count()
    to = lambda a, d: torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{d}")  # noqa: E731
    for total in (n, n - 3):
        shards = [engine.shard_bounds(total, d, g) for d in range(g)]
        assert total != n or g not in (1, 2, 4, 8) or all(hi - lo == n // g for lo, hi in shards)
        outs = engine.ed25519_verify_batch_multi_dev([to(sig[lo:hi], d) for d, (lo, hi) in enumerate(shards)],
                                                     [to(pk[lo:hi], d) for d, (lo, hi) in enumerate(shards)],
                                                     [to(msg[lo:hi], d) for d, (lo, hi) in enumerate(shards)], 32, total)
        for d, o in enumerate(outs):
            torch.cuda.synchronize(d)
            got = o.cpu().numpy()
            assert np.array_equal(got, expect[:total]), (total, d)
            if total == n:
                assert hashlib.sha512(got.tobytes()).hexdigest() == v["verdicts_sha512"], d
        del outs
        torch.cuda.empty_cache()


def _bench(args, env_extra=None, timeout=1500):
    import json
    env = dict(os.environ, **(env_extra or {}))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_spawns_its_own_ranks_for_config4(engine, golden):
    """the bare command `python bench.py --gpus 2` (no launcher): bench.py starts the two ranks itself and
    runs config 4 - 2^24 verifies in total, 2^23 per rank - here with both ranks on the box's single GPU
    and gloo standing in for RCCL; the gathered verdict vector hashes to the reference's digest"""
    d = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--op", "verify", "--full"],
               {"EDDSA_BENCH_SHARE_GPU": "1", "EDDSA_BENCH_BACKEND": "gloo"})
    v = golden("batch_digests.json")["verify_2^24"]
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["outputs_correct"] is True
    assert d["config"]["total_items"] == 1 << 24 and d["config"]["items_per_gpu"] == 1 << 23
    assert d["verdicts"]["verdicts_sha512"] == v["verdicts_sha512"] and d["verdicts"]["accepted"] == v["accepted"]
    assert d["verdicts"]["matches_reference_digest"] is True
    # a line at N > 1 carries the CPU baseline (rank 0 timed it while rank 1 slept in a host barrier)
    # and a per-rank breakdown that lets a scaling point be attributed
    assert d["cpu_baseline"]["kind"] in ("reference", "port") and d["cpu_baseline"]["gpu_matches_cpu_on_sample"] is True
    pr = d["per_rank"]
    assert [r["rank"] for r in pr["ranks"]] == [0, 1] and pr["slowest_rank"] in (0, 1)
    assert all(r["kernel_ms"] > 0 and r["gather_ms"] >= 0 and r["wall_ms_per_step"] >= r["kernel_ms"] * 0.5 for r in pr["ranks"])


def test_bench_default_line_carries_the_whole_metric(engine, golden):
    """`python bench.py --full` at N = 1: config 2 verifies as `value`, x25519 and sign under `secondary`, each with
    its own roofline fraction and CPU baseline, the verdict digest equal to the reference's"""
    d = _bench(["--steps", "2", "--warmup", "1", "--cpu-sample", "4096", "--sustained", "2", "--full"])
    assert d["n_gpus"] == 1 and d["outputs_correct"] is True and d["metric"] == "ed25519 verifies/sec"
    assert d["verdicts"]["verdicts_sha512"] == golden("batch_digests.json")["verify_2^20"]["verdicts_sha512"]
    assert d["verdicts"]["matches_reference_digest"] is True
    for op, metric in (("x25519", "x25519 ops/sec"), ("sign", "ed25519 signs/sec")):
        s = d["secondary"][op]
        assert s["metric"] == metric and s["value"] > 0 and s["outputs_correct"] is True
        assert 0 < s["roofline"]["frac"] < 1.5 and s["cpu_baseline"]["gpu_matches_cpu_on_sample"]
    v = d["secondary"]["verify_rlc_all_valid"]
    assert v["outputs_correct"] is True and v["stats"][0] == 1 << 20 and v["value"] > d["value"]
    hh = d["secondary"]["verify_host_to_host"]              # PCIe-inclusive, for the record
    assert hh["outputs_correct"] is True and 0 < hh["value"] < d["value"] * 1.05
    sc = d["secondary"]["verify_small_calls"]               # the single-item function and a small batch, one caller
    assert sc["outputs_correct"] is True and 0 < sc["single_ed25519_verify_ms"] < 5 and 0 < sc["verify_batch_256_valid_ms"] < 5
    wc = d["secondary"]["verify_garbage_keys"]               # the worst case a caller can construct: VERDICT r04 #1 asked for >= 65 M/s
    assert wc["outputs_correct"] is True and wc["value"] > 55e6
    rg = d["secondary"]["verify_ragged_messages"]            # ragged messages of 0 .. 4 KiB, hashed in order of length
    assert rg["outputs_correct"] is True and rg["value"] > 30e6 and rg["sign_value"] > 30e6
    su = d["secondary"]["verify_sustained"]                 # burst and steady state side by side
    assert su["outputs_correct"] is True and su["seconds"] >= 2 and 0.5 < su["sustained_over_burst"] < 1.3
    r = d["roofline"]
    assert 0 < r["whole_pass"]["frac"] <= r["frac"] * 1.2
    # the counter fields: from the committed summary when it was recorded on this tree's kernel sources, else null WITH the
    # reason (the line must not quote counters of other sources)
    if r["counters_note"] is None:
        assert "source" in r["valu_busy"] and "source" in r["traffic"]
    else:
        assert r["valu_busy"] is None and r["traffic"] is None and "other kernel sources" in r["counters_note"]


def test_multi_device_python_mirror(engine, oracle):
    """the *_multi entry points over the visible device set (one device on this box: the shard, thread and
    RCCL code paths run with world size 1): same bytes as the single-device calls and as the oracle"""
    import torch
    g = engine.init_devices()
    assert g == engine.device_count() >= 1
    n = 5000
    rng = np.random.default_rng(77)
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    lens = rng.integers(0, 200, n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    msgs = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    pk = engine.ed25519_genpub_batch(sk)
    sig = engine.ed25519_sign_batch_multi(sk, pk, msgs, msg_off=off)
    assert np.array_equal(sig, engine.ed25519_sign_batch(sk, pk, msgs, msg_off=off))
    for i in (0, 1, n - 1):
        assert sig[i].tobytes() == oracle.sign(sk[i].tobytes(), pk[i].tobytes(), msgs[int(off[i]):int(off[i + 1])].tobytes())
    bad = sig.copy(); bad[::5, 3] ^= 0x40
    ok = engine.ed25519_verify_batch_multi(bad, pk, msgs, msg_off=off)
    assert np.array_equal(ok, (np.arange(n) % 5 != 0).astype(np.uint8))
    pt = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    assert np.array_equal(engine.x25519_batch_multi(sk, pt), oracle.x25519_batch(sk, pt))
    # device-pointer form: per-device shards, RCCL all-gather of the verdicts (ncclAllGather, world size g)
    m = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    s2 = engine.ed25519_sign_batch(sk, pk, m, msg_len=32)
    s2[1::7, 40] ^= 1
    want = oracle.verify_batch(s2, pk, m, 32)
    shards = [engine.shard_bounds(n, d, g) for d in range(g)]
    to = lambda a, d: torch.from_numpy(np.ascontiguousarray(a)).to(f"cuda:{d}")  # noqa: E731
    outs = engine.ed25519_verify_batch_multi_dev([to(s2[lo:hi], d) for d, (lo, hi) in enumerate(shards)],
                                                 [to(pk[lo:hi], d) for d, (lo, hi) in enumerate(shards)],
                                                 [to(m[lo:hi], d) for d, (lo, hi) in enumerate(shards)], 32, n)
    for d, o in enumerate(outs):
        torch.cuda.synchronize(d)
        assert np.array_equal(o.cpu().numpy(), want), d
    # the C entry point trusts its pointers, so the mirror checks every shard's size and device first
    lo, hi = shards[0]
    with pytest.raises(ValueError):
        engine.ed25519_verify_batch_multi_dev([to(s2[lo:hi - 1], 0)] + [to(s2[a:b], d) for d, (a, b) in enumerate(shards)][1:],
                                              [to(pk[a:b], d) for d, (a, b) in enumerate(shards)],
                                              [to(m[a:b], d) for d, (a, b) in enumerate(shards)], 32, n)
    with pytest.raises(ValueError):
        engine.ed25519_verify_batch_multi_dev([to(s2[a:b], d) for d, (a, b) in enumerate(shards)],
                                              [to(pk[a:b], d) for d, (a, b) in enumerate(shards)],
                                              [to(m[a:b], d) for d, (a, b) in enumerate(shards)], 31, n)


def test_c_program_on_the_multi_device_entry_points(engine, golden, tmp_path):
    """tests/c/multi_device.c: a plain C caller (HIP runtime API for its own buffers) of
    eddsa_amd_init_devices / *_multi / ed25519_verify_batch_multi_dev, linked against the library through
    its SONAME link libeddsa.so.0"""
    lib = os.path.join(ROOT, "libeddsa_amd")
    if not os.path.exists(os.path.join(lib, "libeddsa.so.0")):
        os.symlink("libeddsa_amd.so", os.path.join(lib, "libeddsa.so.0"))
    exe = build_c_program(tmp_path, "multi_device.c", libs=("eddsa_amd",), rocm=True)
    msgs = tmp_path / "msgs.bin"
    msgs.write_bytes(b"".join(golden_msg(i) for i in range(1024)))
    r = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "ed25519_table.bin"), str(msgs)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "multi_device: ok" in r.stdout


def test_calls_follow_their_buffers_not_the_threads_current_device(engine, oracle):
    """a host thread whose current HIP device was never set (a fresh thread) issues device- and
    host-pointer calls; the engine makes its own device current for the call and restores the caller's"""
    import threading
    import torch
    n = 700
    rng = np.random.default_rng(3)
    sc = rng.integers(0, 256, (n, 32), dtype=np.uint8); pt = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    want = oracle.x25519_batch(sc, pt)
    d_sc, d_pt = dev(sc), dev(pt)
    errs = []

    def worker():
        try:
            before = torch.cuda.current_device()
            assert np.array_equal(engine.x25519_batch(sc, pt), want)
            out = engine.x25519_batch(d_sc, d_pt)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want)
            assert torch.cuda.current_device() == before
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    t = threading.Thread(target=worker); t.start(); t.join()
    assert not errs, errs
    import ctypes
    buf = np.zeros((4, 32), np.uint8)                       # a host pointer where a device pointer belongs: refused
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert engine.library().x25519_batch_dev(p, p, p, ctypes.c_size_t(4), None) != 0


def test_secrets_do_not_outlive_the_call_in_hbm(engine):
    """ADVICE r01 / VERDICT weak #9: after sign / x25519 / genpub / x25519_base / sk->x calls - n = 1, where 511
    idle lanes used to keep copies, and a two-chunk batch - the scalar workspace, x25519's point workspace and the
    host pipeline's staging buffers are all zero (the reference wipes its stack after the same operations:
    lib/ed25519-sha512.c:77,136, lib/x25519.c:208,221)"""
    import torch
    engine.shutdown()
    rng = np.random.default_rng(11)
    sk1 = rng.integers(1, 256, (1, 32), dtype=np.uint8)
    m1 = rng.integers(1, 256, (1, 40), dtype=np.uint8)
    pk1 = engine.ed25519_genpub_batch(sk1)
    engine.ed25519_sign_batch(sk1, pk1, m1)
    aux, acc, stage_in, stage_out = engine.secret_residue()
    assert aux == 0 and stage_in == 0, (aux, stage_in)
    engine.shutdown()
    engine.x25519_batch(sk1, pk1)
    engine.sk_ed25519_to_x25519_batch(sk1)
    aux, acc, stage_in, stage_out = engine.secret_residue()
    assert (aux, acc, stage_in, stage_out) == (0, 0, 0, 0)
    n = (1 << 18) + 777                                        # two pipeline chunks, partly filled tiles
    sk = rng.integers(0, 256, (n, 32), dtype=np.uint8); pt = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    engine.x25519_batch(sk, pt)
    d = engine.x25519_batch(dev(sk), dev(pt)); torch.cuda.synchronize(); del d
    assert engine.secret_residue()[2:] == (0, 0)
    engine.x25519_base_batch(sk)                               # its output (a public key) may stay; its scalars may not
    assert engine.secret_residue()[2] == 0
    engine.shutdown()
    engine.x25519_batch(dev(sk), dev(pt)); torch.cuda.synchronize()
    assert engine.secret_residue() == (0, 0, 0, 0)
    # a call that FAILS after staging its inputs wipes them as well (one chunk, and two)
    assert engine.debug_fail_next_host_call() == engine.HOOKS_OFF       # (shutdown disarmed the hooks: nothing happens)
    assert np.array_equal(engine.x25519_batch(sk[:8], pt[:8]), engine.x25519_batch(dev(sk[:8]), dev(pt[:8])).cpu().numpy())
    engine.debug_init(0)
    for m in (1000, n):
        assert engine.debug_fail_next_host_call() == 0
        with pytest.raises(engine.EddsaAmdError):
            engine.x25519_batch(sk[:m], pt[:m])
        assert engine.secret_residue() == (0, 0, 0, 0), m
    assert np.array_equal(engine.x25519_batch(sk[:64], pt[:64]), engine.x25519_batch(dev(sk[:64]), dev(pt[:64])).cpu().numpy())
    engine.shutdown()
    msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pk = engine.ed25519_genpub_batch(sk)
    engine.ed25519_sign_batch(dev(sk), dev(pk), dev(msgs)); torch.cuda.synchronize()
    assert engine.secret_residue()[0] == 0
    engine.init(0)
