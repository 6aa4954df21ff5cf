#!/usr/bin/env python3
"""bench.py - headline benchmark of the MI355X Ed25519 / X25519 engine.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--op all|verify|x25519|sign] [--log2n L]
                    [--dump-outputs DIR] [--full]

Metric (BASELINE.json): ed25519 verifies/s and x25519 ops/s at batch 2^20 on 1/2/4/8 MI355X.
One "step" = one pass of the hot path over the whole synthetic batch, inputs already resident in HBM.

  N = 1   config 2: 2^20 ed25519 verifies (SURVEY 8d workload: seed 1, 1/16 corrupted, edge vectors
          spliced in).  `value` = verifies/s.
  N > 1   config 4: 2^24 verifies in total (seed 3), contiguous shards of 2^24/N items per GPU, one
          rank per GPU, no data-path collective; the step ends with the RCCL all-gather of the
          verdict bytes.  Total work fixed: "strong".  --log2n overrides the per-GPU size
          (then "weak").

A plain run sets up, warms up, times exactly K steps, writes the last step's outputs (--dump-outputs DIR:
DIR/<name>.npy, float32, see dump_outputs) and prints the line: the headline keys, and `outputs_correct`
(verify: the verdicts equal the constructed ones; x25519 / sign: null, their checks need --full).
Everything below is measured or checked only with --full.

With --full, after the verify region the same process times config 3 (2^20 x25519 per GPU) and config 5 (2^20
signs per GPU) with the same step count and reports them under "secondary" (--op all, the default),
together with the opt-in batch verification on the config's items before corruption.

`--gpus N` without a torch.distributed environment spawns the N ranks itself (a child
`python -m torch.distributed.run`, started before this process touches the GPU) and relays rank 0's line.

Prints ONE JSON line on rank 0 (see the driver contract); with --full, three extra objects:
  verdicts      (verify) the SHA-512 of the whole verdict vector, checked against the reference's digest of that batch
  roofline      the verify pass (three kernels; the dominant one, k_verify_main_half, is broken out under
                "dominant") against the integer-VALU multiply-issue roofline SURVEY 8(d) prescribes for
                this path, plus the HBM view of the same launch
  cpu_baseline  the reference itself (oracle/_ref, compiled from its own sources) timed on this
                box's host cores on a bounded sample of the same workload (rank 0; at N > 1 the other ranks
                sleep in a host-side barrier meanwhile)
At N = 1 (--full) `secondary.verify_host_to_host` is the PCIe-inclusive rate of the same batch through the host-pointer entry
point (for the record; `value` never includes transfers), `secondary.verify_small_calls` the latency of one single-item
call and of a batch of 256 through the same entry points, and `secondary.verify_sustained` repeats the config-2 pass back to back for --sustained seconds (default 10)
and reports the rate of the last half with the power and clock rocm-smi shows: the headline region lasts 0.2 s,
which a power-bound chip runs above its steady-state clock.  At N > 1 (--full) `per_rank` breaks the step down by rank
(device, kernel ms, gather ms, wall ms, clock and power, the slowest rank) and `rccl` states what the result gather ran over
(world size == N, backend, RCCL version, every rank on a device of its own - the run exits non-zero otherwise), so that a
scaling point can be attributed.
"""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import libeddsa_amd as ed  # noqa: E402
import workload  # noqa: E402
ed.use_debug_library()   # libeddsa_amd_debug.so = the product's object files (the same kernels) plus the hooks this harness reads: phase timings, route selection

# canonical 32x32->64 multiply counts per item (BASELINE.md "Work per item")
MUL32_VERIFY = 312370
MUL32_X25519 = 202050
MUL32_SIGN = 64570
MUL32 = {"verify": MUL32_VERIFY, "x25519": MUL32_X25519, "sign": MUL32_SIGN}
BYTES = {"verify": 129, "x25519": 96, "sign": 160}      # algorithmic HBM bytes per item
UNIT = {"verify": "verifies/s", "x25519": "ops/s", "sign": "signs/s"}
KERNELS = {"verify": "k_verify_prepare + k_verify_halve + k_verify_main_half", "x25519": "k_x25519_ladder + k_x25519_finish", "sign": "k_sign_point + k_sign_finish"}
# v_mad_u64_u32 issue peak: 256 CU x 4 SIMD x 16 lanes/clk x 2.4 GHz (profiles/r01_valu_rates.txt
# measures 36-37 T lane-MAC/s at the clock the chip holds under this load)
PEAK_TMUL32 = 256 * 4 * 16 * 2.4e9 / 1e12
PEAK_HBM_GBS = 8000.0
PMC_SOURCE = "profiles/pmc_summary.json (rocprofv3 --pmc, separate passes of this command; not measured in this run)"


def make_workload(op, n, first, device, seed=None, config=None):
    """SURVEY 8(d) seeded synthetic batch from tools/workload.py (SplitMix64 streams; this rank owns
    items first .. first+n-1 of the stream).  verify: 32-byte messages, random keys, items with
    i % 16 == 5 corrupted by one flipped bit in R, S, A or the message (round-robin), edge vectors
    spliced in at fixed indices.  Signatures and public keys come from the engine's own sign/genpub
    kernels (parity-tested separately; the batches are the ones whose digests
    tests/golden/batch_digests.json pins)."""
    up = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    if op == "x25519":
        sc, pt = workload.x25519_inputs(n, first=first)
        return {"scalars": up(sc), "points": up(pt)}
    if op == "sign":
        sk, msg = workload.sign_inputs(n, first=first)
        sk, msg = up(sk), up(msg)
        return {"secs": sk, "pubs": ed.ed25519_genpub_batch(sk), "msgs": msg}
    sk, msg = workload.sign_inputs(n, seed=seed, config=config, first=first)
    d_sk = up(sk)
    pk = ed.ed25519_genpub_batch(d_sk)
    sig = ed.ed25519_sign_batch(d_sk, pk, up(msg)).cpu().numpy()
    pk = pk.cpu().numpy()
    valid = (up(sig.copy()), up(pk.copy()), up(msg.copy()))   # the same items before corruption: the batch-verification line
    expect = workload.corrupt_for_verify(sig, pk, msg, seed=seed, config=config, first=first)
    return {"sigs": up(sig), "pubs": up(pk), "msgs": up(msg), "expect": up(expect), "valid": valid}


PMC_PATH = os.path.join(ROOT, "profiles", "pmc_summary.json")
_PMC_CACHE = {}


def pmc_profile():
    """The committed counter summary - but only if it was measured on THIS tree's device code: tools/summarize_profile.py
    stores the hash of the kernel sources with the counters (tools/source_hash.py) and a summary recorded from other
    sources is not printed (the line must not keep quoting stale counters after a kernel change).
    -> (per-kernel dict, None) or ({}, the reason)."""
    if PMC_PATH in _PMC_CACHE:
        return _PMC_CACHE[PMC_PATH]
    try:
        prof = json.load(open(PMC_PATH))
    except (OSError, ValueError):
        res = ({}, "no counter summary committed (tools/profile.sh)")
    else:
        import source_hash
        want, have = source_hash.device_source_hash(), (prof.get("_source") or {}).get("sha256")
        if have != want:
            res = ({}, f"profiles/pmc_summary.json was recorded from other kernel sources (its hash {str(have)[:12]}, this tree "
                       f"{want[:12]}): re-run tools/profile.sh")
        else:
            res = (prof, None)
    _PMC_CACHE[PMC_PATH] = res
    return res


def pmc_note():
    """why the counter fields of this line are null, or None"""
    return pmc_profile()[1]


def pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` from the rocprofv3 PMC passes of tools/profile.sh (same
    command, separate passes), as committed in profiles/: WRITE_SIZE (KB, exact) + 2 x FETCH_SIZE
    (KB; gfx950 reports half the bytes of 16-byte-per-lane reads, MI355X_MICROARCH.md, HBM).
    None when no profile has been committed."""
    try:
        prof = pmc_profile()[0]
        ks = [prof["ed::" + name.strip()] for name in kernel.split("+")]
        fetch, write = sum(k["FETCH_SIZE"] for k in ks), sum(k["WRITE_SIZE"] for k in ks)
        return {"bytes": (2.0 * fetch + write) * 1024.0, "fetch_size_kb_raw": fetch, "write_size_kb_raw": write,
                "source": PMC_SOURCE}
    except (KeyError, TypeError):
        return None


def pmc_valu_busy(kernel):
    """VALU-busy fraction of `kernel` from the same committed PMC passes: SQ_INSTS_VALU wave-instructions
    x 4 clocks (one VALU instruction per SIMD per 4 clocks, profiles/r01_valu_rates.txt) / (1024 SIMDs x
    GRBM_GUI_ACTIVE / 8 XCDs).  None when the profile lacks the counters."""
    try:
        ks = [pmc_profile()[0]["ed::" + name.strip()] for name in kernel.split("+")]
        return {"value": 4.0 * sum(k["SQ_INSTS_VALU"] for k in ks) / (1024.0 * sum(k["GRBM_GUI_ACTIVE"] for k in ks) / 8.0),
                "source": PMC_SOURCE}
    except (KeyError, TypeError, ZeroDivisionError):
        return None


def pmc_executed(kernel, items):
    """VALU lane-instructions per item that `kernel` executed in the committed PMC pass (SQ_INSTS_VALU counts
    wave-instructions, 64 lanes each)"""
    try:
        ks = [pmc_profile()[0]["ed::" + name.strip()] for name in kernel.split("+")]
        return {"value": 64.0 * sum(k["SQ_INSTS_VALU"] for k in ks) / items, "source": PMC_SOURCE}
    except (KeyError, TypeError, ZeroDivisionError):
        return None


def run_step(op, w):
    if op == "verify":
        return ed.ed25519_verify_batch(w["sigs"], w["pubs"], w["msgs"], msg_len=32)
    if op == "x25519":
        return ed.x25519_batch(w["scalars"], w["points"])
    return ed.ed25519_sign_batch(w["secs"], w["pubs"], w["msgs"], msg_len=32)


def usable_cores():
    """host cores this process may actually use: affinity mask, capped by the cgroup CPU quota"""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            cores = max(1, min(cores, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return cores


def cpu_baseline(op, w, gpu_out, sample):
    """Time the reference (oracle/_ref, kind "reference"; else the C restatement, kind "port") on
    all host cores over the first `sample` items of the same workload; check the GPU against it."""
    cores = usable_cores()
    refdrv = os.path.join(ROOT, "oracle", "_ref", "libref_driver.so")
    if os.path.exists(refdrv):
        lib, kind = ctypes.CDLL(refdrv), "reference"
        fn = {"verify": lib.refdrv_verify_batch, "x25519": lib.refdrv_x25519_batch, "sign": lib.refdrv_sign_batch}[op]
    else:
        lib, kind = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so")), "port"
        fn = {"verify": lib.orc_ed25519_verify_batch, "x25519": lib.orc_x25519_batch, "sign": lib.orc_ed25519_sign_batch}[op]
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    host = {k: v[:sample].cpu().numpy().copy() for k, v in w.items() if k not in ("expect", "valid")}
    if op == "verify":
        out = np.zeros(sample, np.uint8)
        args = (P(out), P(host["sigs"]), P(host["pubs"]), P(host["msgs"]), ctypes.c_size_t(32), ctypes.c_size_t(sample), cores)
    elif op == "x25519":
        out = np.zeros((sample, 32), np.uint8)
        args = (P(out), P(host["scalars"]), P(host["points"]), ctypes.c_size_t(sample), cores)
    else:
        out = np.zeros((sample, 64), np.uint8)
        args = (P(out), P(host["secs"]), P(host["pubs"]), P(host["msgs"]), ctypes.c_size_t(32), ctypes.c_size_t(sample), cores)
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        fn(*args)
        best = min(best, time.perf_counter() - t0)
    same = bool(np.array_equal(out.reshape(sample, -1), gpu_out[:sample].cpu().numpy().reshape(sample, -1)))
    return {"value": sample / best, "unit": UNIT[op], "cores": cores, "kind": kind,
            "sample": f"first {sample} items of the same batch, {cores} pthreads, best of 3",
            "per_core": sample / best / cores, "gpu_matches_cpu_on_sample": same}


class SmiSampler:
    """power / sclk of this GPU from `rocm-smi` about once a second while a region runs (None when unreadable)"""

    def __init__(self, index):
        import threading
        self.index, self.samples, self.stop = index, [], threading.Event()
        self.thread = threading.Thread(target=self.run, daemon=True)

    def read(self):
        import re
        try:
            txt = subprocess.run(["rocm-smi", "-d", str(self.index), "--showpower", "--showclocks"], capture_output=True,
                                 text=True, timeout=5).stdout
        except (OSError, subprocess.SubprocessError):
            return None
        pw = re.search(r"Power[^\n]*?:\s*([0-9.]+)", txt)
        ck = re.search(r"sclk clock level[^\n]*?\((\d+)Mhz\)", txt)
        if not pw and not ck:
            return None
        return (time.perf_counter(), float(pw.group(1)) if pw else None, int(ck.group(1)) if ck else None)

    def run(self):
        while not self.stop.is_set():
            r = self.read()
            if r:
                self.samples.append(r)
            self.stop.wait(0.8)

    def __enter__(self):
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.thread.join(timeout=10)

    def summary(self, since):
        rows = [r for r in self.samples if r[0] >= since]
        pw = [r[1] for r in rows if r[1] is not None]
        ck = [r[2] for r in rows if r[2] is not None]
        if not rows:
            return None
        return {"samples": len(rows), "power_w": [min(pw), max(pw)] if pw else None, "sclk_mhz": [min(ck), max(ck)] if ck else None,
                "source": "rocm-smi --showpower --showclocks, about one sample per second during the measured half"}


def sustained_verify(w, n, seconds, local, burst_rate):
    """config 2's pass back to back for `seconds`; the rate over the LAST HALF of that time (HIP events, kernel
    time plus launch gaps), beside the burst rate of the headline region"""
    torch.cuda.synchronize()
    marks = []
    with SmiSampler(local) as smi:
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            for _ in range(16):
                ev = torch.cuda.Event(enable_timing=True)
                out = ed.ed25519_verify_batch(w["sigs"], w["pubs"], w["msgs"], msg_len=32)
                ev.record()
                marks.append((time.perf_counter(), ev))
            marks[-1][1].synchronize()                  # keep the queue bounded: at most 16 passes ahead
        torch.cuda.synchronize()
        t_end = time.perf_counter()
    half = t0 + (t_end - t0) / 2
    tail = [ev for t, ev in marks if t >= half]
    ms = tail[0].elapsed_time(tail[-1]) if len(tail) > 1 else float("nan")
    rate = (len(tail) - 1) * n / (ms * 1e-3)
    return {"metric": "ed25519 verifies/sec sustained: the same pass back to back, rate over the last half of the run",
            "value": rate, "unit": UNIT["verify"], "seconds": t_end - t0, "passes": len(marks), "measured_passes": len(tail) - 1,
            "ms_per_step": ms / max(1, len(tail) - 1), "burst_value": burst_rate, "sustained_over_burst": rate / burst_rate,
            "outputs_correct": bool(torch.equal(out, w["expect"])), "rocm_smi": smi.summary(half),
            "note": "the chip is power-bound under this kernel (DESIGN.md 7): the 0.2-second headline region runs above the "
                    "clock it can hold; this is the steady state"}


def ragged_messages(steps, device):
    """Ragged messages: 2^18 items with lengths drawn uniformly from 0 .. 4096 bytes, in the caller's (random)
    order, device-resident.  A lane hashes its message block by block and a wave ends with its longest message; the hashing
    kernels take such a batch in order of length (csrc/kernels.hip: msg_order).  Signed on the GPU, verified on the GPU, a sample
    of signatures and verdicts checked against the oracle item by item."""
    m, top = 1 << 18, 4096
    g = torch.Generator(device="cpu").manual_seed(20250105)
    lens = torch.randint(0, top + 1, (m,), generator=g, dtype=torch.int64)
    off = torch.zeros(m + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(lens, 0)
    blob = torch.randint(0, 256, (int(off[-1]),), dtype=torch.uint8, generator=g).to(device)
    sk = torch.randint(0, 256, (m, 32), dtype=torch.uint8, generator=g).to(device)
    d_off = off.to(device)
    pk = ed.ed25519_genpub_batch(sk)
    sig = ed.ed25519_sign_batch(sk, pk, blob, msg_off=d_off)
    bad = sig.clone()
    bad[::9, 40] ^= 4
    res = {}
    for name, fn in (("verify", lambda: ed.ed25519_verify_batch(bad, pk, blob, msg_off=d_off)),
                     ("sign", lambda: ed.ed25519_sign_batch(sk, pk, blob, msg_off=d_off))):
        for _ in range(2):
            out = fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        res[name] = (out, e0.elapsed_time(e1) / steps)
    ok = res["verify"][0].cpu().numpy()
    expect = np.ones(m, np.uint8); expect[::9] = 0
    orc = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))     # the checker, after the timed region
    hs, hp, hk, hb, hsig = (t.cpu().numpy() for t in (bad, pk, sk, blob, res["sign"][0]))
    same = bool(np.array_equal(ok, expect))
    want_sig = ctypes.create_string_buffer(64)
    for i in list(range(0, 96)) + list(range(m - 32, m)):
        lo, hi = int(off[i]), int(off[i + 1])
        mb = hb[lo:hi].tobytes()
        same = same and bool(orc.orc_ed25519_verify(hs[i].tobytes(), hp[i].tobytes(), mb, ctypes.c_size_t(hi - lo))) == bool(ok[i])
        orc.orc_ed25519_sign(want_sig, hk[i].tobytes(), hp[i].tobytes(), mb, ctypes.c_size_t(hi - lo))
        same = same and want_sig.raw == hsig[i].tobytes()
    total = int(off[-1])
    return {"metric": "ed25519 verifies/sec on ragged messages, lengths uniform in 0 .. 4096 bytes, 2^18 items in HBM",
            "value": m / (res["verify"][1] * 1e-3), "unit": UNIT["verify"], "ms_per_step": res["verify"][1],
            "sign_value": m / (res["sign"][1] * 1e-3), "sign_ms_per_step": res["sign"][1], "items": m, "message_bytes": total,
            "message_gbs_verify": total / (res["verify"][1] * 1e-3) / 1e9, "outputs_correct": same,
            "note": "the hashing kernels take a ragged batch in order of message length (per-pass counting sort); "
                    "profiles/r05_msglen.txt has the same batch before and after, and the long-message floor"}


def garbage_keys(w, m, steps, device):
    """The worst case a caller can construct: the config's genuine signatures under RANDOM 32-byte keys.  ed_import never
    fails (reference lib/ed.c:100-149), about half of all strings are no curve point, and for those the reference's bytes
    depend on its exact sequence of formulas - so half the batch goes through the reference-order chain
    (k_verify_exact_quad, four lanes per item, strided over the whole work list) on top of the windowed pass.  Verdicts
    checked against the compiled reference (else the oracle) on a sample."""
    g = torch.Generator(device="cpu").manual_seed(20250104)
    keys = torch.randint(0, 256, (m, 32), dtype=torch.uint8, generator=g)
    keep = torch.arange(m) % 16 == 3                          # one genuine key in sixteen stays: some accepts to check
    keys[keep] = w["valid"][1][:m].cpu()[keep]
    dk = keys.to(device)
    sig, msg = w["valid"][0][:m], w["valid"][2][:m]
    for _ in range(2):
        ok = ed.ed25519_verify_batch(sig, dk, msg, msg_len=32)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        ok = ed.ed25519_verify_batch(sig, dk, msg, msg_len=32)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    sample = min(4096, m)
    hs, hk, hm = (np.ascontiguousarray(t[:sample].cpu().numpy()) for t in (sig, dk, msg))
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    want = np.zeros(sample, np.uint8)
    refdrv = os.path.join(ROOT, "oracle", "_ref", "libref_driver.so")
    if os.path.exists(refdrv):
        ctypes.CDLL(refdrv).refdrv_verify_batch(P(want), P(hs), P(hk), P(hm), ctypes.c_size_t(32), ctypes.c_size_t(sample), usable_cores())
    else:
        ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle.so")).orc_ed25519_verify_batch(
            P(want), P(hs), P(hk), P(hm), ctypes.c_size_t(32), ctypes.c_size_t(sample), usable_cores())
    got = ok.cpu().numpy()
    p, d = 2**255 - 19, (-121665 * pow(121666, 2**255 - 21, 2**255 - 19)) % (2**255 - 19)
    off = 0
    for row in hk[:1024]:                                     # which keys are no curve point: (y^2 - 1) / (d y^2 + 1) is no square
        y = int.from_bytes(row.tobytes(), "little") % 2**255 % p
        x2 = (y * y - 1) * pow(d * y * y + 1, p - 2, p) % p
        off += x2 != 0 and pow(x2, (p - 1) // 2, p) != 1
    good = bool(np.array_equal(got[:sample], want)) and int(got.sum()) == int(keep.sum()) and bool(np.array_equal(got.astype(bool), keep.numpy()))
    return {"metric": "ed25519 verifies/sec, worst case: genuine signatures under random 32-byte keys (one genuine key in 16 kept)",
            "value": m / (ms * 1e-3), "unit": UNIT["verify"], "ms_per_step": ms, "items": m, "accepted": int(got.sum()),
            "off_curve_fraction_of_1024_keys": off / min(1024, sample), "outputs_correct": good,
            "note": "keys that are no curve point take the reference-order chain (bit-exactness needs the reference's own "
                    "sequence of formulas there); checked against the reference on the first 4096 items"}


def gather_results(out, world, everywhere=True):
    """N > 1: the final result gather, the only exchange of the path.  Verdict bytes (1 B per item) are
    all-gathered, so that every rank holds the whole vector; the 32- and 64-byte results of x25519 and sign are
    gathered at rank 0 (everywhere=False), where a caller would collect them."""
    if world == 1:
        return out
    if dist.get_backend() == "gloo":                    # test hook (see main): stage through the host
        out = out.cpu()
    if everywhere:
        full = torch.empty((world * out.shape[0],) + tuple(out.shape[1:]), dtype=out.dtype, device=out.device)
        dist.all_gather_into_tensor(full, out)          # concatenated along dim 0: valid on nccl and gloo
        return full.view((world,) + tuple(out.shape))
    parts = [torch.empty_like(out) for _ in range(world)] if dist.get_rank() == 0 else None
    dist.gather(out, parts, dst=0)
    return torch.stack(parts) if parts is not None else None


def timed_region(step, steps, world, sync, device):
    """EXACTLY `steps` steps between two (barrier + device sync) brackets; returns the MAX over
    ranks of the elapsed seconds and the last step's output."""
    sync()
    if world > 1:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    out = None
    for _ in range(steps):
        out = step()
    sync()
    if world > 1:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    LOCAL_ELAPSED[0] = elapsed
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed, out


LOCAL_ELAPSED = [0.0]       # this rank's own wall time of the last timed region (the line reports the max over ranks)
HOST_GROUP = [None]         # gloo group beside the RCCL one: host-side barriers and small host gathers


def host_barrier():
    if HOST_GROUP[0] is not None:
        dist.barrier(group=HOST_GROUP[0])


def per_rank_breakdown(world, rank, steps, k_ms, g_ms):
    """N > 1: every rank's kernel ms, gather ms and wall ms per step, collected at rank 0 over the host group"""
    if world == 1:
        return None
    dev = my_device()
    smi = SmiSampler(dev).read() if dev >= 0 else None       # one sample right after the region: boxes (and ranks) differ in the clock they hold
    mine = {"rank": rank, "device": dev, "kernel_ms": k_ms, "gather_ms": g_ms,
            "wall_ms_per_step": LOCAL_ELAPSED[0] / steps * 1e3, "power_w": smi[1] if smi else None, "sclk_mhz": smi[2] if smi else None}
    rows = [None] * world
    dist.all_gather_object(rows, mine, group=HOST_GROUP[0])
    slow = max(rows, key=lambda r: r["kernel_ms"])       # (the walls agree: every step ends in the gather, which waits for this one)
    ks = [r["kernel_ms"] for r in rows]
    return {"ranks": rows, "slowest_rank": slow["rank"], "kernel_ms_min_max": [min(ks), max(ks)],
            "gather_ms_max": max(r["gather_ms"] for r in rows),
            "note": "kernel_ms: HIP events around the pass on the rank's stream; gather_ms: from the kernels' end to the end of the "
                    "result gather on that stream (includes waiting for the slowest rank's kernels)"}


def my_device():
    """this rank's HIP device, -1 where there is none (the CPU tests of the N > 1 plumbing)"""
    return torch.cuda.current_device() if torch.cuda.is_available() else -1


def devices_distinct(devs, world, shared_gpu):
    """every rank on a device of its own?  Otherwise exit non-zero - unless the one-GPU test hook asked for sharing"""
    distinct = len(devs) == world and len(set(devs)) == world
    if not distinct and not shared_gpu:
        raise SystemExit(f"bench.py: {world} ranks on devices {devs}: one rank per GPU is the contract")
    return distinct


def collective_facts(world, backend, shared_gpu):
    """N > 1: what the result gather ran over, and that every rank owns a device of its own.  Exits non-zero when two
    ranks sit on one device (a scaling point measured that way would be meaningless) - unless the one-GPU test hook
    EDDSA_BENCH_SHARE_GPU asked for exactly that, which the line then says."""
    devs = [None] * world
    dist.all_gather_object(devs, my_device(), group=HOST_GROUP[0])
    distinct = devices_distinct(devs, world, shared_gpu)
    try:
        ver = ".".join(str(x) for x in torch.cuda.nccl.version()) if backend == "nccl" else None
    except Exception:                                       # noqa: BLE001  (a version string is not worth a failed run)
        ver = None
    return {"world": dist.get_world_size(), "backend": dist.get_backend(), "version": ver, "is_rccl": backend == "nccl",
            "devices": devs, "devices_distinct": distinct, "shared_gpu_test_hook": bool(shared_gpu)}


def all_ranks_agree(flag, world, device):
    if world == 1:
        return flag
    t = torch.tensor([int(flag)], dtype=torch.int32, device=device if dist.get_backend() == "nccl" else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(t.item())


def measure(op, w, n, steps, warmup, world, device, detail=True):
    """warm up, then time `steps` steps of `op` on this rank's n items (plus the result gather);
    -> (elapsed seconds, last output, average kernel-only ms from HIP events on the launch stream,
        verify's per-kernel phase times or None, the gathered result, average gather ms).
    detail=False (a plain run): no HIP events and no phase timing in the steps; kernel and gather ms are None"""
    marks, gathered = [], [None]

    def step():
        if detail:
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
        out = run_step(op, w)
        if detail:
            e1.record()
        gathered[0] = gather_results(out, world, everywhere=(op == "verify"))   # the final result gather (RCCL over xGMI)
        if detail:
            e2.record()
            marks.append((e0, e1, e2))
        return out

    for _ in range(warmup):
        step()
    marks.clear()
    if detail and op == "verify":
        ed.set_profiling(True)
    elapsed, out = timed_region(step, steps, world, torch.cuda.synchronize, device)
    if not detail:
        return elapsed, out, None, None, gathered[0], None
    phases = ed.verify_phase_ms() if op == "verify" else None
    ed.set_profiling(False)
    k_ms = sum(a.elapsed_time(b) for a, b, _ in marks) / len(marks)
    g_ms = sum(b.elapsed_time(c) for _, b, c in marks) / len(marks)       # kernels' end -> gather's end on this rank's stream
    return elapsed, out, k_ms, phases, gathered[0], g_ms


DUMP_NAMES = {"verify": "verdicts", "x25519": "x25519_outputs", "sign": "signatures"}
DUMP_ITEM_BYTES = {"verify": 1, "x25519": 32, "sign": 64}
DUMP_MAX_BYTES = 32 << 20        # float32 bytes written at most (the largest default output, 2^20 x 64 signature bytes, is 256 MiB)
DUMP_SEED = 20251016


def dump_outputs(path, op, result):
    """--dump-outputs: what a caller of the timed path received from its last step - the verdict bytes (n,), the x25519
    outputs (n, 32) or the signatures (n, 64), gathered over the ranks at N > 1 - as <path>/<name>.npy in float32 (byte
    values 0..255).  When that is more than DUMP_MAX_BYTES, the file holds a fixed sample: the items whose indices a
    generator seeded with DUMP_SEED draws without replacement, in ascending order - the same items for the same arguments."""
    width = DUMP_ITEM_BYTES[op]
    a = result.cpu().numpy().reshape(-1, width)
    keep = DUMP_MAX_BYTES // (4 * width)
    if a.shape[0] > keep:
        a = a[np.sort(np.random.default_rng(DUMP_SEED).choice(a.shape[0], keep, replace=False))]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, DUMP_NAMES[op] + ".npy"), (a[:, 0] if width == 1 else a).astype(np.float32))


def fixture_check(full, world, n, seed, config):
    """verify: SHA-512 of the whole (gathered) verdict vector against the digest the compiled reference
    produced for this seeded batch (tests/golden/batch_digests.json, data only); None when the batch
    is not one of the pinned ones"""
    import hashlib
    ok = full.reshape(-1).cpu().numpy()
    digest = hashlib.sha512(ok.tobytes()).hexdigest()
    try:
        pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "batch_digests.json")))
        total = world * n
        key = f"verify_2^{total.bit_length() - 1}"
        fx = pinned[key] if total & (total - 1) == 0 else None
        if not fx or (fx.get("seed", 1), fx.get("config", 2)) != (seed, config):
            fx = None
    except (OSError, ValueError, KeyError):
        fx = None
    return {"verdicts_sha512": digest, "accepted": int(ok.sum()),
            "matches_reference_digest": None if fx is None else bool(fx["verdicts_sha512"] == digest)}


def roofline_of(op, n, k_ms, phases, ms_per_step, passes):
    """the kernels of the op against the integer-VALU multiply-issue roofline, per launch of at most 2^20 items
    (HIP events around the pass).  SURVEY 8(d): achieved = rate x the reference's canonical product count, so an
    evaluation that needs fewer products than the reference's (verify: half-length scalars, windows, no final
    inversion) scores above its executed-instruction share; "valu_busy" and "executed_valu_per_item" (PMC) say
    what was actually issued."""
    kernel = KERNELS[op]
    main_ms, k_mul32, items = k_ms / passes, MUL32[op], n / passes
    achieved = items * k_mul32 / (main_ms * 1e-3) / 1e12
    r = {
        "bound": "valu", "kernel": kernel, "achieved": achieved, "peak": PEAK_TMUL32,
        "unit": "Tmul32/s", "frac": achieved / PEAK_TMUL32, "traffic": pmc_traffic(kernel),
        "valu_busy": pmc_valu_busy(kernel), "executed_valu_per_item": pmc_executed(kernel, 1 << 20),
        "counters_note": pmc_note(),                 # why traffic / valu_busy / executed_valu_per_item are null, or null
        "kernel_ms": main_ms, "items_per_launch": items, "canonical_mul32_per_item": k_mul32,
        "whole_pass": {"kernels_ms": k_ms, "canonical_mul32_per_item": MUL32[op],
                       "achieved": n * MUL32[op] / (k_ms * 1e-3) / 1e12,
                       "frac": n * MUL32[op] / (k_ms * 1e-3) / 1e12 / PEAK_TMUL32},
        "note": "integer-VALU multiply-issue roofline (SURVEY 8d): canonical 32x32->64 products of the "
                "reference's radix-2^25.5 schoolbook per item / v_mad_u64_u32 issue peak; the path is not "
                "HBM- or MFMA-bound",
        "hbm": {"achieved": n * BYTES[op] / (ms_per_step * 1e-3) / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                "frac": n * BYTES[op] / (ms_per_step * 1e-3) / 1e9 / PEAK_HBM_GBS,
                "algorithmic_bytes_per_item": BYTES[op]},
    }
    if phases:
        r["phase_ms"] = {"k_verify_prepare + k_verify_halve": phases[0], "k_verify_main_half": phases[1]}
        r["dominant"] = {"kernel": "k_verify_main_half", "kernel_ms": phases[1], "share_of_pass": phases[1] / main_ms,
                         "valu_busy": pmc_valu_busy("k_verify_main_half"),
                         "executed_valu_per_item": pmc_executed("k_verify_main_half", 1 << 20)}
    return r


def spawn_ranks(n, argv):
    """--gpus N without a torch.distributed environment: start the N ranks as a child process, before
    this process has touched the GPU, and hand its exit code back"""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    # HSA_ENABLE_IPC_MODE_LEGACY: this pool's host driver supports dmabuf IPC only - with the legacy mode RCCL's buffer
    # exchange between the ranks fails in hipIpcGetMemHandle ("invalid argument").  The image and the GPU boxes export 0;
    # the ranks inherit whatever the caller's environment says, and 0 only when it says nothing (ROCm 7.2.0 / RCCL 2.2x of
    # this image; nothing else in the repository touches the variable).
    return subprocess.call(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--op", choices=("all", "verify", "x25519", "sign"), default="all")
    ap.add_argument("--log2n", type=int, default=None,
                    help="items per GPU = 2^log2n (default: 2^20 at N = 1; config 4's 2^24 / N verifies at N > 1)")
    ap.add_argument("--cpu-sample", type=int, default=1 << 18, help="items of the CPU baseline (--full)")
    ap.add_argument("--sustained", type=float, default=10.0,
                    help="seconds of back-to-back verify passes for secondary.verify_sustained (N = 1, --op all, --full; 0 = skip)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the last step as DIR/<name>.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="also the roofline, the reference's digest, the CPU baseline, the per-rank breakdown and, with "
                         "--op all, the secondary ops and configurations")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s)")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the engine has no CPU fallback")
    # Test hooks, so that the N > 1 code path can be exercised on a one-GPU box: EDDSA_BENCH_SHARE_GPU=1
    # maps every rank onto the visible devices round-robin, EDDSA_BENCH_BACKEND=gloo replaces RCCL
    # (which refuses two ranks on one device).  Neither is set by the driver's runs.
    if os.environ.get("EDDSA_BENCH_SHARE_GPU") == "1":
        local %= torch.cuda.device_count()
    backend = os.environ.get("EDDSA_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
        HOST_GROUP[0] = dist.new_group(backend="gloo")     # host-side barriers and small host gathers
        # a misconfigured node fails here, in seconds, before a 2^24-item workload is generated: every rank on a device
        # of its own (exits otherwise), the ranks the launcher was asked for, and a collective library that answers
        facts = collective_facts(world, backend, os.environ.get("EDDSA_BENCH_SHARE_GPU") == "1")
        if facts["world"] != args.gpus:
            raise SystemExit(f"bench.py: the process group has {facts['world']} ranks, --gpus says {args.gpus}")
        if backend == "nccl" and not facts["version"]:
            raise SystemExit("bench.py: torch.cuda.nccl.version() gives nothing: no RCCL behind torch.distributed")
    ed.init(local)

    # sizes: config 2 at N = 1, config 4 (2^24 in total) at N > 1, unless --log2n says otherwise
    main_op = "verify" if args.op == "all" else args.op
    if args.log2n is not None:
        n, scaling, seed, config = 1 << args.log2n, "weak", 1, 2
        what = f"batch=2^{args.log2n} per GPU"
    elif world > 1 and main_op == "verify":
        n, scaling, seed, config = (1 << 24) // world, "strong", 3, 4
        what = f"config 4: batch=2^24 sharded over {world} GPUs ({n} items each), RCCL gather of the verdicts"
    else:
        n, scaling, seed, config = 1 << 20, "weak", 1, 2
        what = "config 2: batch=2^20 per GPU" if main_op == "verify" else "batch=2^20 per GPU"
    n2 = min(n, 1 << 20) if args.log2n is not None else 1 << 20        # secondary ops: 2^20 per GPU

    w = make_workload(main_op, n, rank * n, device, seed, config)
    torch.cuda.synchronize()
    elapsed, out, k_ms, phases, full, g_ms = measure(main_op, w, n, args.steps, args.warmup, world, device, detail=args.full)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, main_op, full)
    correct = bool(torch.equal(out, w["expect"])) if main_op == "verify" else True
    correct = all_ranks_agree(correct, world, device)
    ms_per_step = elapsed / args.steps * 1e3
    line = {
        "metric": {"verify": "ed25519 verifies/sec", "x25519": "x25519 ops/sec", "sign": "ed25519 signs/sec"}[main_op],
        "value": world * n * args.steps / elapsed, "unit": UNIT[main_op],
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
        "dtype": "u32 (radix-2^25.5 limbs, u64 accumulators)", "data": "synthetic",
        "config": {"workload": f"{what}, " + ("x25519 variable-base" if main_op == "x25519" else f"ed25519 {main_op}"),
                   "msg_len": 32 if main_op != "x25519" else None, "items_per_gpu": n, "total_items": world * n,
                   "parallelism": f"shard{world}+allgather" if world > 1 else "single"},
        "outputs_correct": correct if main_op == "verify" or args.full else None,
    }
    if args.full:
        per_rank = per_rank_breakdown(world, rank, args.steps, k_ms, g_ms)
        pinned = fixture_check(full, world, n, seed, config) if main_op == "verify" and rank == 0 else None
        if pinned and pinned["matches_reference_digest"] is False:
            correct = False
        # the CPU baseline: rank 0 times it on all host cores while the other ranks sleep in a host-side barrier
        base = cpu_baseline(main_op, w, out, min(args.cpu_sample, n)) if rank == 0 else None
        host_barrier()
        correct = correct and (base is None or base["gpu_matches_cpu_on_sample"])
        passes = (n + (1 << 20) - 1) >> 20
        line.update({"outputs_correct": correct, "verdicts": pinned,
                     "roofline": roofline_of(main_op, n, k_ms, phases, ms_per_step, passes), "cpu_baseline": base})
        if per_rank:
            line["per_rank"] = per_rank
        if world > 1:
            line["rccl"] = collective_facts(world, backend, os.environ.get("EDDSA_BENCH_SHARE_GPU") == "1")
            if line["rccl"]["world"] != args.gpus:
                raise SystemExit(f"bench.py: the process group has {line['rccl']['world']} ranks, --gpus says {args.gpus}")
    secondary = {}
    if args.full and args.op == "all" and main_op == "verify":
        # SURVEY 8(f)-3, opt-in: the same items BEFORE corruption through ed25519_verify_batch_rlc (groups of 8192
        # checked by one random linear combination; a group that fails falls back to the per-item kernels)
        m = min(n, 1 << 20)
        vs, vp, vm = w["valid"][0][:m], w["valid"][1][:m], w["valid"][2][:m]
        for _ in range(max(1, args.warmup)):
            ed.ed25519_verify_batch_rlc(vs, vp, vm, msg_len=32)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            okr = ed.ed25519_verify_batch_rlc(vs, vp, vm, msg_len=32)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        okr2, st = ed.ed25519_verify_batch_rlc(vs, vp, vm, msg_len=32, return_stats=True)   # (the statistics are read back by the host: after the timed passes)
        okr = okr & okr2
        # (calls below the library's break-even size skip the combination: then st[1] == m)
        good = all_ranks_agree(bool(okr.all()) and st[0] + st[1] == m and (st[0] == m or m < ed.RLC_MIN_ITEMS_DEFAULT), world, device)
        correct = correct and good
        secondary["verify_rlc_all_valid"] = {
            "metric": "ed25519 verifies/sec, opt-in batch verification, the config's items before corruption (all valid)",
            "value": world * m * args.steps / el, "unit": UNIT["verify"], "ms_per_step": el / args.steps * 1e3,
            "items_per_gpu": m, "stats": st, "outputs_correct": good,
            "note": "not the headline: verdicts equal the per-item path's, see include/eddsa_amd.h for the caveat; "
                    "time of this rank (no gather)"}
    if args.full and args.op == "all" and main_op == "verify" and world == 1:
        # PCIe-inclusive, for the record only (never `value`): the same batch from ordinary host memory to host memory through
        # the host-pointer entry point (staging, three lanes: libeddsa_amd/csrc/host_pipe.c)
        m = min(n, 1 << 20)
        hs, hp, hm = (w[k][:m].cpu().numpy() for k in ("sigs", "pubs", "msgs"))
        for _ in range(2):
            okh = ed.ed25519_verify_batch(hs, hp, hm, msg_len=32)
        best = float("inf")
        for _ in range(5):
            t0 = time.perf_counter()
            okh = ed.ed25519_verify_batch(hs, hp, hm, msg_len=32)
            best = min(best, time.perf_counter() - t0)
        good = bool(np.array_equal(okh, w["expect"][:m].cpu().numpy()))
        correct = correct and good
        secondary["verify_host_to_host"] = {
            "metric": "ed25519 verifies/sec, PCIe-inclusive: numpy (malloc) arrays in, numpy array out, best of 5",
            "value": m / best, "unit": UNIT["verify"], "ms_per_call": best * 1e3, "items": m, "outputs_correct": good,
            "note": "not the headline: `value` is measured with inputs resident in HBM"}
        # the drop-in side of the boundary: one call of the reference's single-item function (eddsa.h), host buffers,
        # a pass of one item on the GPU; and a small batch, where the pass costs its latency whatever it carries
        one = [hs[0].tobytes(), hp[0].tobytes(), hm[0].tobytes()]
        for _ in range(20):
            ok1 = ed.ed25519_verify(*one)
        t0 = time.perf_counter()
        for _ in range(200):
            ok1 = ed.ed25519_verify(*one)
        t_one = (time.perf_counter() - t0) / 200
        sel = np.flatnonzero(w["expect"][:8192].cpu().numpy())[:256]     # 256 genuine signatures (a key off the curve adds the exact path's 0.5 ms)
        s256, p256, m256 = (np.ascontiguousarray(a[sel]) for a in (hs, hp, hm))
        for _ in range(5):
            ok256 = ed.ed25519_verify_batch(s256, p256, m256, msg_len=32)
        t0 = time.perf_counter()
        for _ in range(50):
            ok256 = ed.ed25519_verify_batch(s256, p256, m256, msg_len=32)
        t_256 = (time.perf_counter() - t0) / 50
        good = bool(ok1) == bool(w["expect"][0].item()) and len(sel) == 256 and bool(ok256.all())
        correct = correct and good
        secondary["verify_small_calls"] = {
            "metric": "latency of host-pointer calls, one caller in a loop", "single_ed25519_verify_ms": t_one * 1e3,
            "verify_batch_256_valid_ms": t_256 * 1e3, "outputs_correct": good,
            "note": "concurrent single-item calls are merged into one launch (tests/c/threaded_callers.c measures that)"}
    if args.full and args.op == "all" and main_op == "verify" and world == 1:
        secondary["verify_garbage_keys"] = garbage_keys(w, min(n, 1 << 20), args.steps, device)
        correct = correct and secondary["verify_garbage_keys"]["outputs_correct"]
        secondary["verify_ragged_messages"] = ragged_messages(max(2, args.steps // 2), device)
        correct = correct and secondary["verify_ragged_messages"]["outputs_correct"]
    if args.full and args.op == "all" and main_op == "verify" and world == 1 and args.sustained > 0:
        secondary["verify_sustained"] = sustained_verify(w, n, args.sustained, local, line["value"])
        correct = correct and secondary["verify_sustained"]["outputs_correct"]
    del w, out, full

    if args.full and args.op == "all":                  # the rest of BASELINE's metric, same process, same step count
        for op in ("x25519", "sign"):
            w2 = make_workload(op, n2, rank * n2, device)
            torch.cuda.synchronize()
            el2, out2, k2, _, _, g2 = measure(op, w2, n2, args.steps, max(1, args.warmup), world, device)
            pr2 = per_rank_breakdown(world, rank, args.steps, k2, g2)
            base2 = cpu_baseline(op, w2, out2, min(4096, n2)) if rank == 0 else None
            host_barrier()
            ok2 = all_ranks_agree(base2 is None or base2["gpu_matches_cpu_on_sample"], world, device)
            correct = correct and ok2
            ms2 = el2 / args.steps * 1e3
            secondary[op] = {"metric": {"x25519": "x25519 ops/sec", "sign": "ed25519 signs/sec"}[op],
                             "value": world * n2 * args.steps / el2, "unit": UNIT[op], "ms_per_step": ms2,
                             "items_per_gpu": n2, "scaling": "weak", "outputs_correct": ok2,
                             "roofline": roofline_of(op, n2, k2, None, ms2, 1), "cpu_baseline": base2}
            if pr2:
                secondary[op]["per_rank"] = pr2
            del w2, out2
        line["secondary"] = secondary
        line["outputs_correct"] = correct
    if rank == 0:
        print(json.dumps(line))
    if world > 1:
        dist.destroy_process_group()
    if not correct:
        raise SystemExit("bench.py: GPU outputs differ from the expected verdicts / CPU reference")


if __name__ == "__main__":
    main()
