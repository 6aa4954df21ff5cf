#!/usr/bin/env python3
"""Key-set verification against the unkeyed call (ed25519_verify_keyed_dev against ed25519_verify_batch_dev over the SAME items),
device-resident inputs, device events, in the style of tools/dom2_rate.py:

  row 1   2^20 valid items over 32-byte messages whose keys are drawn from 1, 1024, 2^16 and 2^20 distinct keys: the unkeyed and
          the keyed pass alternating, per key count
  row 2   the per-kernel split of both passes with 1024 keys (verify_phase_ms: prepare (+ halve), main, finish)
  row 3   host buffer to host buffer with 1024 keys (ordinary memory): ed25519_verify_batch against ed25519_verify_keyed
  row 4   the one-off cost of eddsa_amd_keyset_create for 1024 and 2^20 keys (host keys; upload, tables, synchronisation)
  row 5   small passes (1 .. 2^18 items), keyed against unkeyed
  row 6   (with --parent LIB) ed25519_verify_batch_dev of this build against another build of the library, alternating in fresh
          processes: whether the unkeyed pass moved

Every repeat is `iters` calls between two events; the spread of a form is max - min over its repeats.  Before anything is timed
both passes accept every item, and the keyed pass rejects items whose index is shifted by one.

  tools/keyed_rate.py [repeats=5] [log2 of the batch=20] [--parent path/to/libeddsa_amd_debug.so] [--only-small]
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libeddsa_amd as ed  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
PARENT = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
if PARENT:
    args.remove(PARENT)
ONLY_UNKEYED = "--only-unkeyed" in sys.argv        # (the child processes of row 6)
REPEATS = int(args[0]) if len(args) > 0 else 5
LOG_N = int(args[1]) if len(args) > 1 else 20
assert REPEATS >= 3
if not os.environ.get("EDDSA_AMD_LIBRARY"):
    ed.use_debug_library()                         # the product's objects plus the phase timer (a --parent library is bound as given)
import torch  # noqa: E402

ed.init(0)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(forms, repeats=REPEATS):
    iters = {}
    for k, fn in forms.items():
        fn(); torch.cuda.synchronize()
        iters[k] = max(2, min(50, int(100.0 / max(timed(fn, 2), 1e-3))))
    out = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            out[k].append(timed(fn, iters[k]))
    return {k: sorted(v) for k, v in out.items()}


def show(label, n, ms, base=None):
    med = ms[len(ms) // 2]
    rel = "" if base is None else f"  {100 * (med - base) / base:+6.2f} % against the unkeyed pass"
    print(f"  {label:44s} {med:9.3f} ms  [{ms[0]:.3f} .. {ms[-1]:.3f}]  spread {ms[-1] - ms[0]:.3f} ms  {n / med / 1e3:8.2f} M/s{rel}", flush=True)
    return med


n = 1 << LOG_N
g = torch.Generator(device="cuda").manual_seed(215)
rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)   # noqa: E731
sk_all, msg = rnd(n, 32), rnd(n, 32)
pk_all = ed.ed25519_genpub_batch(sk_all)


def items(nkeys):
    """the batch with its keys drawn from the first nkeys: item i under key (i * 2654435761) mod nkeys"""
    who = (torch.arange(n, device="cuda", dtype=torch.int64) * 2654435761) % nkeys
    sk, pk = sk_all[who].contiguous(), pk_all[who].contiguous()
    sig = ed.ed25519_sign_batch(sk, pk, msg, msg_len=32)
    return sig, pk, who.to(torch.int32).contiguous()


def small_passes():
    print("small passes, valid items under 1024 keys, device-pointer forms (the keyed pass has the one-lane kernels only):")
    sig, pk, idx = items(1024)
    with ed.keyset_create(pk_all[:1024].contiguous()) as ks:
        for m in (1, 1 << 8, 1 << 11, 1 << 14, 1 << 16, 1 << 18):
            if m > n:
                break
            s_, p_, i_, m_ = (t[:m].contiguous() for t in (sig, pk, idx, msg))
            forms = {"unkeyed": lambda: ed.ed25519_verify_batch(s_, p_, m_, msg_len=32), "keyed": lambda: ed.ed25519_verify_keyed(s_, ks, i_, m_, msg_len=32)}
            assert bool(forms["unkeyed"]().all()) and bool(forms["keyed"]().all())
            r = alternate(forms)
            base = show(f"{m:7d} items  ed25519_verify_batch_dev", m, r["unkeyed"])
            show(f"{m:7d} items  ed25519_verify_keyed_dev", m, r["keyed"], base)
    print()


if "--only-small" in sys.argv:
    small_passes()
    sys.exit(0)

if ONLY_UNKEYED:
    sig, pk, _ = items(1024)
    assert bool(ed.ed25519_verify_batch(sig, pk, msg, msg_len=32).all())
    r = alternate({"u": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32)}, 3)["u"]
    print("UNKEYED", " ".join(f"{x:.4f}" for x in r))
    sys.exit(0)

print(f"verify, 2^{LOG_N} valid items in HBM, 32-byte messages, device-pointer forms, the two alternating ({REPEATS} repeats):")
kept = None
for nkeys in (1, 1024, 1 << 16, n):
    sig, pk, idx = items(nkeys)
    ks = ed.keyset_create(pk_all[:nkeys].contiguous())
    forms = {"unkeyed": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32),
             "keyed": lambda: ed.ed25519_verify_keyed(sig, ks, idx, msg, msg_len=32)}
    assert bool(forms["unkeyed"]().all()) and bool(forms["keyed"]().all())
    if nkeys > 1:
        assert not bool(ed.ed25519_verify_keyed(sig[:4096], ks, ((idx[:4096] + 1) % nkeys).contiguous(), msg[:4096], msg_len=32).any())
    r = alternate(forms)
    print(f" {nkeys} distinct keys (key set: {nkeys * (32 + 1 + 1152) / 1e6:.1f} MB):")
    base = show("ed25519_verify_batch_dev", n, r["unkeyed"])
    show("ed25519_verify_keyed_dev", n, r["keyed"], base)
    if nkeys == 1024:
        print("  per kernel (ms): prepare (+ tables, halve) / main / finish")
        for k, fn in forms.items():
            ed.set_profiling(True)
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            ph = ed.verify_phase_ms()
            ed.set_profiling(False)
            print(f"    {k:8s} {ph[0]:.3f} / {ph[1]:.3f} / {ph[2]:.3f}")
        kept = (sig.cpu().numpy(), pk.cpu().numpy(), idx.cpu().numpy().view(np.uint32), msg.cpu().numpy(), pk_all[:1024].cpu().numpy())
    ks.close()
print()

hs, hp, hi, hm, hk = kept
print(f"host buffer to host buffer, 2^{LOG_N} valid items, 1024 keys, ordinary memory ({REPEATS} repeats, one call each):")
with ed.keyset_create(hk) as ks:
    hforms = {"unkeyed": lambda: ed.ed25519_verify_batch(hs, hp, hm, msg_len=32), "keyed": lambda: ed.ed25519_verify_keyed(hs, ks, hi, hm, msg_len=32)}
    out = {k: [] for k in hforms}
    for k, fn in hforms.items():
        assert bool(fn().all())
    for _ in range(REPEATS):
        for k, fn in hforms.items():
            t0 = time.perf_counter(); fn(); out[k].append(1e3 * (time.perf_counter() - t0))
    base = show("ed25519_verify_batch", n, sorted(out["unkeyed"]))
    show("ed25519_verify_keyed", n, sorted(out["keyed"]), base)
print()

print("eddsa_amd_keyset_create from host keys (upload, tables, synchronisation), ms:")
hall = pk_all.cpu().numpy()
for nkeys in (1024, n):
    t = []
    for _ in range(REPEATS):
        t0 = time.perf_counter(); ks = ed.keyset_create(hall[:nkeys]); t.append(1e3 * (time.perf_counter() - t0)); ks.close()
    t.sort()
    print(f"  {nkeys:8d} keys  {t[len(t) // 2]:9.3f} ms  [{t[0]:.3f} .. {t[-1]:.3f}]")
print()

small_passes()

if PARENT:
    print(f"ed25519_verify_batch_dev, this build against {os.path.relpath(PARENT, ROOT)}, fresh processes alternating (1024 keys' items):")
    mine = os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd_debug.so")
    rows = {"parent": [], "this": []}
    for _ in range(REPEATS):
        for label, lib in (("parent", PARENT), ("this", mine)):
            o = subprocess.check_output([sys.executable, os.path.abspath(__file__), "3", str(LOG_N), "--only-unkeyed"],
                                        env=dict(os.environ, EDDSA_AMD_LIBRARY=lib), text=True, timeout=300)
            rows[label] += [float(x) for x in o.split("UNKEYED")[1].split()]
    show("parent build", n, sorted(rows["parent"]))
    show("this build", n, sorted(rows["this"]))
