#!/usr/bin/env python3
"""Comb key sets against plain key sets and the unkeyed call (ed25519_verify_keyed_dev over a comb set, over a plain set, and
ed25519_verify_batch_dev over the SAME items), device-resident inputs, device events, after tools/keyed_rate.py:

  row 1   2^20 valid items over 32-byte messages under 1, 1024 and 16 384 keys: the three forms alternating, in off-curve modes 0
          and 1 and under the cofactored equation
  row 2   the per-kernel split of the three passes with 1024 keys (verify_phase_ms: prepare (+ tables, halve), main, finish)
  row 3   small passes (2^7, 2^10, 2^14, 2^16 items) under 1024 keys
  row 4   the one-off cost of eddsa_amd_keyset_create_comb and the HBM the set holds, for 1024 and 16 384 keys
  row 5   (with --parent LIB) the two unchanged calls of this build against another build of the library, alternating in fresh
          processes: whether they moved

Every repeat is `iters` calls between two events; the spread of a form is max - min over its repeats.  Before anything is timed
all three passes accept every item, and the comb pass rejects items whose index is shifted by one.

  tools/keyed_comb_rate.py [repeats=5] [log2 of the batch=20] [--parent path/to/libeddsa_amd_debug.so]
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libeddsa_amd as ed  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
PARENT = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
if PARENT:
    args.remove(PARENT)
ONLY_UNCHANGED = "--only-unchanged" in sys.argv    # (the child processes of row 5)
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


def show(label, n, ms, base=None, against="the plain key set"):
    med = ms[len(ms) // 2]
    rel = "" if base is None else f"  {100 * (med - base) / base:+6.2f} % against {against}"
    print(f"  {label:46s} {med:9.3f} ms  [{ms[0]:.3f} .. {ms[-1]:.3f}]  spread {ms[-1] - ms[0]:.3f} ms  {n / med / 1e3:8.2f} M/s{rel}", flush=True)
    return med


n = 1 << LOG_N
g = torch.Generator(device="cuda").manual_seed(216)
rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)   # noqa: E731
MAX_KEYS = min(ed.KEYSET_COMB_MAX_KEYS, n) if hasattr(ed, "KEYSET_COMB_MAX_KEYS") else 1024
sk_all, msg = rnd(MAX_KEYS, 32), rnd(n, 32)
pk_all = ed.ed25519_genpub_batch(sk_all)


def items(nkeys):
    """the batch with its keys drawn from the first nkeys: item i under key (i * 2654435761) mod nkeys"""
    who = (torch.arange(n, device="cuda", dtype=torch.int64) * 2654435761) % nkeys
    sk, pk = sk_all[who].contiguous(), pk_all[who].contiguous()
    sig = ed.ed25519_sign_batch(sk, pk, msg, msg_len=32)
    return sig, pk, who.to(torch.int32).contiguous()


if ONLY_UNCHANGED:
    sig, pk, idx = items(1024)
    with ed.keyset_create(pk_all[:1024].contiguous()) as ks:
        forms = {"u": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32), "k": lambda: ed.ed25519_verify_keyed(sig, ks, idx, msg, msg_len=32)}
        assert bool(forms["u"]().all()) and bool(forms["k"]().all())
        r = alternate(forms, 3)
    print("UNKEYED", " ".join(f"{x:.4f}" for x in r["u"]))
    print("KEYED", " ".join(f"{x:.4f}" for x in r["k"]))
    sys.exit(0)


def three(sig, pk, idx, m_, plain, comb):
    return {"unkeyed": lambda: ed.ed25519_verify_batch(sig, pk, m_, msg_len=32),
            "plain": lambda: ed.ed25519_verify_keyed(sig, plain, idx, m_, msg_len=32),
            "comb": lambda: ed.ed25519_verify_keyed(sig, comb, idx, m_, msg_len=32)}


print(f"verify, 2^{LOG_N} valid items in HBM, 32-byte messages, device-pointer forms, the three alternating ({REPEATS} repeats):")
for nkeys in (1, 1024, MAX_KEYS):
    sig, pk, idx = items(nkeys)
    plain, comb = ed.keyset_create(pk_all[:nkeys].contiguous()), ed.keyset_create(pk_all[:nkeys].contiguous(), comb=True)
    forms = three(sig, pk, idx, msg, plain, comb)
    print(f" {nkeys} distinct keys (plain key set: {plain.nbytes / 2**20:.2f} MiB, comb key set: {comb.nbytes / 2**20:.2f} MiB):")
    for label, kw in (("mode 1 (default)", dict(mode=1)), ("mode 0 (reject)", dict(mode=0)), ("cofactored equation", dict(mode=1, cofactored=True))):
        ed.set_offcurve_mode(kw["mode"])
        ed.set_verify_equation(kw.get("cofactored", False))
        try:
            assert all(bool(fn().all()) for fn in forms.values())
            if nkeys > 1:
                assert not bool(ed.ed25519_verify_keyed(sig[:4096], comb, ((idx[:4096] + 1) % nkeys).contiguous(), msg[:4096], msg_len=32).any())
            r = alternate(forms)
            print(f"  {label}:")
            u = show("ed25519_verify_batch_dev", n, r["unkeyed"])
            p = show("ed25519_verify_keyed_dev, plain key set", n, r["plain"], u, "the unkeyed pass")
            show("ed25519_verify_keyed_dev, comb key set", n, r["comb"], p)
            if nkeys == 1024 and label.startswith("mode 1"):
                print("  per kernel (ms): prepare (+ tables, halve) / main / finish")
                for k, fn in forms.items():
                    ed.set_profiling(True)
                    for _ in range(10):
                        fn()
                    torch.cuda.synchronize()
                    ph = ed.verify_phase_ms()
                    ed.set_profiling(False)
                    print(f"    {k:8s} {ph[0]:.3f} / {ph[1]:.3f} / {ph[2]:.3f}")
        finally:
            ed.set_verify_equation(False)
            ed.set_offcurve_mode(1)
    plain.close()
    comb.close()
print()

print("small passes, valid items under 1024 keys, device-pointer forms:")
sig, pk, idx = items(1024)
with ed.keyset_create(pk_all[:1024].contiguous()) as plain, ed.keyset_create(pk_all[:1024].contiguous(), comb=True) as comb:
    for m in (1 << 7, 1 << 10, 1 << 14, 1 << 16):
        if m > n:
            break
        s_, p_, i_, m_ = (t[:m].contiguous() for t in (sig, pk, idx, msg))
        forms = three(s_, p_, i_, m_, plain, comb)
        assert all(bool(fn().all()) for fn in forms.values())
        r = alternate(forms)
        u = show(f"{m:7d} items  unkeyed", m, r["unkeyed"])
        p = show(f"{m:7d} items  plain key set", m, r["plain"], u, "the unkeyed pass")
        show(f"{m:7d} items  comb key set", m, r["comb"], p)
        show(f"{m:7d} items  comb key set (again)", m, r["comb"], u, "the unkeyed pass")
print()

print("eddsa_amd_keyset_create_comb from host keys (upload, tables, combs, synchronisation):")
hall = pk_all.cpu().numpy()
for nkeys in (1024, MAX_KEYS):
    for comb_flag in (False, True):
        t = []
        for _ in range(REPEATS):
            t0 = time.perf_counter(); ks = ed.keyset_create(hall[:nkeys], comb=comb_flag); t.append(1e3 * (time.perf_counter() - t0))
            nbytes = ks.nbytes
            ks.close()
        t.sort()
        print(f"  {nkeys:8d} keys  {'comb ' if comb_flag else 'plain'}  {t[len(t) // 2]:9.3f} ms  [{t[0]:.3f} .. {t[-1]:.3f}]  {nbytes} bytes ({nbytes / 2**20:.2f} MiB)")
print()

if PARENT:
    print(f"the unchanged calls, this build against {os.path.relpath(PARENT, ROOT)}, fresh processes alternating (2^{LOG_N} items under 1024 keys):")
    mine = os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd_debug.so")
    rows = {(b, f): [] for b in ("parent", "this") for f in ("UNKEYED", "KEYED")}
    for _ in range(REPEATS):
        for label, lib in (("parent", PARENT), ("this", mine)):
            o = subprocess.check_output([sys.executable, os.path.abspath(__file__), "3", str(LOG_N), "--only-unchanged"],
                                        env=dict(os.environ, EDDSA_AMD_LIBRARY=lib), text=True, timeout=300)
            for f in ("UNKEYED", "KEYED"):
                rows[(label, f)] += [float(x) for x in [l for l in o.splitlines() if l.startswith(f)][0].split()[1:]]
    for f, name in (("UNKEYED", "ed25519_verify_batch_dev"), ("KEYED", "ed25519_verify_keyed_dev, plain key set")):
        show(f"{name}: parent build", n, sorted(rows[("parent", f)]))
        show(f"{name}: this build", n, sorted(rows[("this", f)]))
