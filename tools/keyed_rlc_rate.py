#!/usr/bin/env python3
"""Batch verification over a key set against its two parents, the SAME items through the three device-pointer calls alternating
(ed25519_verify_keyed_rlc_dev, ed25519_verify_batch_rlc_dev, ed25519_verify_keyed_dev), device-resident inputs, device events, in
the style of tools/keyed_rate.py:

  row 1   2^20 valid items over 32-byte messages under 1, 1024 and 8192 keys
  row 2   2^14 .. 2^18 items under 1024 keys, the threshold at 0 (every call is combined): where the keyed combination crosses
          the keyed per-item pass
  row 3   (with --parent LIB) ed25519_verify_batch_rlc_dev and ed25519_verify_keyed_dev of this build against another build of
          the library, alternating in fresh processes: whether the two existing passes moved

Every repeat is `iters` calls between two events; the spread of a form is max - min over its repeats.  Before anything is timed
every form accepts every item, the combination decides all of them, and the keyed forms reject items whose index is shifted by one.

  tools/keyed_rlc_rate.py [repeats=5] [log2 of the batch=20] [--parent path/to/libeddsa_amd_debug.so]
  tools/keyed_rlc_rate.py --trace keyed_rlc|rlc|keyed NKEYS    ten passes of one form, for a kernel trace (the per-kernel split)
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libeddsa_amd as ed  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
PARENT = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
TRACE = sys.argv[sys.argv.index("--trace") + 1:][:2] if "--trace" in sys.argv else None
for a in ([PARENT] if PARENT else []) + (TRACE or []):
    args.remove(a)
ONLY_EXISTING = "--only-existing" in sys.argv      # (the child processes of row 3)
REPEATS = int(args[0]) if len(args) > 0 else 5
LOG_N = int(args[1]) if len(args) > 1 else 20
assert REPEATS >= 3
if not os.environ.get("EDDSA_AMD_LIBRARY"):
    ed.use_debug_library()
import torch  # noqa: E402

ed.init(0)
ed.set_rlc_min_items(0)


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


def show(label, n, ms, base=None, against=""):
    med = ms[len(ms) // 2]
    rel = "" if base is None else f"  {100 * (med - base) / base:+6.2f} % against {against}"
    print(f"  {label:44s} {med:9.3f} ms  [{ms[0]:.3f} .. {ms[-1]:.3f}]  spread {ms[-1] - ms[0]:.3f} ms  {n / med / 1e3:8.2f} M/s{rel}", flush=True)
    return med


n = 1 << LOG_N
g = torch.Generator(device="cuda").manual_seed(216)
rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)   # noqa: E731
sk_all, msg = rnd(8192, 32), rnd(n, 32)
pk_all = ed.ed25519_genpub_batch(sk_all)


def items(nkeys):
    """the batch with its keys drawn from the first nkeys: item i under key (i * 2654435761) mod nkeys"""
    who = (torch.arange(n, device="cuda", dtype=torch.int64) * 2654435761) % nkeys
    sk, pk = sk_all[who].contiguous(), pk_all[who].contiguous()
    sig = ed.ed25519_sign_batch(sk, pk, msg, msg_len=32)
    return sig, pk, who.to(torch.int32).contiguous()


def forms_of(ks, sig, pk, idx, m, keyed_rlc=True):
    f = {}
    if keyed_rlc:
        f["keyed_rlc"] = lambda: ed.ed25519_verify_keyed_rlc(sig, ks, idx, m, msg_len=32)
    f["rlc"] = lambda: ed.ed25519_verify_batch_rlc(sig, pk, m, msg_len=32)
    f["keyed"] = lambda: ed.ed25519_verify_keyed(sig, ks, idx, m, msg_len=32)
    return f


NAMES = {"keyed_rlc": "ed25519_verify_keyed_rlc_dev", "rlc": "ed25519_verify_batch_rlc_dev", "keyed": "ed25519_verify_keyed_dev"}

if TRACE:
    nkeys = int(TRACE[1])
    sig, pk, idx = items(nkeys)
    with ed.keyset_create(pk_all[:nkeys].contiguous()) as ks:
        fn = forms_of(ks, sig, pk, idx, msg)[TRACE[0]]
        assert bool(fn().all())
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
    print("TRACED", TRACE[0], nkeys)
    sys.exit(0)

if ONLY_EXISTING:
    sig, pk, idx = items(1024)
    with ed.keyset_create(pk_all[:1024].contiguous()) as ks:
        f = forms_of(ks, sig, pk, idx, msg, keyed_rlc=False)
        assert bool(f["rlc"]().all()) and bool(f["keyed"]().all())
        r = alternate(f, 3)
    for k in ("rlc", "keyed"):
        print("EXISTING", k, " ".join(f"{x:.4f}" for x in r[k]))
    sys.exit(0)

print(f"2^{LOG_N} valid items in HBM, 32-byte messages, device-pointer forms, the three alternating ({REPEATS} repeats):")
for nkeys in (1, 1024, 8192):
    sig, pk, idx = items(nkeys)
    with ed.keyset_create(pk_all[:nkeys].contiguous()) as ks:
        f = forms_of(ks, sig, pk, idx, msg)
        assert all(bool(fn().all()) for fn in f.values())
        ok, st = ed.ed25519_verify_keyed_rlc(sig, ks, idx, msg, msg_len=32, return_stats=True)
        assert st == (n, 0, 0, (n + 8191) // 8192), st
        if nkeys > 1:
            assert not bool(ed.ed25519_verify_keyed_rlc(sig[:8192], ks, ((idx[:8192] + 1) % nkeys).contiguous(), msg[:8192], msg_len=32).any())
        r = alternate(f)
        print(f" {nkeys} keys:")
        base = show(NAMES["rlc"], n, r["rlc"])
        show(NAMES["keyed"], n, r["keyed"], base, "the unkeyed combination")
        show(NAMES["keyed_rlc"], n, r["keyed_rlc"], base, "the unkeyed combination")
print()

print("smaller passes under 1024 keys, the threshold at 0 (every _rlc call is combined):")
sig, pk, idx = items(1024)
with ed.keyset_create(pk_all[:1024].contiguous()) as ks:
    for lg in range(14, 19):
        m = 1 << lg
        if m > n:
            break
        s_, p_, i_, m_ = (t[:m].contiguous() for t in (sig, pk, idx, msg))
        r = alternate(forms_of(ks, s_, p_, i_, m_))
        base = show(f"2^{lg} items  {NAMES['keyed']}", m, r["keyed"])
        show(f"2^{lg} items  {NAMES['rlc']}", m, r["rlc"], base, "the keyed per-item pass")
        show(f"2^{lg} items  {NAMES['keyed_rlc']}", m, r["keyed_rlc"], base, "the keyed per-item pass")
print()

if PARENT:
    print(f"the two existing passes, this build against {os.path.relpath(PARENT, ROOT)}, fresh processes alternating (1024 keys' items):")
    mine = os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd_debug.so")
    rows = {}
    for _ in range(REPEATS):
        for label, lib in (("parent", PARENT), ("this", mine)):
            o = subprocess.check_output([sys.executable, os.path.abspath(__file__), "3", str(LOG_N), "--only-existing"],
                                        env=dict(os.environ, EDDSA_AMD_LIBRARY=lib), text=True, timeout=300)
            for line in o.splitlines():
                if line.startswith("EXISTING"):
                    _, k, *vals = line.split()
                    rows.setdefault((k, label), []).extend(float(x) for x in vals)
    for k in ("rlc", "keyed"):
        for label in ("parent", "this"):
            show(f"{NAMES[k]}, {label} build", n, sorted(rows[(k, label)]))
