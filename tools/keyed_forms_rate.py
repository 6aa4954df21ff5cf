#!/usr/bin/env python3
"""The digest, Ed25519ctx and Ed25519ph forms of key-set verification against their message and unkeyed counterparts,
device-resident inputs, device events, after tools/keyed_rate.py and tools/keyed_comb_rate.py:

  row 1   2^20 valid items under 1024 keys: ed25519_verify_keyed_dev over 32-byte messages against
          ed25519_verify_keyed_digests_dev over their digests, over a plain and over a comb key set, and
          ed25519_verify_keyed_rlc_dev against ed25519_verify_keyed_digests_rlc_dev - all alternating in one process
  row 2   the same items signed as Ed25519ctx and Ed25519ph: the keyed forms over a plain and a comb set against the keyed message
          form and against the unkeyed ctx / ph forms
  row 3   2^16 items of which one in 1024 is 1 MiB long, under 1024 keys, over a comb set: ed25519_verify_keyed_dev on the messages,
          ed25519_verify_keyed_digests_dev on their digests, ed25519ph_verify_keyed_dev on their prehashes.  The digests and
          prehashes are computed before the clock starts: the CALLER's hashing is not part of any figure
  row 4   (with --parent LIB) the unchanged calls of this build against another build of the library, alternating in fresh
          processes: ed25519_verify_keyed_dev over a plain and a comb set, ed25519_verify_keyed_rlc_dev, ed25519_verify_batch_dev

Every repeat is `iters` calls between two events; the spread of a form is max - min over its repeats.  Before anything is timed
every form accepts every item.

  tools/keyed_forms_rate.py [repeats=5] [log2 of the batch=20] [--parent path/to/libeddsa_amd_debug.so]
"""
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libeddsa_amd as ed  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
PARENT = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
if PARENT:
    args.remove(PARENT)
ONLY_UNCHANGED = "--only-unchanged" in sys.argv    # (the child processes of row 4)
REPEATS = int(args[0]) if len(args) > 0 else 5
LOG_N = int(args[1]) if len(args) > 1 else 20
NKEYS = 1024
assert REPEATS >= 3
if not os.environ.get("EDDSA_AMD_LIBRARY"):
    ed.use_debug_library()                         # the product's objects (a --parent library is bound as given)
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
    print(f"  {label:58s} {med:9.3f} ms  [{ms[0]:.3f} .. {ms[-1]:.3f}]  spread {ms[-1] - ms[0]:.3f} ms  {n / med / 1e3:8.2f} M/s{rel}", flush=True)
    return med


def accepts(forms):
    for k, fn in forms.items():
        assert bool(fn().all()), k


n = 1 << LOG_N
g = torch.Generator(device="cuda").manual_seed(217)
rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)   # noqa: E731
sk_all, msg = rnd(NKEYS, 32), rnd(n, 32)
pk_all = ed.ed25519_genpub_batch(sk_all)
who = (torch.arange(n, device="cuda", dtype=torch.int64) * 2654435761) % NKEYS
sk, pk, idx = sk_all[who].contiguous(), pk_all[who].contiguous(), who.to(torch.int32).contiguous()
sig = ed.ed25519_sign_batch(sk, pk, msg, msg_len=32)
plain, comb = ed.keyset_create(pk_all), ed.keyset_create(pk_all, comb=True)

if ONLY_UNCHANGED:
    forms = {"UNKEYED": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32),
             "PLAIN": lambda: ed.ed25519_verify_keyed(sig, plain, idx, msg, msg_len=32),
             "COMB": lambda: ed.ed25519_verify_keyed(sig, comb, idx, msg, msg_len=32),
             "KRLC": lambda: ed.ed25519_verify_keyed_rlc(sig, plain, idx, msg, msg_len=32)}
    accepts(forms)
    for k, v in alternate(forms, 3).items():
        print(k, " ".join(f"{x:.4f}" for x in v))
    sys.exit(0)


def sha512_rows(*parts):
    """SHA-512 over the concatenation of the parts' rows, on the host (hashlib): the caller's work, never timed"""
    host = [p.cpu().numpy() for p in parts]
    out = np.empty((len(host[0]), 64), np.uint8)
    for i in range(len(out)):
        out[i] = np.frombuffer(hashlib.sha512(b"".join(h[i].tobytes() for h in host)).digest(), np.uint8)
    return torch.from_numpy(out).cuda()


print(f"row 1: message against digest, 2^{LOG_N} valid items in HBM under {NKEYS} keys, device-pointer forms, all alternating ({REPEATS} repeats):")
dig = sha512_rows(sig[:, :32], pk, msg)
forms = {"msg_plain": lambda: ed.ed25519_verify_keyed(sig, plain, idx, msg, msg_len=32),
         "dig_plain": lambda: ed.ed25519_verify_keyed_digests(sig, plain, idx, dig),
         "msg_comb": lambda: ed.ed25519_verify_keyed(sig, comb, idx, msg, msg_len=32),
         "dig_comb": lambda: ed.ed25519_verify_keyed_digests(sig, comb, idx, dig),
         "msg_rlc": lambda: ed.ed25519_verify_keyed_rlc(sig, plain, idx, msg, msg_len=32),
         "dig_rlc": lambda: ed.ed25519_verify_keyed_digests_rlc(sig, plain, idx, dig)}
accepts(forms)
assert not bool(ed.ed25519_verify_keyed_digests(sig[:4096], comb, ((idx[:4096] + 1) % NKEYS).contiguous(), dig[:4096]).any())
r = alternate(forms)
for kind, name in (("plain", "plain key set"), ("comb", "comb key set"), ("rlc", "the combination")):
    call = "ed25519_verify_keyed_rlc_dev" if kind == "rlc" else "ed25519_verify_keyed_dev"
    m = show(f"{call}, 32-byte messages, {name}", n, r["msg_" + kind])
    show(f"{call.replace('keyed', 'keyed_digests')}, {name}", n, r["dig_" + kind], m, "its message form")
    spread = r["msg_" + kind][-1] - r["msg_" + kind][0]
    d = r["dig_" + kind][len(r["dig_" + kind]) // 2] - m
    print(f"    the digest form is {'NOT ' if d > spread else ''}within the message form's repeat spread of it or faster ({d:+.3f} ms, spread {spread:.3f} ms)")
msg_plain, msg_comb = r["msg_plain"][REPEATS // 2], r["msg_comb"][REPEATS // 2]
print()

print(f"row 2: Ed25519ctx (a 3-byte context, 32-byte messages) and Ed25519ph (64-byte prehashes), the same keys and item order:")
context = b"ctx"
pre = rnd(n, 64)
sig_ctx = ed.ed25519ctx_sign_batch(sk, pk, msg, context, msg_len=32)
sig_ph = ed.ed25519ph_sign_batch(sk, pk, pre, context)
forms = {"plain": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32),
         "ctx": lambda: ed.ed25519ctx_verify_batch(sig_ctx, pk, msg, context, msg_len=32),
         "ph": lambda: ed.ed25519ph_verify_batch(sig_ph, pk, pre, context),
         "kmsg_plain": lambda: ed.ed25519_verify_keyed(sig, plain, idx, msg, msg_len=32),
         "kctx_plain": lambda: ed.ed25519ctx_verify_keyed(sig_ctx, plain, idx, msg, context, msg_len=32),
         "kph_plain": lambda: ed.ed25519ph_verify_keyed(sig_ph, plain, idx, pre, context),
         "kmsg_comb": lambda: ed.ed25519_verify_keyed(sig, comb, idx, msg, msg_len=32),
         "kctx_comb": lambda: ed.ed25519ctx_verify_keyed(sig_ctx, comb, idx, msg, context, msg_len=32),
         "kph_comb": lambda: ed.ed25519ph_verify_keyed(sig_ph, comb, idx, pre, context)}
accepts(forms)
r = alternate(forms)
u = show("ed25519_verify_batch_dev", n, r["plain"])
uc = show("ed25519ctx_verify_batch_dev", n, r["ctx"], u, "plain Ed25519")
up = show("ed25519ph_verify_batch_dev", n, r["ph"], u, "plain Ed25519")
for kind in ("plain", "comb"):
    km_ = show(f"ed25519_verify_keyed_dev, {kind} key set", n, r["kmsg_" + kind])
    show(f"ed25519ctx_verify_keyed_dev, {kind} key set", n, r["kctx_" + kind], km_, "the keyed message form")
    show(f"  (the same against the unkeyed ctx form)", n, r["kctx_" + kind], uc, "ed25519ctx_verify_batch_dev")
    show(f"ed25519ph_verify_keyed_dev, {kind} key set", n, r["kph_" + kind], km_, "the keyed message form")
    show(f"  (the same against the unkeyed ph form)", n, r["kph_" + kind], up, "ed25519ph_verify_batch_dev")
print()

m3, long_every, long_len = 1 << 16, 1024, 1 << 20
if m3 <= n:
    print(f"row 3: {m3} items under {NKEYS} keys over a comb key set, one message in {long_every} of {long_len} bytes, the others of 32;")
    print("       the digests and prehashes are the caller's and were computed before the clock started: its hashing is in no figure")
    lens = torch.full((m3,), 32, dtype=torch.int64)
    lens[long_every // 2::long_every] = long_len
    off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    blob = rnd(int(off[-1]))
    s3, p3, i3 = sk[:m3].contiguous(), pk[:m3].contiguous(), idx[:m3].contiguous()
    d_off = off.cuda()
    sig3 = ed.ed25519_sign_batch(s3, p3, blob, msg_off=d_off)
    hblob, hoff, hsig, hpk = blob.cpu().numpy(), off.numpy(), sig3.cpu().numpy(), p3.cpu().numpy()
    dig3 = np.empty((m3, 64), np.uint8)
    pre3 = np.empty((m3, 64), np.uint8)
    for i in range(m3):
        m_ = hblob[hoff[i]:hoff[i + 1]].tobytes()
        dig3[i] = np.frombuffer(hashlib.sha512(hsig[i, :32].tobytes() + hpk[i].tobytes() + m_).digest(), np.uint8)
        pre3[i] = np.frombuffer(hashlib.sha512(m_).digest(), np.uint8)
    dig3, pre3 = torch.from_numpy(dig3).cuda(), torch.from_numpy(pre3).cuda()
    sig3ph = ed.ed25519ph_sign_batch(s3, p3, pre3, context)
    forms = {"msg": lambda: ed.ed25519_verify_keyed(sig3, comb, i3, blob, msg_off=d_off),
             "dig": lambda: ed.ed25519_verify_keyed_digests(sig3, comb, i3, dig3),
             "ph": lambda: ed.ed25519ph_verify_keyed(sig3ph, comb, i3, pre3, context)}
    accepts(forms)
    r = alternate(forms)
    m = show("ed25519_verify_keyed_dev on the messages", m3, r["msg"])
    show("ed25519_verify_keyed_digests_dev on their digests", m3, r["dig"], m, "the message form")
    show("ed25519ph_verify_keyed_dev on their prehashes", m3, r["ph"], m, "the message form")
    print()

if PARENT:
    print(f"row 4: the unchanged calls, this build against {os.path.relpath(PARENT, ROOT)}, fresh processes alternating (2^{LOG_N} items under {NKEYS} keys):")
    mine = os.path.join(ROOT, "libeddsa_amd", "libeddsa_amd_debug.so")
    names = (("UNKEYED", "ed25519_verify_batch_dev"), ("PLAIN", "ed25519_verify_keyed_dev, plain key set"),
             ("COMB", "ed25519_verify_keyed_dev, comb key set"), ("KRLC", "ed25519_verify_keyed_rlc_dev"))
    rows = {(b, f): [] for b in ("parent", "this") for f, _ in names}
    plain.close(); comb.close()
    for _ in range(REPEATS):
        for label, lib in (("parent", PARENT), ("this", mine)):
            o = subprocess.check_output([sys.executable, os.path.abspath(__file__), "3", str(LOG_N), "--only-unchanged"],
                                        env=dict(os.environ, EDDSA_AMD_LIBRARY=lib), text=True, timeout=300)
            for f, _ in names:
                rows[(label, f)] += [float(x) for x in [l for l in o.splitlines() if l.startswith(f)][0].split()[1:]]
    for f, name in names:
        p = show(f"{name}: parent build", n, sorted(rows[("parent", f)]))
        t = sorted(rows[("this", f)])
        show(f"{name}: this build", n, t, p, "the parent build")
        lo, hi = min(rows[("parent", f)]), max(rows[("parent", f)])
        print(f"    this build's median is {'inside' if lo <= t[len(t) // 2] <= hi else 'OUTSIDE'} the parent build's own repeats [{lo:.3f} .. {hi:.3f}]")
