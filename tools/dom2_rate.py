#!/usr/bin/env python3
"""Ed25519ctx and Ed25519ph against Ed25519 (ed25519ctx_* / ed25519ph_* against ed25519_verify_batch / ed25519_sign_batch),
device-resident inputs, device events, in the style of tools/digest_rate.py:

  row 1   verify, 2^20 valid items: the plain form over 32-byte messages, the ctx form over the same messages, the ph form over
          64-byte prehashes; a 3-byte context
  row 2   sign, the same three forms
  row 3   sign, 2^16 items of 32 bytes with one message in 1024 of 1 MiB (the skewed row of tools/msglen_table.py):
          ed25519_sign_batch over the messages against ed25519ph_sign_batch over their prehashes.  THE CALLER'S HASHING IS NOT IN
          THE ph FIGURE: the prehashes are random 64-byte strings standing in for SHA-512(M), computed by nobody.

The forms alternate in one process; every repeat is `iters` calls between two events; the spread of a form is max - min over its
repeats.  Before anything is timed the ctx and ph signatures of 512 of the items are checked with hashlib against
ed25519_verify_digests, and every form's verify accepts its own signatures.

  tools/dom2_rate.py [repeats=5] [log2 of the large batches=20]
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libeddsa_amd as ed  # noqa: E402

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
LOG_N = int(sys.argv[2]) if len(sys.argv) > 2 else 20
assert REPEATS >= 3
CONTEXT = b"foo"
TAG = b"SigEd25519 no Ed25519 collisions"
ed.init(0)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()                                            # untimed: the repeat starts from this form's own state, not from its neighbour's
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(forms):
    """forms: {label: callable} -> {label: sorted per-call ms of REPEATS repeats}, the forms taking turns"""
    iters = {}
    for k, fn in forms.items():                     # warm-up; sizes a repeat to about 0.1 s
        fn(); torch.cuda.synchronize()
        iters[k] = max(2, min(50, int(100.0 / max(timed(fn, 2), 1e-3))))
    out = {k: [] for k in forms}
    for _ in range(REPEATS):
        for k, fn in forms.items():
            out[k].append(timed(fn, iters[k]))
    return {k: sorted(v) for k, v in out.items()}


def show(label, n, ms, base=None):
    med = ms[len(ms) // 2]
    rel = "" if base is None else f"  {100 * (med - base) / base:+6.2f} % against the plain form"
    print(f"  {label:44s} {med:9.3f} ms  [{ms[0]:.3f} .. {ms[-1]:.3f}]  spread {ms[-1] - ms[0]:.3f} ms  {n / med / 1e3:8.2f} M/s{rel}", flush=True)
    return med


def spot_check(sig, pk, mprime, flag, count=512):
    """the first `count` signatures of a ctx / ph batch: accepted by ed25519_verify_digests on hashlib's prefixed digest"""
    sig, pk, mprime = (t[:count].cpu().numpy() for t in (sig, pk, mprime))
    dom = TAG + bytes([flag, len(CONTEXT)]) + CONTEXT
    dig = np.stack([np.frombuffer(hashlib.sha512(dom + sig[i, :32].tobytes() + pk[i].tobytes() + mprime[i].tobytes()).digest(), np.uint8)
                    for i in range(len(sig))])
    assert bool(ed.ed25519_verify_digests(sig, pk, dig).all())


n = 1 << LOG_N
g = torch.Generator(device="cuda").manual_seed(8032)
rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)   # noqa: E731
sk, msg, pre = rnd(n, 32), rnd(n, 32), rnd(n, 64)
pk = ed.ed25519_genpub_batch(sk)
sign = {"ed25519_sign_batch": lambda: ed.ed25519_sign_batch(sk, pk, msg, msg_len=32),
        "ed25519ctx_sign_batch": lambda: ed.ed25519ctx_sign_batch(sk, pk, msg, CONTEXT, msg_len=32),
        "ed25519ph_sign_batch": lambda: ed.ed25519ph_sign_batch(sk, pk, pre, CONTEXT)}
sigs = {k: fn() for k, fn in sign.items()}
spot_check(sigs["ed25519ctx_sign_batch"], pk, msg, 0)
spot_check(sigs["ed25519ph_sign_batch"], pk, pre, 1)
verify = {"ed25519_verify_batch": lambda: ed.ed25519_verify_batch(sigs["ed25519_sign_batch"], pk, msg, msg_len=32),
          "ed25519ctx_verify_batch": lambda: ed.ed25519ctx_verify_batch(sigs["ed25519ctx_sign_batch"], pk, msg, CONTEXT, msg_len=32),
          "ed25519ph_verify_batch": lambda: ed.ed25519ph_verify_batch(sigs["ed25519ph_sign_batch"], pk, pre, CONTEXT)}
for k, fn in verify.items():
    assert bool(fn().all()), k
assert not bool(ed.ed25519ctx_verify_batch(sigs["ed25519_sign_batch"][:4096], pk[:4096], msg[:4096], CONTEXT, msg_len=32).any())

for title, forms in ((f"verify, 2^{LOG_N} valid items, 32-byte messages / 64-byte prehashes, context {CONTEXT!r}:", verify),
                     (f"sign, 2^{LOG_N} items, the same:", sign)):
    print(title)
    r = alternate(forms)
    base = None
    for k, ms in r.items():
        med = show(k + "_dev", n, ms, base)
        base = med if base is None else base
    print()

# row 3: the skewed workload of tools/msglen_table.py
n = 1 << 16
sk, pre = sk[:n].contiguous(), pre[:n].contiguous()
pk = pk[:n].contiguous()
lens = np.full(n, 32, np.int64); lens[511::1024] = 1 << 20
off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum(lens)
blob = torch.randint(0, 256, (int(off[-1]),), dtype=torch.uint8, device="cuda", generator=g)
doff = torch.from_numpy(off).cuda()
forms = {"ed25519_sign_batch, messages": lambda: ed.ed25519_sign_batch(sk, pk, blob, msg_off=doff),
         "ed25519ph_sign_batch, prehashes": lambda: ed.ed25519ph_sign_batch(sk, pk, pre, CONTEXT)}
print(f"sign, 2^16 items of 32 bytes, one message in 1024 of 1 MiB ({int(off[-1]) >> 20} MiB in all); the ph form signs 64-byte prehashes,"
      " the caller's hashing EXCLUDED:")
r = alternate(forms)
a = show("ed25519_sign_batch_dev, messages", n, r["ed25519_sign_batch, messages"])
b = show("ed25519ph_sign_batch_dev, prehashes", n, r["ed25519ph_sign_batch, prehashes"])
print(f"  the ph form takes {100 * b / a:.2f} % of the message form's time ({a / b:.0f} times the rate)")
