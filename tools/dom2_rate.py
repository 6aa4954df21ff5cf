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
import sys

import numpy as np
import torch

import rate_kit
from rate_kit import alternate

REPEATS, LOG_N, _, _ = rate_kit.cli(sys.argv[1:])
CONTEXT = b"foo"
TAG = b"SigEd25519 no Ed25519 collisions"
ed = rate_kit.bind(debug=False)


def show(label, n, ms, base=None):
    return rate_kit.show(label, n, ms, base, "the plain form")


def spot_check(sig, pk, mprime, flag, count=512):
    """the first `count` signatures of a ctx / ph batch: accepted by ed25519_verify_digests on hashlib's prefixed digest"""
    sig, pk, mprime = (t[:count].cpu().numpy() for t in (sig, pk, mprime))
    dom = TAG + bytes([flag, len(CONTEXT)]) + CONTEXT
    dig = np.stack([np.frombuffer(hashlib.sha512(dom + sig[i, :32].tobytes() + pk[i].tobytes() + mprime[i].tobytes()).digest(), np.uint8)
                    for i in range(len(sig))])
    assert bool(ed.ed25519_verify_digests(sig, pk, dig).all())


n = 1 << LOG_N
rnd = rate_kit.rnd(8032)
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
    r = alternate(forms, REPEATS)
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
blob = rnd(int(off[-1]))
doff = torch.from_numpy(off).cuda()
forms = {"ed25519_sign_batch, messages": lambda: ed.ed25519_sign_batch(sk, pk, blob, msg_off=doff),
         "ed25519ph_sign_batch, prehashes": lambda: ed.ed25519ph_sign_batch(sk, pk, pre, CONTEXT)}
print(f"sign, 2^16 items of 32 bytes, one message in 1024 of 1 MiB ({int(off[-1]) >> 20} MiB in all); the ph form signs 64-byte prehashes,"
      " the caller's hashing EXCLUDED:")
r = alternate(forms, REPEATS)
a = show("ed25519_sign_batch_dev, messages", n, r["ed25519_sign_batch, messages"])
b = show("ed25519ph_sign_batch_dev, prehashes", n, r["ed25519ph_sign_batch, prehashes"])
print(f"  the ph form takes {100 * b / a:.2f} % of the message form's time ({a / b:.0f} times the rate)")
