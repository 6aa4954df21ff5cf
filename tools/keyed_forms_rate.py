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
import sys

import numpy as np
import torch

import rate_kit
from rate_kit import alternate, show

REPEATS, LOG_N, PARENT, FLAGS = rate_kit.cli(sys.argv[1:])
NKEYS = 1024
ed = rate_kit.bind()                               # the product's objects (a --parent library is bound as given)
ed.set_rlc_min_items(0)


def accepts(forms):
    for k, fn in forms.items():
        assert bool(fn().all()), k


n = 1 << LOG_N
rnd = rate_kit.rnd(217)
sk_all, msg = rnd(NKEYS, 32), rnd(n, 32)
pk_all = ed.ed25519_genpub_batch(sk_all)
sig, pk, idx = rate_kit.keyed_items(n, NKEYS, sk_all, pk_all, msg)
sk = sk_all[idx.long()].contiguous()
plain, comb = ed.keyset_create(pk_all), ed.keyset_create(pk_all, comb=True)

if rate_kit.CHILD_FLAG in FLAGS:                    # (the child processes of row 4)
    forms = {"UNKEYED": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32),
             "PLAIN": lambda: ed.ed25519_verify_keyed(sig, plain, idx, msg, msg_len=32),
             "COMB": lambda: ed.ed25519_verify_keyed(sig, comb, idx, msg, msg_len=32),
             "KRLC": lambda: ed.ed25519_verify_keyed_rlc(sig, plain, idx, msg, msg_len=32)}
    accepts(forms)
    rate_kit.emit(alternate(forms, 3))
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
r = alternate(forms, REPEATS)
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
r = alternate(forms, REPEATS)
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
    r = alternate(forms, REPEATS)
    m = show("ed25519_verify_keyed_dev on the messages", m3, r["msg"])
    show("ed25519_verify_keyed_digests_dev on their digests", m3, r["dig"], m, "the message form")
    show("ed25519ph_verify_keyed_dev on their prehashes", m3, r["ph"], m, "the message form")
    print()

if PARENT:
    print(f"row 4: the unchanged calls, this build against {os.path.relpath(PARENT, rate_kit.ROOT)}, fresh processes alternating (2^{LOG_N} items under {NKEYS} keys):")
    names = (("UNKEYED", "ed25519_verify_batch_dev"), ("PLAIN", "ed25519_verify_keyed_dev, plain key set"),
             ("COMB", "ed25519_verify_keyed_dev, comb key set"), ("KRLC", "ed25519_verify_keyed_rlc_dev"))
    plain.close(); comb.close()
    rows = rate_kit.parent_ab(__file__, LOG_N, REPEATS, rate_kit.CHILD_FLAG, [f for f, _ in names], PARENT, rate_kit.DEBUG_LIBRARY)
    for f, name in names:
        p = show(f"{name}: parent build", n, rows[("parent", f)])
        t = rows[("this", f)]
        show(f"{name}: this build", n, t, p, "the parent build")
        lo, hi = rows[("parent", f)][0], rows[("parent", f)][-1]
        print(f"    this build's median is {'inside' if lo <= t[len(t) // 2] <= hi else 'OUTSIDE'} the parent build's own repeats [{lo:.3f} .. {hi:.3f}]")
