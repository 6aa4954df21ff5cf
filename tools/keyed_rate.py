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
import sys
import time

import numpy as np
import torch  # noqa: F401  (loaded before the library, as in every script that uses it)

import rate_kit
from rate_kit import alternate, show

REPEATS, LOG_N, PARENT, FLAGS = rate_kit.cli(sys.argv[1:])
ed = rate_kit.bind()                               # the product's objects plus the phase timer (a --parent library is bound as given)
AGAINST = "the unkeyed pass"

n = 1 << LOG_N
rnd = rate_kit.rnd(215)
sk_all, msg = rnd(n, 32), rnd(n, 32)
pk_all = ed.ed25519_genpub_batch(sk_all)


def items(nkeys):
    return rate_kit.keyed_items(n, nkeys, sk_all, pk_all, msg)


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
            r = alternate(forms, REPEATS)
            base = show(f"{m:7d} items  ed25519_verify_batch_dev", m, r["unkeyed"])
            show(f"{m:7d} items  ed25519_verify_keyed_dev", m, r["keyed"], base, AGAINST)
    print()


if "--only-small" in FLAGS:
    small_passes()
    sys.exit(0)

if rate_kit.CHILD_FLAG in FLAGS:                    # (the child processes of row 6)
    sig, pk, _ = items(1024)
    assert bool(ed.ed25519_verify_batch(sig, pk, msg, msg_len=32).all())
    rate_kit.emit(alternate({"UNKEYED": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32)}, 3))
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
    r = alternate(forms, REPEATS)
    print(f" {nkeys} distinct keys (key set: {nkeys * (32 + 1 + 1152) / 1e6:.1f} MB):")
    base = show("ed25519_verify_batch_dev", n, r["unkeyed"])
    show("ed25519_verify_keyed_dev", n, r["keyed"], base, AGAINST)
    if nkeys == 1024:
        rate_kit.phase_split(forms)
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
    show("ed25519_verify_keyed", n, sorted(out["keyed"]), base, AGAINST)
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
    print(f"ed25519_verify_batch_dev, this build against {os.path.relpath(PARENT, rate_kit.ROOT)}, fresh processes alternating (1024 keys' items):")
    rows = rate_kit.parent_ab(__file__, LOG_N, REPEATS, rate_kit.CHILD_FLAG, ("UNKEYED",), PARENT, rate_kit.DEBUG_LIBRARY)
    show("parent build", n, rows[("parent", "UNKEYED")])
    show("this build", n, rows[("this", "UNKEYED")])
