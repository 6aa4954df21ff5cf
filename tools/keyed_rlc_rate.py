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
import sys

import torch

import rate_kit
from rate_kit import alternate, show

ARGV = sys.argv[1:]
TRACE = None
if "--trace" in ARGV:
    at = ARGV.index("--trace")
    TRACE = ARGV[at + 1:at + 3]
    del ARGV[at:at + 3]
REPEATS, LOG_N, PARENT, FLAGS = rate_kit.cli(ARGV)
ed = rate_kit.bind()
ed.set_rlc_min_items(0)

n = 1 << LOG_N
rnd = rate_kit.rnd(216)
sk_all, msg = rnd(8192, 32), rnd(n, 32)
pk_all = ed.ed25519_genpub_batch(sk_all)


def items(nkeys):
    return rate_kit.keyed_items(n, nkeys, sk_all, pk_all, msg)


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

if rate_kit.CHILD_FLAG in FLAGS:                    # (the child processes of row 3)
    sig, pk, idx = items(1024)
    with ed.keyset_create(pk_all[:1024].contiguous()) as ks:
        f = forms_of(ks, sig, pk, idx, msg, keyed_rlc=False)
        assert bool(f["rlc"]().all()) and bool(f["keyed"]().all())
        rate_kit.emit(alternate(f, 3))
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
        r = alternate(f, REPEATS)
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
        r = alternate(forms_of(ks, s_, p_, i_, m_), REPEATS)
        base = show(f"2^{lg} items  {NAMES['keyed']}", m, r["keyed"])
        show(f"2^{lg} items  {NAMES['rlc']}", m, r["rlc"], base, "the keyed per-item pass")
        show(f"2^{lg} items  {NAMES['keyed_rlc']}", m, r["keyed_rlc"], base, "the keyed per-item pass")
print()

if PARENT:
    print(f"the two existing passes, this build against {os.path.relpath(PARENT, rate_kit.ROOT)}, fresh processes alternating (1024 keys' items):")
    rows = rate_kit.parent_ab(__file__, LOG_N, REPEATS, rate_kit.CHILD_FLAG, ("rlc", "keyed"), PARENT, rate_kit.DEBUG_LIBRARY)
    for k in ("rlc", "keyed"):
        for build in ("parent", "this"):
            show(f"{NAMES[k]}, {build} build", n, rows[(build, k)])
