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
import sys
import time

import torch  # noqa: F401  (loaded before the library, as in every script that uses it)

import rate_kit
from rate_kit import alternate

REPEATS, LOG_N, PARENT, FLAGS = rate_kit.cli(sys.argv[1:])
ed = rate_kit.bind()                               # the product's objects plus the phase timer (a --parent library is bound as given)


def show(label, n, ms, base=None, against="the plain key set"):
    return rate_kit.show(label, n, ms, base, against)


n = 1 << LOG_N
rnd = rate_kit.rnd(216)
MAX_KEYS = min(ed.KEYSET_COMB_MAX_KEYS, n) if hasattr(ed, "KEYSET_COMB_MAX_KEYS") else 1024
sk_all, msg = rnd(MAX_KEYS, 32), rnd(n, 32)
pk_all = ed.ed25519_genpub_batch(sk_all)


def items(nkeys):
    return rate_kit.keyed_items(n, nkeys, sk_all, pk_all, msg)


if rate_kit.CHILD_FLAG in FLAGS:                    # (the child processes of row 5)
    sig, pk, idx = items(1024)
    with ed.keyset_create(pk_all[:1024].contiguous()) as ks:
        forms = {"UNKEYED": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32),
                 "KEYED": lambda: ed.ed25519_verify_keyed(sig, ks, idx, msg, msg_len=32)}
        assert all(bool(fn().all()) for fn in forms.values())
        rate_kit.emit(alternate(forms, 3))
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
            r = alternate(forms, REPEATS)
            print(f"  {label}:")
            u = show("ed25519_verify_batch_dev", n, r["unkeyed"])
            p = show("ed25519_verify_keyed_dev, plain key set", n, r["plain"], u, "the unkeyed pass")
            show("ed25519_verify_keyed_dev, comb key set", n, r["comb"], p)
            if nkeys == 1024 and label.startswith("mode 1"):
                rate_kit.phase_split(forms)
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
        r = alternate(forms, REPEATS)
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
    print(f"the unchanged calls, this build against {os.path.relpath(PARENT, rate_kit.ROOT)}, fresh processes alternating (2^{LOG_N} items under 1024 keys):")
    rows = rate_kit.parent_ab(__file__, LOG_N, REPEATS, rate_kit.CHILD_FLAG, ("UNKEYED", "KEYED"), PARENT, rate_kit.DEBUG_LIBRARY)
    for f, name in (("UNKEYED", "ed25519_verify_batch_dev"), ("KEYED", "ed25519_verify_keyed_dev, plain key set")):
        show(f"{name}: parent build", n, rows[("parent", f)])
        show(f"{name}: this build", n, rows[("this", f)])
