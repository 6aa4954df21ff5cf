#!/usr/bin/env python3
"""What point classification costs (ed25519_point_classify_batch_dev, include/eddsa_amd.h), device-resident inputs, device events, in
the style of tools/keyed_rate.py and tools/sign_keyed_rate.py:

  row 1   2^20 strings in HBM, the four forms alternating in one process:
            ed25519_point_classify_batch_dev over honest public keys (every lane walks the chain [l]P)
            ed25519_point_classify_batch_dev over random 32-byte strings (about half leave before the chain; their waves do not)
            pk_ed25519_to_x25519_batch_dev over the honest keys (one decoding and one inversion)
            ed25519_verify_batch_dev over valid signatures under those keys (132 doublings, about 84 additions and everything else)
  row 2   (with --parent LIB) ed25519_verify_batch_dev of this build against another build of the library, alternating in fresh
          processes: whether the unchanged pass moved

Before anything is timed the classes are checked: every honest key is canonical and in the prime-order subgroup, about half of the
random strings are no curve point, and about one in eight of the others is in the subgroup.

  tools/classify_rate.py [repeats=5] [log2 of the batch=20] [--parent path/to/libeddsa_amd_debug.so]
"""
import os
import sys

import torch

import rate_kit
from rate_kit import alternate, show

REPEATS, LOG_N, PARENT, FLAGS = rate_kit.cli(sys.argv[1:])
ed = rate_kit.bind()                               # the product's objects (a --parent library is bound as given)

n = 1 << LOG_N
rnd = rate_kit.rnd(25519)
sk, msg = rnd(n, 32), rnd(n, 32)
pk = ed.ed25519_genpub_batch(sk)
sig = ed.ed25519_sign_batch(sk, pk, msg, msg_len=32)
assert bool(ed.ed25519_verify_batch(sig, pk, msg, msg_len=32).all())

if rate_kit.CHILD_FLAG in FLAGS:                    # (the child processes of row 2)
    rate_kit.emit(alternate({"VERIFY": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32)}, 3))
    sys.exit(0)

garbage = rnd(n, 32)
fit = ed.POINT_ON_CURVE | ed.POINT_CANONICAL | ed.POINT_PRIME_SUBGROUP
assert bool((ed.point_classify_batch(pk) == fit).all())
cls = ed.point_classify_batch(garbage)
off = int((cls == 0).sum())
sub = int(((cls & ed.POINT_PRIME_SUBGROUP) != 0).sum())
assert 0.45 * n < off < 0.55 * n and 0.10 * (n - off) < sub < 0.15 * (n - off), (off, sub)

print(f"{torch.cuda.get_device_name(0)}; repeats {REPEATS}; every row: min .. max over the repeats, median in front")
print(f"random strings: {off} of {n} are no curve point, {sub} of the other {n - off} are in the prime-order subgroup\n")
print(f"row 1: 2^{LOG_N} items in HBM, the forms alternating:")
r = alternate({"honest": lambda: ed.point_classify_batch(pk),
               "garbage": lambda: ed.point_classify_batch(garbage),
               "pk_to_x": lambda: ed.pk_ed25519_to_x25519_batch(pk),
               "verify": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32)}, REPEATS)
base = show("ed25519_verify_batch_dev, valid signatures", n, r["verify"])
show("pk_ed25519_to_x25519_batch_dev, honest keys", n, r["pk_to_x"], base, "the verify pass")
show("ed25519_point_classify_batch_dev, honest keys", n, r["honest"], base, "the verify pass")
show("ed25519_point_classify_batch_dev, random strings", n, r["garbage"], base, "the verify pass")
print()

if PARENT:
    print(f"row 2: ed25519_verify_batch_dev, this build against {os.path.relpath(PARENT, rate_kit.ROOT)}, fresh processes alternating:")
    rows = rate_kit.parent_ab(__file__, LOG_N, REPEATS, rate_kit.CHILD_FLAG, ("VERIFY",), PARENT, rate_kit.DEBUG_LIBRARY)
    p = rows[("parent", "VERIFY")]
    show("parent build", n, p)
    med = show("this build", n, rows[("this", "VERIFY")], p[len(p) // 2], "the parent build")
    print(f"  -> this build's median is {'inside' if p[0] <= med <= p[-1] else 'OUTSIDE'} the parent build's own repeat spread [{p[0]:.3f} .. {p[-1]:.3f}] ms")
