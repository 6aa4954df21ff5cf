#!/usr/bin/env python3
"""What [m]P + [a]B costs (ed25519_point_muladd_batch_dev, include/eddsa_amd.h), device-resident inputs, device events, in the style
of tools/classify_rate.py:

  row 1   2^20 items in HBM, the four forms alternating in one process:
            ed25519_point_muladd_batch_dev with both scalar arrays (honest public keys, random 256-bit scalars)
            ... with mul alone ([h]A, blinding) and with add alone (A + [z]B, soft derivation)
            ed25519_verify_batch_dev in off-curve mode 0 over as many valid signatures: the same main kernel between a prepare kernel
            that also hashes and a finish kernel that also compares with R
  row 2   passes of 2^7, 2^10, 2^14 and 2^16 items: both scalar arrays beside that verify pass
  row 3   (with --parent LIB) ed25519_verify_batch_dev in the default mode, this build against another build of the library,
          alternating in fresh processes: whether the unchanged pass moved

Before anything is timed the outputs are checked against one another: with both arrays absent the call re-encodes the honest
keys, m = 1 and a = 0 spelled out give what the absent arrays give, and no honest key gives the no-point string.

  tools/point_muladd_rate.py [repeats=5] [log2 of the batch=20] [--parent path/to/libeddsa_amd_debug.so]
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

if rate_kit.CHILD_FLAG in FLAGS:                    # (the child processes of row 3)
    rate_kit.emit(alternate({"VERIFY": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32)}, 3))
    sys.exit(0)

m, a = rnd(n, 32), rnd(n, 32)
zero = torch.zeros_like(m)
assert torch.equal(ed.point_muladd_batch(pk), pk)                                   # honest keys are canonical
assert torch.equal(ed.point_muladd_batch(pk, None, zero), pk)
one = zero.clone(); one[:, 0] = 1
assert torch.equal(ed.point_muladd_batch(pk, one, a), ed.point_muladd_batch(pk, None, a))
both = ed.point_muladd_batch(pk, m, a)
assert not bool((both == torch.tensor(list(ed.NO_POINT), dtype=torch.uint8, device="cuda")).all(dim=1).any())

print(f"{torch.cuda.get_device_name(0)}; repeats {REPEATS}; every row: min .. max over the repeats, median in front\n")
ed.set_offcurve_mode(0)
try:
    print(f"row 1: 2^{LOG_N} items in HBM, the forms alternating (verify in off-curve mode 0: prepare, k_verify_main, finish):")
    r = alternate({"both": lambda: ed.point_muladd_batch(pk, m, a),
                   "mul": lambda: ed.point_muladd_batch(pk, m, None),
                   "add": lambda: ed.point_muladd_batch(pk, None, a),
                   "verify": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32)}, REPEATS)
    base = show("ed25519_verify_batch_dev, mode 0, valid signatures", n, r["verify"])
    show("ed25519_point_muladd_batch_dev, mul and add", n, r["both"], base, "that verify pass")
    show("ed25519_point_muladd_batch_dev, mul alone", n, r["mul"], base, "that verify pass")
    show("ed25519_point_muladd_batch_dev, add alone", n, r["add"], base, "that verify pass")
    print()
    print("row 2: small passes, mul and add beside the verify pass in mode 0:")
    for log_s in (7, 10, 14, 16):
        s = 1 << log_s
        if s > n:
            continue
        cut = [t[:s].contiguous() for t in (pk, m, a, sig, msg)]
        r = alternate({"both": lambda: ed.point_muladd_batch(cut[0], cut[1], cut[2]),
                       "verify": lambda: ed.ed25519_verify_batch(cut[3], cut[0], cut[4], msg_len=32)}, REPEATS)
        base = show(f"2^{log_s}: ed25519_verify_batch_dev, mode 0", s, r["verify"])
        show(f"2^{log_s}: ed25519_point_muladd_batch_dev", s, r["both"], base, "that verify pass")
    print()
finally:
    ed.set_offcurve_mode(1)

if PARENT:
    print(f"row 3: ed25519_verify_batch_dev, default mode, this build against {os.path.relpath(PARENT, rate_kit.ROOT)}, fresh processes alternating:")
    rows = rate_kit.parent_ab(__file__, LOG_N, REPEATS, rate_kit.CHILD_FLAG, ("VERIFY",), PARENT, rate_kit.DEBUG_LIBRARY)
    p = rows[("parent", "VERIFY")]
    show("parent build", n, p)
    med = show("this build", n, rows[("this", "VERIFY")], p[len(p) // 2], "the parent build")
    print(f"  -> this build's median is {'inside' if p[0] <= med <= p[-1] else 'OUTSIDE'} the parent build's own repeat spread [{p[0]:.3f} .. {p[-1]:.3f}] ms")
