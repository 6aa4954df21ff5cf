#!/usr/bin/env python3
"""What the opt-in strict rules (include/eddsa_amd.h: EDDSA_AMD_VERIFY_*; kernels.hip: k_verify_policy) cost a verify pass:
ed25519_verify_batch on 2^20 device-resident VALID items with 32-byte messages (every item is accepted, so the policy kernel
does its work on every lane), device events, under policy 0, each bit alone and all four.  The policies take turns in one
process; every repeat is `iters` calls between two events; the spread of a row is max - min over its repeats.

  tools/policy_cost.py [repeats=5] [log2 items=20] [baseline]

baseline: policy 0 only and no call of set_verify_policy - the row to compare between two builds of the library on one box
(tools/ab.sh with EDDSA_AMD_LIBRARY; a build from before the rules existed reads the bits as "exact").
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import libeddsa_amd as ed  # noqa: E402

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
LOG_N = int(sys.argv[2]) if len(sys.argv) > 2 else 20
BASELINE = len(sys.argv) > 3 and sys.argv[3] == "baseline"
assert REPEATS >= 3
ed.init(0)
n = 1 << LOG_N
g = torch.Generator(device="cuda").manual_seed(20261019)
dsk = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
dmsg = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
dpk = ed.ed25519_genpub_batch(dsk)
dsig = ed.ed25519_sign_batch(dsk, dpk, dmsg, msg_len=32)
verify = lambda: ed.ed25519_verify_batch(dsig, dpk, dmsg, msg_len=32)   # noqa: E731
assert bool(verify().all())

ROWS = [("policy 0", 0)]
if not BASELINE:
    ROWS += [("S_BELOW_L", ed.VERIFY_S_BELOW_L), ("A_CANONICAL", ed.VERIFY_A_CANONICAL), ("A_NOT_SMALL", ed.VERIFY_A_NOT_SMALL),
             ("R_NOT_SMALL", ed.VERIFY_R_NOT_SMALL), ("STRICT", ed.VERIFY_STRICT)]


def timed(policy, iters):
    if not BASELINE:
        ed.set_verify_policy(policy)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    verify()                                        # untimed: the repeat starts from this policy's own state
    a.record()
    for _ in range(iters):
        verify()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


try:
    iters = {}
    for label, policy in ROWS:                      # warm-up (honest signatures satisfy every rule); sizes a repeat to about 0.1 s
        if not BASELINE:
            ed.set_verify_policy(policy)
        assert bool(verify().all())
        iters[label] = max(2, min(50, int(100.0 / max(timed(policy, 2), 1e-3))))
    ms = {label: [] for label, _ in ROWS}
    for _ in range(REPEATS):
        for label, policy in ROWS:
            ms[label].append(timed(policy, iters[label]))
finally:
    if not BASELINE:
        ed.set_verify_policy(0)

print(f"{ed.library_path()}: 2^{LOG_N} valid items, msg_len 32, {REPEATS} repeats")
base = sorted(ms["policy 0"])[REPEATS // 2]
for label, _ in ROWS:
    v = sorted(ms[label])
    med = v[REPEATS // 2]
    print(f"  {label:12s} {med:8.3f} ms  [{v[0]:.3f} .. {v[-1]:.3f}]  spread {v[-1] - v[0]:.3f} ms ({100 * (v[-1] - v[0]) / med:.1f} %)"
          f"  {n / med / 1e3:7.2f} M/s  {100 * (med - base) / base:+6.2f} % against policy 0", flush=True)
