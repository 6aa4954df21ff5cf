#!/usr/bin/env python3
"""What the opt-in strict rules (include/eddsa_amd.h: EDDSA_AMD_VERIFY_*; kernels.hip: k_verify_policy) cost a verify pass:
ed25519_verify_batch on 2^20 device-resident VALID items with 32-byte messages (every item is accepted, so the policy kernel
does its work on every lane), device events, under policy 0, each bit alone and all four.  The policies take turns in one
process; every repeat is `iters` calls between two events; the spread of a row is max - min over its repeats.

  tools/policy_cost.py [repeats=5] [log2 items=20] [baseline]

baseline: policy 0 only and no call of set_verify_policy - the row to compare between two builds of the library on one box
(tools/ab.sh with EDDSA_AMD_LIBRARY; a build from before the rules existed reads the bits as "exact").
"""
import sys

import torch  # noqa: F401  (loaded before the library, as in every script that uses it)

import rate_kit

REPEATS, LOG_N, _, FLAGS = rate_kit.cli(sys.argv[1:])
BASELINE = "baseline" in FLAGS
ed = rate_kit.bind(debug=False)
n = 1 << LOG_N
rnd = rate_kit.rnd(20261019)
dsk, dmsg = rnd(n, 32), rnd(n, 32)
dpk = ed.ed25519_genpub_batch(dsk)
dsig = ed.ed25519_sign_batch(dsk, dpk, dmsg, msg_len=32)
verify = lambda: ed.ed25519_verify_batch(dsig, dpk, dmsg, msg_len=32)   # noqa: E731
assert bool(verify().all())

ROWS = [("policy 0", 0)]
if not BASELINE:
    ROWS += [("S_BELOW_L", ed.VERIFY_S_BELOW_L), ("A_CANONICAL", ed.VERIFY_A_CANONICAL), ("A_NOT_SMALL", ed.VERIFY_A_NOT_SMALL),
             ("R_NOT_SMALL", ed.VERIFY_R_NOT_SMALL), ("STRICT", ed.VERIFY_STRICT)]


try:
    forms = {}
    for label, policy in ROWS:                      # honest signatures satisfy every rule; baseline never touches the switch
        switch = None if BASELINE else (lambda policy=policy: ed.set_verify_policy(policy))
        if switch:
            switch()
        assert bool(verify().all())
        forms[label] = (switch, verify)
    ms = rate_kit.alternate(forms, REPEATS)
finally:
    if not BASELINE:
        ed.set_verify_policy(0)

print(f"{ed.library_path()}: 2^{LOG_N} valid items, msg_len 32, {REPEATS} repeats")
base = ms["policy 0"][REPEATS // 2]
for label, _ in ROWS:                              # its own row: the kit's label width, the spread also in per cent
    v = ms[label]
    med = v[REPEATS // 2]
    print(f"  {label:{rate_kit.LABEL_WIDTH}s} {med:8.3f} ms  [{v[0]:.3f} .. {v[-1]:.3f}]  spread {v[-1] - v[0]:.3f} ms ({100 * (v[-1] - v[0]) / med:.1f} %)"
          f"  {n / med / 1e3:7.2f} M/s  {100 * (med - base) / base:+6.2f} % against policy 0", flush=True)
