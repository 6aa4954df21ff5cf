#!/usr/bin/env python3
"""What the opt-in cofactored equation (include/eddsa_amd.h: eddsa_amd_set_verify_equation; kernels.hip: k_cofactor_*) costs a
verify pass: ed25519_verify_batch on 2^20 device-resident items with 32-byte messages, device events.  The rows take turns in one
process; every repeat is `iters` calls between two events; the spread of a row is max - min over its repeats.

  tools/cofactored_cost.py [repeats=5] [log2 items=20] [baseline]

  equation 0             the default: nothing is queued
  equation 1, valid      the pass in reject mode on the full-length route, k_cofactor_list over its verdicts (an empty list) and
                         S < l in the policy kernel
  equation 1, 1 % bad    one signature in a hundred has a bit of S flipped: the list holds 1 % of the pass
  equation 1, all bad    every signature has: the worst case a caller can construct, a full-length evaluation of every item on
                         top of the pass
  rlc, equation 0 / 1    ed25519_verify_batch_rlc on the valid items

baseline: equation 0 only and no call of set_verify_equation - the row to compare between two builds of the library on one box
(tools/ab.sh with EDDSA_AMD_LIBRARY; a build from before the equation existed has no such symbol).

Measured (profiles/verify_cofactored.txt, one MI355X): equation 0 9.51 ms; equation 1 on valid items 10.55 ms (+11 %), with 1 %
bad 11.87 ms (+25 %), all bad 22.20 ms (+134 %); rlc 4.38 -> 4.40 ms (+0.4 %); equation 0 against the parent commit 9.48-9.49 ms
against 9.48-9.49 ms.  The 1 % row shows the one-lane evaluation dominating a short list: 1.3 ms for 10 486 items, the latency of
one chain; a four-lane form for short lists is a follow-up.
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
some_bad, all_bad = dsig.clone(), dsig.clone()
some_bad[::100, 40] ^= 1                            # a bit of S: still below l or not, the equation fails either way
all_bad[:, 40] ^= 1
verify = lambda sig: ed.ed25519_verify_batch(sig, dpk, dmsg, msg_len=32)   # noqa: E731
rlc = lambda sig: ed.ed25519_verify_batch_rlc(sig, dpk, dmsg, msg_len=32)   # noqa: E731
assert bool(verify(dsig).all())

# label, equation, call, signatures, accepted items
ROWS = [("equation 0", 0, verify, dsig, n)]
if not BASELINE:
    ROWS += [("eq 1, valid", 1, verify, dsig, n), ("eq 1, 1 % bad", 1, verify, some_bad, n - (n + 99) // 100),
             ("eq 1, all bad", 1, verify, all_bad, 0), ("rlc, eq 0", 0, rlc, dsig, n), ("rlc, eq 1", 1, rlc, dsig, n)]


try:
    forms = {}
    for label, equation, call, sig, accepted in ROWS:   # the verdicts; baseline never touches the switch
        switch = None if BASELINE else (lambda equation=equation: ed.set_verify_equation(equation))
        if switch:
            switch()
        assert int(call(sig).sum()) == accepted, label
        forms[label] = (switch, lambda call=call, sig=sig: call(sig))
    ms = rate_kit.alternate(forms, REPEATS)
finally:
    if not BASELINE:
        ed.set_verify_equation(0)

print(f"{ed.library_path()}: 2^{LOG_N} items, msg_len 32, {REPEATS} repeats")
base = ms["equation 0"][REPEATS // 2]
for row in ROWS:                                   # its own row: the kit's label width, the spread also in per cent
    v = ms[row[0]]
    med = v[REPEATS // 2]
    print(f"  {row[0]:{rate_kit.LABEL_WIDTH}s} {med:8.3f} ms  [{v[0]:.3f} .. {v[-1]:.3f}]  spread {v[-1] - v[0]:.3f} ms ({100 * (v[-1] - v[0]) / med:.1f} %)"
          f"  {n / med / 1e3:7.2f} M/s  {100 * (med - base) / base:+7.2f} % against equation 0", flush=True)
