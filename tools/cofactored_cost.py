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
import os
import sys

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


def timed(row, iters):
    _, equation, call, sig, _ = row
    if not BASELINE:
        ed.set_verify_equation(equation)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call(sig)                                       # untimed: the repeat starts from this row's own state
    a.record()
    for _ in range(iters):
        call(sig)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


try:
    iters = {}
    for row in ROWS:                                # warm-up and the verdicts; sizes a repeat to about 0.1 s
        if not BASELINE:
            ed.set_verify_equation(row[1])
        assert int(row[2](row[3]).sum()) == row[4], row[0]
        iters[row[0]] = max(2, min(50, int(100.0 / max(timed(row, 2), 1e-3))))
    ms = {row[0]: [] for row in ROWS}
    for _ in range(REPEATS):
        for row in ROWS:
            ms[row[0]].append(timed(row, iters[row[0]]))
finally:
    if not BASELINE:
        ed.set_verify_equation(0)

print(f"{ed.library_path()}: 2^{LOG_N} items, msg_len 32, {REPEATS} repeats")
base = sorted(ms["equation 0"])[REPEATS // 2]
for row in ROWS:
    v = sorted(ms[row[0]])
    med = v[REPEATS // 2]
    print(f"  {row[0]:14s} {med:8.3f} ms  [{v[0]:.3f} .. {v[-1]:.3f}]  spread {v[-1] - v[0]:.3f} ms ({100 * (v[-1] - v[0]) / med:.1f} %)"
          f"  {n / med / 1e3:7.2f} M/s  {100 * (med - base) / base:+7.2f} % against equation 0", flush=True)
