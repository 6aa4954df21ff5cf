#!/usr/bin/env python3
"""ms per verify pass of 2^20 genuine signatures under keys of which every k-th is a random string (k = 1, 2, 16): the
worst case a sender can construct, device-resident, HIP events.  For A/B runs through tools/ab.sh."""
import numpy as np, torch
import rate_kit, workload
ed = rate_kit.bind()
n = 1 << 20
sk, msg = workload.sign_inputs(n)
d = lambda a: torch.from_numpy(a).cuda()
pk = ed.ed25519_genpub_batch(d(sk)); sig = ed.ed25519_sign_batch(d(sk), pk, d(msg)); dm = d(msg)
garbage = d(np.random.default_rng(1).integers(0, 256, (n, 32), dtype=np.uint8))
out = []
for step in (1, 2, 16):
    keys = pk.clone(); keys[::step] = garbage[::step]
    for _ in range(2): ok = ed.ed25519_verify_batch(sig, keys, dm)
    ms = rate_kit.timed(lambda: ed.ed25519_verify_batch(sig, keys, dm), 8)     # (its own untimed call is the third)
    out.append("1/%d random: %.2f ms (%d accepted)" % (step, ms, int(ok.sum())))
print(" | ".join(out))
