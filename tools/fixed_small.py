#!/usr/bin/env python3
"""Time of one pass of the fixed-base operations for small and mid-size batches, device-resident, back to back"""
import numpy as np, torch
import rate_kit, workload
ed = rate_kit.bind()
d = lambda a: torch.from_numpy(a).cuda()
for name in ("genpub", "sign", "x25519_base"):
    print(f"{name:12s}", end=" ")
    for l in (0, 6, 10, 12, 13, 14, 15, 16, 18):
        n = 1 << l
        sk, msg = workload.sign_inputs(n, seed=1, config=5)
        dsk, dmsg = d(sk), d(msg)
        pk = ed.ed25519_genpub_batch(dsk)
        f = {"genpub": lambda: ed.ed25519_genpub_batch(dsk), "sign": lambda: ed.ed25519_sign_batch(dsk, pk, dmsg),
             "x25519_base": lambda: ed.x25519_base_batch(dsk)}[name]
        print(f"2^{l}: {rate_kit.steady(f):.3f}", end="  ")
    print("ms")
