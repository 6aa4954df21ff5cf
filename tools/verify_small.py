"""Time of one verify pass for small batches, device-resident, back to back (no host sync between calls):
valid signatures only (no key off the curve, so the exact path has nothing to do) and the config-2 recipe
(corruptions and edge vectors: the reference-order chain for the off-curve keys sets the floor)."""
import numpy as np, torch
import rate_kit, workload
ed = rate_kit.bind()
d = lambda a: torch.from_numpy(a).cuda()
for algo in (0, 1):
    ed.set_verify_algo(algo)
    for clean in (True, False):
        print(f"algo {algo} {'valid only   ' if clean else 'config-2 mix '}", end=" ")
        for l in (17, 16, 15, 14, 13, 12, 11, 10, 8, 6, 0):
            n = 1 << l
            sk, msg = workload.sign_inputs(n, seed=1, config=2)
            pk = ed.ed25519_genpub_batch(d(sk)); sig = ed.ed25519_sign_batch(d(sk), pk, d(msg)).cpu().numpy(); pk = pk.cpu().numpy()
            if not clean: workload.corrupt_for_verify(sig, pk, msg)
            ds, dp, dm = d(sig), d(pk), d(msg)
            print(f"2^{l}: {rate_kit.steady(lambda: ed.ed25519_verify_batch(ds, dp, dm)):.3f}", end="  ")
        print("ms")
