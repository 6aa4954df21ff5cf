"""where the four-lane route and the mid-size arrangement cross: one valid-only pass, ms, algo 0 (default) / 3 (mid-size arrangement forced)"""
import numpy as np, torch
import rate_kit, workload
ed = rate_kit.bind()
d = lambda a: torch.from_numpy(a).cuda()
n0 = 1 << 15
sk, msg = workload.sign_inputs(n0, seed=1, config=2)
pk = ed.ed25519_genpub_batch(d(sk)); sig = ed.ed25519_sign_batch(d(sk), pk, d(msg))
dm = d(msg)
for algo in (0, 3):
    ed.set_verify_algo(algo)
    print(f"algo {algo}", end="  ")
    for n in (16384, 18000, 20000, 22000, 24576, 26000, 28000, 30000, 32768):
        a, b, c = sig[:n].contiguous(), pk[:n].contiguous(), dm[:n].contiguous()
        print(f"{n}: {rate_kit.steady(lambda: ed.ed25519_verify_batch(a, b, c)):.3f}", end="  ")
    print("ms")
ed.set_verify_algo(0)
