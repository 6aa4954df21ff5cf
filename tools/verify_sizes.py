"""One verify pass (config-2 mix, device-resident) by size: SIZES=19,18,17 python tools/verify_sizes.py"""
import os, time
import numpy as np
import torch
import rate_kit, workload
ed = rate_kit.bind()
if os.environ.get("OFFCURVE_MODE"): ed.set_offcurve_mode(int(os.environ["OFFCURVE_MODE"]))
if os.environ.get("VERIFY_ALGO"): ed.set_verify_algo(int(os.environ["VERIFY_ALGO"]))   # 1 full-length, 2 half-length, whatever the size
for lg in [int(x) for x in os.environ.get("SIZES", "20,19,18,17,16,15,14,13,12").split(",")]:
    n = 1 << lg
    sk, msg = workload.sign_inputs(n, seed=1, config=2)
    pk = ed.ed25519_genpub_batch(sk); sig = ed.ed25519_sign_batch(sk, pk, msg)
    expect = workload.corrupt_for_verify(sig, pk, msg)
    def timeit(fn, reps=5):
        fn(); best = 1e9
        for _ in range(reps):
            t0 = time.perf_counter(); out = fn(); best = min(best, time.perf_counter() - t0)
        return best, out
    dt, ok = timeit(lambda: ed.ed25519_verify_batch(sig, pk, msg)); assert np.array_equal(ok, expect)
    d = lambda a: torch.from_numpy(a).cuda()
    ds, dp, dm = d(sig), d(pk), d(msg)
    def dev():
        o = ed.ed25519_verify_batch(ds, dp, dm); torch.cuda.synchronize(); return o
    dt2, _ = timeit(dev)
    print(f"n=2^{lg}: host {dt*1e3:7.2f} ms {n/dt/1e6:6.1f} M/s | device {dt2*1e3:7.2f} ms {n/dt2/1e6:6.1f} M/s")
