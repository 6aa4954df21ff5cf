"""Mid-size verify passes: the default routes (algo 0), the mid-size arrangement forced (3) and one lane per item throughout (2) - verdicts against the constructed ones, then ms per pass."""
import numpy as np, torch
import rate_kit, workload
ed = rate_kit.bind()
d = lambda a: torch.from_numpy(a).cuda()
for n in (1000, 1 << 15, (1 << 16) + 5, 1 << 17, (1 << 18) - 3):
    sk, msg = workload.sign_inputs(n, seed=3, config=2)
    pk = ed.ed25519_genpub_batch(d(sk)); sig = ed.ed25519_sign_batch(d(sk), pk, d(msg)).cpu().numpy(); pk = pk.cpu().numpy()
    want = workload.corrupt_for_verify(sig, pk, msg)
    ds, dp, dm = d(sig), d(pk), d(msg)
    res = {}
    for algo in (0, 3, 2):
        ed.set_verify_algo(algo)
        res[algo] = ed.ed25519_verify_batch(ds, dp, dm).cpu().numpy()
    print(n, "algo3==want", np.array_equal(res[3], want), "algo0==want", np.array_equal(res[0], want), "algo2==want", np.array_equal(res[2], want))
for clean in (True, False):
    for algo in (0, 3, 2):
        ed.set_verify_algo(algo)
        print(f"algo {algo} {'valid only   ' if clean else 'config-2 mix '}", end=" ")
        for l in (17, 16, 15, 14, 13):
            n = 1 << l
            sk, msg = workload.sign_inputs(n, seed=1, config=2)
            pk = ed.ed25519_genpub_batch(d(sk)); sig = ed.ed25519_sign_batch(d(sk), pk, d(msg)).cpu().numpy(); pk = pk.cpu().numpy()
            if not clean: workload.corrupt_for_verify(sig, pk, msg)
            ds, dp, dm = d(sig), d(pk), d(msg)
            print(f"2^{l}: {rate_kit.steady(lambda: ed.ed25519_verify_batch(ds, dp, dm)):.3f}", end="  ")
        print("ms")
