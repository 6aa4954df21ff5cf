"""Time of one x25519 pass for small and mid-size batches, device-resident, back to back."""
import numpy as np, torch
import rate_kit, workload
ed = rate_kit.bind()
d = lambda a: torch.from_numpy(a).cuda()
print("x25519      ", end=" ")
for l in (0, 10, 12, 13, 14, 15, 16):
    n = 1 << l
    sc, pt = workload.x25519_inputs(n)
    a, b = d(sc), d(pt)
    print(f"2^{l}: {rate_kit.steady(lambda: ed.x25519_batch(a, b)):.3f}", end="  ")
print("ms")
