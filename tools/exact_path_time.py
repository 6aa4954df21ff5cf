#!/usr/bin/env python3
"""Cost of the exact (reference-order) path for off-curve public keys: time of a verify pass over
n items as a function of the share of off-curve keys."""
import torch, numpy as np
import rate_kit, workload
ed = rate_kit.bind()
n = 1 << 20
sk, msg = workload.sign_inputs(n)
d = lambda a: torch.from_numpy(a).cuda()
pk = ed.ed25519_genpub_batch(d(sk)); sig = ed.ed25519_sign_batch(d(sk), pk, d(msg)); dm = d(msg)
rng = np.random.default_rng(1)
garbage = d(rng.integers(0, 256, (n, 32), dtype=np.uint8))


def row(label, keys):
    ok = ed.ed25519_verify_batch(sig, keys, dm)
    dt = rate_kit.steady(lambda: ed.ed25519_verify_batch(sig, keys, dm), warm=0, iters=5) / 1e3
    print(f"{label}: {dt*1e3:.2f} ms  {n/dt/1e6:.1f} M/s  accepted {int(ok.sum())}")


for share in (0, 1 / 1024, 1 / 128, 1 / 16, 1 / 4, 1 / 2, 1):
    keys = pk.clone()
    if share:
        step = int(1 / share)
        keys[::step] = garbage[::step]
    row(f"garbage keys 1/{int(1/share) if share else 0}", keys)

# the former cliff: the four-lane chain took 65 536 work-list entries and a spilling one-lane kernel the rest (rounds 1-3);
# now every stretch of 65 536 entries is one more launch of the same kernel.  Exactly k keys off the curve, k around 65 536:
ed.debug_init(0, True)
flags = ed.debug_layer("ed_import_export", [bytes(r) for r in garbage[:400000].cpu().numpy()], 33)
off = np.array([f[32] == 0 for f in flags])
idx_off = np.nonzero(off)[0]
for k in (2048, 4096, 8192, 16384, 32768, 65536, 131072):
    keys = pk.clone()
    sel = torch.from_numpy(idx_off[:k]).cuda()
    keys[sel] = garbage[sel]
    row(f"exactly {k} keys off the curve", keys)
ed.debug_init(0, False)

ed.set_offcurve_mode(False)
keys = pk.clone(); keys[::128] = garbage[::128]
row("reject mode, garbage keys 1/128", keys)
ed.set_offcurve_mode(True)
