#!/usr/bin/env python3
"""Signing over a signer set against signing with per-item keys (ed25519_sign_keyed* against ed25519_sign_batch*, and the ctx / ph
forms), device-resident inputs, device events, in the style of tools/keyed_rate.py and tools/dom2_rate.py:

  row 1   2^20 items of 32 bytes: ed25519_sign_batch_dev against ed25519_sign_keyed_dev under 1, 1024 and 2^20 signers
  row 2   the ctx and ph forms, unkeyed against keyed, under 1024 signers (a 3-byte context; ph: 64-byte prehashes)
  row 3   passes of 2^7, 2^10, 2^14 and 2^16 items under 1024 signers, unkeyed against keyed
  row 4   host to host from ordinary memory, 2^20 items: ed25519_sign_batch against ed25519_sign_keyed (wall clock)
  row 5   eddsa_amd_signer_create for 1024 and 2^20 keys (wall clock, the destroy not included)

The forms of a row alternate in one process; every repeat is `iters` calls between two events; the spread of a form is max - min
over its repeats.  Before anything is timed every keyed form's signatures are compared, byte for byte, with the unkeyed form's.

  tools/sign_keyed_rate.py [repeats=5] [log2 of the large batches=20]
  tools/sign_keyed_rate.py unchanged [repeats=5]     only ed25519_sign_batch_dev over 2^20 items: the row that is measured
                                                     against the build of the commit before, alternating in fresh processes
                                                     (tools/ab.sh; the library comes from EDDSA_AMD_LIBRARY)
"""
import sys
import time

import numpy as np
import torch

import rate_kit
from rate_kit import alternate, show, timed, wall

REPEATS, LOG_N, _, FLAGS = rate_kit.cli(sys.argv[1:])
UNCHANGED = "unchanged" in FLAGS
CONTEXT = b"foo"
ed = rate_kit.bind(debug=False)


def pair(title, n, unkeyed_label, unkeyed, keyed_label, keyed, clock=timed):
    want, got = unkeyed(), keyed()
    assert bool(torch.equal(want, got)) if torch.is_tensor(want) else np.array_equal(want, got), title
    del want, got
    print(title)
    r = alternate({unkeyed_label: unkeyed, keyed_label: keyed}, REPEATS, clock)
    base = show(unkeyed_label, n, r[unkeyed_label])
    show(keyed_label, n, r[keyed_label], base, "the unkeyed form")
    print()


n = 1 << LOG_N
g = torch.Generator(device="cuda").manual_seed(2520)    # its own generator: the signer indices are drawn from it as well
rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)   # noqa: E731
seeds, msg, pre = rnd(n, 32), rnd(n, 32), rnd(n, 64)

if UNCHANGED:
    pk = ed.ed25519_genpub_batch(seeds)
    r = alternate({"sign": lambda: ed.ed25519_sign_batch(seeds, pk, msg, msg_len=32)}, REPEATS)
    show(f"ed25519_sign_batch_dev, 2^{LOG_N} items", n, r["sign"])
    sys.exit(0)

print(f"{torch.cuda.get_device_name(0)}; repeats {REPEATS}; every row: min .. max over the repeats, median in front\n")
seeds_host = seeds.cpu().numpy()
signers = {}
for count in (1, 1024, n):
    t = time.perf_counter()
    signers[count] = ed.signer_create(secs=seeds_host[:count])
    first = (time.perf_counter() - t) * 1e3
    print(f"signer_create, {count} keys: {first:.2f} ms (the first call of its size)")
print()

# row 1
for count in (1, 1024, n):
    idx = torch.randint(0, count, (n,), dtype=torch.int32, device="cuda", generator=g)
    sk = seeds[idx.long()].contiguous()
    pk = ed.ed25519_genpub_batch(sk)
    pair(f"sign, 2^{LOG_N} items of 32 bytes under {count} signers:", n,
         "ed25519_sign_batch_dev", lambda: ed.ed25519_sign_batch(sk, pk, msg, msg_len=32),
         "ed25519_sign_keyed_dev", lambda: ed.ed25519_sign_keyed(signers[count], idx, msg, msg_len=32))

# rows 2 and 3 under 1024 signers
signer = signers[1024]
idx = torch.randint(0, 1024, (n,), dtype=torch.int32, device="cuda", generator=g)
sk = seeds[idx.long()].contiguous()
pk = ed.ed25519_genpub_batch(sk)
pair(f"Ed25519ctx, 2^{LOG_N} items of 32 bytes, context {CONTEXT!r}, 1024 signers:", n,
     "ed25519ctx_sign_batch_dev", lambda: ed.ed25519ctx_sign_batch(sk, pk, msg, CONTEXT, msg_len=32),
     "ed25519ctx_sign_keyed_dev", lambda: ed.ed25519ctx_sign_keyed(signer, idx, msg, CONTEXT, msg_len=32))
pair(f"Ed25519ph, 2^{LOG_N} prehashes of 64 bytes, context {CONTEXT!r}, 1024 signers:", n,
     "ed25519ph_sign_batch_dev", lambda: ed.ed25519ph_sign_batch(sk, pk, pre, CONTEXT),
     "ed25519ph_sign_keyed_dev", lambda: ed.ed25519ph_sign_keyed(signer, idx, pre, CONTEXT))
for log_m in (7, 10, 14, 16):
    m = 1 << log_m
    s, p, i, d = sk[:m].contiguous(), pk[:m].contiguous(), idx[:m].contiguous(), msg[:m].contiguous()
    pair(f"small passes: 2^{log_m} items of 32 bytes, 1024 signers:", m,
         "ed25519_sign_batch_dev", lambda: ed.ed25519_sign_batch(s, p, d, msg_len=32),
         "ed25519_sign_keyed_dev", lambda: ed.ed25519_sign_keyed(signer, i, d, msg_len=32))

# row 4: host to host, ordinary memory
sk_h, pk_h, msg_h = sk.cpu().numpy(), pk.cpu().numpy(), msg.cpu().numpy()
idx_h = idx.cpu().numpy().view(np.uint32)
pair(f"host to host from ordinary memory, 2^{LOG_N} items of 32 bytes, 1024 signers (wall clock):", n,
     "ed25519_sign_batch", lambda: ed.ed25519_sign_batch(sk_h, pk_h, msg_h, msg_len=32),
     "ed25519_sign_keyed", lambda: ed.ed25519_sign_keyed(signer, idx_h, msg_h, msg_len=32), clock=wall)

# row 5: creation
print("eddsa_amd_signer_create from host seeds (wall clock, each set destroyed outside the timed part):")
for count in (1024, n):
    ms = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        s = ed.signer_create(secs=seeds_host[:count])
        ms.append((time.perf_counter() - t) * 1e3)
        s.close()
    ms.sort()
    print(f"  {count:8d} keys  {ms[len(ms) // 2]:9.3f} ms  [{ms[0]:.3f} .. {ms[-1]:.3f}]  ({count * 96 / 1048576:.2f} MiB held)")
for s in signers.values():
    s.close()
