#!/usr/bin/env python3
"""What verifying items in place costs (ed25519_verify_scattered_dev, include/eddsa_amd.h): the front kernel that gathers and
hashes, in front of a digest pass.  Device-resident inputs, device events, on tools/rate_kit.py:

  row 1   2^20 valid items with 32-byte messages in HBM, four forms alternating in one process:
            ed25519_verify_batch_dev over the items packed
            ed25519_verify_scattered_dev over the same items laid out as 128-byte packets (signature, key, message)
            the same call with 8 signatures sharing each message (packets of 32 + 8 * 96 bytes)
            ed25519ctx_verify_batch_dev over as many valid Ed25519ctx signatures: the existing form with a front kernel, for scale
  row 2   passes of 2^7, 2^10, 2^14 and 2^16 items: packed beside scattered
  row 3   the host form from ordinary memory beside ed25519_verify_batch from ordinary memory, host clock
  row 4   (with --parent LIB) ed25519_verify_batch_dev, this build against another build of the library, alternating in fresh
          processes: whether the unchanged pass moved

Before anything is timed every form's verdicts are checked: all items accepted, and with one byte of every 1000th item's
message, signature or key spoilt the scattered call rejects exactly what the packed call rejects.

  tools/scattered_rate.py [repeats=5] [log2 of the batch=20] [--parent path/to/libeddsa_amd_debug.so]
"""
import os
import sys

import torch

import rate_kit
from rate_kit import alternate, show

REPEATS, LOG_N, PARENT, FLAGS = rate_kit.cli(sys.argv[1:])
ed = rate_kit.bind()                               # the product's objects (a --parent library is bound as given)

n = 1 << LOG_N
rnd = rate_kit.rnd(25519)
sk, msg = rnd(n, 32), rnd(n, 32)
pk = ed.ed25519_genpub_batch(sk)
sig = ed.ed25519_sign_batch(sk, pk, msg, msg_len=32)
assert bool(ed.ed25519_verify_batch(sig, pk, msg, msg_len=32).all())

if rate_kit.CHILD_FLAG in FLAGS:                    # (the child processes of row 4)
    rate_kit.emit(alternate({"VERIFY": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32)}, 3))
    sys.exit(0)


def offsets(count, stride, first):
    return (torch.arange(count, device="cuda", dtype=torch.int64) * stride + first).to(torch.int32).contiguous()


# 128-byte packets: signature | key | message
packets = torch.cat([sig, pk, msg], dim=1).contiguous().reshape(-1)
p_idx = (offsets(n, 128, 0), offsets(n, 128, 64), offsets(n, 128, 96), torch.full((n,), 32, dtype=torch.int32, device="cuda"))
# 8 signers per message: message | 8 x (signature | key); item i is signer i % 8 of packet i / 8, all over that packet's message
shared_msg = msg[::8].contiguous()                                                     # (n / 8, 32)
who = torch.arange(n, device="cuda") // 8
sig8 = ed.ed25519_sign_batch(sk, pk, shared_msg[who].contiguous(), msg_len=32)
pairs = torch.cat([sig8, pk], dim=1).reshape(n // 8, 8 * 96)
shared = torch.cat([shared_msg, pairs], dim=1).contiguous().reshape(-1)
PKT = 32 + 8 * 96
item = torch.arange(n, device="cuda", dtype=torch.int64)
s_off = ((item // 8) * PKT + 32 + (item % 8) * 96).to(torch.int32).contiguous()
s_idx = (s_off, (s_off + 64).contiguous(), ((item // 8) * PKT).to(torch.int32).contiguous(),
         torch.full((n,), 32, dtype=torch.int32, device="cuda"))
ctx_sig = ed.ed25519ctx_sign_batch(sk, pk, msg, b"ctx", msg_len=32)

assert bool(ed.ed25519_verify_scattered(packets, *p_idx).all())
assert bool(ed.ed25519_verify_scattered(shared, *s_idx).all())
assert bool(ed.ed25519ctx_verify_batch(ctx_sig, pk, msg, b"ctx", msg_len=32).all())
spoilt = packets.clone().reshape(n, 128)
spoilt[0::3000, 100] ^= 1; spoilt[1000::3000, 7] ^= 1; spoilt[2000::3000, 70] ^= 1
want = ed.ed25519_verify_batch(spoilt[:, :64].contiguous(), spoilt[:, 64:96].contiguous(), spoilt[:, 96:].contiguous(), msg_len=32)
assert torch.equal(ed.ed25519_verify_scattered(spoilt.reshape(-1), *p_idx), want) and int(want.sum()) == n - len(range(0, n, 1000))

print(f"{torch.cuda.get_device_name(0)}; repeats {REPEATS}; every row: min .. max over the repeats, median in front\n")
print(f"row 1: 2^{LOG_N} valid items, 32-byte messages, in HBM, the forms alternating:")
r = alternate({"packed": lambda: ed.ed25519_verify_batch(sig, pk, msg, msg_len=32),
               "scattered": lambda: ed.ed25519_verify_scattered(packets, *p_idx),
               "shared": lambda: ed.ed25519_verify_scattered(shared, *s_idx),
               "ctx": lambda: ed.ed25519ctx_verify_batch(ctx_sig, pk, msg, b"ctx", msg_len=32)}, REPEATS)
base = show("ed25519_verify_batch_dev, packed", n, r["packed"])
show("ed25519_verify_scattered_dev, 128-byte packets", n, r["scattered"], base, "the packed pass")
show("ed25519_verify_scattered_dev, 8 signatures per message", n, r["shared"], base, "the packed pass")
show("ed25519ctx_verify_batch_dev, packed, 3-byte context", n, r["ctx"], base, "the packed pass")
print()
print("row 2: small passes, packed beside scattered (128-byte packets):")
for log_s in (7, 10, 14, 16):
    s = 1 << log_s
    if s > n:
        continue
    cut = [t[:s].contiguous() for t in (sig, pk, msg)]
    cut_idx = [t[:s].contiguous() for t in p_idx]
    cut_data = packets[:128 * s].contiguous()
    r = alternate({"packed": lambda: ed.ed25519_verify_batch(cut[0], cut[1], cut[2], msg_len=32),
                   "scattered": lambda: ed.ed25519_verify_scattered(cut_data, *cut_idx)}, REPEATS)
    base = show(f"2^{log_s}: ed25519_verify_batch_dev", s, r["packed"])
    show(f"2^{log_s}: ed25519_verify_scattered_dev", s, r["scattered"], base, "the packed pass")
print()
print(f"row 3: host to host from ordinary memory, 2^{LOG_N} items, host clock:")
h_sig, h_pk, h_msg, h_packets = (t.cpu().numpy() for t in (sig, pk, msg, packets))
h_idx = [t.cpu().numpy().view("uint32") for t in p_idx]
r = alternate({"packed": lambda: ed.ed25519_verify_batch(h_sig, h_pk, h_msg, msg_len=32),
               "scattered": lambda: ed.ed25519_verify_scattered(h_packets, *h_idx)}, REPEATS, clock=rate_kit.wall)
base = show("ed25519_verify_batch (staging pipeline)", n, r["packed"])
show("ed25519_verify_scattered (upload, one call, download)", n, r["scattered"], base, "the packed call")
print()

if PARENT:
    print(f"row 4: ed25519_verify_batch_dev, this build against {os.path.relpath(PARENT, rate_kit.ROOT)}, fresh processes alternating:")
    rows = rate_kit.parent_ab(__file__, LOG_N, REPEATS, rate_kit.CHILD_FLAG, ("VERIFY",), PARENT, rate_kit.DEBUG_LIBRARY)
    p = rows[("parent", "VERIFY")]
    show("parent build", n, p)
    med = show("this build", n, rows[("this", "VERIFY")], p[len(p) // 2], "the parent build")
    print(f"  -> this build's median is {'inside' if p[0] <= med <= p[-1] else 'OUTSIDE'} the parent build's own repeat spread [{p[0]:.3f} .. {p[-1]:.3f}] ms")
