#!/usr/bin/env python3
"""Message form against digest form (ed25519_verify_batch / ed25519_verify_digests), device-resident inputs, device events:

  row 1   2^20 items of the config-2 mix (tools/workload.py), 32-byte messages
  row 2   the same mix over 1024-byte messages
  row 3   2^16 items of 32 bytes with one message in 1024 of 1 MiB (the skewed row of tools/msglen_table.py), and the same
          items with every message 32 bytes: the digest form never reads a message, so its time must not tell them apart

The two forms alternate in one process; every repeat is `iters` calls between two events; the spread of a form is max - min
over its repeats.  Digests are hashlib's SHA-512(R || A || M) over the batch as it is verified; both forms must return the
workload's expected verdicts before anything is timed.

  tools/digest_rate.py [repeats=5] [log2 of the large batches=20]
"""
import hashlib
import sys

import numpy as np
import torch

import rate_kit
import workload
from rate_kit import alternate

REPEATS, LOG_N, _, _ = rate_kit.cli(sys.argv[1:])
ed = rate_kit.bind(debug=False)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731


def digests_of(sig, pk, msgs):
    out = np.empty((len(sig), 64), np.uint8)
    for i in range(len(sig)):
        out[i] = np.frombuffer(hashlib.sha512(sig[i, :32].tobytes() + pk[i].tobytes() + bytes(msgs[i])).digest(), np.uint8)
    return out


def show(label, n, ms):
    """this script's own row (the kit's label width; the spread also as a share of the median, which its conditions read): returns
    the median and the spread"""
    med = ms[len(ms) // 2]
    print(f"  {label:{rate_kit.LABEL_WIDTH}s} {med:9.3f} ms  [{ms[0]:.3f} .. {ms[-1]:.3f}]  spread {ms[-1] - ms[0]:.3f} ms ({100 * (ms[-1] - ms[0]) / med:.1f} %)"
          f"  {n / med / 1e3:8.2f} M/s", flush=True)
    return med, ms[-1] - ms[0]


def config2(n, mlen):
    """the config-2 mix over mlen-byte messages (the workload's 32 bytes, then random ones) -> sig, pk, msg, expected verdicts"""
    sk, msg = workload.sign_inputs(n, seed=1, config=2)
    if mlen > 32:
        g = torch.Generator(device="cuda").manual_seed(11)
        tail = torch.randint(0, 256, (n, mlen - 32), dtype=torch.uint8, device="cuda", generator=g).cpu().numpy()
        msg = np.concatenate([msg, tail], axis=1)
    pk = ed.ed25519_genpub_batch(dev(sk))
    sig = ed.ed25519_sign_batch(dev(sk), pk, dev(msg), msg_len=mlen).cpu().numpy()
    pk = pk.cpu().numpy()
    expect = workload.corrupt_for_verify(sig, pk, msg)
    return sig, pk, msg, expect


def fixed_row(n, mlen):
    sig, pk, msg, expect = config2(n, mlen)
    dsig, dpk, dmsg, ddig = dev(sig), dev(pk), dev(msg), dev(digests_of(sig, pk, msg))
    by_msg = lambda: ed.ed25519_verify_batch(dsig, dpk, dmsg, msg_len=mlen)      # noqa: E731
    by_dig = lambda: ed.ed25519_verify_digests(dsig, dpk, ddig)                  # noqa: E731
    assert np.array_equal(by_msg().cpu().numpy(), expect) and np.array_equal(by_dig().cpu().numpy(), expect)
    print(f"2^{LOG_N} items, config-2 mix, msg_len {mlen} ({int(expect.sum())} accepted):")
    r = alternate({"message": by_msg, "digest": by_dig}, REPEATS)
    m, m_spread = show("message form", n, r["message"])
    d, _ = show("digest form", n, r["digest"])
    print(f"  digest form against message form: {100 * (d - m) / m:+.2f} %", flush=True)
    return m, m_spread, d


n = 1 << LOG_N
m, m_spread, d = fixed_row(n, 32)
print(f"  condition (digest form not slower than the message form by more than the message form's repeat spread, {m_spread:.3f} ms): "
      f"{'met' if d - m <= m_spread else 'MISSED'} ({d - m:+.3f} ms)\n", flush=True)
fixed_row(n, 1024)
print()

# row 3: valid signatures, as tools/msglen_table.py's skewed row
n = 1 << 16
g = torch.Generator(device="cuda").manual_seed(7)
dsk = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
dpk = ed.ed25519_genpub_batch(dsk)
pk = dpk.cpu().numpy()
sets = {}
short = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
for name, long_len in (("all 32 B", 32), ("1 in 1024 of 1 MiB", 1 << 20)):
    # the SAME items in both sets but for the messages at 511, 1535, ..: a verify pass's time depends on its data (an item without
    # a short pair takes the exact path), so sets of other signatures would differ by that, whatever the form
    lens = np.full(n, 32, np.int64); lens[511::1024] = long_len
    off = np.zeros(n + 1, np.int64); off[1:] = np.cumsum(lens)
    blob = torch.randint(0, 256, (int(off[-1]),), dtype=torch.uint8, device="cuda", generator=g)
    keep = np.nonzero(lens == 32)[0]
    at = torch.from_numpy(off[keep][:, None] + np.arange(32)[None, :]).cuda()
    blob[at] = short[torch.from_numpy(keep).cuda()]
    doff = torch.from_numpy(off).cuda()
    dsig = ed.ed25519_sign_batch(dsk, dpk, blob, msg_off=doff)
    sig, host = dsig.cpu().numpy(), blob.cpu().numpy()
    ddig = dev(digests_of(sig, pk, [host[off[i]:off[i + 1]] for i in range(n)]))
    sets[name] = (dsig, blob, doff, ddig)
    assert bool(ed.ed25519_verify_batch(dsig, dpk, blob, msg_off=doff).all()) and bool(ed.ed25519_verify_digests(dsig, dpk, ddig).all())
# Order: the message form's pass over the skewed set keeps one wave busy for 65 ms, and whatever is timed right behind such passes
# runs 7 % slower for tens of milliseconds, whichever form and set it is (profiles/digest_verify.txt: the four orders measured).
# So the slow form goes first in every round and the two digest forms, which the condition compares, run next to each other.
forms = {}
for name, (dsig, blob, doff, ddig) in reversed(sets.items()):
    forms["message form, " + name] = lambda dsig=dsig, blob=blob, doff=doff: ed.ed25519_verify_batch(dsig, dpk, blob, msg_off=doff)
for name, (dsig, blob, doff, ddig) in sets.items():
    forms["digest form,  " + name] = lambda dsig=dsig, ddig=ddig: ed.ed25519_verify_digests(dsig, dpk, ddig)
print("2^16 valid items, 32-byte messages / one message in 1024 of 1 MiB:")
r = alternate(forms, REPEATS)
res = {k: show(k, n, v) for k, v in r.items()}
(d0, s0), (d1, s1) = res["digest form,  all 32 B"], res["digest form,  1 in 1024 of 1 MiB"]
print(f"  condition (the digest form's time on the two sets differs by no more than its own repeat spread, {max(s0, s1):.3f} ms): "
      f"{'met' if abs(d1 - d0) <= max(s0, s1) else 'MISSED'} ({d1 - d0:+.3f} ms)")
print(f"  message form on the skewed set: {res['message form, 1 in 1024 of 1 MiB'][0]:.2f} ms; digest form: {d1:.3f} ms")
