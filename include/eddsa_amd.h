/*
 * eddsa_amd.h - batched entry points of the MI355X Ed25519 / X25519 engine.
 *
 * Plain C ABI (pointers and sizes only).  Every function is the batched form of one function
 * of the reference's public header and returns, item by item, exactly what a loop over the
 * reference function returns:
 *
 *   ed25519_verify_batch   loop of ed25519_verify        reference lib/eddsa.h:52
 *   ed25519_verify_records the same over fixed-size (sig, pub, msg) records
 *   ed25519_verify_batch_rlc  the same verdicts by batch verification (opt-in; the reference's TODO,
 *                          lib/ed25519-sha512.c:13-14)
 *   ed25519_verify_digests the same loop for callers that already hold SHA-512(R || A || M): 64 digest bytes per item instead
 *                          of the message (also _rlc, _multi and the device-pointer forms; see the declarations)
 *   ed25519_sign_batch     loop of ed25519_sign          reference lib/eddsa.h:47
 *   ed25519ctx_sign_batch / ed25519ctx_verify_batch, ed25519ph_sign_batch / ed25519ph_verify_batch   the two other variants of
 *                          RFC 8032 (a context; for ph the caller's SHA-512 prehash instead of the message): the reference has
 *                          no such functions, the semantics are stated at the declarations
 *   ed25519_genpub_batch   loop of ed25519_genpub        reference lib/eddsa.h:44
 *   x25519_batch           loop of x25519                reference lib/eddsa.h:67
 *   x25519_base_batch      loop of x25519_base           reference lib/eddsa.h:64
 *   pk_ed25519_to_x25519_batch / sk_ed25519_to_x25519_batch   reference lib/eddsa.h:77, :80
 *
 * Data layout: packed, item-major, no padding: item i of a 32-byte field lives at base + 32*i
 * (signatures: base + 64*i).  Messages are either fixed-length (msg_off == NULL: item i is
 * msgs[i*msg_len .. (i+1)*msg_len)) or ragged (msg_off[0..n]: item i is
 * msgs[msg_off[i] .. msg_off[i+1])).  Verdicts are one byte per item (1 = accept, 0 = reject).
 * The offset table must not decrease, and msg_off[n] is taken for the size of the message buffer.  A host-pointer call
 * checks its table - the span msg_off[n] - msg_off[0] (at most 2^46 bytes, not negative) before anything is touched, the
 * order of the entries chunk by chunk, before each chunk's bytes are - and returns -hipErrorInvalidValue for a bad one; a
 * table that decreases further on is found when its chunk comes up, after earlier chunks have run (outputs unspecified,
 * as on every error).  A device-pointer call cannot inspect a table in HBM without a pass of its own: its kernels CLAMP
 * every item's span into [0, msg_off[n]) and to a length >= 0 instead, so whatever the table holds no lane reads outside
 * the aligned 4-byte words that hold the bytes [msgs, msgs + msg_off[n]) (the hashing kernels load whole words: up to
 * 3 bytes before an unaligned msgs and after the last byte lie in the same word as a byte of the buffer); an item with an
 * inconsistent span is hashed over the clamped one (its verdict / signature is then meaningless, like the table).
 *
 * Two flavours of every entry point:
 *   *_batch      host pointers; copies in, runs, copies out, returns when done.
 *   *_batch_dev  device pointers (HBM-resident buffers, e.g. torch tensors' data_ptr());
 *                enqueues on `stream` (a hipStream_t passed as void*, NULL = default stream)
 *                and returns without synchronising.
 *
 * Return value: 0 on success, otherwise the negated hipError_t of the failing HIP call (the
 * reference has no error channel; a loop over it cannot fail), or EDDSA_AMD_STALLED: a kernel gave up
 * waiting for a hand-off between its own waves (seconds, where the hand-off takes a millisecond: a
 * fault on the device) - the pass's outputs are incomplete.  A host-pointer call reports it itself; a
 * device-pointer call has returned by then, and the next verify call on that device reports it instead
 * (and is not run).  On error the outputs are unspecified.  Ownership: the caller owns every buffer; the library keeps no pointer after a
 * host-pointer call returns / after the stream work of a device-pointer call completes.
 * Devices: the library keeps one engine (tables, workspaces, staging pipeline) per HIP device,
 * created on first use.  A device-pointer call runs on the device that holds its output buffer; a
 * host-pointer call runs on the default device (eddsa_amd_init; otherwise the calling thread's
 * current device at the first call); the *_multi calls run on every device of the set bound by
 * eddsa_amd_init_devices, one contiguous shard each.  Every call makes its device current for its
 * own duration and restores the caller's before it returns.
 * Threading: calls may be issued from several host threads.  Device-pointer calls on different
 * streams use different workspaces (a pool of four per device) and overlap on the GPU; calls on one
 * stream are ordered by the stream.  Host-pointer calls on one device share its staging pipeline: large
 * calls run one after the other; SMALL calls (up to 64 items, fixed-length messages - among them every call
 * of the eddsa.h single-item functions) issued by several threads at once are merged: the calls queued for
 * one operation travel as ONE launch (launches of different operations side by side) and every caller gets
 * its own results back (the reference is
 * reentrant and scales with its caller's threads, lib/eddsa.h:44-80; a GPU pass costs about 0.4 ms however
 * few items it carries).  eddsa_amd_shutdown waits for calls in flight.
 * Host memory: ordinary (malloc) memory is staged through page-locked buffers by a few copier threads
 * (eddsa_amd_set_host_threads); page-locked caller memory (eddsa_amd_host_alloc, hipHostMalloc,
 * hipHostRegister) is used in place.
 * Strict verification: by default every verdict is the reference's permissive one (S is not range-checked, the key is not
 * validated, points of order 1, 2, 4 and 8 pass as keys and as R).  The rules most strict verifiers add - S < l, a canonical
 * key, no small-order key or R - are opt-in and process-wide: EDDSA_AMD_VERIFY_*, set through eddsa_amd_set_offcurve_mode.
 * Test and measurement hooks (fault injection, route selection, probes, traces) are NOT part of this contract: they are
 * declared in eddsa_amd_debug.h and inert unless a test arms them.
 * Secrets: the staging copies of secret keys / scalars / shared secrets and the secret scalars that
 * cross kernel boundaries are zeroed in HBM before a call's stream work completes (the reference
 * wipes its stack after the same operations, lib/ed25519-sha512.c:77,136, lib/x25519.c:208,221).  A signer set
 * (eddsa_amd_signer, at the end of this header) is the one exception by design: it keeps secret scalars and prefixes in HBM from
 * eddsa_amd_signer_create* until eddsa_amd_signer_destroy, which zeroes them before it frees.
 */
#ifndef EDDSA_AMD_H
#define EDDSA_AMD_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__) && defined(EDDSA_BUILD)
#define EDDSA_AMD_DECL __attribute__((visibility("default")))
#else
#define EDDSA_AMD_DECL
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Make HIP device `device` (>= 0) the default device of the host-pointer entry points and of the
 * eddsa.h single-item functions, and build its engine: the base-point tables (what the reference
 * ships as lib/ed_lookup64.h) and the workspace pool.  Idempotent; engines of other devices stay.
 * Without it the first host-pointer call adopts the calling thread's current HIP device. */
EDDSA_AMD_DECL int eddsa_amd_init(int device);
/* Release every engine on every device (waits for calls in flight); the next call builds anew. */
EDDSA_AMD_DECL void eddsa_amd_shutdown(void);

/* ---- several devices in one process (host thread or stream per device, one result
 *      gather over RCCL/xGMI; the loop being sharded is ed25519_verify, lib/ed25519-sha512.c:148-181) ----
 * Bind the device set of the *_multi entry points: an engine on each device of `devices` (n entries,
 * no duplicates; NULL / 0 = every visible device) and, for the device-pointer form's result gather,
 * one RCCL communicator per device (ncclCommInitAll; librccl.so.1 is loaded here, not at link time).
 * Device d of the set owns items [lo, hi) = eddsa_amd_shard_bounds(n, d, count): contiguous,
 * balanced (shards differ by at most one item). */
EDDSA_AMD_DECL int eddsa_amd_init_devices(const int *devices, int n);
EDDSA_AMD_DECL int eddsa_amd_device_count(void);
EDDSA_AMD_DECL int eddsa_amd_device_at(int index);   /* the HIP device that owns shard `index` of the set, or -1 */
EDDSA_AMD_DECL void eddsa_amd_shard_bounds(size_t n, int rank, int world, size_t *lo, size_t *hi);
/* host pointers, whole batch in host memory: one host thread per device runs that device's streaming
 * pipeline on its shard and copies the results straight into the caller's buffer (no collective) */
EDDSA_AMD_DECL int ed25519_verify_batch_multi(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs,
                                              const uint8_t *msgs, const uint64_t *msg_off,
                                              size_t msg_len, size_t n);
EDDSA_AMD_DECL int ed25519_sign_batch_multi(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs,
                                            const uint8_t *msgs, const uint64_t *msg_off,
                                            size_t msg_len, size_t n);
EDDSA_AMD_DECL int x25519_batch_multi(uint8_t *out, const uint8_t *scalars, const uint8_t *points, size_t n);
/* device pointers: sigs[d] / pubs[d] / msgs[d] (fixed msg_len) hold shard d in device d's HBM,
 * ok_full[d] is a buffer of n_total bytes there, streams[d] a stream of device d (NULL entries, or
 * streams == NULL = default stream).  Shard d is verified on device d into its slice of ok_full[d]; then ONE RCCL
 * all-gather (grouped broadcasts when the shards differ in length) leaves the whole verdict vector
 * in every ok_full[d].  Enqueues and returns; the streams order the work. */
EDDSA_AMD_DECL int ed25519_verify_batch_multi_dev(uint8_t *const ok_full[], const uint8_t *const sigs[],
                                                  const uint8_t *const pubs[], const uint8_t *const msgs[],
                                                  size_t msg_len, size_t n_total, void *const streams[]);
/* Page-locked host memory for the arrays of the host-pointer entry points: such buffers are read and written by the DMA
 * engines in place, without the staging copy ordinary memory needs.  NULL when the allocation fails. */
EDDSA_AMD_DECL void *eddsa_amd_host_alloc(size_t bytes);
EDDSA_AMD_DECL void eddsa_amd_host_free(void *p);
/* helper threads that copy ordinary caller memory into the staging buffers beside the calling thread (default 6, at
 * most 16; 0 = the caller copies alone) */
EDDSA_AMD_DECL void eddsa_amd_set_host_threads(int n);
#define EDDSA_AMD_STALLED (-100003)
/* human-readable text for a negative return value */
EDDSA_AMD_DECL const char *eddsa_amd_strerror(int err);
/* How ed25519_verify* treats a public key that does not decode to a curve point (the reference's
 * ed_import never fails, lib/ed.c:100-149).  exact != 0 (default): such items are evaluated in the
 * reference's own order of operations -- the only way to reproduce its bytes for them.  exact == 0:
 * they are rejected outright, which differs from the reference only on a SHA-512 fixed point and
 * saves about 1 ms per pass that contains such keys.  exact == 2: EVERY item is evaluated in the
 * reference's order of operations (JSF/Shamir chain, lib/ed.c:455-507) and the windowed kernel's
 * result is ignored -- same verdicts, latency-bound, meant for self-checks.
 *
 * The same word carries the OPT-IN STRICT RULES in its bits 8-11 (EDDSA_AMD_VERIFY_POLICY_MASK): the call stores
 * exact & EDDSA_AMD_VERIFY_POLICY_MASK as the process-wide verify policy and reads the mode above from
 * exact & ~EDDSA_AMD_VERIFY_POLICY_MASK (2 -> 2, otherwise non-zero -> 1), both under one lock.  0, 1 and 2 therefore mean
 * what they always meant, with policy 0; a value with some of bits 8-11 set, -1 among them, used to mean "exact" and now
 * means "exact plus those rules" (-1: exact and EDDSA_AMD_VERIFY_STRICT).  Policy 0 is the default and is the reference's
 * verdict, byte for byte; no kernel is added to any pass.  The rules: */
#define EDDSA_AMD_VERIFY_S_BELOW_L     0x100   /* reject unless sig[32..64), little-endian, is < l (RFC 8032 5.1.7; S + k l is a
                                                  second encoding of the same signature) */
#define EDDSA_AMD_VERIFY_A_CANONICAL   0x200   /* reject unless the key is an encoding RFC 8032 5.1.3 decodes: y (the low 255 bits)
                                                  < p, (y^2 - 1) / (d y^2 + 1) a square, and not x = 0 with the sign bit set */
#define EDDSA_AMD_VERIFY_A_NOT_SMALL   0x400   /* reject a key with y mod p in {0, 1, -1, y8, -y8}: the eight points of order 1, 2,
                                                  4 and 8 in every encoding, the non-canonical ones included (each of these y is on
                                                  the curve, so y alone decides) */
#define EDDSA_AMD_VERIFY_R_NOT_SMALL   0x800   /* the same test on sig[0..32) */
#define EDDSA_AMD_VERIFY_STRICT        0xF00   /* all four */
#define EDDSA_AMD_VERIFY_POLICY_MASK   0xF00
/* The verdict of an item under policy P is (the reference's verdict for the item) AND (every predicate whose bit is in P): a
 * policy only ever turns accepts into rejects.  It holds for EVERY form of verification in the process - the thirteen names of
 * eddsa.h, the batched, records, digest, _rlc, _multi and device-pointer forms - so a program linked against the reference's
 * library makes one call at start-up, eddsa_amd_set_offcurve_mode(1 | EDDSA_AMD_VERIFY_STRICT), and changes no call site.  A call
 * uses the policy in force when each of its passes is enqueued, like the off-curve mode.
 * There is no R_CANONICAL bit because none is needed: an accepted R equals, byte for byte, what the reference's export step
 * wrote, and that has y < p and the sign bit of its x.  With A_CANONICAL an accepted item is thus made of canonical encodings
 * of curve points only.
 * The opt-in batch verification (ed25519_verify_batch_rlc) keeps its documented caveat under every policy: the rules reject
 * points OF small order, and a point of mixed order (a small-order component on a prime-order point) is not one of those.
 * The rules are one more kernel behind each pass's verdicts (it reads 96 bytes of an accepted item; A_CANONICAL decodes the key
 * once more).  Measured (profiles/verify_policy.txt, tools/policy_cost.py: ed25519_verify_batch_dev, 2^20 valid items in HBM,
 * 32-byte messages, one MI355X): policy 0 9.39 ms per pass, S_BELOW_L 9.44 (+0.5 %), A_NOT_SMALL 9.44 (+0.5 %), R_NOT_SMALL 9.47
 * (+0.8 %), A_CANONICAL 10.23 (+8.9 %), STRICT 10.24 (+9.0 %: 102 M instead of 112 M verifies/s).  Policy 0 against the commit
 * before the rules, alternating on that box: 9.42-9.46 ms against 9.41-9.47 ms - inside the older build's own repeat spread. */
EDDSA_AMD_DECL void eddsa_amd_set_offcurve_mode(int exact);
EDDSA_AMD_DECL void eddsa_amd_set_rlc_min_items(size_t items);   /* see ed25519_verify_batch_rlc */
/* ---- host-pointer entry points ---- */
EDDSA_AMD_DECL int ed25519_verify_batch(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs,
                                        const uint8_t *msgs, const uint64_t *msg_off, size_t msg_len,
                                        size_t n);
/* The same loop of ed25519_verify (reference lib/eddsa.h:52) over n fixed-size RECORDS, for callers
 * that hold (signature, public key, message) together: record i starts at records + i * stride and
 * has its 64-byte signature at sig_off, its 32-byte key at pub_off and its msg_len-byte message at
 * msg_off (e.g. stride 128 = sig | pub | 32-byte digest).  Fields may overlap nothing in particular
 * and need no alignment; every field must lie inside the record, otherwise hipErrorInvalidValue is
 * returned (negated).  One upload instead of three on the host path. */
EDDSA_AMD_DECL int ed25519_verify_records(uint8_t *ok, const uint8_t *records, size_t stride,
                                          size_t sig_off, size_t pub_off, size_t msg_off,
                                          size_t msg_len, size_t n);
/* OPT-IN batch verification by random linear combination: the reference's own TODO
 * (lib/ed25519-sha512.c:13-14, "batch verification"); same arguments and verdict bytes as
 * ed25519_verify_batch, about twice its rate on batches whose signatures are (nearly) all valid.
 * Groups of 8192 items are checked as  (sum z_i S_i) B - sum (z_i t_i) A_i - sum z_i R_i = 0  with
 * 126-bit odd coefficients z_i derived from a SHA-512 tree over the whole batch; a group that fails, or
 * that contains a key that is no curve point or a key / R of small order, is decided item by item by the
 * ordinary kernels, and an R that is not a canonical point encoding is rejected at once.  The verdicts
 * equal ed25519_verify_batch's whenever every A and R lies in the prime-order subgroup (all honestly
 * generated keys and signatures) -- up to a 2^-125 chance per group; crafted inputs with small-order
 * COMPONENTS in several items of one group can make the group pass although the reference's
 * cofactorless check rejects one of them.  That is why this is never the default.
 * Under the COFACTORED equation (eddsa_amd_set_verify_equation, below) that caveat does not exist: the verdicts equal the
 * per-item ones of that equation, up to 2^-125 per group, for every input; an R that is no canonical encoding then sends its
 * group to the per-item kernels instead of being rejected at once.
 * stats (4 words, may be NULL) receives: items decided by the combination, items decided per item,
 * groups sent to the per-item kernels, groups decided by the combination.
 * The device-pointer form synchronises `stream` once per pass (it reads the group verdicts).
 * The combination has about 1 ms of latency of its own (hash tree over the batch, one serial Horner per
 * group), so it pays from about 2^17 items (x1.5 at 2^18, x2.1 at 2^19, x2.2 from 2^20): calls with fewer items than
 * eddsa_amd_set_rlc_min_items (default EDDSA_AMD_RLC_MIN_ITEMS_DEFAULT; 0 = always combine) go straight to the per-item
 * kernels. */
#define EDDSA_AMD_RLC_MIN_ITEMS_DEFAULT ((size_t)5 << 15)
EDDSA_AMD_DECL int ed25519_verify_batch_rlc(uint8_t *ok, uint32_t stats[4], const uint8_t *sigs,
                                            const uint8_t *pubs, const uint8_t *msgs,
                                            const uint64_t *msg_off, size_t msg_len, size_t n);
/* Verification from CALLER-SUPPLIED DIGESTS.  The reference's ed25519_verify uses the message for one thing only,
 * t = SHA-512(R || A || M) mod l (lib/ed25519-sha512.c:165-171); a caller who has hashed already - on the thread that received
 * the message, incrementally while a large block streamed by - hands over the digest and no message byte is uploaded or hashed
 * on the device (a lane hashes 10-13 MB/s: one 1 MiB message stretches a pass of 2^16 short ones from 0.8 ms to 65 ms).
 * digests: packed, 64 bytes per item, in the order SHA-512 emits them (what hashlib.sha512(R + A + M).digest() returns), no
 * alignment required.  Item i is accepted exactly when the reference's ed25519_verify accepts (sigs[i], pubs[i], M) for an M
 * with SHA-512(R_i || A_i || M) = digests[i].  The digest's only use is t = (the 64 bytes as a little-endian integer) mod l,
 * the sc_import(t, h, 64) of lib/ed25519-sha512.c:171; any 64 bytes are legal input.  Everything else is ed25519_verify_batch's,
 * byte for byte: S is not range-checked, off-curve keys and the strict rules follow eddsa_amd_set_offcurve_mode, EDDSA_AMD_STALLED is reported as
 * there; return values, ownership, device selection, threading and page-locked memory follow the rules at the top.
 * THE CALLER VOUCHES that digests[i] was computed over the R bytes (sigs[i][0..32)) and the A bytes (pubs[i]) of THIS call,
 * followed by the message.  A digest computed over other bytes verifies a different statement, and the library cannot tell:
 * it never sees the message.
 * The _rlc forms are ed25519_verify_batch_rlc's combination with the same rules (groups of 8192, per-item fallback,
 * eddsa_amd_set_rlc_min_items, stats, one synchronisation of `stream` in the device-pointer form); the item's leaf of the batch
 * hash tree is taken from the digest bytes.  _multi shards over the device set like ed25519_verify_batch_multi.
 * These calls are never merged by the small-call combiner (like the records form): each call is a pass of its own. */
EDDSA_AMD_DECL int ed25519_verify_digests(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs,
                                          const uint8_t *digests, size_t n);
EDDSA_AMD_DECL int ed25519_verify_digests_rlc(uint8_t *ok, uint32_t stats[4], const uint8_t *sigs,
                                              const uint8_t *pubs, const uint8_t *digests, size_t n);
EDDSA_AMD_DECL int ed25519_verify_digests_multi(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs,
                                                const uint8_t *digests, size_t n);
EDDSA_AMD_DECL int ed25519_sign_batch(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs,
                                      const uint8_t *msgs, const uint64_t *msg_off, size_t msg_len,
                                      size_t n);
EDDSA_AMD_DECL int ed25519_genpub_batch(uint8_t *pubs, const uint8_t *secs, size_t n);
EDDSA_AMD_DECL int x25519_batch(uint8_t *out, const uint8_t *scalars, const uint8_t *points, size_t n);
EDDSA_AMD_DECL int x25519_base_batch(uint8_t *out, const uint8_t *scalars, size_t n);
EDDSA_AMD_DECL int pk_ed25519_to_x25519_batch(uint8_t *out, const uint8_t *in, size_t n);
EDDSA_AMD_DECL int sk_ed25519_to_x25519_batch(uint8_t *out, const uint8_t *in, size_t n);

/* ---- device-pointer entry points (asynchronous on `stream`) ---- */
EDDSA_AMD_DECL int ed25519_verify_batch_dev(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs,
                                            const uint8_t *msgs, const uint64_t *msg_off,
                                            size_t msg_len, size_t n, void *stream);
EDDSA_AMD_DECL int ed25519_verify_records_dev(uint8_t *ok, const uint8_t *records, size_t stride,
                                              size_t sig_off, size_t pub_off, size_t msg_off,
                                              size_t msg_len, size_t n, void *stream);
EDDSA_AMD_DECL int ed25519_verify_batch_rlc_dev(uint8_t *ok, uint32_t *stats /* device, 4 words, or NULL */,
                                                const uint8_t *sigs, const uint8_t *pubs,
                                                const uint8_t *msgs, const uint64_t *msg_off,
                                                size_t msg_len, size_t n, void *stream);
/* caller-supplied digests (see ed25519_verify_digests): digests in HBM, 64 bytes per item, any alignment */
EDDSA_AMD_DECL int ed25519_verify_digests_dev(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs,
                                              const uint8_t *digests, size_t n, void *stream);
EDDSA_AMD_DECL int ed25519_verify_digests_rlc_dev(uint8_t *ok, uint32_t *stats /* device, 4 words, or NULL */,
                                                  const uint8_t *sigs, const uint8_t *pubs,
                                                  const uint8_t *digests, size_t n, void *stream);
EDDSA_AMD_DECL int ed25519_sign_batch_dev(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs,
                                          const uint8_t *msgs, const uint64_t *msg_off,
                                          size_t msg_len, size_t n, void *stream);
EDDSA_AMD_DECL int ed25519_genpub_batch_dev(uint8_t *pubs, const uint8_t *secs, size_t n, void *stream);
EDDSA_AMD_DECL int x25519_batch_dev(uint8_t *out, const uint8_t *scalars, const uint8_t *points,
                                    size_t n, void *stream);
EDDSA_AMD_DECL int x25519_base_batch_dev(uint8_t *out, const uint8_t *scalars, size_t n, void *stream);
EDDSA_AMD_DECL int pk_ed25519_to_x25519_batch_dev(uint8_t *out, const uint8_t *in, size_t n, void *stream);
EDDSA_AMD_DECL int sk_ed25519_to_x25519_batch_dev(uint8_t *out, const uint8_t *in, size_t n, void *stream);

/* ---- Ed25519ctx and Ed25519ph: the two other variants of RFC 8032 (section 5.1), batched ----
 * Both are Ed25519 with dom2(F, C) = "SigEd25519 no Ed25519 collisions" (32 ASCII bytes) || F || len(C) || C in front of the two
 * hashes that see the message (RFC 8032 section 2), C a context of 0..255 bytes:
 *   sign     h = SHA-512(sk), clamped as in ed25519_sign_batch;  r = SHA-512(dom2 || h[32..64) || M') mod l;  R = r B;
 *            t = SHA-512(dom2 || R || A || M') mod l;  S = r + t a       (reference lib/ed25519-sha512.c:84-122 with the prefix)
 *   verify   item i is accepted exactly when ed25519_verify_digests accepts (sigs[i], pubs[i], SHA-512(dom2 || R || A || M')):
 *            the reference's permissive check with t from the prefixed hash.  The off-curve mode and the strict rules of
 *            eddsa_amd_set_offcurve_mode apply unchanged, EDDSA_AMD_STALLED is reported as for every verify form.
 *   Ed25519ctx  F = 0, M' = the message (fixed-length or ragged, as in ed25519_sign_batch / ed25519_verify_batch).
 *   Ed25519ph   F = 1, M' = SHA-512(M): THE CALLER supplies these 64 bytes per item (prehashes: packed, any alignment, what
 *               hashlib.sha512(M).digest() returns) and the library never sees M.  A signer or verifier of large objects hashes
 *               each object once, wherever its bytes stream by; the device then spends three to five SHA-512 blocks on an item
 *               whatever the size of M, where ed25519_sign_batch hashes M twice at 10-13 MB/s per lane and cannot be handed a
 *               digest (r needs the secret prefix).  The ph forms are the ctx forms with F = 1, msg_len 64 and no offset table.
 * context: a HOST pointer in every form, the device-pointer ones too; one context per call; it is copied during the call and
 * may be freed on return.  NULL is allowed with context_len 0.  An empty context is legal under both flags - RFC 8032 says
 * a context SHOULD NOT be empty for Ed25519ctx - and dom2(0, "") is still not plain Ed25519: the three variants never accept
 * one another's signatures.  context_len > 255 returns -hipErrorInvalidValue before anything is touched.
 * Everything else - layout, ragged-table rules and clamping, return values, device selection, ownership, threading, page-locked
 * memory, the wiping of secrets - follows the rules at the top.  Host-pointer calls go through the staging pipeline and are
 * never merged by the small-call combiner (two calls may carry different contexts).  Out of scope: _rlc, _multi and records
 * forms, and single-item convenience names.
 * Measured (profiles/dom2.txt, tools/dom2_rate.py: device-pointer forms, 2^20 valid items in HBM, a 3-byte context, one MI355X,
 * the forms alternating): verify 9.65 ms per pass as Ed25519 over 32-byte messages, 9.84 ms as Ed25519ctx over the same (+2.0 %),
 * 9.86 ms as Ed25519ph over 64-byte prehashes (+2.2 %); sign 2.21 / 2.36 (+7 %) / 2.49 ms (+13 %: two more SHA-512 blocks per item
 * than a 32-byte Ed25519 message needs).  What the ph form is for: 2^16 items of which one in 1024 is 1 MiB take ed25519_sign_batch_dev
 * 124 ms and ed25519ph_sign_batch_dev 0.275 ms on their prehashes - the caller's own hashing of the objects not included.
 * (Declared with a macro of their own, the same attribute: tests of earlier additions count the EDDSA_AMD_DECL names above.) */
#if defined(__GNUC__) && defined(EDDSA_BUILD)
#define RFC8032_EDDSA_DECL __attribute__((visibility("default")))
#else
#define RFC8032_EDDSA_DECL
#endif
RFC8032_EDDSA_DECL int ed25519ctx_sign_batch(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs, const uint8_t *msgs,
                                             const uint64_t *msg_off, size_t msg_len, size_t n,
                                             const uint8_t *context, size_t context_len);
RFC8032_EDDSA_DECL int ed25519ctx_verify_batch(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs, const uint8_t *msgs,
                                               const uint64_t *msg_off, size_t msg_len, size_t n,
                                               const uint8_t *context, size_t context_len);
RFC8032_EDDSA_DECL int ed25519ph_sign_batch(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs,
                                            const uint8_t *prehashes /* 64 bytes per item */, size_t n,
                                            const uint8_t *context, size_t context_len);
RFC8032_EDDSA_DECL int ed25519ph_verify_batch(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs,
                                              const uint8_t *prehashes /* 64 bytes per item */, size_t n,
                                              const uint8_t *context, size_t context_len);
/* device pointers (the context stays a host pointer): enqueue on `stream` and return */
RFC8032_EDDSA_DECL int ed25519ctx_sign_batch_dev(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs, const uint8_t *msgs,
                                                 const uint64_t *msg_off, size_t msg_len, size_t n,
                                                 const uint8_t *context, size_t context_len, void *stream);
RFC8032_EDDSA_DECL int ed25519ctx_verify_batch_dev(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs, const uint8_t *msgs,
                                                   const uint64_t *msg_off, size_t msg_len, size_t n,
                                                   const uint8_t *context, size_t context_len, void *stream);
RFC8032_EDDSA_DECL int ed25519ph_sign_batch_dev(uint8_t *sigs, const uint8_t *secs, const uint8_t *pubs,
                                                const uint8_t *prehashes, size_t n,
                                                const uint8_t *context, size_t context_len, void *stream);
RFC8032_EDDSA_DECL int ed25519ph_verify_batch_dev(uint8_t *ok, const uint8_t *sigs, const uint8_t *pubs,
                                                  const uint8_t *prehashes, size_t n,
                                                  const uint8_t *context, size_t context_len, void *stream);

/* ---- the equation an item is held to: cofactorless (the reference's, default) or COFACTORED (the rules of ZIP-215) ----
 * Opt-in and process-wide, like the strict rules, but a call of its own: eddsa_amd_set_offcurve_mode's word, its policy mask and
 * what its values mean are untouched.  Returns 0, or -hipErrorInvalidValue for any value other than the two below, in which
 * case the setting stays what it was.  A call uses the equation in force when each of its passes is enqueued, under the same
 * lock as the off-curve mode and the policy.
 * Under EDDSA_AMD_EQUATION_COFACTORED an item is accepted exactly when ALL of these hold:
 *   - sig[32..64), read little-endian, is below l;
 *   - A (pub) decodes: y = the low 255 bits mod p (a non-canonical y counts), (y^2 - 1) / (d y^2 + 1) is a square, x takes the
 *     sign bit, and x = 0 with the sign bit set is accepted as x = 0;
 *   - R (sig[0..32)) decodes by the same rule;
 *   - [8]([S]B - [t]A - R) is the neutral element, t = SHA-512(R || A || M) mod l over the bytes as given (the digest forms:
 *     t from the caller's 64 bytes; Ed25519ctx / Ed25519ph: t from the dom2-prefixed hash - as for the cofactorless check).
 * A key or an R that is no curve point is rejected: off-curve modes 0 and 1 then give the same verdicts (mode 1 runs as mode 0
 * and the reference-order chain is not launched; mode 2 keeps its meaning as a self-check).  The strict rules compose as they
 * do with the reference's check: the verdict is (the cofactored verdict) AND (every predicate of the policy) - A_NOT_SMALL on
 * top of this equation rejects every small-order key, for instance.  The setting holds for EVERY form of verification: the
 * thirteen names of eddsa.h (calls merged by the small-call combiner included), the batched, records and digest forms,
 * Ed25519ctx and Ed25519ph, _rlc, _multi and the device-pointer forms.
 * Why: this is the one per-item rule under which single and batch verification always agree, which is what nodes that must
 * reach the same verdict need.  Under it ed25519_verify_batch_rlc's verdicts EQUAL the per-item ones, up to 2^-125 per group,
 * for EVERY input: the caveat in that function's description (crafted small-order components) is gone, because a group the
 * combination accepts consists - up to that bound - of items this equation accepts, and a group that fails, or that holds a
 * key or an R of small order, a key off the curve or an R that is no canonical encoding, is decided item by item by this rule.
 * How: the pass runs unchanged (full-length route, off-curve keys rejected, S < l added to the policy kernel); what it accepts
 * this equation accepts too, so only the items it REJECTED are listed and evaluated again, one lane each: the same 252
 * doublings and 80 additions, - R added, three doublings and a projective neutrality test (no inversion).  With the
 * cofactorless equation nothing is queued and no kernel's arguments change.
 * Measured (profiles/verify_cofactored.txt, tools/cofactored_cost.py: ed25519_verify_batch_dev, 2^20 items in HBM, 32-byte
 * messages, one MI355X, the rows alternating): equation 0 9.51 ms per pass; cofactored, every item valid 10.55 ms (+11 %: the
 * full-length route of the reject mode, the listing kernel, S < l); with 1 % of the items rejected 11.87 ms (+25 %: the one-lane
 * evaluation of a short list costs its latency, 1.3 ms, behind the pass - a four-lane form for short lists is a follow-up);
 * with EVERY item rejected, the worst case a caller can construct, 22.20 ms (+134 %: a second full-length evaluation, 47 M
 * items/s); _rlc on valid items 4.40 ms against 4.38 (+0.4 %).  Equation 0 against the commit before the equation, alternating
 * on that box: 9.48-9.49 ms against 9.48-9.49 ms - inside the older build's own repeat spread.
 * (Declared with the macro of the RFC 8032 variants: tests of earlier additions count the EDDSA_AMD_DECL names.) */
#define EDDSA_AMD_EQUATION_COFACTORLESS 0
#define EDDSA_AMD_EQUATION_COFACTORED   1
RFC8032_EDDSA_DECL int eddsa_amd_set_verify_equation(int equation);

/* ---- KEY SETS: register the public keys once, verify by key index ----
 * For callers whose signatures come from a few hundred or a few thousand keys known in advance (validator sets).  Every other
 * form takes 32 key bytes per item and, per item, decompresses the key (a square root), builds the table 0..8 * (-A), writes its
 * 1152 bytes into the workspace and reads them back 34 times.  A key set does that once per KEY: it holds, in HBM, the key
 * bytes, one flag byte per key (the key decodes to a curve point) and 1152 bytes of table per key - 1.1 MB for 1024 keys - and
 * a keyed pass takes all three by index; the host-pointer form uploads 4 bytes per item where ed25519_verify_batch uploads 32.
 * Verdicts: ok[i] is byte for byte what ed25519_verify_batch returns for (sigs[i], keys[key_idx[i]], message i), under the
 *   off-curve mode (0, 1, 2), the strict rules and the equation in force when each pass is enqueued; the settings in force when
 *   the key set was created play no part.  A key set holds ANY 32-byte strings - strings that are no curve point, non-canonical
 *   encodings, small-order points: the reference's ed_import never fails, and neither does registration.
 * Out-of-range indices: an item with key_idx[i] >= count is rejected (ok[i] = 0) under every setting, in both forms; nothing is
 *   read outside the key set for it, and the verdicts of its neighbours are unaffected.
 * Creating: eddsa_amd_keyset_create takes a host pointer and runs on the default device (the rule of the host-pointer calls);
 *   eddsa_amd_keyset_create_dev takes a device pointer and runs on the device that holds `keys`.  Both return once the tables are
 *   built (create_dev synchronises `stream`); the caller's `keys` may be freed then.  count == 0,
 *   count > EDDSA_AMD_KEYSET_MAX_KEYS, out == NULL or keys == NULL return -hipErrorInvalidValue and leave *out NULL (where out
 *   is not NULL itself), before any device is touched.  On every other error *out is NULL too.
 * Ownership and lifetime: a key set is immutable after creation and may be used by any number of threads and streams at once;
 *   no pass writes it.  It owns its HBM, SURVIVES eddsa_amd_shutdown, and is freed only by eddsa_amd_keyset_destroy (NULL
 *   allowed), which synchronises the key set's device before it frees: destroy it after the last call that uses it has returned.
 * Devices: a device-pointer call whose `ok` lies on another device than the key set returns -hipErrorInvalidValue; a
 *   host-pointer call runs on the key set's device.
 * key_idx: packed uint32, one per item, host memory in ed25519_verify_keyed and HBM in ed25519_verify_keyed_dev.  Everything
 *   else - layout, ragged-table rules and clamping, return values, EDDSA_AMD_STALLED, page-locked memory, threading - follows the
 *   rules at the top.  Host-pointer keyed calls are never merged by the small-call combiner (two calls may carry two key sets).
 * Routes: a keyed pass always takes the one-lane kernels, whatever its size (half-length scalars in off-curve modes 1 and 2,
 *   full-length windows in mode 0 and under the cofactored equation): the four-lane forms that serve unkeyed passes below 2^18
 *   items have no keyed counterpart, so a SMALL keyed pass pays the latency of the one-lane forms: 0.58-0.64 ms from 1 to 2^16
 *   items, where the unkeyed pass takes 0.27-0.36 ms up to 2^14 - the two meet at about 2^16 items (profiles/verify_keyed.txt).
 *   An item that needs the reference-order chain (a key off the curve in mode 1, every item in mode 2, an item without a short
 *   scalar pair) gets a table of its own in the workspace, as in an unkeyed pass.
 * Out of scope: _rlc, _multi, records, digest, Ed25519ctx / Ed25519ph and single-item forms; tables wider than nine entries.
 *   (Of these, _rlc has since been added for the message form: ed25519_verify_keyed_rlc, further down; the digest forms with
 *   their _rlc, Ed25519ctx and Ed25519ph at the end of this header: ed25519_verify_keyed_digests and its neighbours.)
 * Measured (profiles/verify_keyed.txt, tools/keyed_rate.py: device-pointer forms, 2^20 valid items in HBM, 32-byte messages, one
 * MI355X, the two passes alternating, repeat spread 0.03-0.04 ms): items under 1024 distinct keys 9.44 ms per pass through
 * ed25519_verify_batch_dev, 8.31 ms through ed25519_verify_keyed_dev (-12.0 %: 126 M instead of 111 M verifies/s); under ONE key
 * 9.51 / 8.23 ms (-13.4 %), under 2^16 keys 9.43 / 8.43 ms (-10.6 %), under 2^20 distinct keys - a 1.2 GB key set read in random
 * order - 9.45 / 8.55 ms (-9.6 %).  The gain is the square root and the table store that the prepare kernel no longer does (the
 * kernels in front of the main kernel: 2.68 -> 1.65 ms); the main kernel itself gains 1.8 % from tables that stay in L2.  Host to
 * host, 1024 keys, ordinary memory: 10.26 -> 9.04 ms (-11.9 %).  eddsa_amd_keyset_create: 0.11 ms for 1024 keys, 1.75 ms for 2^20.
 * ed25519_verify_batch_dev against the commit before key sets, alternating on that box: 9.413 ms against 9.407 (that build's own
 * repeats: 9.376-9.419).
 * (Declared with the macro of the RFC 8032 variants: tests of earlier additions count the EDDSA_AMD_DECL names.) */
typedef struct eddsa_amd_keyset eddsa_amd_keyset;          /* opaque */
#define EDDSA_AMD_KEYSET_MAX_KEYS ((size_t)1 << 20)
RFC8032_EDDSA_DECL int eddsa_amd_keyset_create(eddsa_amd_keyset **out, const uint8_t *keys /* host, 32 bytes per key */, size_t count);
RFC8032_EDDSA_DECL int eddsa_amd_keyset_create_dev(eddsa_amd_keyset **out, const uint8_t *keys /* device */, size_t count, void *stream);
RFC8032_EDDSA_DECL void eddsa_amd_keyset_destroy(eddsa_amd_keyset *ks);
RFC8032_EDDSA_DECL size_t eddsa_amd_keyset_count(const eddsa_amd_keyset *ks);
RFC8032_EDDSA_DECL int eddsa_amd_keyset_device(const eddsa_amd_keyset *ks);   /* the HIP device that holds the key set */
RFC8032_EDDSA_DECL int ed25519_verify_keyed(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                                            const uint8_t *msgs, const uint64_t *msg_off, size_t msg_len, size_t n);
RFC8032_EDDSA_DECL int ed25519_verify_keyed_dev(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                                                const uint8_t *msgs, const uint64_t *msg_off, size_t msg_len, size_t n, void *stream);

/* ---- KEY SETS, BATCH VERIFICATION: ed25519_verify_batch_rlc with item i's key taken from a key set ----
 * OPT-IN like ed25519_verify_batch_rlc, for the same callers as key sets: large batches of valid signatures from a few hundred or
 * a few thousand known keys.  The combination of a group of 8192 items is the unkeyed one with the key terms collected per key,
 *     (sum z_i S_i) B  +  sum_k (sum_{i: key_idx[i] = k} z_i t_i mod 8 l) (-A_k)  +  sum_i z_i (-R_i)  =  0,
 * so its key side has `count` points per group and window instead of 8192, and a pass decompresses at most `count` keys
 * instead of one per item.
 * Verdicts: ok[i] is what ed25519_verify_batch_rlc returns for (sigs[i], keys[key_idx[i]], message i): the same off-curve mode,
 *   strict rules and equation (those in force when each pass is enqueued), the same bound of 2^-125 per group and the same
 *   caveat under the cofactorless equation (two or more crafted items of small-order defect in one group may cancel).  Under
 *   the cofactored equation the verdicts equal the per-item verdicts for every input, as in the unkeyed form.
 * Out-of-range indices: an item with key_idx[i] >= count gets ok[i] = 0 under every setting; nothing outside the key set is
 *   read for it, it contributes to no sum, it does not send its group to the per-item kernels, and its neighbours' verdicts are
 *   unaffected.
 * Per-item route: a group that fails, a group with an item that refers to a key that is off the curve or of small order, a
 *   group that holds an R of small order and, under the cofactored equation, a group that holds an R that is no canonical
 *   encoding are decided by the kernels of ed25519_verify_keyed, and `stats` says so (the four counters of
 *   ed25519_verify_batch_rlc).  A key set may CONTAIN such keys: a group with no item that refers to one is still combined.
 * Large key sets: a key set of more than 8192 keys is not combined - the digit rows and bucket lists of a pass index 8192
 *   entries per group; the call runs as ed25519_verify_keyed and reports every item as decided per item.  Wider sets are out
 *   of scope here.
 * Small calls: calls of fewer items than eddsa_amd_set_rlc_min_items go to the keyed per-item kernels - one knob for the keyed
 *   and the unkeyed form.  Measured crossover under 1024 keys: the keyed combination takes 1.03 ms for 2^16 items where the keyed
 *   per-item pass takes 0.65 ms, and 1.20 ms for 2^17 where that pass takes 1.48 ms; the default threshold lies above it.
 * Workspace: 64 bytes per item of workspace capacity (the per-key accumulators) and 1 MiB + 8 KiB (the pass's key points and
 *   flags) on top of the unkeyed form's, allocated with it.
 * Everything else follows ed25519_verify_keyed and ed25519_verify_batch_rlc where each covers the point: layout, ragged-table
 *   rules and clamping, EDDSA_AMD_STALLED and return values; a key set or `ok` on the wrong device, NULL arguments, ownership
 *   and threading; never merged by the small-call combiner; the device form synchronises `stream` once per pass.
 * Still out of scope: the digest, records, _multi, Ed25519ctx / Ed25519ph and single-item forms of keyed verification.
 *   (Of these, the digest forms - with their own _rlc - and Ed25519ctx / Ed25519ph have since been added: ed25519_verify_keyed_digests
 *   and its neighbours, at the end of this header.)
 * Measured (profiles/verify_keyed_rlc.txt, tools/keyed_rlc_rate.py: the three device-pointer forms alternating over the same 2^20
 * valid items in HBM, 32-byte messages, one MI355X, repeat spread 0.01-0.04 ms for the two combinations): under 1024 keys 3.11 ms
 * per pass against 4.47 ms through ed25519_verify_batch_rlc_dev (-30 %: 337 M instead of 235 M verifies/s) and 8.71 ms through
 * ed25519_verify_keyed_dev; under ONE key 2.74 against 4.43 ms (-38 %); under 8192 keys 3.97 against 4.46 ms (-11 %).  The gain is
 * the per-item square root of the key (k_rlc_points 1.79 -> 0.95 ms) and the -A windows of the bucket launch (2.47 -> 1.52 ms),
 * less 0.3 ms for the per-key sums.  The two existing calls against the commit before this one, alternating on that box: 4.463
 * against 4.465 ms and 8.700 against 8.714 ms, inside the older build's own repeats. */
RFC8032_EDDSA_DECL int ed25519_verify_keyed_rlc(uint8_t *ok, uint32_t stats[4], const eddsa_amd_keyset *ks, const uint32_t *key_idx,
                                                const uint8_t *sigs, const uint8_t *msgs, const uint64_t *msg_off, size_t msg_len, size_t n);
RFC8032_EDDSA_DECL int ed25519_verify_keyed_rlc_dev(uint8_t *ok, uint32_t *stats /* device or NULL */, const eddsa_amd_keyset *ks,
                                                    const uint32_t *key_idx, const uint8_t *sigs, const uint8_t *msgs,
                                                    const uint64_t *msg_off, size_t msg_len, size_t n, void *stream);

/* ---- KEY SETS WITH A COMB PER KEY: verify without the doubling chain ----
 * OPT-IN at creation, for key sets of up to 2^14 keys.  A plain key set saves the per-item square root and table, but every valid
 * item still runs the full chain (132 doublings and about 84 additions on the half-length route, 252 and 80 on the full-length
 * one).  A key known in advance allows fixed-base arithmetic for BOTH scalars: the 6-bit signed comb that signing uses for B
 * (44 lookups, 6 doublings), built once per key on -A, makes S B - t A cost 88 additions and 6 doublings - no half-length
 * scalars, no decompression of R, no per-item table.
 * What a comb key set is: a key set.  It holds everything a plain one holds (key bytes, flags, the nine-entry tables: the exact
 *   path, the cofactored kernels and _rlc read those) and, on top, 704 entries of 128 bytes per key: 88 KiB of HBM per key, 88 MiB
 *   for 1024 keys, 1.375 GiB at the limit of EDDSA_AMD_KEYSET_COMB_MAX_KEYS = 2^14 keys.  eddsa_amd_keyset_bytes reports the HBM a
 *   set holds (plain sets too), eddsa_amd_keyset_is_comb whether it has the comb.  Callers with more keys use a plain set.
 * Every call that takes a key set accepts it - ed25519_verify_keyed[_dev], ed25519_verify_keyed_rlc[_dev]; there is no new verify
 *   entry point.  A keyed pass over a comb set takes the comb route in every mode (off-curve modes 0, 1 and 2) and at every size:
 *   the keyed prepare kernel, one main kernel that reads S B through the library's comb of B and t (-A) through the key's comb,
 *   and the finish kernel of the full-length route; in modes 1 and 2 the exact path serves the keys off the curve (mode 2: every
 *   item) as on that route.  The route is what the caller chose at creation: there is no size switch.  The combination of
 *   ed25519_verify_keyed_rlc does not use the comb; the groups it sends to the per-item kernels take the comb route.
 * Verdicts: ok[i] is byte for byte what ed25519_verify_keyed returns over a plain key set of the same keys: in every mode,
 *   under every strict rule and under both equations; out-of-range indices are rejected as there.
 * The S reduction: S is not range-checked by default and may be any 256-bit string, while the comb covers 264 bits of S + offset;
 *   the comb's digits are cut from S mod l (B has order l: (S mod l) B = S B), which every route's prepare kernel computes.  Under
 *   the strict rules and the cofactored equation S < l is checked on the raw signature bytes, as for every other route.
 * Creating: eddsa_amd_keyset_create_comb / _create_comb_dev follow eddsa_amd_keyset_create / _create_dev - count == 0,
 *   count > EDDSA_AMD_KEYSET_COMB_MAX_KEYS, out == NULL or keys == NULL return -hipErrorInvalidValue and leave *out NULL, before any
 *   device is touched; a failed allocation returns its HIP error with *out NULL.  Lifetime, devices, eddsa_amd_keyset_destroy and
 *   "survives eddsa_amd_shutdown" are those of a plain key set; the four functions above and plain key sets behave as before.
 * Out of scope: four-lane forms of the comb route, combs wider than 6 bits, the digest, records, _multi and ctx / ph keyed forms.
 *   (The digest and ctx / ph keyed forms have since been added and take the comb route over a comb set: the end of this header.)
 * Measured (profiles/verify_keyed_comb.txt, tools/keyed_comb_rate.py: device-pointer forms over the same 2^20 valid items in HBM,
 * 32-byte messages, one MI355X, ed25519_verify_batch_dev / ed25519_verify_keyed_dev over a plain set / the same call over a comb
 * set alternating, repeat spread 0.01-0.14 ms): under 1024 keys 9.95 / 8.78 / 3.84 ms per pass in mode 1 (-56 % against the plain
 * set: 273 M instead of 119 M verifies/s), 11.02 / 9.48 / 3.79 ms in mode 0 (-60 %), 11.07 / 9.53 / 3.83 ms under the cofactored
 * equation (-60 %); under ONE key 9.82 / 8.62 / 3.72 ms; under 16 384 keys - a 1.4 GiB comb read in random order - 9.95 / 8.85 /
 * 4.21 ms (-52 %).  Per kernel under 1024 keys: prepare 0.23 ms (the plain route: 1.69 with halve), main 3.44 ms (7.02), finish
 * 0.17 ms.  Small passes under 1024 keys (unkeyed / plain / comb): 2^7 items 0.24 / 0.58 / 0.32 ms, 2^10 0.26 / 0.59 / 0.33,
 * 2^14 0.33 / 0.60 / 0.34, 2^16 0.64 / 0.62 / 0.35 - the comb route closes most of the small-pass gap of key sets but is NOT
 * faster than the unkeyed four-lane kernels up to 2^14 items (+32 % at 2^7, +4 % at 2^14); the crossover lies between 2^14 and
 * 2^16 items, and against a plain key set the comb route is faster at every size and key count measured.
 * eddsa_amd_keyset_create_comb from host keys: 0.79 ms for 1024 keys (89.2 MiB held), 3.8-114 ms for 16 384 keys (1426.5 MiB
 * held; the allocation dominates and varies), where the plain sets take 0.10 and 0.14 ms.  The two unchanged calls against the
 * commit before this one, alternating in fresh processes on that box: 9.923 against 9.917 ms (that build's own repeats:
 * 9.870-10.021) and 8.708 against 8.725 ms (8.690-8.802). */
#define EDDSA_AMD_KEYSET_COMB_MAX_KEYS ((size_t)1 << 14)     /* 88 KiB per key: 1.375 GiB at the limit */
RFC8032_EDDSA_DECL int eddsa_amd_keyset_create_comb(eddsa_amd_keyset **out, const uint8_t *keys /* host */, size_t count);
RFC8032_EDDSA_DECL int eddsa_amd_keyset_create_comb_dev(eddsa_amd_keyset **out, const uint8_t *keys /* device */, size_t count, void *stream);
RFC8032_EDDSA_DECL int eddsa_amd_keyset_is_comb(const eddsa_amd_keyset *ks);   /* 1 / 0; NULL: 0 */
RFC8032_EDDSA_DECL size_t eddsa_amd_keyset_bytes(const eddsa_amd_keyset *ks);  /* HBM the set holds; NULL: 0 */

/* ---- KEY SETS: the digest, Ed25519ctx and Ed25519ph forms ----
 * The forms of verification that take something other than plain Ed25519 over message bytes, over a key set: caller-supplied
 * digests (ed25519_verify_digests, ed25519_verify_digests_rlc) and the two context variants of RFC 8032 5.1
 * (ed25519ctx_verify_batch, ed25519ph_verify_batch), with `pubs` replaced by a key set and one uint32 index per item.  A caller
 * that hashes its messages while they stream in, or signs under a domain-separating context, keeps what the key set buys: no
 * per-item square root and table, the comb route over a comb set, one scalar per key in the combination.
 * Verdicts: ok[i] is byte for byte what the unkeyed form of the same name returns for (sigs[i], keys[key_idx[i]], digest /
 *   message / prehash i) - ed25519_verify_digests, ed25519_verify_digests_rlc, ed25519ctx_verify_batch, ed25519ph_verify_batch -
 *   under the off-curve mode (0, 1, 2), the strict rules and the equation in force when each pass is enqueued, over plain key sets
 *   and over comb key sets.  A comb set takes the comb route in the per-item forms; the combination does not use the comb, and
 *   the groups it sends to the per-item kernels take the comb route, as in ed25519_verify_keyed_rlc.
 * The digest forms: the caller vouches that digests[i] = SHA-512(R_i || keys[key_idx[i]] || M_i) - the statement of
 *   ed25519_verify_digests with the key set's bytes in the place of pubs[i]; any 64 bytes are legal input, and a digest over other
 *   bytes (another key's, say) is simply verified as the challenge it is: the item is rejected, its neighbours are not affected.
 * Out-of-range indices: key_idx[i] >= count gives ok[i] = 0 under every setting, and nothing outside the key set is read for
 *   that item.  In the _rlc form it contributes to no sum and does not send its group to the per-item kernels.  In the ctx / ph
 *   forms its challenge hash runs over the bytes that stand for "no key" in every keyed pass (02 00 .. 00, a string that is no
 *   curve point), so the cofactored re-evaluation rejects it too.
 * Everything else follows the existing key-set forms: a key set or `ok` on the wrong device returns -hipErrorInvalidValue; NULL
 *   arguments (ks, ok, key_idx, sigs, digests / prehashes, fixed-length messages) are checked before any device is touched;
 *   host-pointer calls run on the key set's device and are never merged by the small-call combiner; a key set of more than 8192
 *   keys makes the _rlc form run as the per-item form, with every item counted as decided per item; eddsa_amd_set_rlc_min_items
 *   governs the _rlc form as it does the other two; the _rlc device form synchronises `stream` once per pass; `context` is a host
 *   pointer in every form, and context_len > 255 (or a NULL context with a length) returns -hipErrorInvalidValue before anything
 *   is touched.  The host-pointer forms upload 64 bytes of signature, 4 of index and 64 of digest or prehash per item.
 * Kernels: the keyed prepare kernel and the keyed hash kernel of the combination in digest forms that take t from the 64 bytes
 *   unhashed, and one kernel in front of the ctx / ph pass that hashes dom2 || R || keys[key_idx] || M' per item; everything
 *   behind them is the keyed pass as it was.  The seed and the coefficients of a keyed digest combination equal those of
 *   ed25519_verify_digests_rlc over the expanded keys (the leaf is SHA-512(digest || S) in both).
 * Out of scope: _rlc forms of ctx / ph (the unkeyed forms have none either); _multi, records and single-item keyed forms.
 * Measured (profiles/verify_keyed_forms.txt, tools/keyed_forms_rate.py: device-pointer forms alternating over the same 2^20 valid
 * items in HBM under 1024 keys, one MI355X, repeat spread 0.01-0.07 ms): digests against 32-byte messages 8.47 against 8.49 ms over
 * a plain set, 3.73 against 3.73 ms over a comb set (281 M verifies/s), 2.98 against 3.09 ms in the combination (352 M verifies/s) -
 * no digest form is slower than its message form.  Ed25519ctx / Ed25519ph over a plain set 8.77 / 8.79 ms (+3.6 / +3.9 % on the
 * keyed message form, -10.5 % on the unkeyed ctx / ph forms), over a comb set 4.02 / 4.00 ms (+7.3 / +6.6 %, -59 %): the hashing
 * kernel in front costs 0.25-0.3 ms, against 0.2 ms in the unkeyed forms.  What the forms are for - 2^16 items of which one in
 * 1024 is 1 MiB long, over a comb set: 62.0 ms through ed25519_verify_keyed_dev, 0.37 ms from the caller's digests and 0.38 ms from
 * its prehashes (the caller's own hashing, done while the messages stream in, is in neither figure).  The unchanged calls against
 * the commit before this one, alternating in fresh processes on that box: 9.639 against 9.652 ms (ed25519_verify_batch_dev), 8.485
 * against 8.481 and 3.753 against 3.750 ms (ed25519_verify_keyed_dev, plain and comb), 3.088 against 3.091 ms
 * (ed25519_verify_keyed_rlc_dev), each inside the older build's own repeats. */
RFC8032_EDDSA_DECL int ed25519_verify_keyed_digests(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                                                    const uint8_t *digests /* 64 bytes per item */, size_t n);
RFC8032_EDDSA_DECL int ed25519_verify_keyed_digests_dev(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                                                        const uint8_t *digests, size_t n, void *stream);
RFC8032_EDDSA_DECL int ed25519_verify_keyed_digests_rlc(uint8_t *ok, uint32_t stats[4], const eddsa_amd_keyset *ks, const uint32_t *key_idx,
                                                        const uint8_t *sigs, const uint8_t *digests, size_t n);
RFC8032_EDDSA_DECL int ed25519_verify_keyed_digests_rlc_dev(uint8_t *ok, uint32_t *stats /* device or NULL */, const eddsa_amd_keyset *ks,
                                                            const uint32_t *key_idx, const uint8_t *sigs, const uint8_t *digests, size_t n,
                                                            void *stream);
RFC8032_EDDSA_DECL int ed25519ctx_verify_keyed(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                                               const uint8_t *msgs, const uint64_t *msg_off, size_t msg_len, size_t n,
                                               const uint8_t *context /* host */, size_t context_len);
RFC8032_EDDSA_DECL int ed25519ctx_verify_keyed_dev(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                                                   const uint8_t *msgs, const uint64_t *msg_off, size_t msg_len, size_t n,
                                                   const uint8_t *context /* host */, size_t context_len, void *stream);
RFC8032_EDDSA_DECL int ed25519ph_verify_keyed(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                                              const uint8_t *prehashes /* 64 bytes per item */, size_t n,
                                              const uint8_t *context /* host */, size_t context_len);
RFC8032_EDDSA_DECL int ed25519ph_verify_keyed_dev(uint8_t *ok, const eddsa_amd_keyset *ks, const uint32_t *key_idx, const uint8_t *sigs,
                                                  const uint8_t *prehashes, size_t n, const uint8_t *context /* host */, size_t context_len,
                                                  void *stream);

/* ---- SIGNER SETS: register the secret keys once, sign by key index ----
 * For callers that sign very many items with a few keys (token issuers, log and timestamp signers, oracles).  ed25519_sign_batch
 * takes 32 bytes of seed and 32 bytes of public key per item and spends one of the item's three SHA-512 compressions on
 * SHA-512(seed), again and again for the same few keys.  A signer set does that once per KEY, derives the public key itself -
 * a `pubs` that does not belong to `secs` cannot happen: that mismatch yields signatures that leak the secret scalar - and
 * signs with keys that have no seed at all: expanded secret keys (scalar, prefix), as BIP32-Ed25519 derivation, key blinding
 * and libraries with an "expanded secret key" type produce them.
 * What a set holds: per key, in HBM: the scalar a mod l (32 bytes), the prefix (32 bytes) and the public key A = (a mod l) B
 *   encoded (32 bytes) - 96 bytes per key.
 * Seeds (eddsa_amd_signer_create): (a, prefix) is what ed25519_sign_batch derives: h = SHA-512(seed), a = h[0..32) clamped,
 *   prefix = h[32..64).  sigs[i] is byte for byte what ed25519_sign_batch writes for (secs[key_idx[i]], its public key, message i);
 *   the ctx / ph forms give byte for byte what ed25519ctx_sign_batch / ed25519ph_sign_batch write under the same context.
 * Expanded keys (eddsa_amd_signer_create_expanded): 64 bytes per key.  The first 32 bytes are a as a little-endian 256-bit
 *   integer, used mod l and NOT clamped (derived and blinded keys rely on that); the last 32 bytes are the prefix.  Then
 *   r = SHA-512([dom2 ||] prefix || M') mod l, R = r B, t = SHA-512([dom2 ||] R || A || M') mod l, S = (r + t a) mod l.
 *   Any 64 bytes are legal input; a = 0 mod l gives the neutral element as A and is not an error.  A set created from seeds and a
 *   set created from the expansions of the same seeds are indistinguishable.
 * Out-of-range indices: the device-pointer forms write 64 zero bytes for an item with key_idx[i] >= count; they read nothing
 *   outside the set for it and leave its neighbours alone.  The host-pointer forms check the whole index array first and return
 *   -hipErrorInvalidValue before anything is touched.
 * Argument checks, before any device is touched: the create calls refuse out == NULL, secs / expanded == NULL, count == 0 and
 *   count > EDDSA_AMD_SIGNER_MAX_KEYS with -hipErrorInvalidValue; *out is left NULL on these and on every other error.  The sign
 *   calls refuse a NULL s, sigs, key_idx or fixed-length msgs / prehashes, context_len > 255 and a NULL context with a length;
 *   the NULL signer is refused even for n == 0, like ed25519_verify_keyed.  eddsa_amd_signer_pubs refuses a NULL s or pubs.
 * Devices: a set is created on the default device, by the rule of the host-pointer calls.  A device-pointer call whose `sigs`
 *   lie on another device returns -hipErrorInvalidValue; host-pointer calls run on the set's device.
 * Lifetime and use: a set is immutable and usable from any number of threads and streams; no pass writes it.  It SURVIVES
 *   eddsa_amd_shutdown and is freed only by eddsa_amd_signer_destroy (NULL allowed), which synchronises the set's device:
 *   destroy it after the last call that uses it has returned.
 * Secrets: a signer set is the one place where secrets stay in HBM by design.  destroy overwrites the scalars and prefixes with
 *   zeros on the device and waits for that before it frees; create zeroes its staging copy before it returns.  The per-pass
 *   copies of a and r in the workspace are wiped by the finish kernel, exactly as in ed25519_sign_batch; the keyed finish kernel
 *   zeroes the pass's projective points R as well, and a host-pointer call zeroes its staging copies of the indices and of the
 *   signatures.
 * Combiner and upload: host-pointer calls are never merged by the small-call combiner (two calls may carry two signer sets).
 *   They upload 4 bytes of index and the message per item, where ed25519_sign_batch uploads 64 bytes and the message.
 * key_idx: packed uint32, one per item, host memory in the host-pointer forms and HBM in the _dev forms; `context` is a host
 *   pointer in every form.  Everything else - layout, ragged-table rules and clamping, return values, page-locked memory,
 *   threading - follows the rules at the top.
 * Kernels: three per pass, the shape of the Ed25519ctx / Ed25519ph sign pass: one that takes a and the prefix by index and hashes
 *   r, the point kernel R = r B of that pass unchanged, and a finish kernel that takes A by index.  This shape is the one kept: it
 *   is faster than ed25519_sign_batch_dev's two kernels at every size measured (below), so the other shape - the nonce hash fused
 *   into a keyed form of the point kernel, as in ed25519_sign_batch - was not built and has no figure.
 * Out of scope: creation from device pointers; _multi and single-item forms.  ed25519_sign_batch* are unchanged.
 * Measured (profiles/sign_keyed.txt, tools/sign_keyed_rate.py: device-pointer forms, 2^20 items of 32 bytes in HBM, one MI355X, the two
 * forms alternating, repeat spread 0.001-0.005 ms): under 1024 signers 2.206 ms per pass through ed25519_sign_batch_dev, 2.095 ms
 * through ed25519_sign_keyed_dev (-5.0 %: 501 M instead of 475 M signs/s); under ONE signer 2.202 / 2.093 ms (-5.0 %), under 2^20
 * distinct signers - a 96 MiB set read in random order - 2.205 / 2.104 ms (-4.6 %).  Ed25519ctx 2.369 / 2.288 ms (-3.4 %), Ed25519ph
 * 2.497 / 2.425 ms (-2.9 %).  Small passes under 1024 signers (unkeyed / keyed): 2^7 items 0.145 / 0.137 ms, 2^10 0.151 / 0.143,
 * 2^14 0.157 / 0.149, 2^16 0.236 / 0.221.  What one of three SHA-512 compressions and 60 bytes of input per item are worth: about
 * 0.11 ms in 2.2, although the pass has a third launch (the same shape costs the unkeyed ctx form +7 %).  Host to host from ordinary
 * memory, 1024 signers, the keyed call is NOT faster: 44.6 ms against 40.1 ms (+11 %; the repeats overlap, 39.9-44.7 against
 * 35.2-45.4 ms) - such a call is bound by staging and copies, and the keyed rows zero the signatures in the staging buffers
 * after the download, which costs more than the smaller upload saves.  eddsa_amd_signer_create: 0.36 ms for 1024 keys, 3.7 ms for
 * 2^20.  ed25519_sign_batch_dev against the commit before signer sets, alternating in fresh processes on that box: 2.208-2.217 ms
 * against 2.208-2.222 ms (the medians of five processes each) - inside the older build's own repeat spread.
 * (Declared with the macro of the RFC 8032 variants: tests of earlier additions count the EDDSA_AMD_DECL names.) */
typedef struct eddsa_amd_signer eddsa_amd_signer;            /* opaque */
#define EDDSA_AMD_SIGNER_MAX_KEYS ((size_t)1 << 20)
RFC8032_EDDSA_DECL int eddsa_amd_signer_create(eddsa_amd_signer **out, const uint8_t *secs /* host, 32 bytes per key: seeds */, size_t count);
RFC8032_EDDSA_DECL int eddsa_amd_signer_create_expanded(eddsa_amd_signer **out, const uint8_t *expanded /* host, 64 bytes per key: scalar | prefix */,
                                                        size_t count);
RFC8032_EDDSA_DECL void eddsa_amd_signer_destroy(eddsa_amd_signer *s);        /* NULL allowed */
RFC8032_EDDSA_DECL size_t eddsa_amd_signer_count(const eddsa_amd_signer *s);
RFC8032_EDDSA_DECL int eddsa_amd_signer_device(const eddsa_amd_signer *s);    /* the HIP device that holds the set */
RFC8032_EDDSA_DECL int eddsa_amd_signer_pubs(const eddsa_amd_signer *s, uint8_t *pubs /* host, 32 bytes per key */);
RFC8032_EDDSA_DECL int ed25519_sign_keyed(uint8_t *sigs, const eddsa_amd_signer *s, const uint32_t *key_idx, const uint8_t *msgs,
                                          const uint64_t *msg_off, size_t msg_len, size_t n);
RFC8032_EDDSA_DECL int ed25519_sign_keyed_dev(uint8_t *sigs, const eddsa_amd_signer *s, const uint32_t *key_idx, const uint8_t *msgs,
                                              const uint64_t *msg_off, size_t msg_len, size_t n, void *stream);
RFC8032_EDDSA_DECL int ed25519ctx_sign_keyed(uint8_t *sigs, const eddsa_amd_signer *s, const uint32_t *key_idx, const uint8_t *msgs,
                                             const uint64_t *msg_off, size_t msg_len, size_t n, const uint8_t *context /* host */, size_t context_len);
RFC8032_EDDSA_DECL int ed25519ctx_sign_keyed_dev(uint8_t *sigs, const eddsa_amd_signer *s, const uint32_t *key_idx, const uint8_t *msgs,
                                                 const uint64_t *msg_off, size_t msg_len, size_t n, const uint8_t *context /* host */,
                                                 size_t context_len, void *stream);
RFC8032_EDDSA_DECL int ed25519ph_sign_keyed(uint8_t *sigs, const eddsa_amd_signer *s, const uint32_t *key_idx,
                                            const uint8_t *prehashes /* 64 bytes per item */, size_t n, const uint8_t *context /* host */,
                                            size_t context_len);
RFC8032_EDDSA_DECL int ed25519ph_sign_keyed_dev(uint8_t *sigs, const eddsa_amd_signer *s, const uint32_t *key_idx, const uint8_t *prehashes, size_t n,
                                                const uint8_t *context /* host */, size_t context_len, void *stream);

/* ---- POINT CLASSIFICATION: what a 32-byte string is as a curve point ----
 * For callers that qualify keys once, at registration (validator sets, token issuers, consensus nodes), and then rely on the fast
 * paths.  The verify forms decode anything; the strict rules (EDDSA_AMD_VERIFY_*) only turn accepts into rejects inside a pass and do
 * not cover a point of mixed order; the _rlc forms promise the per-item verdicts "whenever every A and R lies in the prime-order
 * subgroup"; key sets register ANY 32-byte strings.  These calls answer the question on its own: one class byte per item, the OR of
 *   EDDSA_AMD_POINT_ON_CURVE        the string decodes under the reference's permissive import (ed_import, what every verify form
 *                                   applies to A): y is the low 255 bits mod p, so a y >= p counts, and x = 0 takes either sign bit.
 *   EDDSA_AMD_POINT_CANONICAL       the string is an encoding that RFC 8032 5.1.3 decodes: y < p, a root exists, and not x = 0 with
 *                                   the sign bit set.  It implies ON_CURVE.
 *   EDDSA_AMD_POINT_SMALL_ORDER     the point is on the curve and [8]P is the neutral element (y mod p is one of the five values of
 *                                   the eight points of order 1, 2, 4 and 8).  The neutral element has this bit.
 *   EDDSA_AMD_POINT_PRIME_SUBGROUP  the point is on the curve and [l]P is the neutral element.  The neutral element has this bit
 *                                   too: it is the only point with both SMALL_ORDER and PRIME_SUBGROUP.  A point of mixed order (a
 *                                   small-order component on a prime-order point) has ON_CURVE and neither of the two order bits.
 * A string that is no curve point classifies as 0.  The class depends on the 32 bytes only: the off-curve mode, the strict rules and
 * the equation play no part, and no policy bit is added (the meanings of eddsa_amd_set_offcurve_mode's values are untouched).
 * What a caller does with it: a key fit for registration has
 *   (cls & 0x0F) == (EDDSA_AMD_POINT_ON_CURVE | EDDSA_AMD_POINT_CANONICAL | EDDSA_AMD_POINT_PRIME_SUBGROUP).
 * What the class buys: if every key of a key set has PRIME_SUBGROUP, the cofactorless caveat of the _rlc forms is about R alone -
 *   two or more crafted R with small-order components in one group can still cancel; such a caller can classify the R strings of a
 *   batch with the same call (copied out of the signatures: see "out of scope").  Under the cofactored equation
 *   (eddsa_amd_set_verify_equation) there was no caveat to begin with.
 * Calls: layout packed, 32 bytes per item in and one byte out; `points` and `cls` may have any alignment.  An empty batch (n == 0)
 *   returns 0; a NULL cls or points with n > 0 returns -hipErrorInvalidValue before any device is touched.  The device form runs on the
 *   device that holds `cls`, enqueues on `stream` and returns.  The host form goes through the staging pipeline like every host-pointer
 *   call and is never merged by the small-call combiner.
 * eddsa_amd_keyset_classify runs the same kernel over the set's own key bytes in HBM, on the set's device (made current for the
 *   call's duration), downloads eddsa_amd_keyset_count(ks) bytes into `cls` and returns when done.  It works on plain and on comb sets,
 *   and after eddsa_amd_shutdown - a key set survives shutdown, and the kernel needs no table and no workspace.  It refuses a NULL ks or
 *   cls with -hipErrorInvalidValue.  It changes nothing: not key-set creation (ANY strings are still registered), not the set's
 *   contents, not eddsa_amd_keyset_bytes.  A caller that wants only qualified keys in a set classifies first and registers what passed.
 * A library built without the HIP translation unit answers -hipErrorNotSupported from all three.
 * Kernel: one lane per string - the decoding of the verify pass (one square-root chain), the y < p test, the five-value small-order
 *   test, and for strings on the curve the chain [l]P over the non-adjacent form of l (46 nonzero digits): 252 doublings and 45 additions
 *   of P or -P, with P held in registers (no table, no memory, no inversion: the neutrality test is projective).  The digits are derived from l
 *   at compile time; which digit comes is the same in every lane, so the chain does not diverge.  The group law is complete on the
 *   curve: points of small and of mixed order take the same path as honest keys.  Nothing here is secret.
 * Out of scope: strided input (the R of packed signatures in place); _multi and single-item forms; a strict rule that requires the
 *   subgroup inside a verify pass; four-lane forms for small batches.
 * Measured (profiles/point_classify.txt, tools/classify_rate.py: device-pointer forms, 2^20 items in HBM, one MI355X, the forms
 *   alternating in one process, repeat spread 0.002-0.026 ms): 2^20 honest public keys 8.231 ms per pass (127 M strings/s); 2^20
 *   random strings, half of them no curve point, 8.216 ms - the same, because a wave ends early only when all 64 of its strings leave
 *   before the chain; beside them pk_ed25519_to_x25519_batch_dev over the same keys 0.716 ms and ed25519_verify_batch_dev over valid
 *   signatures under them 9.364 ms: classifying a key costs 12 % less than verifying one signature under it, once per key.  The
 *   kernel holds 224 VGPRs without scratch or spills - two waves per SIMD, like the verify main kernels - and was not tuned further.
 *   ed25519_verify_batch_dev against the commit before, alternating in fresh processes: 9.345 ms against 9.341 ms, inside the older
 *   build's own repeat spread (9.329-9.359 ms); every older kernel has the older build's metadata.
 * (Declared with the macro of the RFC 8032 variants: tests of earlier additions count the EDDSA_AMD_DECL names.) */
#define EDDSA_AMD_POINT_ON_CURVE        0x01
#define EDDSA_AMD_POINT_CANONICAL       0x02
#define EDDSA_AMD_POINT_SMALL_ORDER     0x04
#define EDDSA_AMD_POINT_PRIME_SUBGROUP  0x08
RFC8032_EDDSA_DECL int ed25519_point_classify_batch(uint8_t *cls, const uint8_t *points /* host, 32 bytes per item */, size_t n);
RFC8032_EDDSA_DECL int ed25519_point_classify_batch_dev(uint8_t *cls, const uint8_t *points /* device */, size_t n, void *stream);
RFC8032_EDDSA_DECL int eddsa_amd_keyset_classify(const eddsa_amd_keyset *ks, uint8_t *cls /* host, eddsa_amd_keyset_count(ks) bytes */);

/* ---- DERIVED PUBLIC KEYS: out[i] = [m_i]P_i + [a_i]B, the Edwards counterpart of x25519_batch ----
 * NOT FOR SECRETS.  The chain's table lookups and additions depend on the scalars' digits, and the scalars lie unwiped in the verify
 * workspace afterwards.  The inputs are PUBLIC keys and PUBLIC derivation scalars.  Secret scalars belong to signer sets
 * (eddsa_amd_signer_create_expanded) and to x25519_batch, which are constant-time and wipe what they stage.
 * For the verifying side of the schemes eddsa_amd_signer_create_expanded names: a watch-only wallet derives BIP32-Ed25519 child
 * public keys as A' = A + [z]B, a verifier of blinded keys derives A' = [h]A.  Such a party holds no secret, cannot call
 * eddsa_amd_signer_pubs, and has thousands to millions of keys to derive before it can fill a key set.
 * Result: out[i] is the canonical RFC 8032 encoding of [m_i]P_i + [a_i]B, where m_i = mul[i] and a_i = add[i] are 32-byte
 *   little-endian strings read as integers in [0, 2^256): not clamped, not range-checked.
 * Torsion: the result is the integer multiple for EVERY curve point, points with a small-order component included.  The group has
 *   8 l elements: a is reduced mod l (B has order l), m is reduced mod 8 l and never mod l - for a P that carries torsion [m]P and
 *   [m mod l]P are different points.
 * Absent arrays: mul == NULL means every m_i = 1 (soft derivation, A + [z]B); add == NULL means every a_i = 0 (blinding, [h]A); with
 *   both NULL the call re-encodes P canonically.  Nothing is read, staged or uploaded for an absent array.
 * Decoding of points[i]: the reference's permissive import, the rule every verify form applies to a key and the meaning of
 *   EDDSA_AMD_POINT_ON_CURVE: y is the low 255 bits mod p, and x = 0 takes either sign bit.
 * Off-curve input: a string that is no curve point gives out[i] = 02 00 .. 00 (EDDSA_AMD_NO_POINT_BYTE0 and 31 zero bytes), the
 *   string the keyed passes use for "no key".  Its y = 2 is on no curve point, so it can never be a valid result; a key set that
 *   registers it rejects its items in reject mode and under the cofactored equation.  The neighbours of such an item are unaffected.
 * Settings: the result depends on the input bytes only.  The off-curve mode, the strict rules and the equation play no part.
 * Aliasing: `out` may be the very buffer `points` (in-place derivation).  Any other overlap is undefined.
 * Arguments: packed arrays of any alignment.  n == 0 returns 0; a NULL out or points with n > 0 returns -hipErrorInvalidValue before
 *   any device is touched.  The device form runs on the device that holds `out`, enqueues on `stream` and returns without
 *   synchronising.  The host form goes through the staging pipeline like every host-pointer call and is never merged by the
 *   small-call combiner.  A library built without the HIP translation unit answers -hipErrorNotSupported from both.
 * Kernels: a pass is three kernels over the verify workspace, in chunks of 2^20 items, ordered against verify passes on the same
 *   workspace like one of them.  A prepare kernel decodes P, centres m mod 8 l as |m'| <= 4 l with its sign, and writes the digit
 *   words and the nine-entry table of sign * P; the verify pass's own main kernel, unchanged, walks 64 windows with the table of
 *   multiples of B; a finish kernel shares one inversion among eight items per lane and encodes.  No existing kernel changed.
 * Out of scope: constant-time forms; four-lane forms for small passes; _multi and single-item forms; a key-set constructor that
 *   derives in place (derive into a device buffer and hand it to eddsa_amd_keyset_create_dev); hashing the derivation scalars,
 *   which is the caller's scheme.
 * Measured (profiles/point_muladd.txt, tools/point_muladd_rate.py: device-pointer forms, 2^20 items in HBM, one MI355X, the rows
 *   alternating in one process, seven repeats, repeat spread 0.015-0.022 ms): both arrays given 10.255 ms per pass (102 M keys/s),
 *   mul only 10.219 ms, add only 10.162 ms; beside them ed25519_verify_batch_dev in off-curve mode 0 over as many valid signatures
 *   10.382 ms - the muladd pass is 1.2 to 2.1 % faster than the verify pass that runs the same main kernel.  Per kernel (kernel
 *   trace): k_verify_main 9.18 ms in both passes, k_point_muladd_prepare 1.10 ms against k_verify_prepare's 1.22 ms,
 *   k_point_muladd_finish 0.164 ms against k_verify_finish's 0.157 ms.  Small passes: 2^16 items 0.814 ms against 0.837 ms for
 *   that verify pass; 2^7, 2^10 and 2^14 items 0.768, 0.775 and 0.801 ms against 0.452, 0.459 and 0.487 ms - SLOWER, and the
 *   kernel that costs the time is the one-lane k_verify_main (0.625 ms at 2^10 items: one wave's chain of 252 doublings), where a
 *   verify pass of up to 2^14 items runs the four-lane k_verify_main_quad (0.299 ms); the four-lane form is out of scope above.
 *   ed25519_verify_batch_dev in the default mode against the commit before, alternating in fresh processes: 9.088 ms against
 *   9.084 ms, inside the older build's own repeat spread (9.045-9.120 ms); every older kernel has the older build's metadata, and
 *   the two new kernels hold 247 and 134 VGPRs without scratch or spills.
 * (Declared with the macro of the RFC 8032 variants: tests of earlier additions count the EDDSA_AMD_DECL names.) */
#define EDDSA_AMD_NO_POINT_BYTE0 0x02   /* out[i] = 02 00 .. 00 (32 bytes): "no curve point" */
RFC8032_EDDSA_DECL int ed25519_point_muladd_batch    (uint8_t *out, const uint8_t *points, const uint8_t *mul, const uint8_t *add, size_t n);
RFC8032_EDDSA_DECL int ed25519_point_muladd_batch_dev(uint8_t *out, const uint8_t *points, const uint8_t *mul, const uint8_t *add, size_t n, void *stream);

/* ---- ITEMS IN PLACE: verify (signature, key, message) triples given by byte offsets into one buffer ----
 * For callers that hold a buffer of network packets (transactions, votes): a packet carries one message and several (signature, key)
 * pairs at positions that differ from packet to packet, and all the caller has per item is "signature at byte s, key at byte p,
 * message at byte m, length l".  The packed forms would make it copy a message once per signer (two items can never share a span of
 * msg_off[0..n]), and ed25519_verify_records takes one stride and three offsets for the whole call.
 * Item i consists of three spans of `data`: the signature data[sig_off[i] .. +64), the key data[pub_off[i] .. +32) and the message
 *   data[msg_off[i] .. +msg_len[i]).  The four index arrays are packed uint32, one entry per item: host memory in the first form, HBM
 *   in the second, like key_idx.
 * Verdicts: ok[i] is byte for byte what ed25519_verify_batch returns for those three spans, under the off-curve mode (0, 1, 2), the
 *   strict rules and the equation in force when each pass is enqueued: the pass runs as a pass of ed25519_verify_digests, whose
 *   contract says so.
 * Overlap and alignment: spans may have any alignment; they may overlap each other and the spans of other items - several items
 *   sharing one message is the point of the call.  `data` is only read.  `ok` must not overlap it.
 * data_len: the caller vouches for it as the size of the buffer.  data_len >= 2^32 returns -hipErrorInvalidValue, and so does a NULL
 *   ok, data or index array with n > 0 - both before any device is touched.  n == 0 returns 0.
 * Spans that leave the buffer (the three conditions are computed in 64 bits, nothing wraps): in the device-pointer form an item with
 *   sig_off[i] + 64 > data_len, pub_off[i] + 32 > data_len or msg_off[i] + msg_len[i] > data_len gets ok[i] = 0 under every setting;
 *   no byte of `data` is read for that item, and the verdicts of its neighbours are unaffected.  This is the keyed forms' rule for an
 *   index outside the set, not the ragged table's "hash the clamped span": an item that is not entirely in the buffer is no item.
 *   The host-pointer form checks all four arrays first and returns -hipErrorInvalidValue with `ok` untouched, like a bad ragged table.
 * Reads at the edge: for items inside the buffer the statement at the top of this header about whole-word loads applies unchanged -
 *   the hashing lane may read the aligned 4-byte words that hold the first and last byte of a span, so up to 3 bytes outside
 *   [data, data + data_len) lie in the same word as a byte of the buffer.
 * Other rules: EDDSA_AMD_STALLED, return values, ownership and threading as at the top of this header.  The device-pointer form runs
 *   on the device that holds `ok`; `data` must live on that device (-hipErrorInvalidValue otherwise).  The call is never merged by the
 *   small-call combiner.  A library built without the HIP translation unit answers -hipErrorNotSupported from both.
 * Host-pointer form: a plain wrapper, NOT chunked through the staging pipeline - a chunk of items may refer to any byte of `data`, so
 *   the buffer has to be resident before the first pass.  It checks the arrays, allocates HBM for `data` and the four arrays on the
 *   default device, uploads, runs the device form on a stream of its own, downloads `ok`, frees, and reports EDDSA_AMD_STALLED itself.
 * Kernels: one kernel in front of a digest pass, as k_dom_challenge is for Ed25519ctx / Ed25519ph.  k_scatter_challenge, one lane per
 *   item, gathers the 64 signature bytes and the 32 key bytes into packed areas of the verify workspace and writes
 *   SHA-512(R || A || M) beside them; the prepare, halve, main, exact, finish, policy and cofactor kernels then see ordinary packed
 *   input.  An item outside the buffer is written as the signature 00 .. 00, the digest 00 .. 00 and the key 02 00 .. 00
 *   (EDDSA_AMD_NO_POINT_BYTE0), which every route rejects.  From 4096 items on the lanes take the items longest
 *   message first.  The signature area costs 64 bytes of HBM per item of a workspace's capacity and exists only in a workspace that
 *   has served a scattered pass.  No existing kernel changed.
 * Out of scope: _rlc, keyed (key_idx in place of pub_off), digest, ctx / ph and _multi forms of the scattered call; 64-bit offsets; a
 *   streaming host pipeline for the host-pointer form.
 * Measured (profiles/verify_scattered.txt, tools/scattered_rate.py): device-pointer forms, 2^20 valid items with 32-byte messages in HBM, one
 *   MI355X, the rows alternating in one process, seven repeats, repeat spread 0.03-0.11 ms): ed25519_verify_batch_dev over the items
 *   packed 9.330 ms per pass; ed25519_verify_scattered_dev over the same items as 128-byte packets 9.507 ms (+1.9 %), with 8
 *   signatures sharing each message 9.509 ms (+1.9 %); ed25519ctx_verify_batch_dev, the existing form with a front kernel, 9.569 ms
 *   (+2.6 %) - the expectation was that form's 2 %.  Small passes, packed against scattered: 2^7 items 0.239 / 0.250 ms, 2^10
 *   0.254 / 0.269 ms, 2^14 0.319 / 0.351 ms (+10 %: the order of length adds four small launches from 4096 items on), 2^16
 *   0.638 / 0.663 ms.  The host form from ordinary memory, host to host: 16.21 ms against 10.66 ms for ed25519_verify_batch through
 *   the staging pipeline - 52 % SLOWER, the price of the plain wrapper above.  ed25519_verify_batch_dev against the commit before,
 *   alternating in fresh processes: 9.326 ms against 9.342 ms, inside the older build's own repeat spread (9.279-9.400 ms); every
 *   older kernel has the older build's metadata, and k_scatter_challenge holds 110 VGPRs without scratch or spills.
 * (Declared with the macro of the RFC 8032 variants: tests of earlier additions count the EDDSA_AMD_DECL names.) */
RFC8032_EDDSA_DECL int ed25519_verify_scattered    (uint8_t *ok, const uint8_t *data, size_t data_len,
                                                    const uint32_t *sig_off, const uint32_t *pub_off,
                                                    const uint32_t *msg_off, const uint32_t *msg_len, size_t n);
RFC8032_EDDSA_DECL int ed25519_verify_scattered_dev(uint8_t *ok, const uint8_t *data, size_t data_len,
                                                    const uint32_t *sig_off, const uint32_t *pub_off,
                                                    const uint32_t *msg_off, const uint32_t *msg_len, size_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EDDSA_AMD_H */
