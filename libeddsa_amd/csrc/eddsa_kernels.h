// eddsa_kernels.h - internal interface between the C host library (eddsa_amd.c) and the HIP
// translation unit (kernels.hip).  Not installed; the public contract is include/eddsa_amd.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "edk_layout.h"             /* the tables' sizes, the per-item slots of the workspaces, the words of offcount */

#define EDK_LEN_BINS 2048           /* bins of the per-pass counting sort of ragged messages by length (kernels.hip: k_len_*) */
#define EDK_EXACT_PATIENCE (1u << 21) /* polls (a microsecond or two each) a wave of k_verify_exact_lane_chain spends on one hand-off */

#ifdef __cplusplus
extern "C" {
#endif

hipError_t edk_init_tables(uint32_t* base16, uint32_t* comb, uint32_t* comb_img, hipStream_t stream);

#define EDK_SUMS_MAX_ITEMS ((size_t)1 << 11)          /* passes of up to this many items add their windows' sums first (kernels.hip: k_verify_window_sums) */
#define EDK_SUMS_BYTES (EDK_SUMS_MAX_ITEMS * 64 * 40 * sizeof(uint32_t))   /* 64 windows x four multipliers of ten limbs per item */
#define EDK_STATUS_STALLED 1u
#define EDK_EXACT_SLOTS 65536                        /* items k_verify_exact_quad has in flight at once (4096 waves of 16); a longer work list is walked in strides of this */
#define EDK_EXACT_PAD_BYTES ((size_t)EDK_EXACT_SLOTS * 960)   /* per slot: four addends x five factors x 12 words (quad_lanes.h: QUAD_ITEM_WORDS) */

/* The dom2(F, C) prefix of Ed25519ctx (F = 0) and Ed25519ph (F = 1), RFC 8032 section 2: the 32 bytes "SigEd25519 no Ed25519
 * collisions", F, len(C), C - len = 34 + len(C) bytes as little-endian words, zero behind the last byte.  Built on the host per call
 * (eddsa_amd.c: dom2_fill) and handed BY VALUE to the kernels that hash under it, and to no other kernel: the caller's context
 * need not outlive the call, and a lane reads the words by uniform index (sha512.h: sha512_dom_msg). */
typedef struct edk_dom {
  uint32_t len;
  uint32_t w[EDK_DOM_WORDS];
} edk_dom;

/* verify workspace for up to `capacity` items (a multiple of VERIFY_TILE), all in HBM */
typedef struct edk_verify_ws {
  size_t capacity;
  uint32_t* digits;   /* capacity * VERIFY_DIGIT_WORDS words */
  uint32_t* table;    /* capacity / 256 tiles * VERIFY_TABLE_WORDS_PER_TILE words */
  uint32_t* acc;      /* capacity * ACC_WORDS words */
  uint32_t* hdigits;  /* capacity * HALF_DIGIT_WORDS words: the half-length scalars (kernels.hip k_verify_halve) */
  uint32_t* rtable;   /* like table: 0..8 times -R' */
  uint8_t* flags;     /* capacity bytes: kernel_io.h, VERIFY_WINDOWED ... */
  uint32_t* offlist;  /* capacity words: the exact path's work list (keys off the curve; large passes: items without a short pair) */
  uint32_t* onlist;   /* capacity words: the items the windowed evaluation decides (every other item); the half-length route's
                         k_verify_halve / k_verify_main_half run over this list */
  uint32_t* perm;     /* capacity words: ragged passes: the items in order of message length (kernels.hip: msg_order) */
  uint32_t* lenbins;  /* 2 * EDK_LEN_BINS words: that sort's counts and cursors */
  uint32_t* offcount; /* EDK_OFFCOUNT_WORDS words, zeroed at allocation: the lengths of the two lists, the one-lane exact path's counters and
                         shared entry, hooks (edk_layout.h: EDK_*_WORD) */
  uint32_t* exact_pad;/* EDK_EXACT_PAD_BYTES: scratchpad of k_verify_exact_quad: the addends of the items in flight, one slot per quad */
  uint32_t* sums;     /* EDK_SUMS_BYTES: the windows' sums of a small pass */
  uint32_t* status;   /* one word of page-locked host memory shared by the engine's workspaces (or NULL): a kernel that had to give up
                         stores EDK_STATUS_STALLED there; the host side turns it into EDDSA_AMD_STALLED (eddsa_amd.c: take_async_error) */
  hipStream_t side;   /* the exact path runs here, beside the main kernel */
  hipEvent_t ev_prepared, ev_exact;
  int algo;           /* 0: half-length scalars (four lanes per item up to 24 576 items, one above); 1: always full-length; 2: half-length, one lane per item;
                         3: the mid-size arrangement below 2^18 items, full-length from there on.  The table: kernels.hip, verify_route_of */
  int exact_offcurve; /* 1: replay the reference's chain for off-curve keys (default); 0: reject them; 2: replay for every item */
  uint8_t* domdig;    /* capacity * EDK_DOM_DIGEST_BYTES: Ed25519ctx / Ed25519ph passes: the items' SHA-512(dom2 | R | A | M'), written by
                         k_dom_challenge[_keyed] and read by the digest forms of the prepare kernels (kernels.hip: edk_verify) */
  uint8_t* keybytes;  /* capacity * 32: keyed passes (edk_verify_src.ks_table): the items' key bytes, written by the keyed prepare kernel;
                         the kernels behind it read `pubs` there with stride 32 */
  const uint32_t* comb; /* the engine's comb of the base point in its global layout (edk_init_tables), not owned: keyed passes over a comb
                         key set (edk_verify_src.ks_comb) read S*B through it */
  uint8_t* gsigs;     /* capacity * 64, or NULL: scattered passes (edk_verify_src.sc_data): the items' signatures, gathered by
                         k_scatter_challenge (edk_scatter.h) beside their keys (keybytes) and digests (domdig).  Allocated by the first
                         scattered pass a slot serves (eddsa_amd.c: verify_on) and freed with the slot: no other call pays for it */
} edk_verify_ws;

/* where the items of a verify pass live: item i has its signature at sigs + i * sig_stride, its key
 * at pubs + i * pub_stride and its message at msgs + i * msg_stride (msg_len bytes) or, for ragged
 * messages, at msgs + msg_off[i].  Packed arrays: strides 64 / 32 / msg_len; records: one stride.
 * The host side writes the fields in one place, by name (engine.h: verify_src, verify_src_records): what a form does not set is 0 / NULL. */
typedef struct {
  const uint8_t *sigs, *pubs, *msgs;
  const uint64_t* msg_off;
  size_t msg_len, sig_stride, pub_stride, msg_stride;
  const uint64_t* msg_end;   /* ragged messages: the LAST entry of the call's offset table = the size of the message buffer; every
                                item's span is clamped into it (lanes.h: msg_span).  verify_on / rlc_on fill it in. */
  int digest;                /* != 0 (ed25519_verify_digests*): the message slot holds the caller's SHA-512(R || A || M), 64 bytes per
                                item (msg_len 64, no offset table); the hashing kernels' digest forms take t from it unhashed */
  int policy;                /* the EDDSA_AMD_VERIFY_* bits in force (include/eddsa_amd.h), 0 = none: != 0 adds k_verify_policy behind the
                                pass's verdicts (kernels.hip).  Filled in by src_at (eddsa_amd.c) for verify_on / rlc_on alike.  Host side
                                only, like `digest` */
  const edk_dom* dom;        /* != NULL (ed25519ctx_verify_batch*, ed25519ph_verify_batch*): t comes from SHA-512(dom2 || R || A || M') - one
                                kernel hashes every item under the prefix into ws->domdig and the pass goes on as a digest pass over that
                                area.  Host side only (the pointer is read while the pass is enqueued); never set together with
                                `digest` */
  int equation;              /* EDDSA_AMD_EQUATION_* (include/eddsa_amd.h), 0 = the reference's cofactorless check: != 0 adds the
                                k_cofactor_* kernels behind the pass's verdicts and S < l to its policy (kernels.hip: edk_verify), and
                                sends a group with a non-canonical R to the per-item kernels (rlc.hip).  Filled in by src_at like
                                `policy`, read beside it.  Host side only */
  /* ks_table != NULL (ed25519_verify_keyed*): a KEYED pass - `pubs` is not read; item i's key is entry key_idx[i] of a key set
     (include/eddsa_amd.h: eddsa_amd_keyset), whose HBM these point to: ks_keys 32 bytes, ks_flags one byte (on the curve),
     ks_table VERIFY_ITEM_TABLE_WORDS words per key, ks_count keys.  key_idx lies in HBM like the other arrays of the pass and
     is advanced with them by src_at.  Host side only: the keyed kernels take the pointers as arguments of their own
     (keyed_kernels.h).  With `digest` (ed25519_verify_keyed_digests*) or `dom`
     (ed25519ctx_verify_keyed*, ed25519ph_verify_keyed*) the keyed kernels run in their digest forms; the combination takes
     `digest` and refuses `dom` (rlc.hip: edk_verify_rlc) */
  const uint8_t *ks_keys, *ks_flags;
  const uint32_t* ks_table;
  size_t ks_count;
  const uint32_t* key_idx;
  const uint32_t* ks_comb;   /* != NULL: the key set is a COMB key set (eddsa_amd_keyset_create_comb) - KEYSET_COMB_WORDS words per key,
                                [key][row][m - 1] = m * 2^(2 COMB_W row) * (-A); the pass takes the comb route (kernels.hip: verify_route_of).
                                NULL for plain sets */
  /* sc_data != NULL (ed25519_verify_scattered*): a SCATTERED pass - item i's signature, key and message lie at sc_sig_off[i],
     sc_pub_off[i] and sc_msg_off[i] (sc_msg_len[i] bytes) of sc_data[0 .. sc_data_len), four packed uint32 arrays in HBM that
     src_at advances with the chunk; sc_data is the same for every chunk.  Host side only: verify_on (eddsa_amd.c) runs
     edk_scatter_challenge (edk_scatter.h) in front of edk_verify and points sigs, pubs and msgs at what it left in the workspace,
     so that edk_verify sees the digest pass (`digest` set, strides 64 / 32 / 64) and never reads these fields */
  const uint8_t* sc_data;
  size_t sc_data_len;
  const uint32_t *sc_sig_off, *sc_pub_off, *sc_msg_off, *sc_msg_len;
} edk_verify_src;

/* What the kernels take BY VALUE: the nine fields of edk_verify_src that lanes read, 72 bytes as before the flag existed.  The flag stays
 * on the host side (it selects the kernel): a by-value argument that grows moves every argument behind it, and with the layout of
 * k_verify_prepare's arguments went its scalar register allocation (104 SGPRs, 14 of them spilled to 36 bytes of scratch per lane,
 * where it has 106, 6 and none: profiles/digest_verify.txt). */
typedef struct {
  const uint8_t *sigs, *pubs, *msgs;
  const uint64_t* msg_off;
  size_t msg_len, sig_stride, pub_stride, msg_stride;
  const uint64_t* msg_end;
} edk_verify_items;
static inline edk_verify_items edk_items_of(const edk_verify_src* s) {
  const edk_verify_items it = { s->sigs, s->pubs, s->msgs, s->msg_off, s->msg_len, s->sig_stride, s->pub_stride, s->msg_stride, s->msg_end };
  return it;
}

/* bulk_done (or NULL): recorded on `stream` once every kernel that fills the chip has been queued, before the stream
 * waits for the exact path's side stream (bulk_early != 0: already before the main kernel, so that a following pass on
 * another workspace starts beside it) */
hipError_t edk_verify(uint8_t* ok, const edk_verify_src* src, size_t n, const uint32_t* base16,
                      const edk_verify_ws* ws, hipEvent_t* marks /* 4 events or NULL */, hipEvent_t bulk_done, int bulk_early,
                      hipStream_t stream);

/* workspace of the fixed-base operations for up to `capacity` items (a multiple of VERIFY_TILE) */
typedef struct edk_fixed_ws {
  size_t capacity;
  uint32_t* acc;      /* capacity * ACC_WORDS words: projective result, lane-interleaved per tile */
  uint32_t* aux;      /* capacity * 16 words: sign's secret scalars a, r between its two kernels (zeroed after use) */
  uint32_t* perm;     /* capacity words, and */
  uint32_t* lenbins;  /* 2 * EDK_LEN_BINS words: sign's ragged messages in order of length, as in edk_verify_ws */
  uint32_t* tiles;    /* EDK_TILES_WORDS words; [0] the next 64-item tile a wave of a persistent point kernel takes (zeroed by the launcher before
                         every such launch): kernels.hip, point_tile */
  const edk_dom* dom; /* NULL in the engine's own copy.  sign_step (eddsa_amd.c) hands edk_sign a COPY of the workspace with this set for
                         ed25519ctx_sign_batch* / ed25519ph_sign_batch*: both hashes then run under the prefix (kernels.hip: sign_dom).
                         Host side only, read while the pass is enqueued */
} edk_fixed_ws;

/* workspace of the batch (random-linear-combination) verification for up to `capacity` items: one
 * allocation, carved up by rlc.hip */
typedef struct edk_rlc_ws {
  size_t capacity;
  void* base;
  void* host_gok;     /* pinned host memory, one byte per group of the largest pass: the group verdicts */
} edk_rlc_ws;
#define EDK_RLC_HOST_BYTES 4096
#define EDK_RLC_MAX_KEYS 8192       /* a keyed pass of the combination (src.ks_table set) indexes its digit rows and bucket lists by key: at most
                                       one group's width of keys (rlc.hip: RLC_G); rlc_on sends wider key sets to the per-item kernels */
/* ragged messages: *perm = ws->perm filled with the pass's items in order of message length, or NULL (kernels.hip) */
hipError_t edk_msg_order(const uint32_t** perm, const edk_verify_ws* ws, const uint64_t* msg_off, const uint64_t* msg_end, size_t n,
                         hipStream_t stream);
size_t edk_rlc_ws_bytes(size_t capacity);
size_t edk_rlc_hook_offset(size_t capacity);   /* of the workspace's test-hook word (256 bytes to zero at allocation; rlc.hip: k_rlc_bucket) */
/* for eddsa_amd_debug_rlc_snapshot (the debug build; include/eddsa_amd_debug.h has the region numbers): `count` pieces of `bytes`
 * bytes, `stride` bytes apart, from `offset` in the workspace - one region of a pass of n items, trimmed to its items and groups.
 * Returns 0 when `region` names none or such a pass does not fit the workspace */
typedef struct edk_rlc_span { size_t offset, bytes, stride, count; } edk_rlc_span;
int edk_rlc_region(edk_rlc_span* out, int region, size_t capacity, size_t n);
hipError_t edk_rlc_note_per_item(uint32_t* stats, size_t n, hipStream_t stream);
/* one pass in two halves: edk_verify_rlc enqueues the combination and the copy of the group verdicts to rws->host_gok;
 * the caller synchronises `stream`; edk_verify_rlc_fallback hands the groups that did not pass to the per-item kernels */
hipError_t edk_verify_rlc(uint8_t* ok, uint32_t* stats, const edk_verify_src* src, size_t n, const uint32_t* base16,
                          const edk_verify_ws* ws, const edk_rlc_ws* rws, hipStream_t stream);
hipError_t edk_verify_rlc_fallback(uint8_t* ok, const edk_verify_src* src, size_t n, const uint32_t* base16,
                                   const edk_verify_ws* ws, const edk_rlc_ws* rws, hipStream_t stream);

hipError_t edk_x25519(uint8_t* out, const uint8_t* scalars, const uint8_t* points, size_t n,
                      const edk_fixed_ws* ws, hipStream_t stream);
hipError_t edk_genpub(uint8_t* pubs, const uint8_t* secs, size_t n, const uint32_t* comb,
                      const edk_fixed_ws* ws, hipStream_t stream);
/* msg_end: as in edk_verify_src (NULL with msg_off == NULL) */
hipError_t edk_sign(uint8_t* sigs, const uint8_t* secs, const uint8_t* pubs, const uint8_t* msgs,
                    const uint64_t* msg_off, const uint64_t* msg_end, size_t msg_len, size_t n, const uint32_t* comb,
                    const edk_fixed_ws* ws, hipStream_t stream);
hipError_t edk_x25519_base(uint8_t* out, const uint8_t* scalars, size_t n, const uint32_t* comb,
                           const edk_fixed_ws* ws, hipStream_t stream);
/* test surface (include/eddsa_amd_debug.h).  edk_debug_fail_in: nth > 0 arms the fault (the nth checked HIP call of the
 * verify passes from now on reports hipErrorUnknown instead of being made) and restarts the count; 0 disarms; < 0 only
 * returns the number of checked calls made since the count was restarted */
int edk_debug_fail_in(int nth);
/* the checked calls are counted only while this is on (armed hooks): an unarmed process bumps no shared counter in its passes */
void edk_debug_counting(int on);
hipError_t edk_pk_to_x(uint8_t* out, const uint8_t* in, size_t n, hipStream_t stream);
hipError_t edk_sk_to_x(uint8_t* out, const uint8_t* in, size_t n, hipStream_t stream);

#ifdef __cplusplus
}
#endif
