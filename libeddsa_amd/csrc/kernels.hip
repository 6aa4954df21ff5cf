// kernels.hip - the batched Ed25519 / X25519 kernels for gfx950 and their launchers.
//
// One curve operation per lane, limbs in registers (fe25519.h), no MFMA.  What a lane computes is
// in lanes.h; this file maps items to lanes, stages the shared tables in LDS and moves the packed,
// item-major byte arrays of the batch API (include/eddsa_amd.h) in and out.
//
//   k_x25519_*       x25519.c:129-150 do_x25519                      (config 3)
//   k_verify_*       ed25519-sha512.c:148-181 ed25519_verify        (config 2, 4): prepare / halve / main_half by
//                    default (half-length scalars, halve.h), prepare / main / finish for the full-length route,
//                    *_pair / *_quad forms for small passes; for keys that are not curve points k_verify_exact_quad (short
//                    work lists, four lanes per item) and k_verify_exact_lane_setup / _chain (long ones, two items per lane)
//   k_cofactor_*     the opt-in cofactored equation [8](S B - t A - R) = 0 over the items a pass rejected (cofactor_lanes.h)
//   k_sign_*         ed25519-sha512.c:84-123 sign                    (config 5)
//   k_dom_challenge, k_sign_dom_*             Ed25519ctx / Ed25519ph, RFC 8032 5.1: the same with dom2 in front of the hashes
//   k_genpub_point + k_encode_finish          ed25519-sha512.c:53-67 genpub
//   k_x25519_base_*  x25519.c:158-197 do_x25519_base
//   k_pk_to_x        ed25519-sha512.c:187-232 pk_ed25519_to_x25519
//   k_sk_to_x        ed25519-sha512.c:239-256 sk_ed25519_to_x25519
//   k_init_tables    generates what the reference ships as lib/ed_lookup64.h
//   k_keyset_build, k_verify_*_keyed          key-set verification (keyed_kernels.h): the key's table by index
//   k_keyset_comb_build, k_verify_main_comb_keyed   comb key sets (keyed_kernels.h): a comb per key, both scalars fixed-base
//   k_signer_build, k_sign_keyed_*            signer sets (signer_kernels.h): the secret scalar, the prefix and A by key index
//   k_point_classify                          point classification (classify_kernels.h): curve, canonical, small and prime order
//   k_point_muladd_prepare, _finish           [m]P + [a]B (muladd_kernels.h): set-up and encoding around k_verify_main
//   k_scatter_challenge, k_scatter_len_*      ed25519_verify_scattered (scatter_kernels.h): gather and hash in front of a digest pass
#include "eddsa_kernels.h"
#include "edk_keyed.h"
#include "edk_signer.h"
#include "edk_classify.h"
#include "edk_muladd.h"
#include "edk_scatter.h"
#include "edk_checked.h"
#include "kernel_io.h"
#include "lanes.h"
#include "policy_lanes.h"
#include "cofactor_lanes.h"
#include "quad_lanes.h"
#include "eddsa_amd.h"

#include <atomic>

namespace ed {

constexpr int BLOCK = VERIFY_TILE;         // a block is a tile of the workspaces (kernel_io.h)

// one verify item: R, S, A as words and the message span (packed arrays or fixed-size records)
ED_DEV void verify_item(uint32_t rw[8], uint32_t sw[8], uint32_t aw[8], const uint8_t*& m, size_t& mlen,
                        const edk_verify_items& s, size_t item) {
  load32(rw, s.sigs, item, s.sig_stride);
  load32(sw, s.sigs + 32, item, s.sig_stride);
  load32(aw, s.pubs, item, s.pub_stride);
  msg_span(m, mlen, s.msgs, s.msg_off, s.msg_end, s.msg_len, s.msg_stride, item);
}

// Append to a work list: the lanes of the wave that `want` a slot get consecutive ones from ONE atomic (a pass of 2^20
// items would otherwise send as many atomics to one address).  Callable under divergence: the ballot counts the active
// lanes only, and the leader is one of them.
ED_DEV uint32_t wave_append(uint32_t* counter, bool want) {
  const uint64_t m = __ballot(want);
  if (m == 0) return 0;
  const unsigned lane = __lane_id();
  const int leader = __ffsll((unsigned long long)m) - 1;
  uint32_t base = 0;
  if ((int)lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, leader);
  return base + (uint32_t)__popcll(m & (((uint64_t)1 << lane) - 1));
}

// ---------------------------------------------------------------------------------------------

// X25519 in two kernels, like the fixed-base operations: the ladder leaves (x2 : z2) in the point
// workspace (X and Z slots), the finish kernel inverts z2 once per eight items per lane
// (finish_batch8 below) -- the per-item inversion was 7 % of the work.
__global__ void __launch_bounds__(BLOCK, 4)
k_x25519_ladder(uint32_t* accout, const uint8_t* scalars, const uint8_t* points, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const size_t item = i < n ? i : n - 1;
  uint32_t s[8], pt[8];
  load32(s, scalars, item, 32);
  load32(pt, points, item, 32);
  fe x2, z2;
  x25519_ladder_lane(x2, z2, s, pt);
  if (i >= n) return;                            // an idle lane must not leave a copy of the last item's secret
  uint32_t* o = acc_column(accout, blockIdx.x, threadIdx.x);
#pragma unroll
  for (int j = 0; j < 10; j++) { o[acc_at(ACC_X, j)] = x2.v[j]; o[acc_at(ACC_Z, j)] = z2.v[j]; }
}

// small passes: four lanes per item (quad_lanes.h: x25519_ladder_quad); writes the same workspace slots
constexpr size_t X25519_QUAD_MAX_N = (size_t)1 << 14;
__global__ void __launch_bounds__(BLOCK, 2)
k_x25519_ladder_quad(uint32_t* accout, const uint8_t* scalars, const uint8_t* points, size_t n) {
  const size_t i = ((size_t)blockIdx.x * BLOCK + threadIdx.x) >> 2;          // quads are all-or-nothing
  if (i >= n) return;
  const int q = (int)(threadIdx.x & 3u);
  uint32_t s[8], pt[8];
  load32(s, scalars, i, 32);
  load32(pt, points, i, 32);
  fe r;
  x25519_ladder_quad(r, s, pt, q);
  if (q > 1) return;                             // lane 0: x2 -> the X slot, lane 1: z2 -> the Z slot
  acc_put(acc_column(accout, i / BLOCK, i % BLOCK), q == 0 ? ACC_X : ACC_Z, r);
}

__global__ void __launch_bounds__(64) k_init_tables(uint32_t* base16, uint32_t* comb) {
  const int id = blockIdx.x * 64 + threadIdx.x;
  if (id >= 2 * TABLE_BASE16_ENTRIES + TABLE_COMB_ENTRIES) return;
  if (id < TABLE_BASE16_ENTRIES) {
    table_entry_lane(base16 + (size_t)TABLE_ENTRY_WORDS * id, (uint32_t)id, 0);
  } else if (id < 2 * TABLE_BASE16_ENTRIES) {     // k * 2^128 * B: the high half of s' in the half-length verification
    table_entry_lane(base16 + (size_t)TABLE_ENTRY_WORDS * id, (uint32_t)(id - TABLE_BASE16_ENTRIES), 128);
  } else {
    const int c = id - 2 * TABLE_BASE16_ENTRIES;  // comb[i][k], c = COMB_HALF i + k
    table_entry_lane(comb + TABLE_ENTRY_WORDS * c, (uint32_t)(c % COMB_HALF) + 1, 2u * COMB_W * (uint32_t)(c / COMB_HALF));
  }
}

// the LDS image of the comb (lanes.h: comb_select), one thread per entry
__global__ void __launch_bounds__(64) k_init_comb_image(uint32_t* img, const uint32_t* comb) {
  const int id = blockIdx.x * 64 + threadIdx.x;
  if (id >= COMB_ROWS * COMB_IMG_ENTRIES) return;
  comb_image_entry_lane(img + COMB_IMG_ENTRY_WORDS * id, comb, id / COMB_IMG_ENTRIES, id % COMB_IMG_ENTRIES);
}

// ---------------------------------------------------------------------------------------------
// Ragged messages in order of length.  A lane hashes its message block by block and a wave ends with its longest message:
// with lengths drawn from 0 .. 4 KiB a pass of 2^20 items spent a third of its hashing beside finished lanes (verify 15.7 ->
// 12.4 ms, sign 13.3 -> 8.6 ms when the SAME items are handed over sorted: profiles/r05_msglen.txt).  So the kernels that hash
// take their items through a permutation - position g of the grid works on item perm[g] - built per pass by a counting sort on
// the number of 128-byte blocks, longest first (three small kernels, ~20 us); everything an item leaves in the workspace stays
// indexed by the item, so no other kernel knows.  Passes of at least MSG_ORDER_MIN_N items with an offset table only.
// ---------------------------------------------------------------------------------------------
constexpr int LEN_BINS = EDK_LEN_BINS;           // key = min(length / 128, LEN_BINS - 1), counted from the long end
constexpr size_t MSG_ORDER_MIN_N = (size_t)1 << 12;

ED_DEV uint32_t len_bin_of(size_t len) {
  const size_t blocks = len >> 7;
  return (uint32_t)(LEN_BINS - 1) - (uint32_t)(blocks < (size_t)LEN_BINS - 1 ? blocks : (size_t)LEN_BINS - 1);
}
ED_DEV uint32_t len_bin(const uint64_t* off, const uint64_t* end, size_t item) {
  uint64_t lo, hi;
  ragged_span(lo, hi, off, end, item);                         // (the clamped span: what the hashing kernels will read)
  return len_bin_of((size_t)(hi - lo));
}

// bins[b] += items of bin b (per block in LDS first: a pass whose messages all have one length would otherwise send 2^20 atomics to one word)
__global__ void __launch_bounds__(BLOCK) k_len_count(uint32_t* bins, const uint64_t* off, const uint64_t* end, size_t n) {
  __shared__ uint32_t h[LEN_BINS];
  for (int b = threadIdx.x; b < LEN_BINS; b += BLOCK) h[b] = 0;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i < n) atomicAdd(&h[len_bin(off, end, i)], 1u);
  __syncthreads();
  for (int b = threadIdx.x; b < LEN_BINS; b += BLOCK) if (h[b]) atomicAdd(bins + b, h[b]);
}
// bins[LEN_BINS + b] = items in the bins before b (one block)
__global__ void __launch_bounds__(BLOCK) k_len_starts(uint32_t* bins) {
  __shared__ uint32_t part[BLOCK];
  constexpr int PER = LEN_BINS / BLOCK;
  uint32_t local[PER], sum = 0;
#pragma unroll
  for (int k = 0; k < PER; k++) { local[k] = sum; sum += bins[threadIdx.x * PER + k]; }
  part[threadIdx.x] = sum;
  __syncthreads();
  uint32_t before = 0;
  for (int t = 0; t < (int)threadIdx.x; t++) before += part[t];
#pragma unroll
  for (int k = 0; k < PER; k++) bins[LEN_BINS + threadIdx.x * PER + k] = before + local[k];
}
// perm[start of the item's bin ...] = item: a block reserves its share of every bin with one atomic per bin
__global__ void __launch_bounds__(BLOCK) k_len_place(uint32_t* perm, uint32_t* bins, const uint64_t* off, const uint64_t* end, size_t n) {
  __shared__ uint32_t h[LEN_BINS], base[LEN_BINS];
  for (int b = threadIdx.x; b < LEN_BINS; b += BLOCK) h[b] = 0;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  uint32_t bin = 0, rank = 0;
  if (i < n) { bin = len_bin(off, end, i); rank = atomicAdd(&h[bin], 1u); }
  __syncthreads();
  for (int b = threadIdx.x; b < LEN_BINS; b += BLOCK) if (h[b]) base[b] = atomicAdd(bins + LEN_BINS + b, h[b]);
  __syncthreads();
  if (i < n) perm[base[bin] + rank] = (uint32_t)i;
}

// ---------------------------------------------------------------------------------------------
// Ed25519 verify, the full-length route (passes of up to QUAD_MAIN_MAX_N items, eddsa_amd_set_verify_algo(1), the
// reject mode; larger passes take the half-length route further down, which shares k_verify_prepare and the exact
// path).  Three kernels per chunk, so that each stays inside its register budget and its own I-cache footprint
// (one fused kernel spilled 4.5 KB/lane):
//   k_verify_prepare  hash, scalars -> digit words, decompress -A, table of 0..8 * -A
//   k_verify_main     the 252 doublings + 80 additions            (~85 % of the time)
//   k_verify_finish   invert Z (shared by 8 items per lane), encode, compare with R
//   k_verify_exact_quad (side stream, beside main) the reference's own chain for the items whose key is not a curve
//                     point; owns their verdict bytes
// Workspace (HBM; tile = 256 items):
//   digits [item]                      t + 0x88.., S + 0x80.. as little-endian words
//   table  [item][entry][word]         an entry = ymx | ypx | t2d | z2 packed into 255 bits each (fe_pack), one 128-byte line
//   acc    [tile][word][lane]          X, Y, Z of the result
//   flags  [item]                      VERIFY_WINDOWED: A decoded to a curve point; VERIFY_Z_USABLE (set by finish)
//   offlist[..], offcount              items whose A is off the curve, for k_verify_exact_quad
// (the sizes: edk_layout.h; the slots' accessors and the flag bits: kernel_io.h)
// ---------------------------------------------------------------------------------------------

// DIGEST: the caller supplied SHA-512(R || A || M) (ed25519_verify_digests*): the item's 64 bytes lie in the message slot of
// src and nothing is hashed.  Which instantiation runs is the launcher's choice (src.digest), never a lane's.
template <bool DIGEST>
__global__ void __launch_bounds__(BLOCK, 2)
k_verify_prepare(edk_verify_items src, size_t n, uint32_t* digits,
                 uint32_t* table, uint8_t* flags, uint32_t* onlist, uint32_t* offlist, uint32_t* offcount, int all_exact, const uint32_t* perm) {
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  // position g of the grid works on item perm[g] (ragged messages in order of length, above) or on item g
  const size_t item = perm ? perm[g < n ? g : n - 1] : (g < n ? g : n - 1);
  const size_t i = g < n ? item : g;             // its slot of the workspace: the item's own; idle lanes redo the last item into a slot past the pass
  uint32_t aw[8], sw[8], tw[8];
  if constexpr (DIGEST) {
    uint32_t dw[16];
    load32(aw, src.pubs, item, src.pub_stride);
    load32(dw, src.msgs, item, src.msg_stride);
    load32(dw + 8, src.msgs + 32, item, src.msg_stride);
    verify_digest_lane(tw, dw);
  } else {
    uint32_t rw[8];
    const uint8_t* m; size_t mlen;
    load32(rw, src.sigs, item, src.sig_stride);
    load32(aw, src.pubs, item, src.pub_stride);
    msg_span(m, mlen, src.msgs, src.msg_off, src.msg_end, src.msg_len, src.msg_stride, item);
    verify_hash_lane(tw, rw, aw, m, mlen);
  }
  uint32_t* d = digits + digit_slot(i);
  store8(d, tw);
  load32(sw, src.sigs + 32, item, src.sig_stride);       // S is fetched only now: nothing to hold across the hash
  verify_s_lane(sw);
  store8(d + 8, sw);
  const bool oncurve = verify_table_lane(table + table_slot(i), aw);
  // keys that are not curve points go to the exact (reference-order) kernels: append to their work
  // list (all_exact, a self-check mode: every item does, and the windowed result is not used)
  const bool windowed = oncurve && !all_exact;
  flags[i] = (uint8_t)(windowed ? VERIFY_WINDOWED : 0);
  // Two work lists: the items the windowed evaluation decides (the half-length route's k_verify_halve and
  // k_verify_main_half run over THIS list, not over the pass: a caller who sends nothing but garbage keys then pays for
  // the exact path only, not for a windowed evaluation whose result is discarded on top), and the exact path's.
  const bool live = g < n;
  const uint32_t on_slot = wave_append(offcount + EDK_ONLIST_WORD, live && windowed);
  if (live && windowed) onlist[on_slot] = (uint32_t)i;
  const uint32_t off_slot = wave_append(offcount + EDK_OFFLIST_WORD, live && !windowed);
  if (live && !windowed) offlist[off_slot] = (uint32_t)i;
}

// The exact path: ed25519-sha512.c:148-181 replayed in the reference's own order for the items k_verify_prepare (and, on
// the half-length route, k_verify_halve) listed, with four lanes per item (quad_lanes.h), so that a chain step is a
// squaring and a multiplication deep.  Set-up (joint sparse form of the two scalars and the addends Q, B, Q+B, Q-B, all
// from what k_verify_prepare left in the workspace) and chain are one kernel on the side stream beside k_verify_main,
// which is launched with MAIN_LDS_RESERVE and therefore leaves wave slots, registers and a little LDS free on every CU.
// Why this shape (tools/exact_path_time.py, tools/exact_trace.py timelines, profiles/r02_verify_ab.txt):
// k_verify_main's grid for 2^20 items is an exact number of rounds of resident blocks, so it has no slack:
// whatever holds up ONE of its blocks -- a displaced tile (round 1: chain blocks of four waves at 149 VGPRs
// took a main block's place), or main waves starved by a long chain wave of raised priority on their SIMD --
// costs the latency of one tile at the end (0.7 ms), for 512 off-curve keys as for 65536.  The remedy is to
// disturb every SIMD a little instead of a few a lot: single-wave chain blocks (16 items) spread over the
// whole chip, the short four-lane chain, no displacement.  Cost of the exact path on config 2: 0.94 ms in
// round 1, 0.4 ms in round 2, 0.05 ms now (profiles/r04_small_grid.txt has what it costs passes of one or two rounds).
// The work list may be as long as the pass (a caller can send nothing but garbage keys: ed_import never fails, ed.c:100-149).
// This kernel serves SHORT lists - below EXACT_LANE_MIN_LISTED entries in passes of EXACT_LANE_MIN_N items or more, every list of
// a smaller pass (at most its 65 535 items: EDK_EXACT_SLOTS scratchpad slots, 4096 waves of 16) - and ends at once when the list
// is longer: that one belongs to k_verify_exact_lane_* below, one lane per item at the occupancy of a kernel that fills the
// chip.  (Rounds 1-4 walked long lists with this kernel in stretches of 65 536: 34 M items/s, and a pass of 2^20 random keys
// 26 ms; now 14: profiles/r05_exact_lane.txt.)
constexpr int QUAD_BLOCK = 256;                  // k_verify_main_quad
constexpr int QUAD_CHAIN_BLOCK = 64;             // k_verify_exact_quad: one wave, up to 16 items
constexpr int QUAD_CHAIN_ITEMS = QUAD_CHAIN_BLOCK / 4;
constexpr int QUAD_SPREAD_WAVES = 256;           // a short work list is spread over this many waves, a long one packed 16 items to the wave
static_assert((size_t)EDK_EXACT_SLOTS * QUAD_ITEM_WORDS * 4 <= EDK_EXACT_PAD_BYTES, "scratchpad too small");
static_assert(EDK_EXACT_SLOTS % QUAD_CHAIN_ITEMS == 0, "whole waves");

// Set-up and chain in ONE kernel (round 2 had two, 0.37-0.75 + 0.75 ms however few the items: a pass of 2^14 items
// with a handful of off-curve keys took 1.02 ms instead of 0.39; now 0.79).  A wave carries 16 items when the list is
// long - beside a full k_verify_main_half that is what costs it least - and as few as one when it is short (up to
// QUAD_SPREAD_WAVES waves: a small pass waits for this kernel, and a wave with one item skips the addition of every step
// without digits, quad_lanes.h; spreading 540 items of a 2^16-item pass one to the wave was measured slower than 34
// full waves - 1.28 against 1.18 ms - their instructions are taken from the main kernel's waves).  The digit pairs
// live in LDS (33 words per item), the addends in the HBM scratchpad, one slot per quad of the grid.
__global__ void __launch_bounds__(QUAD_CHAIN_BLOCK, 2)
k_verify_exact_quad(uint8_t* ok, const uint8_t* sigs, size_t sig_stride, const uint32_t* digits, const uint32_t* table,
                    const uint32_t* offlist, const uint32_t* offcount, const uint32_t* base16, uint32_t* pad, int dense,
                    uint32_t lane_min) {
  __shared__ uint32_t lds_dig[QUAD_CHAIN_ITEMS * QUAD_DIGIT_WORDS];
  __builtin_amdgcn_s_setprio(3);                 // small passes wait for the chain: 1-3 % there; no difference beside a full k_verify_main
  const size_t listed = *offcount;
  if (listed == 0) return;
  if (lane_min != 0 && listed >= lane_min) return;   // a list this long belongs to the one-lane kernels (k_verify_exact_lane_*)
  const size_t count = listed < (size_t)EDK_EXACT_SLOTS ? listed : (size_t)EDK_EXACT_SLOTS;   // (never more: see the launcher's static_assert)
  // items per wave: 16 in a pass whose main kernel outlasts the chain anyway (dense: the chain's total work is what counts
  // there - every wave issues the chain's 300 k instructions however few items it carries, and in the host pipeline, where
  // the chunks' kernels fill one another's gaps, 557 items spread three to the wave cost a 2^16-item chunk a quarter of its
  // main kernel's work on top); in a small pass, which WAITS for the chain, as few as one (its wave then skips the
  // addition of every step without digits)
  size_t per = dense ? (size_t)QUAD_CHAIN_ITEMS : (count + QUAD_SPREAD_WAVES - 1) / QUAD_SPREAD_WAVES;
  per = per > (size_t)QUAD_CHAIN_ITEMS ? (size_t)QUAD_CHAIN_ITEMS : per;
  const size_t quad = threadIdx.x >> 2;          // quads are all-or-nothing
  const size_t g = (size_t)blockIdx.x * per + quad;
  if (quad >= per || g >= count) return;
  const int q = (int)(threadIdx.x & 3u);
  const size_t i = offlist[g];
  uint32_t* item = pad + g * QUAD_ITEM_WORDS;
  uint32_t* dig = lds_dig + quad * QUAD_DIGIT_WORDS;
  verify_exact_setup_quad(digits + digit_slot(i), table + table_slot(i), base16 + TABLE_ENTRY_WORDS, item, dig, q);
  __syncthreads();                               // one wave: orders the quad's stores (LDS digits, HBM addends) before the other lanes' loads
  uint32_t rw[8];
  load32(rw, sigs, i, sig_stride);
  const bool same = verify_exact_chain_quad(rw, item, dig, q);
  if (q == 1) ok[i] = (uint8_t)same;
}

// The exact path for LONG work lists: lanes.h: verify_exact_setup_table_lane, one lane per item, then exact_pair_iterations,
// TWO items per lane sharing one addition phase - two kernels of persistent blocks on the side stream, ahead of the four-lane
// launch.  Which form serves a pass is decided on the device, by the length of the list: below `min_listed` entries these
// kernels end at once and k_verify_exact_quad does the work (its single-wave blocks answer soonest and disturb a full main
// kernel least); from there on it is the other way round - a wave of the four-lane chain carries 16 items through 300 k
// instructions (1.2 M lane slots per item), a wave of this one 128 through 1.2 M (594 k per item), and a caller who sends
// nothing but garbage keys (47 % of random strings are no curve point) is served at the rate of a kernel that fills the chip:
// profiles/r05_exact_lane.txt.
// The set-up writes into the item's OWN workspace - Q + B and Q - B over entries 2 and 3 of its table, the digit string
// over the first words of its rtable slot - which nobody reads for such an item: the windowed kernels skip it (on the
// half-length route they do not even visit it, see k_verify_prepare) or discard what they compute from it.
// Work is handed out to WAVES, one (stretch, tile) unit at a time from a counter: a tile is 128 entries of the list (two per lane),
// a stretch EXACT_PAIR_ITERS iterations of the walk (lanes.h: exact_pair_iterations; the last one runs to the end), the accumulators cross from stretch to stretch through the items' workspace and
// a wave that draws stretch s of a tile waits for the tile's stretch s - 1 (tile_done; units are drawn in the order stretch 0 of
// every tile, stretch 1 of every tile, ..., so the wait is over before it starts unless the list is shorter than the chip).
// Why not one chain per lane per launch slot: beside k_verify_main_half half of these blocks become resident late, and with a
// fixed share of 4 chains of 2.5 ms each per lane the kernel's tail was 3 ms of a 17 ms pass (profiles/r05_exact_lane.txt).
constexpr uint32_t EXACT_CHAIN_COST = 594;       // executed instructions per item of k_verify_exact_lane_chain, thousands
constexpr unsigned EXACT_LANE_BLOCKS = 512;      // two resident blocks per CU
constexpr int EXACT_DIGITS_AT = 0, EXACT_STATE_AT = 64;   // words of the item's rtable slot: the digit string; the accumulator between stretches (lines of its own)
static_assert(EXACT_STATE_AT + EXACT_STATE_WORDS + 2 <= VERIFY_ITEM_TABLE_WORDS, "the accumulator and the walk (lanes.h: exact_walk_store) fit the slot");
__global__ void __launch_bounds__(BLOCK, 2)
k_verify_exact_lane_setup(const uint32_t* digits, uint32_t* table, uint32_t* rtable, const uint32_t* offlist, uint32_t* offcount,
                          const uint32_t* base16, uint32_t* tile_done, uint32_t min_listed) {
  const size_t listed = *offcount;
  if (listed < min_listed) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) exact_bentry_store(offcount + EDK_BENTRY_WORD);   // (the same bytes in every pass)
  for (size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x; g < listed; g += (size_t)gridDim.x * BLOCK) {
    if ((g & 63) == 0) tile_done[g >> 6] = 0;
    const size_t i = offlist[g];
    verify_exact_setup_table_lane(table + table_slot(i), rtable + table_slot(i) + EXACT_DIGITS_AT, 1, digits + digit_slot(i), base16 + TABLE_ENTRY_WORDS);
  }
}

__global__ void __launch_bounds__(BLOCK, 2)
k_verify_exact_lane_chain(uint8_t* ok, const uint8_t* sigs, size_t sig_stride, const uint32_t* table, uint32_t* rtable,
                          const uint32_t* offlist, uint32_t* offcount, uint32_t* tile_done, uint32_t min_listed, size_t n,
                          uint32_t main_cost, int main_all, uint32_t* status) {
  const size_t listed = *offcount;
  if (listed < min_listed) return;
  // a tile is 128 entries of the list: a lane walks TWO chains, entries L and 64 + L of the tile (lanes.h: exact_pair_iterations)
  const unsigned tiles = (unsigned)((listed + 127) / 128), units = tiles * (unsigned)EXACT_SEGS;
  const unsigned lane = threadIdx.x & 63u;
  // no more waves than tiles: one that drew a later stretch of a tile still in its first would only hold, waiting, a slot
  // that a wave of k_verify_main_half could use
  unsigned waves = tiles;
  // ... and no more than this kernel's SHARE of the wave slots: its persistent waves keep what they take until the list is
  // done, the main kernel beside it fills what is left, and whichever ends first leaves the other to its own tail.  With the
  // slots split like the work (main_cost: the main kernel's instructions per item in thousands, over the on-curve list or -
  // main_all - over the whole pass) the two end together: a pass with every second key random 13.7 -> 12.8 ms, all random unchanged
  // (profiles/r05_exact_lane.txt).
  {
    const uint64_t mine = (uint64_t)listed * EXACT_CHAIN_COST;
    const uint64_t other = (uint64_t)(main_all ? n : (size_t)offcount[EDK_ONLIST_WORD]) * main_cost;
    const uint64_t slots = (uint64_t)gridDim.x * (BLOCK / 64);
    const uint64_t share = (slots * mine + (mine + other) - 1) / (mine + other);
    // (never fewer than 512, or than there are tiles: a short list is done soonest with a wave per tile, long before the main kernel)
    const uint64_t least = tiles < 512u ? tiles : 512u;
    // (and only when the main kernel has the larger part: a chain that is most of the pass is soonest done with every slot it can get
    // - all keys random, a share of 0.70: 14.3 ms with all slots, 14.7 with its share)
    if (share * 5 < slots * 3 && share < waves) waves = (unsigned)(share < least ? least : share);
  }
  if ((blockIdx.x * (unsigned)BLOCK + threadIdx.x) / 64u >= waves) return;
  for (;;) {
    unsigned u = 0;
    if (lane == 0)
      u = __hip_atomic_load(offcount + EDK_STALL_WORD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 ? units
                                                                                                        : atomicAdd(offcount + EDK_EXACT_UNIT_WORD, 1u);
    u = (unsigned)__builtin_amdgcn_readfirstlane((int)u);
    if (u >= units) break;
    const unsigned seg = u / tiles, tile = u - seg * tiles;
    if (seg > 0) {
      // the tile's previous stretch, possibly on another CU: its stores are in L2 once its count is; the acquire drops this
      // CU's stale lines.
      // Why the wait ends: units are drawn in order from ONE counter - stretch s - 1 of every tile before stretch s of any -
      // so the unit waited for was drawn earlier, by a wave that is resident (a wave draws only while it runs) and that
      // itself waits, if at all, for a unit drawn earlier still: the oldest unit in flight waits for nothing.
      // Why it is bounded all the same: if that wave never publishes (a fault in it; the test hook below), spinning for
      // ever would turn one lost hand-off into a hung queue.  After EDK_EXACT_PATIENCE polls - seconds, where a stretch
      // takes a millisecond - the wave raises EDK_STALL_WORD and leaves; every wave looks at that word before it draws or
      // while it waits, so the launch drains, and the host side returns EDDSA_AMD_STALLED for the pass.
      uint32_t stalled = 0;
      if (lane == 0) {
        uint32_t polls = 0;
        while (__hip_atomic_load(tile_done + tile, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < seg) {
          if (++polls == EDK_EXACT_PATIENCE || __hip_atomic_load(offcount + EDK_STALL_WORD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
            stalled = 1;
            break;
          }
          __builtin_amdgcn_s_sleep(16);
        }
        if (stalled) {
          __hip_atomic_store(offcount + EDK_STALL_WORD, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (status) __hip_atomic_store(status, EDK_STATUS_STALLED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
      }
      if (__builtin_amdgcn_readfirstlane((int)stalled)) break;
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    const size_t ga = (size_t)tile * 128 + lane, gb = ga + 64;
    const bool live_a = ga < listed, live_b = gb < listed;
    const uint32_t ia = offlist[live_a ? ga : listed - 1], ib = offlist[live_b ? gb : listed - 1];   // (an idle half walks nothing and stores nothing)
    ge ra, rb;
    exact_walk wa, wb;
    if (seg == 0) {
      ge_neutral(ra); ge_neutral(rb);
      wa = exact_walk_start(rtable + table_slot(ia) + EXACT_DIGITS_AT, 1, live_a);
      wb = exact_walk_start(rtable + table_slot(ib) + EXACT_DIGITS_AT, 1, live_b);
    } else {
      exact_walk_load(ra, wa, rtable + table_slot(ia) + EXACT_STATE_AT);
      exact_walk_load(rb, wb, rtable + table_slot(ib) + EXACT_STATE_AT);
      if (!live_a) { wa.i = -1; wa.pend = false; }
      if (!live_b) { wb.i = -1; wb.pend = false; }
    }
    const bool last = seg == (unsigned)EXACT_SEGS - 1;
    exact_pair_iterations(ra, wa, rb, wb, table, rtable + EXACT_DIGITS_AT, VERIFY_ITEM_TABLE_WORDS, ia, ib, offcount + EDK_BENTRY_WORD, last ? -1 : EXACT_PAIR_ITERS);
    if (last) {
      uint32_t rwa[8], rwb[8];
      load32(rwa, sigs, ia, sig_stride);
      load32(rwb, sigs, ib, sig_stride);
      bool same_a, same_b;
      exact_pair_verdicts(same_a, same_b, ra, rb, rwa, rwb);
      if (live_a) ok[ia] = (uint8_t)same_a;
      if (live_b) ok[ib] = (uint8_t)same_b;
    } else {
      if (live_a) exact_walk_store(rtable + table_slot(ia) + EXACT_STATE_AT, ra, wa);
      if (live_b) exact_walk_store(rtable + table_slot(ib) + EXACT_STATE_AT, rb, wb);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");         // every lane's accumulators are out before the count says so
      // (test hook: the first hand-off of tile EDK_WITHHOLD_WORD - 1 is never published; the word is 0 unless a test set it)
      if (lane == 0 && !(seg == 0 && offcount[EDK_WITHHOLD_WORD] == tile + 1u))
        __hip_atomic_fetch_add(tile_done + tile, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// where a lane of the one-lane main kernels works: its block's tile, its slot i of the workspace (< the capacity) and, in a keyed
// pass (keyed_kernels.h), the item's key - key 0 for a slot past the pass and for an index that names no key
struct main_pos { size_t tile, i; uint32_t key; };
template <bool KEYED = false>
ED_DEV main_pos main_at(const uint32_t* key_idx = nullptr, uint32_t count = 0, size_t n = 0) {
  main_pos p;
  p.tile = blockIdx.x;
  p.i = p.tile * BLOCK + threadIdx.x;
  p.key = 0;
  if constexpr (KEYED) {
    p.key = p.i < n ? key_idx[p.i] : 0u;
    p.key = p.key < count ? p.key : 0u;
  }
  return p;
}

__global__ void __launch_bounds__(BLOCK, 4)
k_verify_main(const uint32_t* digits, const uint32_t* table, const uint32_t* base16, uint32_t* accout) {
  const main_pos p = main_at();
  ge acc;
  verify_main_lane(acc, digits + digit_slot(p.i), table + table_slot(p.i), base16);
  acc_put_xyz(acc_column(accout, p.tile, threadIdx.x), acc);
}

// ---------------------------------------------------------------------------------------------
// Half-length verification (halve.h), one lane per item: the route of passes above HALF_QUAD_MAX_N items (smaller
// ones: k_verify_prepare_pair + k_verify_main_half_quad further down):
//   k_verify_prepare    as above
//   k_verify_halve      (u, v) with v = u t mod 8l from t; s' = |u| S; decompress R strictly, table of 0..8 * -R'
//   k_verify_main_half  132 doublings + 68 + 16 additions, neutral-element test, verdict byte
// No finish kernel: "is the neutral element" needs no inversion.  Items the pair search gives up on join the
// off-curve keys on the exact path's work list (so the list is complete only after k_verify_halve).
// Workspace beside the one above: hdigits [item], rtable like table; flags: VERIFY_WINDOWED: this path owns the verdict,
// VERIFY_R_CANONICAL: R is a canonical encoding of a curve point (kernel_io.h).
// ---------------------------------------------------------------------------------------------
template <int BITS>
__global__ void __launch_bounds__(BLOCK, 2)
k_verify_halve(const uint8_t* sigs, size_t sig_stride, const uint32_t* digits, uint32_t* hdigits,
               uint32_t* rtable, uint8_t* flags, const uint32_t* onlist, uint32_t* offlist, uint32_t* offcount) {
  // over the list of items the windowed evaluation decides (k_verify_prepare), not over the pass: the grid is sized for
  // the pass, the blocks beyond the list end at once
  const size_t slot = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (slot >= (size_t)offcount[EDK_ONLIST_WORD]) return;
  const size_t i = onlist[slot], item = i;
  const uint8_t fl = flags[i];
  uint32_t tdig[8], sdig[8], hd[HALF_DIGIT_WORDS];
  load8(tdig, digits + digit_slot(i));
  load8(sdig, digits + digit_slot(i) + 8);
  verify_half_scalars_lane<BITS>(hd, tdig, sdig);
  if ((hd[HALF_STATUS_WORD] & HALF_PAIR_REFUSED) != 0) atomicAdd(offcount + EDK_REFUSED_WORD, 1u);   // never seen (diagnostic)
  hdigits_store(hdigits, i, hd);
  uint32_t rw[8];
  load32(rw, sigs, item, sig_stride);
  const bool rvalid = verify_half_point_lane(rtable + table_slot(i), rw);
  // An item without a short pair ("long", lanes.h) joins the exact path's work list here: k_verify_main_half's grid
  // has no slack, and both alternatives measured slower at 2^20 items - the long loop inside that kernel for the
  // waves that contain such an item (one in 180: 7.2 -> 7.8 ms) and a separate four-lane kernel for them beside it
  // (7.4 -> 7.65 ms).  Small passes, whose waves have the chip to themselves, do run the long loop in place
  // (k_verify_main_half_quad).
  const bool mine = (fl & VERIFY_WINDOWED) != 0 && (hd[HALF_STATUS_WORD] & HALF_LONG) == 0;
  flags[i] = (uint8_t)((mine ? VERIFY_WINDOWED : 0) | (rvalid ? VERIFY_R_CANONICAL : 0));
  if ((fl & VERIFY_WINDOWED) != 0 && !mine) offlist[atomicAdd(offcount + EDK_OFFLIST_WORD, 1u)] = (uint32_t)i;
}

// dynamic LDS the main kernels are launched with: what keeps a third block off the CU, and where k_verify_main_half keeps its digit words
constexpr unsigned MAIN_LDS_RESERVE = 74 * 1024;   // (2 x 74 of the CU's 160 KB: a third block does not fit, four waves of k_verify_exact_quad do)
// (measured and dropped: three blocks of 128 lanes with 50 KB each, 1.5 waves per SIMD - a resident set of 226 MB, which fits the
// 256 MB Infinity Cache: profiles/r03_verify_ab.txt)
constexpr int MAIN_HALF_BLOCK = BLOCK, MAIN_HALF_BLOCKS_PER_CU = 2;
// The lane's digit words go to LDS once (word w of lane t at [w][t]: no bank conflicts); returns the lane's column.  Read from
// memory window by window they were the hottest lines of L2 - one per resident item, 16 MB of its 32 - and L2 is what the table
// lines need: its hits are worth 12 % to k_verify_main_half (profiles/r04_main_half_loads_ab.txt), and with the digits out of it
// the pass gained 1.5 %.  (The launch reserves MAIN_LDS_RESERVE bytes per block anyway; this uses 28 KB of them.)
ED_DEV const uint32_t* stage_digit_words(const uint32_t* hd) {
  extern __shared__ uint32_t digit_words[];
  const uint4* g = reinterpret_cast<const uint4*>(hd);
#pragma unroll
  for (int q = 0; q < HALF_DIGIT_WORDS / 4; q++) {
    const uint4 v = g[q];
    digit_words[(4 * q) * MAIN_HALF_BLOCK + threadIdx.x] = v.x; digit_words[(4 * q + 1) * MAIN_HALF_BLOCK + threadIdx.x] = v.y;
    digit_words[(4 * q + 2) * MAIN_HALF_BLOCK + threadIdx.x] = v.z; digit_words[(4 * q + 3) * MAIN_HALF_BLOCK + threadIdx.x] = v.w;
  }
  return digit_words + threadIdx.x;
}
// WITH_LONG: after k_verify_prepare_pair (mid-size passes), which leaves the items without a short pair to this kernel:
// the wave of such an item (2 in 10^7 with the wide search) runs the long loop
template <int WINDOWS, bool WITH_LONG = false>
__global__ void __launch_bounds__(MAIN_HALF_BLOCK, MAIN_HALF_BLOCKS_PER_CU)
k_verify_main_half(uint8_t* ok, const uint32_t* hdigits, const uint32_t* table, const uint32_t* rtable,
                   const uint32_t* base16, const uint8_t* flags, const uint32_t* onlist, const uint32_t* offcount) {
  // over the list of items the windowed evaluation decides (k_verify_prepare / k_verify_prepare_pair), like k_verify_halve
  const size_t slot = (size_t)blockIdx.x * MAIN_HALF_BLOCK + threadIdx.x;
  if (slot >= (size_t)offcount[EDK_ONLIST_WORD]) return;
  const size_t i = onlist[slot];
  const uint32_t* hl = stage_digit_words(hdigits + hdigit_slot(i));
  const bool long_loop = WITH_LONG && __any((hl[HALF_STATUS_WORD * MAIN_HALF_BLOCK] & HALF_LONG) != 0);
  // a zero digit reads item 0's entry 0 - the neutral element, like every item's own: one line for the chip, not one per item
  const bool neutral = verify_half_main_lane<WITH_LONG, WINDOWS>(hl, table + table_slot(i), rtable + table_slot(i), base16, long_loop, MAIN_HALF_BLOCK, table);
  // (an item without VERIFY_WINDOWED was handed to the exact path by k_verify_halve; reject mode never comes here)
  half_verdict_store(ok, i, flags[i], neutral, 1);
}

// ---------------------------------------------------------------------------------------------
// "finish" kernels: everything that needs an inversion (ed_export ed.c:161, x25519.c:192) shares
// ONE inversion between FINISH_K items per lane (Montgomery's trick: 254 S + 11 M once, plus three
// multiplications per item).  Lane t of block b handles lane t of tiles b*K .. b*K+K-1 of the
// lane-interleaved point workspace (kernel_io.h: acc_column), so every access stays coalesced.
// A policy P supplies  den(k, z, good): the value to invert for item k (1 when there is nothing to
// invert: item past the end, rejected key, or a zero denominator, which must not poison the shared
// product) and  item(k, zinv, good): the rest of the work of item k.
// ---------------------------------------------------------------------------------------------
constexpr int FINISH_K = 8;
// k_verify_main uses no LDS; launching it with 74 KB (78 until round 3) of dynamic LDS per block limits it to two blocks (eight
// waves) per CU.  Measured (profiles/r02_verify_ab.txt): the kernel itself is about 1 % FASTER that way (two
// waves per SIMD already saturate VALU issue; fewer resident tables), and the exact path's waves fit beside
// it on every CU without taking the place of any of its blocks.

struct finish_pos {
  size_t tile, i;            // tile index and global item index of slot k for this lane
  const uint32_t* acc;       // this lane's column of the tile (kernel_io.h: acc_column)
};
ED_DEV finish_pos finish_at(int k, const uint32_t* accin, int K) {
  finish_pos p;
  p.tile = (size_t)blockIdx.x * K + k;
  p.i = p.tile * BLOCK + threadIdx.x;
  p.acc = acc_column(accin, p.tile, threadIdx.x);
  return p;
}
// i = the lane's global item slot (tile i / BLOCK, lane i % BLOCK), whatever the block size
ED_DEV void acc_store(uint32_t* accout, size_t i, const ge& p) {
  acc_put_xyz(acc_column(accout, i / BLOCK, i % BLOCK), p);
}

// Phase A multiplies the eight denominators together, inverts once and unwinds.  Each denominator is
// written to its Z slot by den(), each prefix product z0 ... zk to the fourth slot (ACC_W) of item k, and
// both are re-read during the unwinding: with the eight prefix products in registers beside the
// inversion's temporaries every finish kernel needed more than 256 VGPRs and spilled 660 bytes per
// lane.  The same lane writes and later reads these slots.  Phase B is an ordinary loop over the
// items, so the (large) per-item code exists once.
ED_DEV void slot_store(uint32_t* acc, int k, int coord, const fe& f, int K) {
  acc_put(acc_column(acc, (size_t)blockIdx.x * K + k, threadIdx.x), coord, f);
}
ED_DEV void slot_load(fe& f, const uint32_t* acc, int k, int coord, int K) {
  acc_load(f, acc_column(acc, (size_t)blockIdx.x * K + k, threadIdx.x), coord);
}
ED_DEV void zinv_store(uint32_t* acc, int k, const fe& zi, int K) { slot_store(acc, k, ACC_Z, zi, K); }

template <class P>
ED_DEV void finish_batch8(const P& pol, uint32_t* acc) {
  const int K = pol.K;                           // items per lane that share the inversion: FINISH_K, fewer in small passes
  fe z, p, u, zi;
  pol.den(0, p);
  slot_store(acc, 0, ACC_W, p, K);
#pragma unroll 1
  for (int k = 1; k < K; k++) {
    pol.den(k, z);
    fe_mul(p, p, z);
    slot_store(acc, k, ACC_W, p, K);             // z0 ... zk
  }
  fe_inv(u, p);                                  // u = 1 / (z0 ... z(K-1))
#pragma unroll 1
  for (int k = K - 1; k >= 1; k--) {
    slot_load(p, acc, k - 1, ACC_W, K);
    fe_mul(zi, u, p);                            // 1 / zk
    slot_load(z, acc, k, ACC_Z, K);
    fe_mul(u, u, z);                             // 1 / (z0 ... z(k-1))
    zinv_store(acc, k, zi, K);
  }
  zinv_store(acc, 0, u, K);
#pragma unroll 1
  for (int k = 0; k < K; k++) pol.item(k);
}

// z := good ? z : 1, committed to slot k's Z so that the unwinding re-reads exactly this value
ED_DEV void den_commit(fe& z, bool good, uint32_t* acc, int k, int K) {
  fe one;
  fe_set(one, 1);
  fe_cmov(one, z, good);
  z = one;
  zinv_store(acc, k, z, K);
}

// verify: encode and compare with R as bytes (ed25519-sha512.c:176-180): a non-canonical R can
// never match.  Items whose A is off the curve are skipped here (k_verify_exact_quad writes their
// verdict; DESIGN.md "Off-curve public keys"); Z = 0 cannot occur for a curve point (the a = -1 law
// is complete) and is rejected defensively.
struct verify_finish_policy {
  uint8_t* ok; const uint8_t* sigs; size_t sig_stride; uint32_t* acc; uint8_t* flags; size_t n; int exact_offcurve; int K;
  ED_DEV void den(int k, fe& z) const {
    const finish_pos p = finish_at(k, acc, K);
    fe_set(z, 1);
    bool good = false;
    if (p.i < n) {
      acc_load(z, p.acc, ACC_Z);
      const uint8_t fl = flags[p.i];
      good = (fl & VERIFY_WINDOWED) != 0 && !fe_iszero(z);
      flags[p.i] = (uint8_t)((fl & VERIFY_WINDOWED) | (good ? VERIFY_Z_USABLE : 0));   // phase B reads it back
    }
    den_commit(z, good, acc, k, K);
  }
  ED_DEV void item(int k) const {
    const finish_pos p = finish_at(k, acc, K);
    if (p.i >= n) return;
    fe x, y, zinv;
    acc_load(x, p.acc, ACC_X); acc_load(y, p.acc, ACC_Y); acc_load(zinv, p.acc, ACC_Z);
    uint32_t rw[8];
    load32(rw, sigs, p.i, sig_stride);
    const uint8_t fl = flags[p.i];
    if ((fl & VERIFY_WINDOWED) == 0) {           // off-curve key
      if (!exact_offcurve) ok[p.i] = 0;          // reject mode; otherwise k_verify_exact_quad owns ok[i]
      return;
    }
    ok[p.i] = (uint8_t)(verify_encode_lane(x, y, zinv, rw) && (fl & VERIFY_Z_USABLE) != 0);
  }
};

// small passes: four lanes per item (quad_lanes.h: verify_main_quad); writes the same workspace
__global__ void __launch_bounds__(QUAD_BLOCK, 2)
k_verify_main_quad(const uint32_t* digits, const uint32_t* table, const uint32_t* base16, uint32_t* accout, size_t n) {
  const size_t i = ((size_t)blockIdx.x * QUAD_BLOCK + threadIdx.x) >> 2;       // quads are all-or-nothing
  if (i >= n) return;
  const int q = (int)(threadIdx.x & 3u);
  fe r;
  verify_main_quad(r, digits + digit_slot(i), table + table_slot(i), base16, q);
  if (q == 2) return;                            // T is not part of the result
  acc_put(acc_column(accout, i / BLOCK, i % BLOCK), q == 0 ? ACC_X : q == 1 ? ACC_Y : ACC_Z, r);
}

__global__ void __launch_bounds__(BLOCK, 2)
k_verify_finish(uint8_t* ok, const uint8_t* sigs, size_t sig_stride, uint32_t* acc, uint8_t* flags, size_t n,
                int exact_offcurve, int K) {
  finish_batch8(verify_finish_policy{ok, sigs, sig_stride, acc, flags, n, exact_offcurve, K}, acc);
}

// The opt-in strict rules (include/eddsa_amd.h: EDDSA_AMD_VERIFY_*; policy_lanes.h: verify_policy_lane) as a pass of their own
// behind every writer of ok[]: an item the pass accepted is rejected when a predicate of `policy` fails on its bytes.  It never
// writes a 1 and reads nothing of the workspace, so it cannot turn a verdict of the kernels before it into an accept.
static_assert(POLICY_S_BELOW_L == EDDSA_AMD_VERIFY_S_BELOW_L && POLICY_A_CANONICAL == EDDSA_AMD_VERIFY_A_CANONICAL &&
              POLICY_A_NOT_SMALL == EDDSA_AMD_VERIFY_A_NOT_SMALL && POLICY_R_NOT_SMALL == EDDSA_AMD_VERIFY_R_NOT_SMALL &&
              EDDSA_AMD_VERIFY_STRICT == (POLICY_S_BELOW_L | POLICY_A_CANONICAL | POLICY_A_NOT_SMALL | POLICY_R_NOT_SMALL), "the lane's bits are the header's");
__global__ void __launch_bounds__(BLOCK)
k_verify_policy(uint8_t* ok, const uint8_t* sigs, size_t sig_stride, const uint8_t* pubs, size_t pub_stride, size_t n, unsigned policy) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n || ok[i] == 0) return;
  uint32_t rw[8], sw[8], aw[8];
  load32(rw, sigs, i, sig_stride);
  load32(sw, sigs + 32, i, sig_stride);
  load32(aw, pubs, i, pub_stride);
  if (!verify_policy_lane(rw, sw, aw, policy)) ok[i] = 0;
}

// The opt-in cofactored equation (include/eddsa_amd.h: eddsa_amd_set_verify_equation; cofactor_lanes.h), three kernels behind
// every writer of ok[] and in front of k_verify_policy.  The pass before them ran unchanged, in reject mode: what it accepted has
// its key on the curve, so with S < l (k_verify_policy, S_BELOW_L forced) the cofactored equation accepts it too - an accepted R
// equals the canonical export and decodes.  Only the REJECTED items can change their verdict:
//   k_cofactor_list    collects them into the onlist storage, which is free after the join (all: self-check mode 2, where the
//                      reference-order chain may have accepted an item whose key is no curve point - there every item is
//                      listed and these kernels own every verdict)
//   k_cofactor_points  S < l, -R decoded into the item's rtable slot, the table of -A rebuilt (the exact path may have written
//                      over entries 2 and 3) -> the item's flags byte
//   k_cofactor_eval    persistent blocks, one lane per listed item: the 252 doublings and 80 additions over the digit words the
//                      prepare kernel left, - R, three doublings, the neutrality test -> ok[i]
// Two kernels for the lane's two steps like k_verify_prepare and k_verify_main: as one they spilled 1160 bytes per lane at the
// evaluation's 128 registers and 240 at 256; apart they take 245 and 124 and no scratch.  No route writes `digits` after its
// prepare kernel (the halve kernels and the exact path's set-ups only read them), flags, rtable and onlist have no reader left
// after the join, and the kernels wait on nothing but the stream.
constexpr unsigned COFACTOR_MAX_BLOCKS = 1024;   // as many as are resident at once (four per CU)
constexpr uint8_t COFACTOR_POINTS_GOOD = 8;      // flags[i] after k_cofactor_points: S < l, A and R on the curve (no bit of kernel_io.h's)
__global__ void __launch_bounds__(BLOCK)
k_cofactor_list(const uint8_t* ok, size_t n, uint32_t* list, uint32_t* offcount, int all) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool want = i < n && (all || ok[i] == 0);
  const uint32_t slot = wave_append(offcount + EDK_COLIST_WORD, want);
  if (want) list[slot] = (uint32_t)i;            // slot < n: one entry per item at the most
}

// over the list, not over the pass: the grid is sized for the pass, the blocks beyond the list end at once (like k_verify_halve)
__global__ void __launch_bounds__(BLOCK, 2)
k_cofactor_points(const uint8_t* sigs, size_t sig_stride, const uint8_t* pubs, size_t pub_stride, uint32_t* table, uint32_t* rtable,
                  uint8_t* flags, const uint32_t* list, const uint32_t* offcount) {
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= (size_t)offcount[EDK_COLIST_WORD]) return;
  const size_t i = list[g];                      // < n: the item's own slots of the workspace
  uint32_t rw[8], sw[8], aw[8];
  load32(rw, sigs, i, sig_stride);
  load32(sw, sigs + 32, i, sig_stride);
  load32(aw, pubs, i, pub_stride);
  flags[i] = cofactor_points_lane(rw, sw, aw, table + table_slot(i), rtable + table_slot(i)) ? COFACTOR_POINTS_GOOD : 0;
}

__global__ void __launch_bounds__(BLOCK, 4)
k_cofactor_eval(uint8_t* ok, const uint32_t* digits, const uint32_t* table, const uint32_t* rtable, const uint32_t* base16,
                const uint8_t* flags, const uint32_t* list, const uint32_t* offcount) {
  const size_t listed = offcount[EDK_COLIST_WORD];
#pragma unroll 1
  for (size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x; g < listed; g += (size_t)gridDim.x * BLOCK) {
    const size_t i = list[g];
    const bool neutral = cofactor_equation_lane(digits + digit_slot(i), table + table_slot(i), rtable + table_slot(i), base16);
    ok[i] = (uint8_t)(neutral && flags[i] == COFACTOR_POINTS_GOOD);
  }
}

// x25519.c:144-149: x2 / z2, and 0 when z2 = 0 (fld_inv(0) = 0): such an item contributes 1 to the
// shared product and its "inverse" is forced to 0
struct x25519_finish_policy {
  uint8_t* out; uint32_t* acc; size_t n; int K;
  ED_DEV void den(int k, fe& z) const {
    const finish_pos p = finish_at(k, acc, K);
    fe_set(z, 1);
    bool good = false;
    if (p.i < n) {
      acc_load(z, p.acc, ACC_Z);
      good = !fe_iszero(z);
      if (!good) {                               // remember it: X := 0 makes the product 0 whatever the "inverse"
        fe zero;
        fe_set(zero, 0);
        acc_put(acc_column(acc, p.tile, threadIdx.x), ACC_X, zero);
      }
    }
    den_commit(z, good, acc, k, K);
  }
  ED_DEV void item(int k) const {
    const finish_pos p = finish_at(k, acc, K);
    fe x, zinv;
    if (p.i < n) { acc_load(x, p.acc, ACC_X); acc_load(zinv, p.acc, ACC_Z); }
    // (x2 : z2), 1/z2 and the prefix products of the shared inversion determine shared secrets: they
    // do not outlive the call in HBM (x25519.c:221 burnstack); slots past the end hold the committed 1
    uint32_t* o = acc_column(acc, p.tile, threadIdx.x);
#pragma unroll
    for (int j = 0; j < 10; j++) { o[acc_at(ACC_X, j)] = 0; o[acc_at(ACC_Z, j)] = 0; o[acc_at(ACC_W, j)] = 0; }
    if (p.i >= n) return;
    uint32_t w[8];
    x25519_finish_lane(w, x, zinv);
    store32(out, p.i, 32, w);
  }
};

__global__ void __launch_bounds__(BLOCK, 2)
k_x25519_finish(uint8_t* out, uint32_t* acc, size_t n, int K) {
  finish_batch8(x25519_finish_policy{out, acc, n, K}, acc);
}

// ---------------------------------------------------------------------------------------------
// fixed-base kernels: the image of the comb (22 rows x 32 entries m * 4096^i * B, m = 1..32, 99 KiB of the CU's
// 160 KiB LDS; one 512-lane block per CU, two waves per SIMD) is staged by every block of a
// "point" kernel; the matching "finish" kernel encodes (and, for sign, hashes and computes S)
// ---------------------------------------------------------------------------------------------

constexpr int POINT_BLOCK = COMB_IMG_WORDS * 4 > 80 * 1024 ? 512 : 256;   // 8 waves per CU either way (768 lanes: 6-101 spilled registers, 1024: 94-314)

// PARTS = 4: four lanes per item for small passes (lanes.h: scale_base_lane<4>) - a block is four waves, wave w holds
// share w of 64 items - and the shares are added through LDS, pairwise: waves 1 and 3 hand theirs to waves 0 and 2,
// then wave 2 to wave 0, which delivers.  The shares are secrets (partial sums of a secret multiple): the slots are
// zeroed once read.
constexpr int POINT_SPLIT = 4, POINT_SPLIT_ITEMS = 64;
// The blocks of a pass that fills the chip are PERSISTENT - one block per CU stages the 99 KB image once - and their WAVES take
// 64-item tiles from a counter until none is left (point_tile below).  Why not a tile per block, or a fixed share per wave:
// the image leaves room for ONE block of eight waves per CU, two waves per SIMD, and the SIMD issues its older wave first; with
// equal shares the older wave of every pair finished at ~60 % of the kernel's time and the younger one ran the rest alone, at
// the issue rate of a single wave (SQ_WAVE_CYCLES: 1.52 waves resident per SIMD on average, VALU-busy 0.92 - the "idle 10 %" of
// VERDICT r03 #8; not the staging, not LDS latency, not the instruction cache: profiles/r04_sign_ab.txt).  Handed out one by
// one, the tiles go to whichever wave is ahead and all waves finish together.  Small passes (no more blocks than CUs, or four
// lanes per item) keep the fixed mapping: block b takes tile b.
constexpr unsigned POINT_MAX_BLOCKS = 256u * (512 / POINT_BLOCK);   // as many as are resident at once

// the next item of this lane, or false when the pass is done.  `it` = the lane's iteration count so far (0 at the start).
// Dynamic hand-out: lane 0 of the wave draws a tile number, the wave takes items 64 t .. 64 t + 63, until the counter is past
// the end (the launcher zeroes it on the pass's stream before every such launch).
template <int PARTS>
ED_DEV bool point_tile(size_t& i, unsigned it, size_t n, uint32_t* tiles) {
  if (PARTS == 1 && tiles != nullptr) {
    unsigned t = 0;
    if ((threadIdx.x & 63u) == 0) t = atomicAdd(tiles, 1u);
    t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
    if ((size_t)t * 64 < n) { i = (size_t)t * 64 + (threadIdx.x & 63u); return true; }
    return false;
  }
  const size_t span = PARTS == 1 ? (size_t)blockDim.x : (size_t)POINT_SPLIT_ITEMS;
  const size_t base = ((size_t)blockIdx.x + (size_t)it * gridDim.x) * span;
  i = base + (PARTS == 1 ? threadIdx.x : (threadIdx.x & 63u));
  return base < n;
}

ED_DEV void share_store(uint32_t* slot, const ge& p) {
#pragma unroll
  for (int j = 0; j < 10; j++) {
    slot[j * 64] = p.X.v[j]; slot[(10 + j) * 64] = p.Y.v[j]; slot[(20 + j) * 64] = p.Z.v[j]; slot[(30 + j) * 64] = p.T.v[j];
  }
}
ED_DEV void share_take(ge& p, uint32_t* slot) {
#pragma unroll
  for (int j = 0; j < 10; j++) {
    p.X.v[j] = slot[j * 64]; p.Y.v[j] = slot[(10 + j) * 64]; p.Z.v[j] = slot[(20 + j) * 64]; p.T.v[j] = slot[(30 + j) * 64];
    slot[j * 64] = 0; slot[(10 + j) * 64] = 0; slot[(20 + j) * 64] = 0; slot[(30 + j) * 64] = 0;
  }
}
// every wave of the block calls it; afterwards the lanes of wave 0 hold the sums (Z, Y, X; T is not computed)
ED_DEV void point_reduce4(ge& a, uint32_t* lds_shares, int part) {
  uint32_t* slot = lds_shares + (part >> 1) * (40 * 64) + (threadIdx.x & 63u);
  ge o;
  ge_cached c;
  if (part & 1) share_store(slot, a);
  __syncthreads();
  if (!(part & 1)) { share_take(o, slot); ge_to_cached(c, o); ge_add_cached(a, a, c, true); }
  __syncthreads();
  slot = lds_shares + (threadIdx.x & 63u);
  if (part == 2) share_store(slot, a);
  __syncthreads();
  if (part == 0) { share_take(o, slot); ge_to_cached(c, o); ge_add_cached(a, a, c, false); }
}

template <int PARTS>
__global__ void __launch_bounds__(POINT_BLOCK, 512 / POINT_BLOCK)
k_genpub_point(uint32_t* accout, const uint8_t* secs, size_t n, const uint32_t* comb, uint32_t* tiles) {
  __shared__ alignas(16) uint32_t lds_comb[COMB_IMG_WORDS];
  stage_table(lds_comb, comb, COMB_IMG_WORDS);
  __shared__ uint32_t lds_shares[PARTS == 1 ? 1 : 2 * 40 * 64];
  // blocks of POINT_BLOCK lanes, or smaller ones for small passes (EDK_POINT_GRID); PARTS = 4: four waves, 64 items
  const int part = PARTS == 1 ? 0 : (int)(threadIdx.x >> 6);
  size_t i;
#pragma unroll 1
  for (unsigned it = 0; point_tile<PARTS>(i, it, n, tiles); it++) {
    uint32_t sk[8];
    load32(sk, secs, i < n ? i : n - 1, 32);
    ge A;
    genpub_point_lane<PARTS>(A, sk, lds_comb, part);
    if (PARTS > 1) point_reduce4(A, lds_shares, part);
    if (PARTS == 1 || (part == 0 && i < n)) acc_store(accout, i, A);
  }
}

// the base of the policies that finish a comb result: its Z is never 0 (B and its multiples are curve points)
struct comb_finish {
  uint32_t* acc; size_t n; int K;
  ED_DEV void den(int k, fe& z) const {
    const finish_pos p = finish_at(k, acc, K);
    fe_set(z, 1);
    if (p.i < n) acc_load(z, p.acc, ACC_Z);
    den_commit(z, true, acc, k, K);
  }
};

struct encode_finish_policy : comb_finish {
  uint8_t* out;
  ED_DEV void item(int k) const {
    const finish_pos p = finish_at(k, acc, K);
    if (p.i >= n) return;
    fe x, y, zinv;
    acc_load(x, p.acc, ACC_X); acc_load(y, p.acc, ACC_Y); acc_load(zinv, p.acc, ACC_Z);
    uint32_t w[8];
    encode_lane(w, x, y, zinv);
    store32(out, p.i, 32, w);
  }
};

__global__ void __launch_bounds__(BLOCK, 2)
k_encode_finish(uint8_t* out, uint32_t* acc, size_t n, int K) {
  finish_batch8(encode_finish_policy{{acc, n, K}, out}, acc);
}

// a | r of a position, the secret scalars of its item, wait in the position's slot of aux between the kernels of a sign pass
constexpr int AUX_WORDS = 16;
ED_DEV void aux_store(uint32_t* aux, size_t pos, const uint32_t aw[8], const uint32_t rw[8]) {
  store8(aux + AUX_WORDS * pos, aw);
  store8(aux + AUX_WORDS * pos + 8, rw);
}

template <int PARTS>
__global__ void __launch_bounds__(POINT_BLOCK, 512 / POINT_BLOCK)
k_sign_point(uint32_t* accout, uint32_t* aux, const uint8_t* secs, const uint8_t* msgs,
             const uint64_t* msg_off, const uint64_t* msg_end, size_t msg_len, size_t n, const uint32_t* comb, const uint32_t* perm,
             uint32_t* tiles) {
  __shared__ alignas(16) uint32_t lds_comb[COMB_IMG_WORDS];
  stage_table(lds_comb, comb, COMB_IMG_WORDS);
  __shared__ uint32_t lds_shares[PARTS == 1 ? 1 : 2 * 40 * 64];
  // blocks of POINT_BLOCK lanes, or smaller ones for small passes (EDK_POINT_GRID); PARTS = 4: four waves, 64 items
  const int part = PARTS == 1 ? 0 : (int)(threadIdx.x >> 6);
  size_t i;
#pragma unroll 1
  for (unsigned it = 0; point_tile<PARTS>(i, it, n, tiles); it++) {
    // position i works on item perm[i] (ragged messages in order of length); the point and the secret scalars stay at the
    // POSITION's slots of the workspace, where k_sign_finish finds them
    const size_t item = perm ? perm[i < n ? i : n - 1] : (i < n ? i : n - 1);
    const uint8_t* m; size_t mlen;
    msg_span(m, mlen, msgs, msg_off, msg_end, msg_len, msg_len, item);
    uint32_t sk[8], aw[8], rw[8];
    load32(sk, secs, item, 32);
    sign_scalars_lane(aw, rw, sk, m, mlen);
    // the secret scalars a and r, for the finish step: handed over BEFORE the comb (sixteen registers less to hold across
    // its 44 additions, which is what lets a row's two lookups be issued ahead of its two additions without a spill).
    // An idle lane must not leave a copy of the last item's secrets.
    if (i < n && part == 0) {
      store8(aux + 16 * i, aw);
      store8(aux + 16 * i + 8, rw);
    }
    ge R;
    scale_base_lane<PARTS>(R, rw, lds_comb, part);
    if (PARTS > 1) point_reduce4(R, lds_shares, part);
    if (PARTS == 1 || (part == 0 && i < n)) acc_store(accout, i, R);
  }
}

// The finish of every sign pass: R encoded, the challenge t hashed - DOM: under the dom2 prefix staged at `dom` (Ed25519ctx /
// Ed25519ph) - and S = r + t a.  KEYED (signer sets, signer_kernels.h): A = pubs[key_idx[item]], the set's key; an index outside
// the set (>= count) gets 64 zero bytes (its a and r are zero, its point the neutral element).
// Secrets: a | r are fetched only after the hash (sixteen registers less across it) and do not outlive the call in HBM: the
// position's slot of aux is zeroed as soon as it is read.  A keyed pass wipes the position's point on top: (X : Y : Z) of R = r B
// and the prefix products of the shared inversion determine r up to the projective factor, and a signer's workspace is the one a
// long-lived signing process keeps.
template <bool DOM, bool KEYED>
struct sign_finish_policy : comb_finish {
  uint8_t* sigs; uint32_t* aux; const uint8_t* pubs; const uint8_t* msgs;
  const uint64_t* msg_off; const uint64_t* msg_end; size_t msg_len; const uint32_t* perm;
  const uint32_t* dom = nullptr; uint32_t dom_len = 0;        // DOM
  uint32_t count = 0; const uint32_t* key_idx = nullptr;      // KEYED
  ED_DEV void item(int k) const {
    const finish_pos p = finish_at(k, acc, K);
    fe x, y, zinv;
    if constexpr (KEYED) {                         // the position's point and prefix products are wiped once read
      if (p.i < n) { acc_load(x, p.acc, ACC_X); acc_load(y, p.acc, ACC_Y); acc_load(zinv, p.acc, ACC_Z); }
      uint32_t* o = acc_column(acc, p.tile, threadIdx.x);   // slots past the end hold the committed 1 (and what an idle lane of the point kernel left)
#pragma unroll
      for (int j = 0; j < 10; j++) { o[acc_at(ACC_X, j)] = 0; o[acc_at(ACC_Y, j)] = 0; o[acc_at(ACC_Z, j)] = 0; o[acc_at(ACC_W, j)] = 0; }
    }
    if (p.i >= n) return;
    const size_t it = perm ? perm[p.i] : p.i;      // the item this position carries (the pass's scalars kernel, or k_sign_point)
    if constexpr (!KEYED) { acc_load(x, p.acc, ACC_X); acc_load(y, p.acc, ACC_Y); acc_load(zinv, p.acc, ACC_Z); }
    const uint32_t key = KEYED ? key_idx[it] : 0u;
    const bool known = !KEYED || key < count;
    uint32_t Rw[8], Sw[8], pub[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    encode_lane(Rw, x, y, zinv);
    if constexpr (KEYED) { if (known) load32(pub, pubs, key, 32); }
    else load32(pub, pubs, it, 32);
    const uint8_t* m; size_t mlen;
    msg_span(m, mlen, msgs, msg_off, msg_end, msg_len, msg_len, it);
    sc t;
    if constexpr (DOM) sign_dom_challenge_lane(t, dom, dom_len, Rw, pub, m, mlen);
    else sign_challenge_lane(t, Rw, pub, m, mlen);
    uint32_t aw[8], rw[8];                         // the secret scalars are fetched only after the hash
    uint32_t* d = aux + AUX_WORDS * p.i;
    load8(aw, d);
    load8(rw, d + 8);
    const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the secrets do not outlive the call in HBM
    store8(d, zero);
    store8(d + 8, zero);
    sign_response_lane(Sw, t, aw, rw);
    if constexpr (KEYED) {                         // an index outside the set: 64 zero bytes
#pragma unroll
      for (int j = 0; j < 8; j++) { Rw[j] = known ? Rw[j] : 0u; Sw[j] = known ? Sw[j] : 0u; }
    }
    store32(sigs, it, 64, Rw);
    store32(sigs + 32, it, 64, Sw);
  }
};

__global__ void __launch_bounds__(BLOCK, 2)
k_sign_finish(uint8_t* sigs, uint32_t* acc, uint32_t* aux, const uint8_t* pubs, const uint8_t* msgs,
              const uint64_t* msg_off, const uint64_t* msg_end, size_t msg_len, size_t n, int K, const uint32_t* perm) {
  finish_batch8(sign_finish_policy<false, false>{{acc, n, K}, sigs, aux, pubs, msgs, msg_off, msg_end, msg_len, perm}, acc);
}

// ---------------------------------------------------------------------------------------------
// Ed25519ctx / Ed25519ph (RFC 8032 5.1): kernels of their own beside the ones above, whose register arrangements stay as they
// are.  The dom2 prefix arrives by value (eddsa_kernels.h: edk_dom), is staged into LDS once per block and read from there by
// uniform index.  Sign is three kernels: the secret scalars (one lane per item, both hashes' only secret input), the point
// R = r B with r taken from aux in every shape of point_shape_of, and the finish with the prefixed challenge.  Verify is one
// kernel in front of the digest route (edk_verify below).
// ---------------------------------------------------------------------------------------------
ED_DEV void stage_dom(uint32_t* lds_dom, const edk_dom& dom) {
  for (unsigned w = threadIdx.x; w < (unsigned)EDK_DOM_WORDS; w += blockDim.x) lds_dom[w] = dom.w[w];
  __syncthreads();
}

// position g hashes item perm[g] (ragged messages in order of length) or item g; the digest goes to the ITEM's slot
__global__ void __launch_bounds__(BLOCK, 2)
k_dom_challenge(edk_verify_items src, size_t n, uint8_t* digests, const uint32_t* perm, edk_dom dom) {
  __shared__ uint32_t lds_dom[EDK_DOM_WORDS];
  stage_dom(lds_dom, dom);
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= n) return;
  const size_t item = perm ? perm[g] : g;
  uint32_t rw[8], aw[8], dig[16];
  const uint8_t* m; size_t mlen;
  load32(rw, src.sigs, item, src.sig_stride);
  load32(aw, src.pubs, item, src.pub_stride);
  msg_span(m, mlen, src.msgs, src.msg_off, src.msg_end, src.msg_len, src.msg_stride, item);
  verify_dom_hash_lane(dig, lds_dom, dom.len, rw, aw, m, mlen);
  store32(digests, item, EDK_DOM_DIGEST_BYTES, dig);
  store32(digests + 32, item, EDK_DOM_DIGEST_BYTES, dig + 8);
}

// a and r of position g's item into the POSITION's slot of aux, where the two kernels behind it find them
__global__ void __launch_bounds__(BLOCK, 2)
k_sign_dom_scalars(uint32_t* aux, const uint8_t* secs, const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* msg_end,
                   size_t msg_len, size_t n, const uint32_t* perm, edk_dom dom) {
  __shared__ uint32_t lds_dom[EDK_DOM_WORDS];
  stage_dom(lds_dom, dom);
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= n) return;                            // (an idle lane holds no item's secrets)
  const size_t item = perm ? perm[g] : g;
  const uint8_t* m; size_t mlen;
  msg_span(m, mlen, msgs, msg_off, msg_end, msg_len, msg_len, item);
  uint32_t sk[8], aw[8], rw[8];
  load32(sk, secs, item, 32);
  sign_dom_scalars_lane(aw, rw, lds_dom, dom.len, sk, m, mlen);
  aux_store(aux, g, aw, rw);
}

// k_sign_point without its hashes: r comes from aux (k_sign_dom_scalars).  An idle lane takes the last position's r and keeps
// the result to itself (split shape) or leaves R - a public point - in a slot past the pass, like k_sign_point.
template <int PARTS>
__global__ void __launch_bounds__(POINT_BLOCK, 512 / POINT_BLOCK)
k_sign_dom_point(uint32_t* accout, const uint32_t* aux, size_t n, const uint32_t* comb, uint32_t* tiles) {
  __shared__ alignas(16) uint32_t lds_comb[COMB_IMG_WORDS];
  stage_table(lds_comb, comb, COMB_IMG_WORDS);
  __shared__ uint32_t lds_shares[PARTS == 1 ? 1 : 2 * 40 * 64];
  const int part = PARTS == 1 ? 0 : (int)(threadIdx.x >> 6);
  size_t i;
#pragma unroll 1
  for (unsigned it = 0; point_tile<PARTS>(i, it, n, tiles); it++) {
    uint32_t rw[8];
    load8(rw, aux + 16 * (i < n ? i : n - 1) + 8);
    ge R;
    scale_base_lane<PARTS>(R, rw, lds_comb, part);
    if (PARTS > 1) point_reduce4(R, lds_shares, part);
    if (PARTS == 1 || (part == 0 && i < n)) acc_store(accout, i, R);
  }
}

__global__ void __launch_bounds__(BLOCK, 2)
k_sign_dom_finish(uint8_t* sigs, uint32_t* acc, uint32_t* aux, const uint8_t* pubs, const uint8_t* msgs,
                  const uint64_t* msg_off, const uint64_t* msg_end, size_t msg_len, size_t n, int K, const uint32_t* perm, edk_dom dom) {
  __shared__ uint32_t lds_dom[EDK_DOM_WORDS];
  stage_dom(lds_dom, dom);
  finish_batch8(sign_finish_policy<true, false>{{acc, n, K}, sigs, aux, pubs, msgs, msg_off, msg_end, msg_len, perm, lds_dom, dom.len}, acc);
}

template <int PARTS>
__global__ void __launch_bounds__(POINT_BLOCK, 512 / POINT_BLOCK)
k_x25519_base_point(uint32_t* accout, const uint8_t* scalars, size_t n, const uint32_t* comb, uint32_t* tiles) {
  __shared__ alignas(16) uint32_t lds_comb[COMB_IMG_WORDS];
  stage_table(lds_comb, comb, COMB_IMG_WORDS);
  __shared__ uint32_t lds_shares[PARTS == 1 ? 1 : 2 * 40 * 64];
  // blocks of POINT_BLOCK lanes, or smaller ones for small passes (EDK_POINT_GRID); PARTS = 4: four waves, 64 items
  const int part = PARTS == 1 ? 0 : (int)(threadIdx.x >> 6);
  size_t i;
#pragma unroll 1
  for (unsigned it = 0; point_tile<PARTS>(i, it, n, tiles); it++) {
    uint32_t s[8];
    load32(s, scalars, i < n ? i : n - 1, 32);
    ge R;
    x25519_base_point_lane<PARTS>(R, s, lds_comb, part);
    if (PARTS > 1) point_reduce4(R, lds_shares, part);
    fe_add(R.X, R.Z, R.Y);                       // the finish step needs z + y, not x
    fe_carry(R.X);
    if (PARTS == 1 || (part == 0 && i < n)) acc_store(accout, i, R);
  }
}

// u = (z + y) / (z - y); z = y gives 0 in the reference (fld_inv(0) = 0, x25519.c:192): such an
// item contributes 1 to the shared product and gets the "inverse" 0 by hand.
struct x25519_base_finish_policy {
  uint8_t* out; uint32_t* acc; size_t n; int K;
  ED_DEV void den(int k, fe& d) const {
    const finish_pos p = finish_at(k, acc, K);
    fe_set(d, 1);
    bool good = false;
    if (p.i < n) {
      fe y, z;
      acc_load(y, p.acc, ACC_Y); acc_load(z, p.acc, ACC_Z);
      fe_sub(d, z, y);                           // 3u
      good = !fe_iszero(d);
    }
    den_commit(d, good, acc, k, K);
  }
  ED_DEV void item(int k) const {
    const finish_pos p = finish_at(k, acc, K);
    if (p.i >= n) return;
    fe x, y, dinv, z, d;
    acc_load(y, p.acc, ACC_Y); acc_load(dinv, p.acc, ACC_Z);     // the Z slot now holds 1/(z - y) (or 1/1)
    // z itself was overwritten; recover the numerator z + y = (z - y) + 2y from X's slot instead:
    // the point kernel stores z + y there (x is not needed for x25519_base)
    acc_load(x, p.acc, ACC_X);                           // = z + y
    fe_sub(d, x, y); fe_sub(d, d, y);                    // z - y, to detect the zero denominator
    fe zero;
    fe_set(zero, 0);
    fe_cmov(dinv, zero, fe_iszero(d));
    fe u;
    fe_mul(u, x, dinv);
    uint32_t w[8];
    fe_tobytes(w, u);
    store32(out, p.i, 32, w);
  }
};

__global__ void __launch_bounds__(BLOCK, 2)
k_x25519_base_finish(uint8_t* out, uint32_t* acc, size_t n, int K) {
  finish_batch8(x25519_base_finish_policy{out, acc, n, K}, acc);
}

__global__ void __launch_bounds__(BLOCK, 2)
k_pk_to_x(uint8_t* out, const uint8_t* in, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8], o[8];
  load32(w, in, i, 32);
  pk_to_x_lane(o, w);
  store32(out, i, 32, o);
}

__global__ void __launch_bounds__(BLOCK, 2)
k_sk_to_x(uint8_t* out, const uint8_t* in, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t sk[8], o[8];
  load32(sk, in, i, 32);
  sk_to_x_lane(o, sk);
  store32(out, i, 32, o);
}

// ---------------------------------------------------------------------------------------------
// The half-length route for SMALL passes (up to QUAD_MAIN_MAX_N items), where what counts is the latency of one
// item: k_verify_prepare_pair does the work of k_verify_prepare + k_verify_halve with three lanes per item in two kinds
// of blocks - the points' blocks, where lane 0 of a pair decompresses A and builds its table while lane 1 does the same
// for R, and the scalars' blocks, where one lane hashes and searches the pair (nothing of the one depends on the other:
// a single item's 0.13 ms became 0.09) - and k_verify_main_half_quad is verify_half_main_lane with a coordinate per
// lane (quad_lanes.h).  Two kernels, 132 doublings and no inversion instead of three, 252 and one.
// ---------------------------------------------------------------------------------------------
template <int BITS, bool DIGEST>
__global__ void __launch_bounds__(BLOCK, 2)
k_verify_prepare_pair(edk_verify_items src, size_t n, uint32_t* digits, uint32_t* hdigits, uint32_t* table, uint32_t* rtable,
                      uint8_t* flags, uint32_t* onlist, uint32_t* offlist, uint32_t* offcount, int all_exact, unsigned point_blocks,
                      const uint32_t* perm) {
  if (blockIdx.x >= point_blocks) {
    // the scalars' blocks, one lane per item: hash, reduce, search the pair.  They need nothing from the points' blocks
    // and those nothing from here: the two square-root chains of an item run BESIDE its hash and its search
    const size_t g = (size_t)(blockIdx.x - point_blocks) * BLOCK + threadIdx.x;
    if (g >= n) return;
    const size_t i = perm ? perm[g] : g;         // (ragged messages in order of length)
    uint32_t sw[8], tw[8], hd[HALF_DIGIT_WORDS];
    if constexpr (DIGEST) {                      // (the caller's SHA-512(R || A || M): the 64 bytes in the message slot)
      uint32_t dw[16];
      load32(dw, src.msgs, i, src.msg_stride);
      load32(dw + 8, src.msgs + 32, i, src.msg_stride);
      load32(sw, src.sigs + 32, i, src.sig_stride);
      verify_digest_lane(tw, dw);
    } else {
      uint32_t rw[8], aw[8];
      const uint8_t* m; size_t mlen;
      verify_item(rw, sw, aw, m, mlen, src, i);
      verify_hash_lane(tw, rw, aw, m, mlen);
    }
    verify_s_lane(sw);
    verify_half_scalars_lane<BITS>(hd, tw, sw);
    store8(digits + digit_slot(i), tw);
    store8(digits + digit_slot(i) + 8, sw);
    hdigits_store(hdigits, i, hd);
    if ((hd[HALF_STATUS_WORD] & HALF_PAIR_REFUSED) != 0) atomicAdd(offcount + EDK_REFUSED_WORD, 1u);
    return;
  }
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const size_t i = g >> 1;                       // pairs are all-or-nothing
  if (i >= n) return;
  const bool second = (g & 1) != 0;
  // lane 0: -A permissively (ed.c:100-149), lane 1: -R' strictly (lanes.h: verify_half_point_lane)
  uint32_t pw[8];
  load32(pw, second ? src.sigs : src.pubs, i, second ? src.sig_stride : src.pub_stride);
  uint32_t* tab = (second ? rtable : table) + table_slot(i);
  bool oncurve;
  ge p;
  ge_frombytes(p, oncurve, pw, true);
  bool top = (pw[7] & 0x7fffffffu) == 0x7fffffffu && pw[0] >= 0xffffffedu;
#pragma unroll
  for (int k = 1; k < 7; k++) top = top && pw[k] == 0xffffffffu;
  const bool strict = oncurve && !top && !((pw[7] >> 31) != 0 && fe_iszero(p.X));
  verify_table_point_lane(tab, p);
  const int mine = second ? (strict ? 1 : 0) : (oncurve ? 1 : 0);
  const int other = __shfl_xor(mine, 1);
  if (!second) {
    const bool keep = oncurve && !all_exact;
    flags[i] = (uint8_t)((keep ? VERIFY_WINDOWED : 0) | (other ? VERIFY_R_CANONICAL : 0));
    // the two work lists of k_verify_prepare (the four-lane evaluations of small passes do not use the first)
    const uint32_t on_slot = wave_append(offcount + EDK_ONLIST_WORD, keep);
    if (keep) onlist[on_slot] = (uint32_t)i;
    const uint32_t off_slot = wave_append(offcount + EDK_OFFLIST_WORD, !keep);
    if (!keep) offlist[off_slot] = (uint32_t)i;
  }
}

template <int WINDOWS>
__global__ void __launch_bounds__(QUAD_BLOCK, 2)
k_verify_main_half_quad(uint8_t* ok, const uint32_t* hdigits, const uint32_t* table, const uint32_t* rtable,
                        const uint32_t* base16, const uint8_t* flags, size_t n, int exact_offcurve) {
  const size_t i = ((size_t)blockIdx.x * QUAD_BLOCK + threadIdx.x) >> 2;      // quads are all-or-nothing
  if (i >= n) return;
  const int q = (int)(threadIdx.x & 3u);
  const bool neutral = verify_half_main_quad<WINDOWS>(hdigits + hdigit_slot(i), table + table_slot(i), rtable + table_slot(i), base16, q);
  if (q == 0) half_verdict_store(ok, i, flags[i], neutral, exact_offcurve);
}

// The smallest passes (quad_lanes.h: verify_half_window_sum_quad): block i adds up the 64 windows of item i, one quad each;
// then the chain over the sums.
template <int WINDOWS>
__global__ void __launch_bounds__(QUAD_BLOCK, 2)
k_verify_window_sums(uint32_t* sums, const uint32_t* hdigits, const uint32_t* table, const uint32_t* rtable, const uint32_t* base16) {
  const size_t i = blockIdx.x;
  const int w = (int)(threadIdx.x >> 2), q = (int)(threadIdx.x & 3u);
  verify_half_window_sum_quad<WINDOWS>(sums + (i * HALF_LONG_WINDOWS + (size_t)w) * HALF_SUM_WORDS, hdigits + hdigit_slot(i),
                              table + table_slot(i), rtable + table_slot(i), base16, w, q);
}

template <int WINDOWS>
__global__ void __launch_bounds__(QUAD_BLOCK, 2)
k_verify_main_sums_quad(uint8_t* ok, const uint32_t* hdigits, const uint32_t* sums, const uint8_t* flags, size_t n, int exact_offcurve) {
  const size_t i = ((size_t)blockIdx.x * QUAD_BLOCK + threadIdx.x) >> 2;      // quads are all-or-nothing
  if (i >= n) return;
  const int q = (int)(threadIdx.x & 3u);
  const bool neutral = verify_half_main_sums_quad<WINDOWS>(hdigits + hdigit_slot(i), sums + i * (HALF_LONG_WINDOWS * HALF_SUM_WORDS), q);
  if (q == 0) half_verdict_store(ok, i, flags[i], neutral, exact_offcurve);
}

}  // namespace ed

#include "keyed_kernels.h"   // key-set verification: kernels of its own beside the ones above
#include "signer_kernels.h"  // signer sets: likewise, beside the sign kernels
#include "classify_kernels.h"  // point classification: one kernel, no workspace
#include "muladd_kernels.h"  // [m]P + [a]B: a prepare and a finish kernel around k_verify_main
#include "scatter_kernels.h"  // items by byte offsets: one gathering and hashing kernel in front of a digest pass

// =============================================================================================
// launchers (host side of this translation unit)
// =============================================================================================

using namespace ed;

constexpr unsigned blocks_of(size_t lanes, size_t block = BLOCK) { return (unsigned)((lanes + block - 1) / block); }

// ---- which kernels a verify pass runs: the thresholds, and verify_route_of, the one function that reads them ----
constexpr size_t QUAD_MAIN_MAX_N = (size_t)1 << 14;   // measured: 0.57 vs 0.86 ms at 2^14, equal at 2^15 (tools/verify_sizes.py)
// the upper bound of k_verify_prepare_pair + k_verify_main_half_quad when the mid-size arrangement below is switched off
// (algo 0 takes that one above PAIR_ONE_MIN_N items, so the four-lane evaluation serves passes of up to 24 576 items)
constexpr size_t HALF_QUAD_MAX_N = (size_t)1 << 15;
// Between 24 576 and 2^18 items: k_verify_prepare_pair, then the ONE-lane evaluation with the long loop in place.  Measured
// (tools/verify_mid.py, valid signatures, ms): 2^15 0.68 (four-lane evaluation) / 0.70 (one lane per item throughout) -> 0.58,
// 2^16 0.71-0.76 -> 0.66, 2^17 1.30 -> 1.28; the config-2 mix, whose floor is the exact path: 2^16 1.16 -> 1.11, else equal.
constexpr size_t PAIR_ONE_MIN_N = (size_t)3 << 13;   // the four-lane evaluation steps up with every 8192 items (0.35 / 0.51 / 0.69 ms: tools/verify_cross.py), this one stays at 0.58
constexpr size_t QUAD_WIDE_MIN_N = 256;               // four-lane passes above this search pairs up to 2^138 as well (see verify_route_of)
constexpr size_t PAIR_ONE_MAX_N = (size_t)1 << 18;    // the mid-size arrangement (three-lane preparation, one-lane evaluation with the long loop in place) ends here
constexpr size_t HALF_WIDE_MIN_N = (size_t)1 << 19;   // one-lane passes below this search pairs up to 2^138 (see edk_verify)
constexpr size_t EXACT_DENSE_MIN_N = (size_t)1 << 16;   // passes from this size on pack the chain's items 16 to the wave whatever their number
constexpr size_t EXACT_LANE_MIN_LISTED = (size_t)1 << 13;   // (the threshold's table: profiles/r05_exact_lane.txt, 5.) work lists from this length on go to k_verify_exact_lane_* ...
constexpr size_t EXACT_LANE_MIN_N = (size_t)1 << 16;      // ... in passes of at least this many items
static_assert(EXACT_LANE_MIN_LISTED <= (size_t)EDK_EXACT_SLOTS && EXACT_LANE_MIN_N <= (size_t)EDK_EXACT_SLOTS, "the four-lane chain's list fits its scratchpad");

enum verify_prepare { PREPARE_ONE, PREPARE_PAIR };     // k_verify_prepare | k_verify_prepare_pair (three lanes per item)
enum verify_eval { EVAL_FULL_ONE, EVAL_FULL_QUAD,      // k_verify_main | k_verify_main_quad, then k_verify_finish
                   EVAL_HALF_ONE, EVAL_HALF_ONE_LONG,  // k_verify_main_half | the same with the long loop in place (WITH_LONG)
                   EVAL_HALF_QUAD, EVAL_SUMS_QUAD,     // k_verify_main_half_quad | k_verify_window_sums + k_verify_main_sums_quad
                   EVAL_COMB_ONE };                    // k_verify_main_comb_keyed (a comb key set), then k_verify_finish
struct verify_route {
  verify_prepare prepare;
  bool halve;           // k_verify_halve runs
  bool wide;            // pairs up to 2^HALF_BITS_SMALL in HALF_WINDOWS_SMALL windows instead of HALF_BITS / HALF_WINDOWS, wherever either is a template argument
  verify_eval eval;
  uint32_t lane_min;    // the exact path.  != 0: the one-lane kernels are launched too and take the work lists of this many entries or more
  int dense;            // k_verify_exact_quad packs its items 16 to the wave whatever their number
  uint32_t main_cost;   // what runs beside k_verify_exact_lane_chain: executed instructions per item, thousands ...
  int main_all;         // ... over the whole pass (1) or over the on-curve list (0)
  bool keyed;           // the keyed forms of the kernels above (keyed_kernels.h): tab_a is the key's table in the key set
  bool balanced;        // k_verify_halve runs the balanced search (halve.h: pairs up to B33) and k_verify_main_half HALF_WINDOWS_BALANCED windows; never with wide
};
static_assert(HALF_WINDOWS_SMALL == HALF_BITS_SMALL / 4 + 1 && HALF_WINDOWS == HALF_BITS / 4 + 1, "a bound is chosen together with its count of signed four-bit windows");
static_assert(HALF_WINDOWS_BALANCED == HALF_WINDOWS - 1, "the balanced search saves one window of the full-size pass");

// algo (eddsa_amd_set_verify_algo) 0: by size, as listed; 1: full-length windows; 2: half-length, one lane per item; 3: the
// mid-size arrangement - below PAIR_ONE_MAX_N items: a larger pass has no such arrangement and takes the full-length route;
// 4: the arrangement of full-size passes (balanced pairs, 33 windows) from one item on, for the tests.
// Reject mode (exact_offcurve == 0) takes the full-length route whatever the algo: the half-length one relies on the exact
// path for its give-ups.      n                   prepare   halve  pairs / windows  evaluation
//   algo 0                    <= 256              pair      -      2^134 / 34       window sums + four-lane chain
//                             257 .. 2048         pair      -      2^138 / 35       window sums + four-lane chain
//                             2049 .. 24 576      pair      -      2^138 / 35       half-length, four lanes
//   algo 0 (3: from 1)        24 577 .. 2^18 - 1  pair      -      2^138 / 35       half-length, one lane, long loop in place
//   algo 0 (2: from 1)        2^18 .. 2^19 - 1    one lane  yes    2^138 / 35       half-length, one lane
//   algo 0, 2 (4: from 1)     >= 2^19             one lane  yes    B33 / 33         half-length, one lane (the balanced search: 1.7 give-ups in 10^3)
//   algo 1; 3 from 2^18; reject mode              one lane  -      -                full-length: four lanes up to 2^14 items, one above
// A KEYED pass (ed25519_verify_keyed*) takes the one-lane forms whatever its size and whatever the algo - the four-lane and
// three-lane kernels have no keyed form, so a small keyed pass pays the latency of the one-lane ones:
//   keyed, modes 1 and 2      < 2^19              one lane  yes    2^138 / 35       half-length, one lane
//                             >= 2^19             one lane  yes    2^134 / 34       half-length, one lane (not yet the balanced search)
//   keyed, reject mode        any                 one lane  -      -                full-length, one lane
// A keyed pass over a COMB key set (eddsa_amd_keyset_create_comb) is the full-length route with another main kernel, in every
// off-curve mode and at every size; in modes 1 and 2 the off-list and the exact path work as on the full-length route:
//   keyed, comb key set       any                 one lane  -      -                both combs, one lane (keyed_lanes.h: verify_comb_lane)
constexpr uint32_t COMB_MAIN_COST = 127;   // k_verify_main_comb_keyed, executed instructions per item, thousands: the static count of its blocks times their trip counts (profiles/verify_keyed_comb.txt, section 1)
constexpr uint32_t HALF_MAIN_COST_34 = 226;   // k_verify_main_half<34>, executed instructions per item, thousands; <33> runs one window (4 doublings + 2 cached additions) less
constexpr verify_route verify_route_of(size_t n, int algo, int exact_offcurve, bool keyed = false, bool comb = false) {
  if (keyed && comb) {
    verify_route c = {PREPARE_ONE, false, false, EVAL_COMB_ONE, 0, 0, COMB_MAIN_COST, 1, true};
    c.lane_min = n >= EXACT_LANE_MIN_N ? (uint32_t)EXACT_LANE_MIN_LISTED : 0u;
    c.dense = n >= EXACT_DENSE_MIN_N;
    return c;
  }
  if (!exact_offcurve) algo = 1;
  if (keyed) algo = exact_offcurve ? 2 : 1;   // (algo 2: the half-length route from one item on)
  verify_route r = {PREPARE_ONE, false, false, n <= QUAD_MAIN_MAX_N && !keyed ? EVAL_FULL_QUAD : EVAL_FULL_ONE, 0, 0, 0, 0};
  // mid-size passes: the three-lane preparation of the small route (its blocks fill the SIMDs that one lane per item leaves
  // with a single wave) and the one-lane evaluation; algo 3 forces it for measurements
  if ((algo == 3 || (algo == 0 && n > PAIR_ONE_MIN_N)) && n < PAIR_ONE_MAX_N)
    r = {PREPARE_PAIR, false, true, EVAL_HALF_ONE_LONG, 0, 0, 0, 0};
  // The four-lane evaluation runs 64 windows in the wave of an item without a short pair, and the pass waits for that wave:
  // with pairs up to 2^134 (8.5 items in 10^5) a pass of 2048 items has such an item one time in six, one of 2^14 three
  // times in four.  Above QUAD_WIDE_MIN_N items the search goes up to 2^138 (2 in 10^7) for a 35th window in every item.
  else if (algo == 0 && n <= HALF_QUAD_MAX_N)
    r = {PREPARE_PAIR, false, n > QUAD_WIDE_MIN_N, n <= EDK_SUMS_MAX_ITEMS ? EVAL_SUMS_QUAD : EVAL_HALF_QUAD, 0, 0, 0, 0};
  else if (algo == 0 || algo == 2 || algo == 4)
    r = {PREPARE_ONE, true, n < HALF_WIDE_MIN_N && algo != 4, EVAL_HALF_ONE, 0, 0, 0, 0};
  // full-size passes search balanced pairs and run 33 windows (the keyed kernels have no such form yet: 34)
  r.balanced = r.halve && !r.wide && !keyed;
  // Passes of EXACT_LANE_MIN_N items or more hand a work list of EXACT_LANE_MIN_LISTED entries or more to the one-lane
  // kernels; which form runs is decided on the device (the host does not know the list's length): the other ends at once.
  r.lane_min = n >= EXACT_LANE_MIN_N ? (uint32_t)EXACT_LANE_MIN_LISTED : 0u;
  r.dense = n >= EXACT_DENSE_MIN_N;
  // (beside the chain: the half-length evaluation over the on-curve list, 218 or 226 k instructions per item, or the full-length one
  // over the whole pass, 323 k: profiles/pmc_summary.json)
  const bool half_main = r.eval == EVAL_HALF_ONE || r.eval == EVAL_HALF_ONE_LONG;
  // (the half-length figure is that of the 33-window kernel, which config 2 of the profile runs; 34 and 35 windows: HALF_MAIN_COST_34)
  r.main_cost = half_main ? 218u : 323u;
  if (half_main && !r.balanced) r.main_cost = HALF_MAIN_COST_34;
  r.main_all = half_main ? 0 : 1;
  r.keyed = keyed;
  return r;
}
constexpr bool route_is(const verify_route& r, verify_prepare prepare, bool halve, bool wide, verify_eval eval) {
  return r.prepare == prepare && r.halve == halve && r.wide == wide && r.eval == eval;
}
static_assert(route_is(verify_route_of(256, 0, 1), PREPARE_PAIR, false, false, EVAL_SUMS_QUAD) && route_is(verify_route_of(257, 0, 1), PREPARE_PAIR, false, true, EVAL_SUMS_QUAD), "QUAD_WIDE_MIN_N");
static_assert(route_is(verify_route_of(2048, 0, 1), PREPARE_PAIR, false, true, EVAL_SUMS_QUAD) && route_is(verify_route_of(2049, 0, 1), PREPARE_PAIR, false, true, EVAL_HALF_QUAD), "EDK_SUMS_MAX_ITEMS");
static_assert(route_is(verify_route_of(24576, 0, 1), PREPARE_PAIR, false, true, EVAL_HALF_QUAD) && route_is(verify_route_of(24577, 0, 1), PREPARE_PAIR, false, true, EVAL_HALF_ONE_LONG), "PAIR_ONE_MIN_N");
static_assert(route_is(verify_route_of((1 << 18) - 1, 0, 1), PREPARE_PAIR, false, true, EVAL_HALF_ONE_LONG) && route_is(verify_route_of(1 << 18, 0, 1), PREPARE_ONE, true, true, EVAL_HALF_ONE), "PAIR_ONE_MAX_N");
static_assert(route_is(verify_route_of((1 << 19) - 1, 0, 1), PREPARE_ONE, true, true, EVAL_HALF_ONE) && route_is(verify_route_of(1 << 19, 0, 1), PREPARE_ONE, true, false, EVAL_HALF_ONE), "HALF_WIDE_MIN_N");
static_assert(verify_route_of(1 << 19, 0, 1).balanced && verify_route_of(1 << 20, 2, 1).balanced && !verify_route_of((1 << 19) - 1, 0, 1).balanced && !verify_route_of((1 << 19) - 1, 2, 1).balanced &&
              !verify_route_of(256, 0, 1).balanced && !verify_route_of(1 << 20, 1, 1).balanced && !verify_route_of(1 << 20, 3, 1).balanced && !verify_route_of(1 << 20, 0, 0).balanced,
              "the balanced search: unkeyed half-length passes of HALF_WIDE_MIN_N items or more, nothing else");
static_assert(route_is(verify_route_of(1, 4, 1), PREPARE_ONE, true, false, EVAL_HALF_ONE) && verify_route_of(1, 4, 1).balanced && verify_route_of(300, 4, 2).balanced && verify_route_of(1 << 20, 4, 1).balanced &&
              route_is(verify_route_of(300, 4, 0), PREPARE_ONE, false, false, EVAL_FULL_QUAD) && !verify_route_of(300, 4, 0).balanced, "algo 4: the balanced arrangement from one item on; reject mode as ever");
static_assert(!verify_route_of(1 << 20, 0, 1, true).balanced && !verify_route_of(1 << 20, 4, 1, true).balanced && !verify_route_of(1 << 20, 0, 1, true, true).balanced && verify_route_of(1 << 20, 0, 1, false, true).balanced,
              "keyed passes keep 34 windows");
static_assert(verify_route_of(1 << 20, 0, 1).main_cost == 218 && verify_route_of(1 << 19, 2, 1).main_cost == 218 && verify_route_of((1 << 19) - 1, 0, 1).main_cost == HALF_MAIN_COST_34 && verify_route_of(1 << 20, 0, 1).main_all == 0 && verify_route_of(1 << 20, 0, 1, true).main_cost == 226 &&
              verify_route_of(1 << 20, 0, 1).lane_min == 8192 && verify_route_of(1, 4, 1).lane_min == 0, "the balanced row: its own cost beside the chain, the exact path's hints by size as ever");
static_assert(route_is(verify_route_of(1 << 14, 1, 1), PREPARE_ONE, false, false, EVAL_FULL_QUAD) && route_is(verify_route_of((1 << 14) + 1, 1, 1), PREPARE_ONE, false, false, EVAL_FULL_ONE), "QUAD_MAIN_MAX_N");
static_assert(route_is(verify_route_of((1 << 18) - 1, 3, 1), PREPARE_PAIR, false, true, EVAL_HALF_ONE_LONG) && route_is(verify_route_of(1 << 18, 3, 1), PREPARE_ONE, false, false, EVAL_FULL_ONE), "algo 3 ends at PAIR_ONE_MAX_N");
static_assert(route_is(verify_route_of(1, 3, 1), PREPARE_PAIR, false, true, EVAL_HALF_ONE_LONG) && route_is(verify_route_of(1, 2, 1), PREPARE_ONE, true, true, EVAL_HALF_ONE), "algo 2 and 3 from one item on");
static_assert(route_is(verify_route_of(2048, 0, 0), PREPARE_ONE, false, false, EVAL_FULL_QUAD) && route_is(verify_route_of(1 << 17, 3, 0), PREPARE_ONE, false, false, EVAL_FULL_ONE) && route_is(verify_route_of(1 << 19, 2, 0), PREPARE_ONE, false, false, EVAL_FULL_ONE), "reject mode");
static_assert(verify_route_of((1 << 16) - 1, 0, 1).lane_min == 0 && !verify_route_of((1 << 16) - 1, 0, 1).dense && verify_route_of(1 << 16, 0, 1).lane_min == 8192 && verify_route_of(1 << 16, 0, 1).dense, "EXACT_LANE_MIN_N, EXACT_DENSE_MIN_N");
static_assert(route_is(verify_route_of(1, 0, 1, true), PREPARE_ONE, true, true, EVAL_HALF_ONE) && route_is(verify_route_of(2048, 3, 2, true), PREPARE_ONE, true, true, EVAL_HALF_ONE) &&
              route_is(verify_route_of((1 << 19) - 1, 0, 1, true), PREPARE_ONE, true, true, EVAL_HALF_ONE) && route_is(verify_route_of(1 << 19, 1, 1, true), PREPARE_ONE, true, false, EVAL_HALF_ONE),
              "a keyed pass in an exact mode: what verify_route_of(n, 2, 1) gives, whatever the algo");
static_assert(route_is(verify_route_of(1, 0, 0, true), PREPARE_ONE, false, false, EVAL_FULL_ONE) && route_is(verify_route_of(1 << 14, 2, 0, true), PREPARE_ONE, false, false, EVAL_FULL_ONE) &&
              route_is(verify_route_of(1 << 20, 0, 0, true), PREPARE_ONE, false, false, EVAL_FULL_ONE), "a keyed pass in reject mode: the one-lane full-length route, also below 2^14 items");
static_assert(verify_route_of(1 << 20, 0, 1, true).keyed && !verify_route_of(1 << 20, 0, 1).keyed && route_is(verify_route_of(1 << 20, 0, 1, true), PREPARE_ONE, true, false, EVAL_HALF_ONE) &&
              verify_route_of(1 << 16, 0, 1, true).lane_min == 8192 && verify_route_of(1 << 16, 0, 1, true).main_cost == 226, "keyed: the exact path's hints as for the unkeyed route");
static_assert(route_is(verify_route_of(1, 0, 0, true, true), PREPARE_ONE, false, false, EVAL_COMB_ONE) && route_is(verify_route_of(1 << 14, 3, 1, true, true), PREPARE_ONE, false, false, EVAL_COMB_ONE) &&
              route_is(verify_route_of(1 << 20, 0, 2, true, true), PREPARE_ONE, false, false, EVAL_COMB_ONE) && verify_route_of(1 << 20, 0, 1, true, true).keyed,
              "a keyed pass over a comb key set: one route in every off-curve mode, at every size, whatever the algo");
static_assert(route_is(verify_route_of(1 << 20, 0, 1, false, true), PREPARE_ONE, true, false, EVAL_HALF_ONE) && !verify_route_of(1 << 20, 0, 1, false, true).keyed, "no comb route without a key set");
static_assert(verify_route_of((1 << 16) - 1, 0, 1, true, true).lane_min == 0 && verify_route_of(1 << 16, 0, 1, true, true).lane_min == 8192 && verify_route_of(1 << 16, 0, 1, true, true).dense &&
              verify_route_of(1 << 16, 0, 1, true, true).main_cost == COMB_MAIN_COST && verify_route_of(1 << 16, 0, 1, true, true).main_all == 1, "comb: the exact path's hints, the main kernel runs over the whole pass");
static_assert(verify_route_of(1 << 16, 0, 1).main_cost == 226 && verify_route_of(1 << 16, 0, 1).main_all == 0 && verify_route_of(1 << 16, 1, 1).main_cost == 323 && verify_route_of(1 << 16, 1, 1).main_all == 1, "the chain's hint follows the evaluation");

// the first kernel of a verify pass: the three-lane preparation or the one-lane one.
// DIGEST: the forms that take t from the caller's digest (edk_verify_src.digest)
template <bool DIGEST>
static hipError_t launch_prepare(const edk_verify_items& src, size_t n, const edk_verify_ws* ws, const verify_route& r, const uint32_t* perm, hipStream_t stream) {
  const unsigned blocks = blocks_of(n), pair_point_blocks = blocks_of(2 * n);
  if (r.prepare == PREPARE_PAIR) {
    const auto k = r.wide ? k_verify_prepare_pair<HALF_BITS_SMALL, DIGEST> : k_verify_prepare_pair<HALF_BITS, DIGEST>;
    EDK_LAUNCH(k, dim3(pair_point_blocks + blocks), dim3(BLOCK), 0, stream, src, n, ws->digits, ws->hdigits, ws->table, ws->rtable, ws->flags,
               ws->onlist, ws->offlist, ws->offcount, ws->exact_offcurve == 2, pair_point_blocks, perm);
  } else
    EDK_LAUNCH(k_verify_prepare<DIGEST>, dim3(blocks), dim3(BLOCK), 0, stream, src, n, ws->digits, ws->table, ws->flags, ws->onlist, ws->offlist,
               ws->offcount, ws->exact_offcurve == 2, perm);
  return hipSuccess;
}

// ---- the fixed-base operations: the shapes of their two kernels ----
// Items per lane that share one inversion in the finish kernels: FINISH_K (8) in a pass that fills the chip; in a smaller
// pass as few as it takes to keep one block of 256 lanes per CU - a lane with one item runs 31 k dependent instructions,
// with eight 70 k, and a pass of 2^12 items would otherwise occupy two CUs.
struct finish_shape { unsigned grid; int k; };
constexpr finish_shape finish_shape_of(size_t n) {
  unsigned k = 1;
  while (k < (unsigned)FINISH_K && (blocks_of(n) + k - 1) / k > 256) k *= 2;
  return {(blocks_of(n) + k - 1) / k, (int)k};
}

// Point kernels stage the comb in LDS per block, one block per CU.  A pass that fills the chip runs blocks of POINT_BLOCK
// lanes (two waves per SIMD).  A smaller pass runs smaller blocks: a block of 512 lanes puts two waves on every SIMD of
// ONE CU, which then take turns (a single ed25519_genpub ran its one useful wave beside seven idle-lane waves redoing
// the same item: 0.23 ms in the point kernel against 0.12 with a wave to itself), and 4096 items occupied 8 CUs of 256.
// So: the smallest block that covers the pass with one block per CU - one, two or four waves, each with a SIMD to itself.
// Passes of up to POINT_SPLIT_MAX_N items spend four lanes on an item (lanes.h: scale_base_lane<4>, k_genpub_point above): the 44 additions of
// the comb in a row were the latency of the pass (a single ed25519_sign: 0.17 ms in k_sign_point, now 0.09).  A pass with more
// tiles than CUs runs POINT_MAX_BLOCKS persistent blocks whose waves draw their tiles from ws->tiles (point_tile above); a smaller
// one a block per tile, without the counter.
constexpr size_t POINT_SPLIT_MAX_N = (size_t)1 << 14;
struct point_shape { int lanes_per_item; unsigned block, grid; bool persistent; };
constexpr point_shape point_shape_of(size_t n) {
  if (n <= POINT_SPLIT_MAX_N) return {POINT_SPLIT, POINT_SPLIT * 64, blocks_of(n, POINT_SPLIT_ITEMS), false};
  const unsigned block = n <= (size_t)64 * 256 ? 64 : n <= (size_t)128 * 256 ? 128 : n <= (size_t)256 * 256 ? 256 : POINT_BLOCK;
  const unsigned tiles = blocks_of(n, block);
  return {1, block, tiles > POINT_MAX_BLOCKS ? POINT_MAX_BLOCKS : tiles, tiles > POINT_MAX_BLOCKS};
}
constexpr bool shape_is(const point_shape& s, int lanes_per_item, unsigned block, unsigned grid, bool persistent) {
  return s.lanes_per_item == lanes_per_item && s.block == block && s.grid == grid && s.persistent == persistent;
}
static_assert(shape_is(point_shape_of(1 << 14), 4, 256, 256, false) && shape_is(point_shape_of((1 << 14) + 1), 1, 128, 129, false), "POINT_SPLIT_MAX_N");
static_assert(shape_is(point_shape_of(1 << 15), 1, 128, 256, false) && shape_is(point_shape_of((1 << 15) + 1), 1, 256, 129, false), "two waves, four waves");
static_assert(shape_is(point_shape_of(1 << 16), 1, 256, 256, false) && shape_is(point_shape_of((1 << 16) + 1), 1, POINT_BLOCK, blocks_of((1 << 16) + 1, POINT_BLOCK), false), "four waves, POINT_BLOCK");
static_assert(shape_is(point_shape_of((size_t)POINT_MAX_BLOCKS * POINT_BLOCK), 1, POINT_BLOCK, POINT_MAX_BLOCKS, false) &&
              shape_is(point_shape_of((size_t)POINT_MAX_BLOCKS * POINT_BLOCK + 1), 1, POINT_BLOCK, POINT_MAX_BLOCKS, true), "more tiles than resident blocks: persistent");

// X25519: the four-lane ladder in small passes, the one-lane ladder above; the finish shares one inversion between 1, 2, 4
// or 8 items.  tests/test_gpu_x25519.py places low-order points in every slot of every lane group at exactly these sizes: a
// retuning of the shapes must move the sizes of that test with it.
constexpr bool x25519_ladder_is_quad(size_t n) { return n <= X25519_QUAD_MAX_N; }
constexpr bool finish_is(const finish_shape& f, int k, unsigned grid) { return f.k == k && f.grid == grid; }
static_assert(x25519_ladder_is_quad(X25519_QUAD_MAX_N) && !x25519_ladder_is_quad(X25519_QUAD_MAX_N + 1) && X25519_QUAD_MAX_N == 16384, "the one-lane ladder from 2^14 + 1 items on");
static_assert(!x25519_ladder_is_quad(17229) && finish_is(finish_shape_of(17229), 1, 68), "one-lane ladder, K = 1");
static_assert(finish_is(finish_shape_of(65536 + 2 * 256 + 77), 2, 130), "259 tiles: K = 2, the last block holds one tile");
static_assert(finish_is(finish_shape_of(131072 + 256 + 77), 4, 129), "514 tiles: K = 4, the last block holds two tiles");
static_assert(finish_is(finish_shape_of(262144 + 2 * 256 + 77), 8, 129), "1027 tiles: K = 8, the last block holds three tiles");

// the point kernel of a pass of n items in the form its shape asks for (split: PARTS = POINT_SPLIT, whole: PARTS = 1); args: the
// kernel's arguments without its last, the tile counter.  Unchecked like every fixed-base launch: the caller asks hipGetLastError
template <class K, class... A>
static hipError_t launch_point(K split, K whole, size_t n, const edk_fixed_ws* ws, hipStream_t stream, A... args) {
  const point_shape s = point_shape_of(n);
  if (s.persistent)
    if (const hipError_t e = hipMemsetAsync(ws->tiles, 0, sizeof(uint32_t), stream); e != hipSuccess) return e;
  hipLaunchKernelGGL(s.lanes_per_item == POINT_SPLIT ? split : whole, dim3(s.grid), dim3(s.block), 0, stream, args..., s.persistent ? ws->tiles : (uint32_t*)nullptr);
  return hipSuccess;
}

extern "C" {

hipError_t edk_init_tables(uint32_t* base16, uint32_t* comb, uint32_t* comb_img, hipStream_t stream) {
  const int total = 2 * TABLE_BASE16_ENTRIES + TABLE_COMB_ENTRIES;
  hipLaunchKernelGGL(k_init_tables, dim3((total + 63) / 64), dim3(64), 0, stream, base16, comb);
  hipLaunchKernelGGL(k_init_comb_image, dim3((COMB_ROWS * COMB_IMG_ENTRIES + 63) / 64), dim3(64), 0, stream, comb_img, comb);
  return hipGetLastError();
}

hipError_t edk_x25519(uint8_t* out, const uint8_t* scalars, const uint8_t* points, size_t n, const edk_fixed_ws* ws, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const finish_shape f = finish_shape_of(n);
  if (x25519_ladder_is_quad(n))
    hipLaunchKernelGGL(k_x25519_ladder_quad, dim3(blocks_of(4 * n)), dim3(BLOCK), 0, stream, ws->acc, scalars, points, n);
  else
    hipLaunchKernelGGL(k_x25519_ladder, dim3(blocks_of(n)), dim3(BLOCK), 0, stream, ws->acc, scalars, points, n);
  hipLaunchKernelGGL(k_x25519_finish, dim3(f.grid), dim3(BLOCK), 0, stream, out, ws->acc, n, f.k);
  return hipGetLastError();
}

// the test hook of edk_checked.h: checked calls made since the count was restarted, and the call that is to fail
static std::atomic<int> g_checked{0}, g_fail_at{0}, g_counting{0};
int edk_fault_tick(void) {
  // Unarmed (every production pass): one relaxed load of a line nobody writes.  The calls are counted only while a fault is
  // pending or a test has restarted the count (g_counting): no shared counter is bumped on the hot path otherwise.
  int at = g_fail_at.load(std::memory_order_relaxed);
  if (at == 0 && !g_counting.load(std::memory_order_relaxed)) return 0;
  const int k = g_checked.fetch_add(1, std::memory_order_relaxed) + 1;
  return at != 0 && k == at && g_fail_at.compare_exchange_strong(at, 0);
}
void edk_debug_counting(int on) { g_counting.store(on != 0); }
int edk_debug_fail_in(int nth) {
  if (nth < 0) return g_checked.load();
  g_fail_at.store(0);
  g_checked.store(0);
  g_fail_at.store(nth);
  return 0;
}

// *perm = buf[0..n) filled with the items in order of message length, longest first (k_len_*; bins = 2 * LEN_BINS words of the
// workspace), or nullptr where the pass takes its items as they come: no offset table, or fewer than MSG_ORDER_MIN_N items
static hipError_t msg_order(const uint32_t** perm, uint32_t* buf, uint32_t* bins, const uint64_t* msg_off, const uint64_t* msg_end, size_t n, hipStream_t stream) {
  *perm = nullptr;
  if (!msg_off || n < MSG_ORDER_MIN_N) return hipSuccess;
  hipError_t e = hipMemsetAsync(bins, 0, (size_t)LEN_BINS * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  static_assert(LEN_BINS % BLOCK == 0, "k_len_starts: a thread takes LEN_BINS / BLOCK bins");
  hipLaunchKernelGGL(k_len_count, dim3(blocks_of(n)), dim3(BLOCK), 0, stream, bins, msg_off, msg_end, n);
  hipLaunchKernelGGL(k_len_starts, dim3(1), dim3(BLOCK), 0, stream, bins);
  hipLaunchKernelGGL(k_len_place, dim3(blocks_of(n)), dim3(BLOCK), 0, stream, buf, bins, msg_off, msg_end, n);
  e = hipGetLastError();
  if (e == hipSuccess) *perm = buf;
  return e;
}

// the verify workspace's order for a pass of n items; rlc.hip's hashing kernel shares it
hipError_t edk_msg_order(const uint32_t** perm, const edk_verify_ws* ws, const uint64_t* msg_off, const uint64_t* msg_end, size_t n, hipStream_t stream) {
  return msg_order(perm, ws->perm, ws->lenbins, msg_off, msg_end, n, stream);
}

// the strict rules over the n verdicts of a pass (edk_checked.h; rlc.hip launches it too); policy 0: nothing is queued
hipError_t verify_policy_launch(uint8_t* ok, const uint8_t* sigs, size_t sig_stride, const uint8_t* pubs, size_t pub_stride, size_t n,
                                int policy, hipStream_t stream) {
  if (policy == 0 || n == 0) return hipSuccess;
  EDK_LAUNCH(k_verify_policy, dim3(blocks_of(n)), dim3(BLOCK), 0, stream, ok, sigs, sig_stride, pubs, pub_stride, n, (unsigned)policy);
  return hipSuccess;
}

// Every HIP call below that orders work or moves data is checked (edk_checked.h): the first failure ends the pass with
// that error.  What has been queued by then still runs; eddsa_amd.c: verify_on waits for it (both streams) before the
// workspace can be handed out again, and the caller learns that the outputs are unspecified.
hipError_t edk_verify(uint8_t* ok, const edk_verify_src* srcp, size_t n, const uint32_t* base16,
                      const edk_verify_ws* ws, hipEvent_t* marks, hipEvent_t bulk_done, int bulk_early, hipStream_t stream) {
  edk_verify_src src = *srcp;
  if (n == 0) return hipSuccess;
  const bool keyed = src.ks_table != nullptr;     // ed25519_verify_keyed*: the keys come from a key set, by src.key_idx
  if (keyed && (!src.key_idx || !src.ks_keys || !src.ks_flags || src.ks_count == 0 || src.ks_count > (size_t)UINT32_MAX)) return hipErrorInvalidValue;
  const bool comb = keyed && src.ks_comb != nullptr;   // ... and the set holds a comb per key: both scalars by fixed-base arithmetic
  if (comb && !ws->comb) return hipErrorInvalidValue;
  const verify_route r = verify_route_of(n, ws->algo, ws->exact_offcurve, keyed, comb);
  const unsigned blocks = blocks_of(n), quad_blocks = blocks_of(4 * n, QUAD_BLOCK);
  // 1. reset: both work lists' lengths, the one-lane exact path's unit counter and its stall flag
  EDK_DO(hipMemsetAsync(ws->offcount, 0, EDK_PASS_WORDS * sizeof(uint32_t), stream));
  if (marks) EDK_DO(hipEventRecord(marks[0], stream));
  // 2. message order: the hashing kernels take ragged messages in order of length
  const uint32_t* perm = nullptr;
  if (!src.digest) EDK_DO(edk_msg_order(&perm, ws, src.msg_off, src.msg_end, n, stream));
  // 3. prepare.  Caller-supplied digests (ed25519_verify_digests*): the same preparations without the hash; everything after
  // them reads t from the workspace and does not know
  hipError_t prepared;
  if (keyed) {
    // the keyed prepare takes the key bytes and the on-curve flag from the key set and leaves the bytes in ws->keybytes: every
    // kernel behind it that reads `pubs` (the cofactored equation, the strict rules) reads them there
    // Its digest form serves ed25519_verify_keyed_digests* (the caller's digests in the message slot) and, behind
    // k_dom_challenge_keyed, the ctx / ph keyed forms: one lane per item hashes dom2 || R || keys[key_idx] || M' into the item's
    // 64 bytes of ws->domdig, and the pass goes on as a keyed digest pass over that area, as the unkeyed one does below
    edk_verify_items items = edk_items_of(&src);
    if (src.dom) {
      EDK_LAUNCH(k_dom_challenge_keyed, dim3(blocks), dim3(BLOCK), 0, stream, items, n, ws->domdig, perm, *src.dom, src.ks_keys, src.key_idx,
                 (uint32_t)src.ks_count);
      items = { src.sigs, nullptr, ws->domdig, nullptr, EDK_DOM_DIGEST_BYTES, src.sig_stride, src.pub_stride, EDK_DOM_DIGEST_BYTES, nullptr };
    }
    const auto prepare = src.digest || src.dom ? k_verify_prepare_keyed<true> : k_verify_prepare_keyed<false>;
    EDK_LAUNCH(prepare, dim3(blocks), dim3(BLOCK), 0, stream, items, n, ws->digits, ws->flags, ws->onlist, ws->offlist, ws->offcount,
               ws->exact_offcurve, src.digest || src.dom ? nullptr : perm, src.ks_keys, src.ks_flags, src.key_idx, (uint32_t)src.ks_count,
               ws->keybytes, ok);
    // the items listed for the exact path get a table of their own (none in reject mode, which has no such path)
    if (ws->exact_offcurve) EDK_LAUNCH(k_keyed_exact_tables, dim3(blocks), dim3(BLOCK), 0, stream, ws->table, ws->keybytes, ws->offlist, ws->offcount);
    src.pubs = ws->keybytes;
    src.pub_stride = 32;
    prepared = hipSuccess;
  } else if (src.dom) {
    // Ed25519ctx / Ed25519ph: one lane per item hashes dom2 || R || A || M' into the item's 64 bytes of ws->domdig (in order of
    // length, like every hashing kernel); from there on the pass IS a digest pass whose message slot is that area
    EDK_LAUNCH(k_dom_challenge, dim3(blocks), dim3(BLOCK), 0, stream, edk_items_of(&src), n, ws->domdig, perm, *src.dom);
    const edk_verify_items hashed = { src.sigs, src.pubs, ws->domdig, nullptr, EDK_DOM_DIGEST_BYTES, src.sig_stride, src.pub_stride, EDK_DOM_DIGEST_BYTES, nullptr };
    prepared = launch_prepare<true>(hashed, n, ws, r, nullptr, stream);
  } else
    prepared = src.digest ? launch_prepare<true>(edk_items_of(&src), n, ws, r, perm, stream) : launch_prepare<false>(edk_items_of(&src), n, ws, r, perm, stream);
  if (prepared != hipSuccess) return prepared;
  // 4. halve.  Below HALF_WIDE_MIN_N items the pass searches pairs up to 2^138 and runs 35 windows (2 t in 10^7 without a pair
  // instead of 8.5 in 10^5; 3 % more instructions in the main kernel): an item without a short pair goes through the exact
  // path's chain, and beside a main kernel of one or two rounds of resident blocks that chain costs the pass 0.3-0.4 ms (the
  // SIMDs its waves sit on finish their tiles that much later and the grid has no slack: profiles/r04_small_grid.txt).  From
  // HALF_WIDE_MIN_N items on an unkeyed pass searches balanced pairs (both values at most B33, halve.h) and runs 33 windows: 1.9 t
  // in 10^3 without a pair, which the chain beside a full-size main kernel absorbs (profiles/verify_balanced_pairs.txt)
  if (r.halve && r.keyed) {
    const auto k = r.wide ? k_verify_halve_keyed<HALF_BITS_SMALL> : k_verify_halve_keyed<HALF_BITS>;
    EDK_LAUNCH(k, dim3(blocks), dim3(BLOCK), 0, stream, src.sigs, src.sig_stride, ws->digits, ws->hdigits, ws->rtable, ws->flags, ws->onlist, ws->offlist, ws->offcount,
               ws->table, src.ks_table, src.key_idx);
  } else if (r.halve) {
    const auto k = r.wide ? k_verify_halve<HALF_BITS_SMALL> : r.balanced ? k_verify_halve<HALF_BITS_BALANCED> : k_verify_halve<HALF_BITS>;
    EDK_LAUNCH(k, dim3(blocks), dim3(BLOCK), 0, stream, src.sigs, src.sig_stride, ws->digits, ws->hdigits, ws->rtable, ws->flags, ws->onlist, ws->offlist, ws->offcount);
  }
  if (marks) EDK_DO(hipEventRecord(marks[1], stream));
  if (bulk_done && bulk_early) EDK_DO(hipEventRecord(bulk_done, stream));   // the next pass may start beside this one's main kernel
  // 5. the exact path depends only on what came before: it runs beside the main kernel on the side stream
  if (ws->exact_offcurve) {
    EDK_DO(hipEventRecord(ws->ev_prepared, stream));
    EDK_DO(hipStreamWaitEvent(ws->side, ws->ev_prepared, 0));
    // The one-lane kernels go FIRST on the side stream: when the list is short they end at once, and they must do so while
    // the chip still has room for their (large) blocks - queued behind the four-lane chain they reached the dispatcher a
    // millisecond into a full k_verify_main_half, where each of their 512 idle blocks had to wait for two wave slots of one
    // SIMD to fall free together (profiles/r05_exact_lane.txt: same-box A/B, 107.2 -> 107.9 M/s on config 2).
    if (r.lane_min != 0) {
      const unsigned lane_blocks = blocks < EXACT_LANE_BLOCKS ? blocks : EXACT_LANE_BLOCKS;
      // (the scratchpad of the four-lane chain is free when these run: it holds their per-tile counts)
      EDK_LAUNCH(k_verify_exact_lane_setup, dim3(lane_blocks), dim3(BLOCK), 0, ws->side, ws->digits, ws->table, ws->rtable, ws->offlist,
                 ws->offcount, base16, ws->exact_pad, r.lane_min);
      EDK_LAUNCH(k_verify_exact_lane_chain, dim3(lane_blocks), dim3(BLOCK), 0, ws->side, ok, src.sigs, src.sig_stride, ws->table, ws->rtable,
                 ws->offlist, ws->offcount, ws->exact_pad, r.lane_min, n, r.main_cost, r.main_all, ws->status);
    }
    // one launch of the four-lane chain: a list it would serve has fewer entries than the scratchpad has slots (lane_min != 0:
    // fewer than lane_min; else the pass itself is smaller than EXACT_LANE_MIN_N)
    const size_t qi = r.lane_min != 0 ? (size_t)r.lane_min : n;
    const size_t dense = (qi + QUAD_CHAIN_ITEMS - 1) / QUAD_CHAIN_ITEMS, spread = qi < (size_t)QUAD_SPREAD_WAVES ? qi : (size_t)QUAD_SPREAD_WAVES;
    EDK_LAUNCH(k_verify_exact_quad, dim3((unsigned)(dense > spread ? dense : spread)), dim3(QUAD_CHAIN_BLOCK), 0, ws->side, ok, src.sigs,
               src.sig_stride, ws->digits, ws->table, ws->offlist, ws->offcount, base16, ws->exact_pad, r.dense, r.lane_min);
    EDK_DO(hipEventRecord(ws->ev_exact, ws->side));
  }
  // 6. evaluation; the half-length ones have no finish kernel: both marks at their end
  switch (r.eval) {
    case EVAL_SUMS_QUAD: {
      static_assert(QUAD_BLOCK == 4 * HALF_LONG_WINDOWS, "a block of k_verify_window_sums is the windows of one item");
      const auto sums = r.wide ? k_verify_window_sums<HALF_WINDOWS_SMALL> : k_verify_window_sums<HALF_WINDOWS>;
      const auto chain = r.wide ? k_verify_main_sums_quad<HALF_WINDOWS_SMALL> : k_verify_main_sums_quad<HALF_WINDOWS>;
      EDK_LAUNCH(sums, dim3((unsigned)n), dim3(QUAD_BLOCK), 0, stream, ws->sums, ws->hdigits, ws->table, ws->rtable, base16);
      EDK_LAUNCH(chain, dim3(quad_blocks), dim3(QUAD_BLOCK), 0, stream, ok, ws->hdigits, ws->sums, ws->flags, n, ws->exact_offcurve);
    } break;
    case EVAL_HALF_QUAD: {
      const auto k = r.wide ? k_verify_main_half_quad<HALF_WINDOWS_SMALL> : k_verify_main_half_quad<HALF_WINDOWS>;
      EDK_LAUNCH(k, dim3(quad_blocks), dim3(QUAD_BLOCK), 0, stream, ok, ws->hdigits, ws->table, ws->rtable, base16, ws->flags, n, ws->exact_offcurve);
    } break;
    case EVAL_HALF_ONE: case EVAL_HALF_ONE_LONG: {
      constexpr unsigned half_lds = MAIN_LDS_RESERVE;
      static_assert(HALF_DIGIT_WORDS * MAIN_HALF_BLOCK * 4 <= half_lds, "k_verify_main_half keeps its digit words in the block's LDS");
      const unsigned hblocks = (blocks * BLOCK + MAIN_HALF_BLOCK - 1) / MAIN_HALF_BLOCK;
      if (r.keyed) {                             // (EVAL_HALF_ONE only: verify_route_of)
        const auto kk = r.wide ? k_verify_main_half_keyed<HALF_WINDOWS_SMALL> : k_verify_main_half_keyed<HALF_WINDOWS>;
        EDK_LAUNCH(kk, dim3(hblocks), dim3(MAIN_HALF_BLOCK), half_lds, stream, ok, ws->hdigits, src.ks_table, src.key_idx, ws->rtable, base16, ws->flags, ws->onlist, ws->offcount);
        break;
      }
      const auto k = r.eval == EVAL_HALF_ONE_LONG ? k_verify_main_half<HALF_WINDOWS_SMALL, true> : r.wide ? k_verify_main_half<HALF_WINDOWS_SMALL> :
                     r.balanced ? k_verify_main_half<HALF_WINDOWS_BALANCED> : k_verify_main_half<HALF_WINDOWS>;
      EDK_LAUNCH(k, dim3(hblocks), dim3(MAIN_HALF_BLOCK), half_lds, stream, ok, ws->hdigits, ws->table, ws->rtable, base16, ws->flags, ws->onlist, ws->offcount);
    } break;
    case EVAL_FULL_QUAD: EDK_LAUNCH(k_verify_main_quad, dim3(quad_blocks), dim3(QUAD_BLOCK), 0, stream, ws->digits, ws->table, base16, ws->acc, n); break;
    case EVAL_FULL_ONE:
      if (r.keyed) EDK_LAUNCH(k_verify_main_keyed, dim3(blocks), dim3(BLOCK), MAIN_LDS_RESERVE, stream, ws->digits, src.ks_table, src.key_idx, (uint32_t)src.ks_count, n, base16, ws->acc);
      else EDK_LAUNCH(k_verify_main, dim3(blocks), dim3(BLOCK), MAIN_LDS_RESERVE, stream, ws->digits, ws->table, base16, ws->acc);
      break;
    case EVAL_COMB_ONE:
      EDK_LAUNCH(k_verify_main_comb_keyed, dim3(blocks), dim3(BLOCK), 0, stream, ws->digits, src.ks_comb, src.ks_table, src.key_idx, (uint32_t)src.ks_count, n, ws->comb, ws->acc);
      break;
  }
  if (marks) EDK_DO(hipEventRecord(marks[2], stream));
  if (r.eval == EVAL_FULL_ONE || r.eval == EVAL_FULL_QUAD || r.eval == EVAL_COMB_ONE) {
    const finish_shape f = finish_shape_of(n);
    EDK_LAUNCH(k_verify_finish, dim3(f.grid), dim3(BLOCK), 0, stream, ok, src.sigs, src.sig_stride, ws->acc, ws->flags, n, ws->exact_offcurve, f.k);
  }
  if (marks) EDK_DO(hipEventRecord(marks[3], stream));
  // everything that fills the chip has been queued; what follows on this stream only waits for the exact path's few
  // latency-bound waves: a caller that pipelines passes over several workspaces starts the next pass from here
  if (bulk_done && !bulk_early) EDK_DO(hipEventRecord(bulk_done, stream));
  // 7. the join: complete when both paths are
  if (ws->exact_offcurve) EDK_DO(hipStreamWaitEvent(stream, ws->ev_exact, 0));
  // 7b. the opt-in cofactored equation: the rejected items are listed and decided again (nothing is queued for equation 0)
  if (src.equation) {
    EDK_DO(hipMemsetAsync(ws->offcount + EDK_COLIST_WORD, 0, sizeof(uint32_t), stream));
    EDK_LAUNCH(k_cofactor_list, dim3(blocks), dim3(BLOCK), 0, stream, ok, n, ws->onlist, ws->offcount, ws->exact_offcurve == 2);
    EDK_LAUNCH(k_cofactor_points, dim3(blocks), dim3(BLOCK), 0, stream, src.sigs, src.sig_stride, src.pubs, src.pub_stride, ws->table,
               ws->rtable, ws->flags, ws->onlist, ws->offcount);
    EDK_LAUNCH(k_cofactor_eval, dim3(blocks < COFACTOR_MAX_BLOCKS ? blocks : COFACTOR_MAX_BLOCKS), dim3(BLOCK), 0, stream, ok, ws->digits,
               ws->table, ws->rtable, base16, ws->flags, ws->onlist, ws->offcount);
  }
  // 8. the opt-in strict rules, behind every writer of ok[] on both streams (nothing is queued for policy 0); the cofactored
  // equation adds S < l for the items the pass itself accepted
  return verify_policy_launch(ok, src.sigs, src.sig_stride, src.pubs, src.pub_stride, n,
                              src.policy | (src.equation ? EDDSA_AMD_VERIFY_S_BELOW_L : 0), stream);
}

// the tables and flags of a key set (edk_keyed.h): `count` keys of 32 bytes in HBM -> table (count slots of a verify item's
// table) and flags (one byte per key).  Asynchronous on `stream`
hipError_t edk_keyset_build(uint32_t* table, uint8_t* flags, const uint8_t* keys, size_t count, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_keyset_build, dim3(blocks_of(count)), dim3(BLOCK), 0, stream, table, flags, keys, count);
  return hipGetLastError();
}

// the combs of a comb key set (edk_keyed.h): KEYSET_COMB_WORDS words per key.  Asynchronous on `stream`
hipError_t edk_keyset_comb_build(uint32_t* comb, const uint8_t* keys, size_t count, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  hipLaunchKernelGGL(k_keyset_comb_build, dim3(blocks_of(count * COMB_ROWS)), dim3(BLOCK), 0, stream, comb, keys, count);
  return hipGetLastError();
}

hipError_t edk_genpub(uint8_t* pubs, const uint8_t* secs, size_t n, const uint32_t* comb, const edk_fixed_ws* ws, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const finish_shape f = finish_shape_of(n);
  if (const hipError_t e = launch_point(k_genpub_point<POINT_SPLIT>, k_genpub_point<1>, n, ws, stream, ws->acc, secs, n, comb); e != hipSuccess) return e;
  hipLaunchKernelGGL(k_encode_finish, dim3(f.grid), dim3(BLOCK), 0, stream, pubs, ws->acc, n, f.k);
  return hipGetLastError();
}

hipError_t edk_sign(uint8_t* sigs, const uint8_t* secs, const uint8_t* pubs, const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* msg_end,
                    size_t msg_len, size_t n, const uint32_t* comb, const edk_fixed_ws* ws, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const finish_shape f = finish_shape_of(n);
  const uint32_t* perm = nullptr;                  // ragged messages: both kernels hash, both take their items in order of length
  if (const hipError_t e = msg_order(&perm, ws->perm, ws->lenbins, msg_off, msg_end, n, stream); e != hipSuccess) return e;
  if (ws->dom) {                                   // Ed25519ctx / Ed25519ph: scalars, point, finish - the same shapes, the prefixed hashes
    hipLaunchKernelGGL(k_sign_dom_scalars, dim3(blocks_of(n)), dim3(BLOCK), 0, stream, ws->aux, secs, msgs, msg_off, msg_end, msg_len, n, perm, *ws->dom);
    if (const hipError_t e = launch_point(k_sign_dom_point<POINT_SPLIT>, k_sign_dom_point<1>, n, ws, stream, ws->acc, (const uint32_t*)ws->aux, n, comb); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sign_dom_finish, dim3(f.grid), dim3(BLOCK), 0, stream, sigs, ws->acc, ws->aux, pubs, msgs, msg_off, msg_end, msg_len, n, f.k, perm, *ws->dom);
    return hipGetLastError();
  }
  if (const hipError_t e = launch_point(k_sign_point<POINT_SPLIT>, k_sign_point<1>, n, ws, stream, ws->acc, ws->aux, secs, msgs, msg_off, msg_end, msg_len, n, comb, perm); e != hipSuccess) return e;
  hipLaunchKernelGGL(k_sign_finish, dim3(f.grid), dim3(BLOCK), 0, stream, sigs, ws->acc, ws->aux, pubs, msgs, msg_off, msg_end, msg_len, n, f.k, perm);
  return hipGetLastError();
}

// a signer set (edk_signer.h): `count` seeds or expanded keys in HBM -> a mod l, the prefixes and the encoded public keys.
// Asynchronous on `stream`
hipError_t edk_signer_build(uint32_t* a, uint32_t* prefix, uint8_t* pubs, const uint8_t* keys, size_t count, int expanded, const uint32_t* comb,
                            hipStream_t stream) {
  if (count == 0) return hipSuccess;
  const dim3 grid(blocks_of(count, POINT_BLOCK)), block(POINT_BLOCK);
  if (expanded) hipLaunchKernelGGL(k_signer_build<true>, grid, block, 0, stream, a, prefix, pubs, keys, count, comb);
  else hipLaunchKernelGGL(k_signer_build<false>, grid, block, 0, stream, a, prefix, pubs, keys, count, comb);
  return hipGetLastError();
}

// edk_sign over a signer set: scalars, point, finish - the shapes of the Ed25519ctx / Ed25519ph pass, whose point kernel it
// shares.  The fused shape (hash and comb in one kernel, as k_sign_point) was not built: include/eddsa_amd.h has the figures
hipError_t edk_sign_keyed(uint8_t* sigs, const edk_signer_set* set, const uint32_t* key_idx, const uint8_t* msgs, const uint64_t* msg_off,
                          const uint64_t* msg_end, size_t msg_len, size_t n, const uint32_t* comb, const edk_fixed_ws* ws, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const finish_shape f = finish_shape_of(n);
  const uint32_t count = (uint32_t)set->count;
  const uint32_t* perm = nullptr;                  // ragged messages: both hashing kernels take their items in order of length
  if (const hipError_t e = msg_order(&perm, ws->perm, ws->lenbins, msg_off, msg_end, n, stream); e != hipSuccess) return e;
  static const edk_dom no_dom = {};
  const edk_dom& dom = ws->dom ? *ws->dom : no_dom;
  const auto scalars = ws->dom ? k_sign_keyed_scalars<true> : k_sign_keyed_scalars<false>;
  const auto finish = ws->dom ? k_sign_keyed_finish<true> : k_sign_keyed_finish<false>;
  hipLaunchKernelGGL(scalars, dim3(blocks_of(n)), dim3(BLOCK), 0, stream, ws->aux, set->a, set->prefix, count, key_idx, msgs, msg_off, msg_end,
                     msg_len, n, perm, dom);
  if (const hipError_t e = launch_point(k_sign_dom_point<POINT_SPLIT>, k_sign_dom_point<1>, n, ws, stream, ws->acc, (const uint32_t*)ws->aux, n, comb); e != hipSuccess) return e;
  hipLaunchKernelGGL(finish, dim3(f.grid), dim3(BLOCK), 0, stream, sigs, ws->acc, ws->aux, set->pubs, count, key_idx, msgs, msg_off, msg_end,
                     msg_len, n, f.k, perm, dom);
  return hipGetLastError();
}

hipError_t edk_x25519_base(uint8_t* out, const uint8_t* scalars, size_t n, const uint32_t* comb, const edk_fixed_ws* ws, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const finish_shape f = finish_shape_of(n);
  if (const hipError_t e = launch_point(k_x25519_base_point<POINT_SPLIT>, k_x25519_base_point<1>, n, ws, stream, ws->acc, scalars, n, comb); e != hipSuccess) return e;
  hipLaunchKernelGGL(k_x25519_base_finish, dim3(f.grid), dim3(BLOCK), 0, stream, out, ws->acc, n, f.k);
  return hipGetLastError();
}

hipError_t edk_pk_to_x(uint8_t* out, const uint8_t* in, size_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_pk_to_x, dim3(blocks_of(n)), dim3(BLOCK), 0, stream, out, in, n);
  return hipGetLastError();
}

hipError_t edk_sk_to_x(uint8_t* out, const uint8_t* in, size_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_sk_to_x, dim3(blocks_of(n)), dim3(BLOCK), 0, stream, out, in, n);
  return hipGetLastError();
}

// point classification (edk_classify.h): one class byte per 32-byte string.  Asynchronous on `stream`
hipError_t edk_point_classify(uint8_t* cls, const uint8_t* points, size_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_point_classify, dim3(blocks_of(n)), dim3(BLOCK), 0, stream, cls, points, n);
  return hipGetLastError();
}

// [m]P + [a]B (edk_muladd.h): one pass of at most ws->capacity items through the verify workspace - prepare, the verify pass's own
// main kernel in its own launch shape, finish.  mul / add NULL: every m = 1 / every a = 0.  Asynchronous on `stream`
hipError_t edk_point_muladd(uint8_t* out, const uint8_t* points, const uint8_t* mul, const uint8_t* add, size_t n, const uint32_t* base16,
                            const edk_verify_ws* ws, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (n > ws->capacity) return hipErrorInvalidValue;
  const unsigned blocks = blocks_of(n);
  const finish_shape f = finish_shape_of(n);
  EDK_LAUNCH(k_point_muladd_prepare, dim3(blocks), dim3(BLOCK), 0, stream, points, mul, add, n, ws->digits, ws->table, ws->flags);
  EDK_LAUNCH(k_verify_main, dim3(blocks), dim3(BLOCK), MAIN_LDS_RESERVE, stream, ws->digits, ws->table, base16, ws->acc);
  EDK_LAUNCH(k_point_muladd_finish, dim3(f.grid), dim3(BLOCK), 0, stream, out, ws->acc, ws->flags, n, f.k);
  return hipSuccess;
}

// the front of a scattered pass (edk_scatter.h): the order of length from MSG_ORDER_MIN_N items on, as msg_order builds it from an
// offset table, then one lane per item.  Asynchronous on `stream`
hipError_t edk_scatter_challenge(const uint8_t* data, size_t data_len, const uint32_t* sig_off, const uint32_t* pub_off,
                                 const uint32_t* msg_off, const uint32_t* msg_len, size_t n, const edk_verify_ws* ws, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (n > ws->capacity || !ws->gsigs || (uint64_t)data_len > (uint64_t)UINT32_MAX) return hipErrorInvalidValue;
  const scatter_spans sp = { sig_off, pub_off, msg_off, msg_len, (uint64_t)data_len };
  const unsigned blocks = blocks_of(n);
  const uint32_t* perm = nullptr;
  if (n >= MSG_ORDER_MIN_N) {
    EDK_DO(hipMemsetAsync(ws->lenbins, 0, (size_t)LEN_BINS * sizeof(uint32_t), stream));
    EDK_LAUNCH(k_scatter_len_count, dim3(blocks), dim3(BLOCK), 0, stream, ws->lenbins, sp, n);
    EDK_LAUNCH(k_len_starts, dim3(1), dim3(BLOCK), 0, stream, ws->lenbins);
    EDK_LAUNCH(k_scatter_len_place, dim3(blocks), dim3(BLOCK), 0, stream, ws->perm, ws->lenbins, sp, n);
    perm = ws->perm;
  }
  EDK_LAUNCH(k_scatter_challenge, dim3(blocks), dim3(BLOCK), 0, stream, data, sp, n, ws->gsigs, ws->keybytes, ws->domdig, perm);
  return hipSuccess;
}

int edk_scatter_spans_inside(size_t data_len, const uint32_t* sig_off, const uint32_t* pub_off, const uint32_t* msg_off,
                             const uint32_t* msg_len, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!scatter_item_inside(sig_off[i], pub_off[i], msg_off[i], msg_len[i], (uint64_t)data_len)) return 0;
  return 1;
}

}  // extern "C"
