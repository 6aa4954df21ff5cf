// keyed_kernels.h - the kernels of key-set verification (include/eddsa_amd.h: eddsa_amd_keyset, ed25519_verify_keyed*), part of
// kernels.hip's translation unit (it uses that file's BLOCK, wave_append, launch shapes and the item bodies it shares with the
// unkeyed kernels) and included by nothing else.
//
//   k_keyset_build           once per key set, one lane per key: the table 0..8 * (-A) and the on-curve flag (keyed_lanes.h)
//   k_verify_prepare_keyed   k_verify_prepare with the key taken by index: no square root and no table; <true>: its digest form
//   k_dom_challenge_keyed    k_dom_challenge with the key taken by index (ed25519ctx_verify_keyed*, ed25519ph_verify_keyed*)
//   k_keyed_exact_tables     the items that kernel listed for the exact path get a table of their own, as in an unkeyed pass
//   k_verify_halve_keyed     k_verify_halve; an item it hands to the exact path gets a copy of its key's table in its own slot
//   k_verify_main_half_keyed, k_verify_main_keyed   the one-lane evaluations with tab_a = the key's table in the key set
//   k_keyset_comb_build      once per COMB key set, one lane per (key, row): the key's comb, 704 entries m * 4096^row * (-A)
//   k_verify_main_comb_keyed the evaluation of a pass over a comb key set: both scalars through combs, 88 additions and 6 doublings
// Kernels of their own rather than one more template argument of the unkeyed ones: their argument lists differ, and the unkeyed
// instantiations keep the code objects they had (profiles/verify_keyed.txt, section 1).  What a lane computes is lanes.h's,
// unchanged: verify_half_main_lane and verify_main_lane take tab_a as a pointer of its own.
// Everything behind the evaluation - the exact path, k_cofactor_*, k_verify_policy, k_verify_finish - runs unchanged: the
// prepare kernel leaves the item's key bytes in the workspace (edk_verify_ws.keybytes, stride 32), where those kernels read
// `pubs`, and the exact path finds the item's table in the item's own slot.  A pass never writes the key set.
#pragma once
#include "keyed_lanes.h"

namespace ed {

__global__ void __launch_bounds__(BLOCK, 2)
k_keyset_build(uint32_t* keytab, uint8_t* keyflags, const uint8_t* keys, size_t count) {
  const size_t k = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (k >= count) return;
  uint32_t aw[8];
  load32(aw, keys, k, 32);
  keyflags[k] = (uint8_t)keyset_build_lane(keytab + table_slot(k), aw);
}

// src.pubs is not read.  An item whose index names no key (key_idx >= count) is decided HERE: ok = 0, on neither work list, and
// the bytes of keyed_no_key in its key-bytes slot, so that the cofactored equation, which decides every rejected item again from
// those bytes, rejects it too.  The kernel holds no square root and builds no table: see k_keyed_exact_tables.
// DIGEST (ed25519_verify_keyed_digests*, and behind k_dom_challenge_keyed): as in k_verify_prepare, the item's 64 bytes of
// SHA-512(R || A || M) lie in the message slot of src and nothing is hashed; perm is not used (the launcher passes none).  Which
// instantiation runs is the launcher's choice (src.digest), never a lane's; <false> is the kernel it was
// (profiles/verify_keyed_forms.txt, section 1).
template <bool DIGEST>
__global__ void __launch_bounds__(BLOCK, 2)
k_verify_prepare_keyed(edk_verify_items src, size_t n, uint32_t* digits, uint8_t* flags, uint32_t* onlist, uint32_t* offlist,
                       uint32_t* offcount, int offcurve_mode, const uint32_t* perm, const uint8_t* keys, const uint8_t* keyflags,
                       const uint32_t* key_idx, uint32_t count, uint8_t* keybytes, uint8_t* ok) {
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const size_t item = perm ? perm[g < n ? g : n - 1] : (g < n ? g : n - 1);
  const size_t i = g < n ? item : g;             // its slot of the workspace, as in k_verify_prepare
  // everything that needs the key set comes first: nothing of it is held across the hash
  const uint32_t k = key_idx[item];
  const bool known = k < count;                  // nothing of the key set is read for an index outside it
  uint32_t aw[8], sw[8], tw[8];
  if (known) load32(aw, keys, k, 32); else keyed_no_key(aw);
  // (bit 0: the index names a key, bit 1: that key is on the curve - one vector register across the hash, not two lane masks)
  uint32_t kf = known ? 1u | (keyflags[k] != 0 ? 2u : 0u) : 0u;
  asm volatile("" : "+v"(kf));
  store32(keybytes, i, 32, aw);
  if (g < n && !known) ok[i] = 0;
  if constexpr (DIGEST) {
    uint32_t dw[16];
    load32(dw, src.msgs, item, src.msg_stride);
    load32(dw + 8, src.msgs + 32, item, src.msg_stride);
    verify_digest_lane(tw, dw);
  } else {
    uint32_t rw[8];
    const uint8_t* m; size_t mlen;
    load32(rw, src.sigs, item, src.sig_stride);
    msg_span(m, mlen, src.msgs, src.msg_off, src.msg_end, src.msg_len, src.msg_stride, item);
    verify_hash_lane(tw, rw, aw, m, mlen);
  }
  uint32_t* d = digits + digit_slot(i);
  store8(d, tw);
  load32(sw, src.sigs + 32, item, src.sig_stride);
  verify_s_lane(sw);
  store8(d + 8, sw);
  // offcurve_mode (edk_verify_ws.exact_offcurve) 2: every item goes to the exact path
  const bool windowed = (kf & 2u) != 0 && offcurve_mode != 2;
  flags[i] = (uint8_t)(windowed ? VERIFY_WINDOWED : 0);
  const bool live = g < n;
  const bool exact = (kf & 1u) != 0 && !windowed;
  const uint32_t on_slot = wave_append(offcount + EDK_ONLIST_WORD, live && windowed);
  if (live && windowed) onlist[on_slot] = (uint32_t)i;
  const uint32_t off_slot = wave_append(offcount + EDK_OFFLIST_WORD, live && exact);
  if (live && exact) offlist[off_slot] = (uint32_t)i;
}

// k_dom_challenge (kernels.hip) with A taken by index: position g hashes item perm[g] (ragged messages in order of length) or
// item g under the dom2 prefix, and SHA-512(dom2 || R || A || M') goes to the ITEM's 64 bytes of `digests` (ws->domdig), which
// k_verify_prepare_keyed<true> reads behind it.  An index outside the key set hashes the bytes of keyed_no_key - what that
// kernel leaves in the item's key-bytes slot, so the cofactored equation decides the item from the same t - and reads nothing
// of the key set.
__global__ void __launch_bounds__(BLOCK, 2)
k_dom_challenge_keyed(edk_verify_items src, size_t n, uint8_t* digests, const uint32_t* perm, edk_dom dom, const uint8_t* keys,
                      const uint32_t* key_idx, uint32_t count) {
  __shared__ uint32_t lds_dom[EDK_DOM_WORDS];
  stage_dom(lds_dom, dom);
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= n) return;
  const size_t item = perm ? perm[g] : g;
  uint32_t rw[8], aw[8], dig[16];
  const uint8_t* m; size_t mlen;
  const uint32_t k = key_idx[item];
  if (k < count) load32(aw, keys, k, 32); else keyed_no_key(aw);
  load32(rw, src.sigs, item, src.sig_stride);
  msg_span(m, mlen, src.msgs, src.msg_off, src.msg_end, src.msg_len, src.msg_stride, item);
  verify_dom_hash_lane(dig, lds_dom, dom.len, rw, aw, m, mlen);
  store32(digests, item, EDK_DOM_DIGEST_BYTES, dig);
  store32(digests + 32, item, EDK_DOM_DIGEST_BYTES, dig + 8);
}

// The exact path reads - and writes over - the item's OWN table, which k_verify_prepare builds for every item.  In a keyed pass
// only the items k_verify_prepare_keyed listed for that path get one (a key off the curve in mode 1, every item in mode 2), built
// here from the item's key bytes, in front of k_verify_halve_keyed: over the list, not over the pass - the grid is sized for the
// pass, the blocks beyond the list end at once.  A kernel of its own because the table needs the square root's 250 squarings
// under a branch few lanes take: inside the prepare kernel that branch spans 150 KB of code, and the long jump across it cost
// the kernel a scratch slot (68 bytes per lane, of which it stored nothing).  Launched only in a pass that has an exact path.
__global__ void __launch_bounds__(BLOCK, 2)
k_keyed_exact_tables(uint32_t* table, const uint8_t* keybytes, const uint32_t* offlist, const uint32_t* offcount) {
  const size_t slot = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (slot >= (size_t)offcount[EDK_OFFLIST_WORD]) return;
  const size_t i = offlist[slot];
  uint32_t aw[8];
  load32(aw, keybytes, i, 32);
  verify_table_lane(table + table_slot(i), aw);
}

// k_verify_halve over the same list.  The items listed have an index inside the key set (k_verify_prepare_keyed).
template <int BITS>
__global__ void __launch_bounds__(BLOCK, 2)
k_verify_halve_keyed(const uint8_t* sigs, size_t sig_stride, const uint32_t* digits, uint32_t* hdigits, uint32_t* rtable, uint8_t* flags,
                     const uint32_t* onlist, uint32_t* offlist, uint32_t* offcount, uint32_t* table, const uint32_t* keytab,
                     const uint32_t* key_idx) {
  const size_t slot = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (slot >= (size_t)offcount[EDK_ONLIST_WORD]) return;
  const size_t i = onlist[slot];
  const uint8_t fl = flags[i];
  uint32_t tdig[8], sdig[8], hd[HALF_DIGIT_WORDS];
  load8(tdig, digits + digit_slot(i));
  load8(sdig, digits + digit_slot(i) + 8);
  verify_half_scalars_lane<BITS>(hd, tdig, sdig);
  if ((hd[HALF_STATUS_WORD] & HALF_PAIR_REFUSED) != 0) atomicAdd(offcount + EDK_REFUSED_WORD, 1u);
  hdigits_store(hdigits, i, hd);
  uint32_t rw[8];
  load32(rw, sigs, i, sig_stride);
  const bool rvalid = verify_half_point_lane(rtable + table_slot(i), rw);
  const bool mine = (fl & VERIFY_WINDOWED) != 0 && (hd[HALF_STATUS_WORD] & HALF_LONG) == 0;
  flags[i] = (uint8_t)((mine ? VERIFY_WINDOWED : 0) | (rvalid ? VERIFY_R_CANONICAL : 0));
  if ((fl & VERIFY_WINDOWED) != 0 && !mine) {
    // an item without a short pair joins the exact path's list: that path reads the item's own table and writes Q + B and Q - B
    // over entries 2 and 3 of it, so the key's nine entries are copied there first (the stream orders the copy before the reader)
    keyed_table_copy(table + table_slot(i), keytab + table_slot(key_idx[i]));
    offlist[atomicAdd(offcount + EDK_OFFLIST_WORD, 1u)] = (uint32_t)i;
  }
}

// k_verify_main_half with the key's table.  A zero digit reads entry 0 of key 0 - the neutral element whatever key 0 is: the
// item's own slot, and item 0's, may never have been written in a keyed pass.
template <int WINDOWS>
__global__ void __launch_bounds__(MAIN_HALF_BLOCK, MAIN_HALF_BLOCKS_PER_CU)
k_verify_main_half_keyed(uint8_t* ok, const uint32_t* hdigits, const uint32_t* keytab, const uint32_t* key_idx, const uint32_t* rtable,
                         const uint32_t* base16, const uint8_t* flags, const uint32_t* onlist, const uint32_t* offcount) {
  const size_t slot = (size_t)blockIdx.x * MAIN_HALF_BLOCK + threadIdx.x;
  if (slot >= (size_t)offcount[EDK_ONLIST_WORD]) return;
  const size_t i = onlist[slot];
  const uint32_t* hl = stage_digit_words(hdigits + hdigit_slot(i));
  const bool neutral = verify_half_main_lane<false, WINDOWS>(hl, keytab + table_slot(key_idx[i]), rtable + table_slot(i), base16, false,
                                                             MAIN_HALF_BLOCK, keytab);
  half_verdict_store(ok, i, flags[i], neutral, 1);
}

// k_verify_main with the key's table.  Slots past the pass and items whose index names no key walk key 0's table: their result
// is discarded (k_verify_finish skips an item without VERIFY_WINDOWED), and nothing outside the key set is read.
__global__ void __launch_bounds__(BLOCK, 4)
k_verify_main_keyed(const uint32_t* digits, const uint32_t* keytab, const uint32_t* key_idx, uint32_t count, size_t n,
                    const uint32_t* base16, uint32_t* accout) {
  const main_pos p = main_at<true>(key_idx, count, n);
  ge acc;
  verify_main_lane(acc, digits + digit_slot(p.i), keytab + table_slot(p.key), base16);
  acc_put_xyz(acc_column(accout, p.tile, threadIdx.x), acc);
}

// ---- comb key sets (eddsa_amd_keyset_create_comb; keyed_lanes.h) ----

// Once per comb key set, one lane per (key, row): the row's COMB_HALF entries of the key's comb.
__global__ void __launch_bounds__(BLOCK, 2)
k_keyset_comb_build(uint32_t* comb, const uint8_t* keys, size_t count) {
  const size_t id = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  const size_t k = id / COMB_ROWS;
  const int row = (int)(id % COMB_ROWS);
  if (k >= count) return;
  uint32_t aw[8];
  load32(aw, keys, k, 32);
  keyset_comb_row_lane(comb + comb_slot(k) + (size_t)row * COMB_HALF * VERIFY_ENTRY_WORDS, aw, row);
}

// k_verify_main_keyed for a comb key set: the same tile of BLOCK lanes per block and the same result in accout for
// k_verify_finish, from 88 additions and 6 doublings (verify_comb_lane).  bcomb: the engine's comb of the base point in its
// global layout (88 KiB, shared by every lane).  Slots past the pass and items whose index names no key walk key 0's comb.
// Two accumulators and two entries in flight: two blocks per CU; the scalars wait in LDS (18 KiB per block), not in registers.
__global__ void __launch_bounds__(BLOCK, 2)
k_verify_main_comb_keyed(const uint32_t* digits, const uint32_t* keycomb, const uint32_t* keytab, const uint32_t* key_idx, uint32_t count,
                         size_t n, const uint32_t* bcomb, uint32_t* accout) {
  const main_pos p = main_at<true>(key_idx, count, n);
  __shared__ uint32_t comb_words[2 * 9 * BLOCK];   // [t | S][word][lane]: the lane's two scalars plus the comb's offset
  uint32_t* yt = comb_words + threadIdx.x;
  uint32_t* ys = yt + 9 * BLOCK;
  verify_comb_words_lane(yt, ys, BLOCK, digits + digit_slot(p.i));
  ge acc;
  verify_comb_lane(acc, yt, ys, BLOCK, keycomb + comb_slot(p.key), keytab + table_slot(p.key), bcomb);
  acc_put_xyz(acc_column(accout, p.tile, threadIdx.x), acc);
}

}  // namespace ed
