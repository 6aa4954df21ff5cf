// rlc_keyed.h - the kernels of batch verification over a key set (include/eddsa_amd.h: ed25519_verify_keyed_rlc*), part of
// rlc.hip's translation unit (it uses that file's layout, constants, helpers and the item bodies it shares with the unkeyed
// kernels) and included by nothing else.
//
//   k_rlc_keys            once per pass, one lane per key of the set (at most RLC_G): -A_k as an affine niels point and the key's
//                         routing flag - the square roots of a pass are `count`, not one per item
//   k_rlc_hash_keyed      k_rlc_hash with the key bytes taken by index; leaves them in edk_verify_ws.keybytes like
//                         k_verify_prepare_keyed, where k_verify_policy reads `pubs`; <true>: its digest form
//   k_rlc_points_keyed    -R only; the item's flags are R's OR its key's routing flag
//   k_rlc_scalars_keyed   k_rlc_scalars, but the key term z t mod 8 l is ADDED to the accumulator of (group, key) instead of
//                         recoded per item
//   k_rlc_key_scalars     per (group, key): the accumulator reduced mod 8 l, centred, recoded: the group's 32 -A rows, indexed by key
// and k_rlc_bucket<true> (rlc.hip) whose -A windows index the pass's key points.  What a lane computes is rlc_keyed_lanes.h's.
// An item whose index names no key (key_idx >= count) has flags 0: rejected like a non-canonical R, no term, no digit, and it
// routes its group nowhere; nothing of the key set is read for it.
// The stages hand over at kernel boundaries only; the accumulators are summed by device-scope atomics on 64-bit words, so the
// result does not depend on the order of arrival.
#pragma once
#include "rlc_keyed_lanes.h"

namespace ed {

__global__ void __launch_bounds__(RLC_BLOCK, 2)
k_rlc_keys(const uint8_t* keys, uint32_t count, uint32_t* keypts, uint8_t* keyflags) {
  const uint32_t k = blockIdx.x * RLC_BLOCK + threadIdx.x;
  if (k >= count) return;
  uint32_t w[8];
  ge_niels nl;
  load32(w, keys, k, 32);
  keyflags[k] = rlc_decode_key_lane(nl, w);
  niels_store(keypts + 32 * (size_t)k, nl);
}

// DIGEST (ed25519_verify_keyed_digests_rlc*): k_rlc_hash_digest's t, S and leaf - item i's 64 bytes of SHA-512(R || A || M) lie
// in the message slot of src, nothing but the leaf is hashed, perm is not used - with the key bytes still taken by index and left
// in keybytes.  The leaf is SHA-512(digest || S) in both forms, as in the unkeyed kernels: the seed and the coefficients of a
// keyed pass are those of the unkeyed pass over the expanded keys.  The launcher chooses the instantiation (src.digest).
template <bool DIGEST>
__global__ void __launch_bounds__(RLC_BLOCK, 2)
k_rlc_hash_keyed(edk_verify_items src, size_t n, uint32_t* ts, uint32_t* leaf, const uint32_t* perm, const uint8_t* keys,
                 const uint32_t* key_idx, uint32_t count, uint8_t* keybytes) {
  const size_t g = (size_t)blockIdx.x * RLC_BLOCK + threadIdx.x;
  if (g >= n) return;
  const size_t i = perm ? perm[g] : g;
  uint32_t aw[8];
  const uint32_t k = key_idx[i];
  if (k < count) load32(aw, keys, k, 32); else keyed_no_key(aw);
  store32(keybytes, i, 32, aw);
  if constexpr (DIGEST) rlc_digest_item(src.msgs, src.msg_stride, src.sigs, src.sig_stride, i, ts, leaf);
  else {
    uint32_t rw[8];
    load32(rw, src.sigs, i, src.sig_stride);
    rlc_hash_item(src, i, rw, aw, ts, leaf);
  }
}

template <bool COFACTORED>
__global__ void __launch_bounds__(RLC_BLOCK, 2)
k_rlc_points_keyed(edk_verify_items src, size_t n, const uint32_t* key_idx, uint32_t count, const uint8_t* keyflags,
                   uint32_t* niels_r, uint8_t* flags, uint32_t* gflags) {
  const size_t i = (size_t)blockIdx.x * RLC_BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  ge_niels nl;
  load32(w, src.sigs, i, src.sig_stride);
  uint8_t fl = rlc_decode_r_lane(nl, w);
  niels_store(niels_r + 32 * i, nl);
  const uint32_t k = key_idx[i];
  if (k < count) {
    fl |= keyflags[k];
    if (COFACTORED && (fl & RLC_R_VALID) == 0) fl |= RLC_PER_ITEM;
  } else
    fl = 0;                                      // (no key: no term, and it routes its group nowhere)
  rlc_route(fl, i, flags, gflags);
}

// acc: `groups` x `count` accumulators of RLC_KEY_ACC_WORDS 64-bit words, zeroed on the stream at the start of the pass.  A
// wave whose items all refer to one key - a single signer, or a batch sorted by key - adds its terms up first and sends eight
// atomics instead of 512 to the same eight addresses.
__global__ void __launch_bounds__(RLC_BLOCK, 2)
k_rlc_scalars_keyed(size_t n, const uint32_t* ts, const uint32_t* seed, const uint8_t* flags, const uint32_t* key_idx, uint32_t count,
                    int8_t* dig, uint32_t* bsum, unsigned long long* acc) {
  const size_t i = (size_t)blockIdx.x * RLC_BLOCK + threadIdx.x;
  const size_t g = i / RLC_G;                    // (the grid covers whole groups; a block lies in one)
  uint32_t zs[9], term[8];
#pragma unroll
  for (int k = 0; k < 9; k++) zs[k] = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) term[k] = 0;
  uint32_t key = 0xffffffffu;                    // no term
  {
    int8_t* d = dig + (g * (size_t)RLC_WINDOWS + RLC_WINDOWS_A) * RLC_G + i % RLC_G;
    if (i < n && (flags[i] & RLC_R_VALID)) {     // (an index outside the key set left the flags 0)
      uint32_t tw[8], sw[8], sd[8];
      load8(tw, ts + 16 * i);
      load8(sw, ts + 16 * i + 8);
#pragma unroll
      for (int q = 0; q < 8; q++) sd[q] = seed[q];
      int8_t dr[RLC_WINDOWS_R];
      rlc_keyed_scalars_lane(term, dr, zs, sd, (uint64_t)i, tw, sw);
      key = key_idx[i];
#pragma unroll
      for (int wd = 0; wd < RLC_WINDOWS_R; wd++) d[(size_t)wd * RLC_G] = dr[wd];
    } else {
#pragma unroll
      for (int wd = 0; wd < RLC_WINDOWS_R; wd++) d[(size_t)wd * RLC_G] = 0;
    }
  }
  {
    const bool has = key < count;
    const unsigned long long who = __ballot(has);
    if (who != 0) {
      const uint32_t k0 = (uint32_t)__shfl((int)key, __ffsll((long long)who) - 1);
      if (__all(!has || key == k0)) {
        unsigned long long* a = acc + (g * count + k0) * RLC_KEY_ACC_WORDS;
#pragma unroll
        for (int q = 0; q < 8; q++) {
          unsigned long long v = term[q];        // (0 for a lane without a term)
#pragma unroll
          for (int stride = 32; stride >= 1; stride >>= 1) v += __shfl_xor(v, stride);
          if ((threadIdx.x & 63u) == 0) atomicAdd(a + q, v);
        }
      } else if (has) {
        unsigned long long* a = acc + (g * count + key) * RLC_KEY_ACC_WORDS;
#pragma unroll
        for (int q = 0; q < 8; q++) atomicAdd(a + q, (unsigned long long)term[q]);
      }
    }
  }
  block_sum9(zs, bsum);
}

// One lane per (group, k < RLC_G): the 32 digits of key k's scalar in that group into column k of the group's -A rows; zero
// for k >= count (the rows are whole) and for a key no item of the group refers to.
__global__ void __launch_bounds__(RLC_BLOCK, 2)
k_rlc_key_scalars(size_t groups, uint32_t count, const unsigned long long* acc, int8_t* dig) {
  const size_t j = (size_t)blockIdx.x * RLC_BLOCK + threadIdx.x;
  const size_t g = j / RLC_G, k = j % RLC_G;
  if (g >= groups) return;
  int8_t da[RLC_WINDOWS_A];
#pragma unroll
  for (int wd = 0; wd < RLC_WINDOWS_A; wd++) da[wd] = 0;
  if (k < count) {
    unsigned long long a[RLC_KEY_ACC_WORDS], any = 0;
#pragma unroll
    for (int q = 0; q < RLC_KEY_ACC_WORDS; q++) { a[q] = acc[(g * count + k) * RLC_KEY_ACC_WORDS + q]; any |= a[q]; }
    if (any != 0) {
      uint64_t aw[RLC_KEY_ACC_WORDS];
#pragma unroll
      for (int q = 0; q < RLC_KEY_ACC_WORDS; q++) aw[q] = a[q];
      rlc_key_sum_lane(da, aw);
    }
  }
  int8_t* d = dig + g * (size_t)RLC_WINDOWS * RLC_G + k;
#pragma unroll
  for (int wd = 0; wd < RLC_WINDOWS_A; wd++) d[(size_t)wd * RLC_G] = da[wd];
}

}  // namespace ed
