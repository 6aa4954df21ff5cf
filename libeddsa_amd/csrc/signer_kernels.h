// signer_kernels.h - the kernels of signer sets (include/eddsa_amd.h: eddsa_amd_signer, ed25519_sign_keyed*), part of kernels.hip's
// translation unit (it uses that file's BLOCK, stage_dom, aux_store, sign_finish_policy and finish_batch8) and included by nothing else.
//
//   k_signer_build<EXPANDED>   once per signer set, one lane per key: a mod l, the prefix and the encoded A = a B (signer_lanes.h)
//   k_sign_keyed_scalars<DOM>  one lane per position: a and the prefix by key index, r = H([dom2 ||] prefix || M') mod l; a | r go
//                              to the position's slot of aux, the layout k_sign_dom_scalars leaves
//   (R = r B)                  k_sign_dom_point<PARTS> through launch_point, unchanged: it takes r from aux in every shape
//   k_sign_keyed_finish<DOM>   sign_finish_policy<DOM, true>: A taken from the set by index
// Kernels of their own around the bodies of the sign kernels, whose code objects stay what they were.  Against ed25519_sign_batch a
// keyed pass hashes two SHA-512 inputs per item instead of three (no SHA-512(seed)) and reads 4 bytes of index where that reads 64
// bytes of keys.  Nothing here branches on, or addresses memory by, a, a prefix or r: the key index and its range check are public.
// <DOM> selects the hash; the dom2 prefix is an argument of both instantiations (a zeroed one where it is not read), so that
// the two share one argument list.
#pragma once
#include "signer_lanes.h"

namespace ed {

// One lane per key, in the blocks of the point kernels (the comb's image in LDS; comb_select needs every lane of a wave active:
// an idle lane works on the last key and stores nothing).  keys: 32 bytes per key (seeds) or 64 (EXPANDED: scalar | prefix).
template <bool EXPANDED>
__global__ void __launch_bounds__(POINT_BLOCK, 512 / POINT_BLOCK)
k_signer_build(uint32_t* set_a, uint32_t* set_prefix, uint8_t* set_pubs, const uint8_t* keys, size_t count, const uint32_t* comb) {
  __shared__ alignas(16) uint32_t lds_comb[COMB_IMG_WORDS];
  stage_table(lds_comb, comb, COMB_IMG_WORDS);
  const size_t g = (size_t)blockIdx.x * POINT_BLOCK + threadIdx.x;
  const size_t k = g < count ? g : count - 1;
  uint32_t aw[8], pw[8], Aw[8];
  if constexpr (EXPANDED) {
    uint32_t ew[16];
    load32(ew, keys, k, 64);
    load32(ew + 8, keys + 32, k, 64);
    signer_expanded_lane(aw, pw, ew);
  } else {
    uint32_t sk[8];
    load32(sk, keys, k, 32);
    signer_seed_lane(aw, pw, sk);
  }
  if (g < count) {                               // the secrets leave the registers before the comb, as in k_sign_point
    store8(set_a + 8 * k, aw);
    store8(set_prefix + 8 * k, pw);
  }
  signer_pub_lane(Aw, aw, lds_comb);
  if (g < count) store32(set_pubs, k, 32, Aw);
}

// a and r of position g's item into the POSITION's slot of aux, where k_sign_dom_point and k_sign_keyed_finish find them.  An
// item whose index names no key (key_idx >= count) leaves zeros and reads nothing of the set; an idle lane holds no secret.
template <bool DOM>
__global__ void __launch_bounds__(BLOCK, 2)
k_sign_keyed_scalars(uint32_t* aux, const uint32_t* set_a, const uint32_t* set_prefix, uint32_t count, const uint32_t* key_idx,
                     const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* msg_end, size_t msg_len, size_t n, const uint32_t* perm,
                     edk_dom dom) {
  __shared__ uint32_t lds_dom[DOM ? EDK_DOM_WORDS : 1];
  if constexpr (DOM) stage_dom(lds_dom, dom);
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= n) return;
  const size_t item = perm ? perm[g] : g;
  const uint32_t k = key_idx[item];
  uint32_t aw[8] = {0, 0, 0, 0, 0, 0, 0, 0}, rw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (k < count) {                               // (the index is public)
    uint32_t pw[8];
    const uint8_t* m; size_t mlen;
    msg_span(m, mlen, msgs, msg_off, msg_end, msg_len, msg_len, item);
    load8(pw, set_prefix + 8 * (size_t)k);
    sign_keyed_nonce_lane<DOM>(rw, lds_dom, dom.len, pw, m, mlen);
    load8(aw, set_a + 8 * (size_t)k);            // fetched behind the hash: eight registers less across it
  }
  aux_store(aux, g, aw, rw);
}

// sign_finish_policy<DOM, true> (kernels.hip): A = the set's key key_idx[item]; it wipes the position's point beside its a | r, and an
// index outside the set gets 64 zero bytes.
template <bool DOM>
__global__ void __launch_bounds__(BLOCK, 2)
k_sign_keyed_finish(uint8_t* sigs, uint32_t* acc, uint32_t* aux, const uint8_t* set_pubs, uint32_t count, const uint32_t* key_idx,
                    const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* msg_end, size_t msg_len, size_t n, int K, const uint32_t* perm,
                    edk_dom dom) {
  __shared__ uint32_t lds_dom[DOM ? EDK_DOM_WORDS : 1];
  if constexpr (DOM) stage_dom(lds_dom, dom);
  finish_batch8(sign_finish_policy<DOM, true>{{acc, n, K}, sigs, aux, set_pubs, msgs, msg_off, msg_end, msg_len, perm, lds_dom, dom.len,
                                              count, key_idx}, acc);
}

}  // namespace ed
