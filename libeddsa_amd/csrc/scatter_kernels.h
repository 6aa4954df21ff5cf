// scatter_kernels.h - the kernels of ed25519_verify_scattered (include/eddsa_amd.h), part of kernels.hip's translation unit (it uses
// that file's BLOCK, LEN_BINS, len_bin_of and k_len_starts) and included by nothing else.
//
//   k_scatter_len_count, _place   k_len_count and k_len_place over msg_len[i] (0 for an item outside the buffer) instead of an offset
//                                 table; k_len_starts runs between them as it is
//   k_scatter_challenge           one lane per item: gather the signature and the key, hash R || A || M, or write the item that
//                                 every route rejects
// The pass behind them is a digest pass (kernels.hip: edk_verify with src.digest) over ws->gsigs, ws->keybytes and ws->domdig.
#pragma once
#include "scatter_lanes.h"

namespace ed {

// the four index arrays of a pass and the size of the buffer they point into
struct scatter_spans {
  const uint32_t *sig_off, *pub_off, *msg_off, *msg_len;
  uint64_t data_len;
  ED_DEV uint32_t bin(size_t i) const { return len_bin_of(scatter_item_len(sig_off[i], pub_off[i], msg_off[i], msg_len[i], data_len)); }
};

// k_len_count and k_len_place (kernels.hip) line by line, with the bin taken from the spans.  They are forms of their own and not
// one body shared with those two: shared through a function of the item's bin, k_len_count left the compiler with another
// arrangement of its exec masks, and the kernels of the existing passes stay what they are, instruction for instruction
__global__ void __launch_bounds__(BLOCK) k_scatter_len_count(uint32_t* bins, scatter_spans sp, size_t n) {
  __shared__ uint32_t h[LEN_BINS];
  for (int b = threadIdx.x; b < LEN_BINS; b += BLOCK) h[b] = 0;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i < n) atomicAdd(&h[sp.bin(i)], 1u);
  __syncthreads();
  for (int b = threadIdx.x; b < LEN_BINS; b += BLOCK) if (h[b]) atomicAdd(bins + b, h[b]);
}
__global__ void __launch_bounds__(BLOCK) k_scatter_len_place(uint32_t* perm, uint32_t* bins, scatter_spans sp, size_t n) {
  __shared__ uint32_t h[LEN_BINS], base[LEN_BINS];
  for (int b = threadIdx.x; b < LEN_BINS; b += BLOCK) h[b] = 0;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  uint32_t bin = 0, rank = 0;
  if (i < n) { bin = sp.bin(i); rank = atomicAdd(&h[bin], 1u); }
  __syncthreads();
  for (int b = threadIdx.x; b < LEN_BINS; b += BLOCK) if (h[b]) base[b] = atomicAdd(bins + LEN_BINS + b, h[b]);
  __syncthreads();
  if (i < n) perm[base[bin] + rank] = (uint32_t)i;
}

// position g works on item perm[g] (the items in order of length) or on item g; what it leaves goes to the ITEM's slots.  No LDS;
// two blocks per CU like k_dom_challenge, whose hash it runs without the prefix
__global__ void __launch_bounds__(BLOCK, 2)
k_scatter_challenge(const uint8_t* data, scatter_spans sp, size_t n, uint8_t* gsigs, uint8_t* keybytes, uint8_t* digests, const uint32_t* perm) {
  const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= n) return;
  const size_t item = perm ? perm[g] : g;
  scatter_challenge_lane(reinterpret_cast<uint32_t*>(gsigs + 64 * item), reinterpret_cast<uint32_t*>(keybytes + 32 * item),
                         reinterpret_cast<uint32_t*>(digests + EDK_DOM_DIGEST_BYTES * item), data, sp.data_len, sp.sig_off[item],
                         sp.pub_off[item], sp.msg_off[item], sp.msg_len[item]);
}

}  // namespace ed
