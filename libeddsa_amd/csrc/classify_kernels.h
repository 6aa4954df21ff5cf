// classify_kernels.h - the kernel of point classification (include/eddsa_amd.h: ed25519_point_classify_batch*, eddsa_amd_keyset_classify),
// part of kernels.hip's translation unit (it uses that file's BLOCK) and included by nothing else.
//
//   k_point_classify   one lane per 32-byte string: decode, the three tests on the encoding, the chain [l]P (classify_lanes.h)
// No workspace, no LDS, no table: the kernel reads its input and writes one byte per item, so it runs without an engine (over a key
// set's own bytes after eddsa_amd_shutdown, for one).  A string that is no curve point leaves its lane idle for the length of the chain;
// the wave ends early only when all 64 of its strings are such.
#pragma once
#include "classify_lanes.h"

namespace ed {

// Two blocks per CU, from the code object's metadata (tools/kernel_metadata.py, profiles/point_classify.txt): the accumulator, P in
// cached form and the temporaries of a doubling want 224 VGPRs, which is two waves per SIMD, without scratch; bounded to three blocks
// (168 registers) the compiler spills 22 of them and to four (128) 64.  Two waves per SIMD is also what the verify main kernels run at.
__global__ void __launch_bounds__(BLOCK, 2)
k_point_classify(uint8_t* cls, const uint8_t* points, size_t n) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8];
  load32(w, points, i, 32);
  cls[i] = (uint8_t)point_classify_lane(w);
}

}  // namespace ed
