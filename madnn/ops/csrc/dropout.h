// Dropout masks generated inside the kernels (K8 attention, K3 residual norm, K16 dropout_add): no
// mask tensor exists in memory, every kernel that needs the mask again regenerates it.
//
// One generator for all of them: Philox4x32 with ten rounds (Salmon et al. 2011), key =
// (seed[31:0], seed[63:32] ^ offset[63:32]), counter word 0 = offset[31:0]; the other three counter
// words name a block of 16 elements, the four output words are its 16 mask bytes, and an element is
// kept iff its byte < threshold = floor((1 - p) * 256 + 0.5) (kept values are scaled by rp = 256 /
// threshold, the reciprocal of the realised keep probability).
//  * K8 (attn.hip): counter (c0, b*H + h, q >> 2, k >> 2), the 4 x 4 block of attention probabilities.
//  * hidden dropout of a [rows, H] activation (K3 DROP, K16): counter (c0, row[31:0], row[63:32],
//    col >> 4), the 16 consecutive columns 16 (col >> 4) .. + 15 of one row; column col owns byte
//    col & 3 of word (col >> 2) & 3.  Keep / drop is a pure function of (seed, offset, row, col,
//    threshold): never of H, the launch shape or the lane.
// Host mirrors (bit-identical): madnn.ops.reference.attention_dropout_mask / hidden_dropout_mask.
#pragma once

#include "common.h"

namespace madnn {

typedef unsigned int drop_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kPhiloxRounds = 10;

struct DropRng {
  uint32_t k0, k1, c0;  // Philox key, counter word 0
};

__device__ __forceinline__ DropRng drop_rng(uint64_t seed, uint64_t offset) {
  return DropRng{(uint32_t)seed, (uint32_t)(seed >> 32) ^ (uint32_t)(offset >> 32), (uint32_t)offset};
}

// Philox4x32 on the counter (c0, bh, qb, kb).  K8: the 16 mask bytes of head bh's 4 x 4 block
// (queries 4 qb..4 qb + 3) x (keys 4 kb..4 kb + 3); word = query & 3, byte = key & 3.
__device__ __forceinline__ drop_u32x4 drop_block(const DropRng& g, uint32_t bh, uint32_t qb, uint32_t kb) {
  uint32_t c0 = g.c0, c1 = bh, c2 = qb, c3 = kb, k0 = g.k0, k1 = g.k1;
#pragma unroll
  for (int r = 0; r < kPhiloxRounds; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return drop_u32x4{c0, c1, c2, c3};
}

__device__ __forceinline__ uint32_t drop_byte(uint32_t word, int i) { return (word >> (8 * i)) & 0xffu; }

// ------------------------------------------------------------------ hidden dropout
// Scalars of one hidden-dropout launch; threshold == 0 never reaches a DROP kernel.
struct HiddenDrop {
  uint64_t seed, offset;
  uint32_t threshold;
  float rp;
};

// the 16 mask bytes of columns 16 cb .. 16 cb + 15 of `row`
__device__ __forceinline__ drop_u32x4 hidden_block(const DropRng& g, int64_t row, uint32_t cb) {
  return drop_block(g, (uint32_t)row, (uint32_t)((uint64_t)row >> 32), cb);
}

__device__ __forceinline__ bool hidden_keep(const DropRng& g, int64_t row, int64_t col, uint32_t threshold) {
  const drop_u32x4 w = hidden_block(g, row, (uint32_t)(col >> 4));
  const int wi = (int)(col >> 2) & 3;
  const uint32_t word = wi == 0 ? w[0] : wi == 1 ? w[1] : wi == 2 ? w[2] : w[3];
  return drop_byte(word, (int)col & 3) < threshold;
}

// A lane that owns the 8 consecutive columns col .. col + 7 (col % 8 == 0) of `row`: the two words of
// their block, words 0, 1 for the lower half (odd = 0), 2, 3 for the upper (odd = (col >> 3) & 1).
// The lane uses half of its Philox call; sharing the call across the lane pair that holds the two
// halves (a DPP swap, as K8's quads do) measured no faster in K3 and K16 -- both stay bound by HBM
// (docs/PERF.md "Hidden dropout") -- and was not kept.
__device__ __forceinline__ void hidden_words(const DropRng& g, int64_t row, uint32_t cb, int odd, uint32_t (&w)[2]) {
  const drop_u32x4 b = hidden_block(g, row, cb);
  w[0] = odd ? b[2] : b[0];
  w[1] = odd ? b[3] : b[1];
}

// element j (0..7) of a lane's 8 columns is kept
__device__ __forceinline__ bool hidden_kept(const uint32_t (&w)[2], int j, uint32_t threshold) {
  return drop_byte(w[j >> 2], j & 3) < threshold;
}

}  // namespace madnn
