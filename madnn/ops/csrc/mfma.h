// Shared MFMA-tile helpers for the GEMM-shaped gfx950 kernels (K8 attention, K9 conv1x1, K12, K13).
//
// v_mfma_f32_32x32x16_bf16 operand maps (cdna_hip_programming.md §3): lane l holds
// A[row l&31][k 8(l>>5) .. +7] and B[k 8(l>>5) .. +7][col l&31]; the accumulator holds
// D[row acc_row(r, l>>5)][col l&31] in register r.  LDS tiles are XOR-swizzled so that
// the two read kinds used here are bank-conflict-free:
//   * row reads (ds_read_b128): a [R][64] bf16 tile (128-B rows), lane reads row l&31,
//     16-B chunk 2s + (l>>5) -> swz<64> (ds_read_b128 groups {0-3,12-15,20-27} / {4-11,16-19,28-31}:
//     the 8 even and the 8 odd rows of a group get 8 distinct XOR terms -> 16 distinct 16-B slots);
//   * transposed reads (2 x ds_read_b64_tr_b16, lds_col / lds_col_acc below): a [64][C] tile
//     (C = 64 or 128), lane half h reads 8 of rows 16s .. 16s + 15 of column c0 + (l&31) -> swz<C>
//     (C = 128: the dual-use image (b) of cdna_hip_programming.md T10).
// For the transposed read each 32-lane half touches 4 rows x 4 aligned 16-B chunks per
// instruction; the XOR term gives the 4 rows 4 different chunk groups, i.e. 16 distinct
// 16-B slots = all 64 banks (for 128-B rows, two rows per bank row, and for 256-B rows).
#pragma once

#include "common.h"

namespace madnn {
namespace mf {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x16 mfma(const bf16x8& a, const bf16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

// accumulator register r of lane half h -> row within the 32-row block
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// byte offset of 16-B chunk `ch` of row `row` in a tile with C bf16 per row (C = 64 or 128)
template <int C>
__device__ __forceinline__ int swz(int row, int ch) {
  static_assert(C == 64 || C == 128, "swizzled tiles have 64 or 128 columns");
  if constexpr (C == 64) {
    return row * 128 + 16 * (ch ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3)));
  } else {
    return row * 256 + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
  }
}

// operand fragment with k along the row: 8 bf16 of row `row`, chunk `ch` of a [R][C] tile
template <int C = 64>
__device__ __forceinline__ bf16x8 lds_row(const uint16_t* tile, int row, int ch) {
  return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(tile) + swz<C>(row, ch));
}

// the two ds_read_b64_tr_b16 results of a transposed operand read -> one fragment
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
__device__ __forceinline__ bf16x8 join_tr(const s16x4& lo, const s16x4& hi) {
  const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

// Operand fragment with k down the rows of a [64][C] tile, column c0 + (lane & 31): a 16-lane group
// reads a quad of 4 rows per ds_read_b64_tr_b16, and the fragment is two such quads.  Which 16 rows
// the two lane halves cover, in which order, is the k order of the fragment -- it must be the k order
// of the OTHER operand of the same MFMA:
//                  element j of lane half h = tile[r0 + ...][col]   other operand
//   lds_col      :  8h + j                   (natural order)         lds_row / lds_col fragments
//   lds_col_acc  :  8(j >> 2) + 4h + (j & 3) (= acc_row(j, h))       pack_acc(): registers 8s..8s+7 of
//                                                                    an f32x16 accumulator as bf16
// i.e. quads at rows {8h, 8h + 4} against {4h, 4h + 8}; same columns, same swizzle, same bank behaviour.
template <int C, bool ACC_ORDER>
__device__ __forceinline__ bf16x8 lds_col_any(const uint16_t* tile, int r0, int c0, int lane) {
  constexpr int half = ACC_ORDER ? 4 : 8, quad = ACC_ORDER ? 8 : 4;
  const int g = lane >> 4, i = lane & 15;
  const int col = c0 + 16 * (g & 1) + 4 * (i & 3);
  const int row = r0 + half * (g >> 1) + (i >> 2);
  const char* base = reinterpret_cast<const char*>(tile);
  const int sub = 8 * ((col >> 2) & 1);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + swz<C>(row, col >> 3) + sub));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + swz<C>(row + quad, col >> 3) + sub));
  return join_tr(lo, hi);
}
template <int C>
__device__ __forceinline__ bf16x8 lds_col(const uint16_t* tile, int r0, int c0, int lane) {
  return lds_col_any<C, false>(tile, r0, c0, lane);
}
template <int C>
__device__ __forceinline__ bf16x8 lds_col_acc(const uint16_t* tile, int r0, int c0, int lane) {
  return lds_col_any<C, true>(tile, r0, c0, lane);
}

// registers 8s..8s+7 of an accumulator -> bf16 operand fragment (v_cvt_pk_bf16_f32)
__device__ __forceinline__ bf16x8 pack_acc(const f32x16& x, int s) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = static_cast<__bf16>(x[8 * s + j]);
  return r;
}

__device__ __forceinline__ void store4_bf16(uint16_t* p, float a, float b, float c, float d) {
  *reinterpret_cast<u32x2*>(p) = u32x2{pack_bf16x2(a, b), pack_bf16x2(c, d)};
}

__device__ __forceinline__ float round_bf16(float v) { return bf16_to_f32(f32_to_bf16(v)); }

}  // namespace mf
}  // namespace madnn
