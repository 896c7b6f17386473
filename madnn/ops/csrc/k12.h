// K12 building blocks shared by the 256x256 LDS-DMA GEMM kernels (gemm.hip: one tile per
// workgroup, K12 / K12W / K12W16; gemmp.hip: persistent, epilogues overlapped with the next tile's
// loads): tile constants, the kernel arguments and the workgroup -> tile decode, the per-lane DMA
// source offsets of the XOR-swizzled LDS images and the fragment reads.  Layout and schedule
// derivation: gemm.hip header.
#pragma once

#include "gelu.h"
#include "mfma.h"

namespace madnn {
namespace k12 {

using namespace mf;

constexpr int kThreads = 512;
constexpr int kT = 256;                  // output tile (both i and j)
constexpr int kBK = 64;
constexpr int kHalf = 128 * kBK;         // bf16 elements of one half-tile (16 KiB)
constexpr int kStage = 4 * kHalf;        // A0 A1 B0 B1
constexpr int kLds = 2 * kStage;         // 128 KiB

struct Args {
  const uint16_t* a;
  const uint16_t* b;
  uint16_t* out;
  const uint16_t* res;  // epilogue: out = y + res (same [j][i] layout, row stride ldr), or null
  const void* bias;     // [I] fp32 (bias_f32) or bf16, or null
  uint16_t* aux;        // pre-activation store (row stride ldx), or null
  int64_t lda, ldb, ldo, ldr, ldx;
  int64_t I, J, K;
  int i_tiles, j_tiles;
  int bias_f32, act;    // act: 0 none, 1 tanh-GELU, 2 erf-GELU
  float* ws;            // split-K: fp32 partial slabs [splits][J][I] (null: bf16 epilogue)
  int splits;           // workgroups per output tile along the reduction
  int64_t kper;         // reduction elements per split (multiple of kBK)
};

// This workgroup's share of an Args problem: XCD-grouped logical id (common.h), i tile fastest, then
// the split; `nk` K tiles from reduction element kbeg.  Returned by value and copied to scalars by the
// kernels: what a lambda captures must not be the argument struct (hipcc spills it to scratch).
// K12W and K12W16 use it; K12's own gemm_kernel keeps the same lines spelled out (gemm.hip says why).
struct Tile {
  int split;
  int64_t i0, j0, kbeg;
  int nk;
};
__device__ __forceinline__ Tile decode_tile(int i_tiles, int j_tiles, int64_t K, int64_t kper) {
  int wid = xcd_group_id(blockIdx.x, gridDim.x);
  const int ntile = i_tiles * j_tiles;
  const int split = wid / ntile;
  wid -= split * ntile;
  const int it = wid % i_tiles, jt = wid / i_tiles;
  const int64_t kbeg = (int64_t)split * kper;
  const int64_t klen = K - kbeg < kper ? K - kbeg : kper;
  return Tile{split, (int64_t)it * kT, (int64_t)jt * kT, kbeg, (int)(klen / kBK)};
}

__device__ __forceinline__ void barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// per-lane source offset (elements) of DMA instruction `inst` (0..15) of a half-tile, relative to
// the half-tile's first row (row mode) / first column at its first k row (col mode)
// Row-tile image for the 16x16x32 reads: slot s of row r holds chunk s ^ (r & 6).  A ds_read_b128
// lane group ({0-3,12-15,20-27}, ... MI355X_MICROARCH.md §LDS) reads rows x+0..15 at chunks c, c^1:
// per row parity the 8 rows get 8 distinct slots (c ^ {0,2,4,6} and c ^ 1 ^ {0,2,4,6}), so the read
// is conflict-free; the swz<64> image (built for the 32x32x16 read, row = lane & 31) is 2-way here
// (measured: SQ_LDS_BANK_CONFLICT 1.6e8 cycles on the forward, 0 on the all-transposed wgrad).
__device__ __forceinline__ int swz16(int row, int ch) { return row * 128 + 16 * (ch ^ (row & 6)); }

template <bool COL>
__device__ __forceinline__ int64_t dma_offset(int inst, int lane, int64_t ld, int64_t first, int64_t lim) {
  if constexpr (!COL) {
    // [128 rows][64 k], 128-B rows: LDS slot s of row r holds chunk s ^ f(r) (swz16 / swz<64>)
    const int r = inst * 8 + (lane >> 3);
    const int ch = (lane & 7) ^ (r & 6);
    int64_t row = first + r;
    row = row < lim ? row : lim - 1;
    return (row - first) * ld + 8 * ch;
  } else {
    // [64 k][128 cols], 256-B rows: slot s of k row r holds chunk s ^ g(r) (swz<128>)
    const int r = inst * 4 + (lane >> 4);
    const int ch = (lane & 15) ^ (((r & 3) << 2) | ((r >> 2) & 3));
    int64_t col = first + 8 * ch;
    col = col + 8 <= lim ? col : lim - 8;
    return (int64_t)r * ld + (col - first);
  }
}

// v_mfma_f32_16x16x32_bf16 operands (cdna_hip_programming.md §3): lane l holds
// A[row l&15][k 8(l>>4) + j] and B[k 8(l>>4) + j][col l&15]; the accumulator holds
// D[row 4(l>>4) + r][col l&15] in register r.  On random data the chip holds a higher clock on
// this shape than on 32x32x16 at equal cycles per FLOP (MI355X_MICROARCH.md, DVFS give-back 7).
__device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// k-step s (32 deep) of the operand whose 16 rows/cols start at x: row tiles [128][64] read by
// ds_read_b128 (row x + l&15, 16-B chunk 4s + l>>4); col tiles [64][128] by two
// ds_read_b64_tr_b16 (a 16-lane group g reads k rows 32s + 8g .. +7 of columns x .. x+15 and
// lane i of the group receives column x + i).  Both reads are bank-conflict-free on the
// swz<64> / swz<128> images (16 distinct 16-B slots per 16 lanes / per half-wave).
template <bool COL>
__device__ __forceinline__ bf16x8 frag16(const uint16_t* tile, int s, int x, int lane) {
  if constexpr (COL) {
    const int g = lane >> 4, i = lane & 15;
    const int col = x + 4 * (i & 3);
    const int row = 32 * s + 8 * g + (i >> 2);
    const char* base = reinterpret_cast<const char*>(tile);
    const int sub = 8 * ((col >> 2) & 1);
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + swz<128>(row, col >> 3) + sub));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + swz<128>(row + 4, col >> 3) + sub));
    return join_tr(lo, hi);
  } else {
    const int row = x + (lane & 15);
    return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(tile) + swz16(row, 4 * s + (lane >> 4)));
  }
}

__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// transposed-pair fragment read from two per-lane LDS byte addresses (row quads lo / hi) + an immediate
template <int IMM>
__device__ __forceinline__ bf16x8 frag_tr(const unsigned (&ad)[2]) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(size_t)(ad[0] + IMM));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(size_t)(ad[1] + IMM));
  return join_tr(lo, hi);
}

}  // namespace k12
}  // namespace madnn
