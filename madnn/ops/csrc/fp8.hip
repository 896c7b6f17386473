// K17 -- fp8 GEMM on v_mfma_f32_32x32x64_f8f6f4 for gfx950, and the per-tensor quantiser that feeds it:
// the forward and the data gradient of an opt-in FP8 Linear (ops.linear(fp8=True), madnn.nn.Fp8Linear).
// K17W, the weight gradient of that Linear on the same MFMA (ops.linear(fp8="wgrad")), has its own header below,
// and so have K17X, the MX block-scaled GEMM (ops.linear(fp8="mx")), its one-pass quantiser, and K17XW, the MX
// weight gradient (ops.linear(fp8="mx_wgrad")) with the quantiser's column-blocked mode.
//
// Formats: OCP e4m3fn (activations, weights) and e5m2 (output gradients), bit for bit torch's
// float8_e4m3fn / float8_e5m2.  Scaling is per tensor and current: scale = 2^floor(log2(FMAX / amax)) of the
// tensor being quantised (FMAX 448 / 57344; amax == 0 -> 1; exponent clamped to +-126 so scale and 1 / scale are
// normal fp32).  A power-of-two scale makes x * scale exact in fp32: the cast is the only rounding step and the
// dequantisation is exact.  The scale is formed on the device and stays there ([scale, 1 / scale] fp32): no
// host sync, graph-capturable.
//
// Quantiser (3 launches, no float atomics): partial amax rows, one per workgroup (the max of |bf16| is taken
// on the bit patterns: exact) -> a one-wave finalize that also forms the scale pair -> the cast pass, which
// reads the scale from device memory, casts with v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32 (round to nearest even)
// and writes the fp8 image [R][C] with one 16-B store per lane.  On request the same launch writes the
// transposed image [C][R]: the 64 x 64 fp8 tile goes through LDS and leaves as 16-B stores down the columns.
//
// GEMM: C[M][N] (bf16) = (A[M][K] . B[N][K]^T) inv_a inv_b (+ bias[N]) (+ residual[M][N]), both operands fp8
// with the reduction contiguous ("NT"), each with its own format flag; inv_a / inv_b are device pointers.
//   forward : A = x8 [tokens][in], B = w8 [out][in];   data gradient : A = dy8 [tokens][out], B = w8t [in][out].
// Both operands being k-contiguous is what shapes the kernel: every MFMA operand is 32 consecutive k bytes of
// one row -- two ds_read_b128 of a row-major LDS image -- and there is no transposed read anywhere.
//
// Geometry: 256 x 256 output tile per 512-thread workgroup; 8 waves = 2 (wr: 128-row m half) x 4 (wc: 64-column
// n quarter); a wave owns 128 x 64 of D as 4 x 2 accumulators of 32 x 32 (128 registers).  A K step is 128
// bytes per row = two MFMA k steps of 64: 16 MFMAs per wave and K step.  LDS: 2 stages x (A image [256][128 B]
// + B image [256][128 B]) = 2 x 64 KiB = 128 KiB, one workgroup per CU.
// The MFMA's first operand is the B-matrix (n) fragment and its second the A-matrix (m) fragment, so the
// accumulator rows run along n: register r of lane l holds C[m = l & 31][n = 8 (r >> 2) + 4 (l >> 5) + (r & 3)]
// of its 32 x 32 block, 4 consecutive n per register quad.  cbsz therefore carries B's format, blgp A's.
// Operand layout (CDNA4 ISA, 32x32x64 f8f6f4 with 8-bit formats): lane l holds row l & 31, k bytes
// 32 (l >> 5) .. + 31 of the 64-deep step, in register order.  Both operands are read with the same map, so a
// reduction index meets itself; the exact-integer test (tests/test_fp8_gpu.py) is the proof.
//
// Staging: LDS-DMA (glds16, common.h): wave w streams 8 pieces of 1 KiB (8 rows) per stage -- waves 0..3 the A
// image, waves 4..7 the B image -- and waits for them with a counted vmcnt: the pieces of K tile t + 1 are
// issued before the wait for K tile t (vmcnt(8): 8 younger pieces stay in flight), a barrier publishes the
// tile, and the barrier after the tile's last fragment read (lgkmcnt(0) first) opens its stage for K tile
// t + 2.  The images are lane-linear (a piece lands at base + 16 * lane), so the swizzle is applied to the
// per-lane SOURCE address and to the read address.
// Ragged M, N, K: a piece's lane whose row or 16-B k chunk lies outside the operand reads a 16-B block of
// zeros instead (bounded loads that fill zeros): no second kernel, no out-of-bounds address is ever formed.
// Contract: K % 16 == 0 (whole chunks), N % 8 == 0 (whole 16-B output chunks), 16-B aligned rows.
//
// Swizzle: 16-B slot s of row r holds chunk s ^ f(r), f(r) = 4 * bit1(r) + (r >> 2 & 3) (mfma.h swz<64>).
// A fragment read is two ds_read_b128 with row = l & 31 (+ a multiple of 32) and chunk c, c ^ 1 uniform per
// 32-lane half.  ds_read_b128 serves lane groups {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} (and the same
// +32) per pass; a 128-B row is half a 256-B bank row, so a lane's 16-B slot among the 16 of a bank row is
// 8 * (r & 1) + (c ^ f(r)).  Group one: even rows 0, 2, 12, 14, 20, 22, 24, 26 have f = 0, 4, 3, 7, 1, 5, 2, 6
// and the odd rows r + 1 the same f (bit 0 does not enter f); group two: even rows 4, 6, 8, 10, 16, 18, 28, 30
// have f = 1, 5, 2, 6, 0, 4, 3, 7.  Eight distinct XOR terms on one chunk give eight distinct slots per row
// parity: 16 distinct slots per pass, all 64 banks once -- both reads of the 32-byte fragment are
// conflict-free.
//
// Epilogue: acc * (inv_a * inv_b) in fp32, staged through LDS as fp32 in two 128-row halves ([128][256] fp32 =
// 128 KiB, 16-B chunk ch of row r at slot ch ^ (r & 15): the 16 lanes of a ds_write_b128 pass hold 16
// different r & 15); the row pass adds the bias (fp32) and the residual (bf16 -> fp32) and rounds ONCE to
// bf16, storing 16 B per lane, 512-B runs per row.
#include "abi.h"
#include "mfma.h"

namespace madnn {
namespace fp8 {

using namespace mf;

constexpr int kE5M2 = 1;  // format flag: 0 = e4m3fn, 1 = e5m2 (the MFMA's cbsz / blgp codes)

// ------------------------------------------------------------------------------------------ quantiser
constexpr int kQThreads = 256;
constexpr int kQTile = 64;

// bit pattern of max |x| over a [R][C] bf16 matrix with row stride ldx, one partial per workgroup
__global__ __launch_bounds__(kQThreads) void amax_partial_kernel(const uint16_t* __restrict__ x, int64_t ldx, int64_t R,
                                                                 int C, float* __restrict__ partial) {
  __shared__ unsigned wmax[kQThreads / kWave];
  const int cpr = C >> 3;  // 16-B chunks per row
  const int64_t n = R * cpr;
  unsigned m = 0;  // non-negative floats order as their bit patterns
  for (int64_t i = (int64_t)blockIdx.x * kQThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kQThreads) {
    const int64_t r = i / cpr;
    const int c = (int)(i - r * cpr);
    const u32x4 v = *reinterpret_cast<const u32x4*>(x + r * ldx + 8 * c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned lo = v[e] & 0x7fffu, hi = (v[e] >> 16) & 0x7fffu;
      m = m > lo ? m : lo;
      m = m > hi ? m : hi;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)m, off, kWave);
    m = m > o ? m : o;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kQThreads / kWave; ++w) m = m > wmax[w] ? m : wmax[w];
    partial[blockIdx.x] = __uint_as_float(m << 16);
  }
}

// scales[0] = 2^e, scales[1] = 2^-e with e = floor(log2(FMAX / amax)) clamped to [-126, 126], from the exponent
// and fraction fields of amax (no rounded division): FMAX = 1.75 * 2^(EF - 1), amax = (1 + f) * 2^(E - 127)
// -> e = EF - (E - 126) - (1 + f > 1.75)
template <int FMT>
__global__ __launch_bounds__(kWave) void scale_finalize_kernel(const float* __restrict__ partial, int G,
                                                               float* __restrict__ scales) {
  unsigned m = 0;
  for (int i = threadIdx.x; i < G; i += kWave) {
    const unsigned v = __float_as_uint(partial[i]);
    m = m > v ? m : v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)m, off, kWave);
    m = m > o ? m : o;
  }
  if (threadIdx.x == 0) {
    constexpr int EF = FMT == kE5M2 ? 16 : 9;
    const int E = (int)(m >> 23), frac = (int)(m & 0x7fffffu);
    int e;
    if (m == 0) e = 0;
    else if (E == 0) e = 126;      // subnormal amax: the clamp
    else if (E == 255) e = -126;   // inf / nan
    else e = EF - (E - 126) - (frac > 0x600000 ? 1 : 0);
    e = e > 126 ? 126 : (e < -126 ? -126 : e);
    scales[0] = __uint_as_float((unsigned)(127 + e) << 23);
    scales[1] = __uint_as_float((unsigned)(127 - e) << 23);
  }
}

// four floats -> four fp8 bytes, lowest address first
template <int FMT>
__device__ __forceinline__ unsigned cvt4(float a, float b, float c, float d) {
  int v;
  if constexpr (FMT == kE5M2) {
    v = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false);
    v = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, v, true);
  } else {
    v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
  }
  return (unsigned)v;
}

// One 64 x 64 tile per workgroup: lane (row tid / 4, columns 16 (tid & 3) .. + 15) casts 16 values and stores
// them as one 16-B run of q; with TR the tile is also laid into LDS and lane (column tid & 63, rows
// 16 (tid / 64) .. + 15) gathers 16 bytes down its column into one 16-B run of qt (R % 16 == 0: whole runs).
template <int FMT, bool TR>
__global__ __launch_bounds__(kQThreads) void cast_kernel(const uint16_t* __restrict__ x, int64_t ldx, int64_t R, int C,
                                                         const float* __restrict__ scales, uint8_t* __restrict__ q,
                                                         uint8_t* __restrict__ qt) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kQTile * kQTile];
  const int ctiles = (C + kQTile - 1) / kQTile;
  const int64_t rt = blockIdx.x / ctiles;
  const int ct = (int)(blockIdx.x - rt * ctiles);
  const float s = scales[0];
  const int tid = threadIdx.x, lr = tid >> 2, lc = 16 * (tid & 3);
  const int64_t r = rt * kQTile + lr;
  const int c = ct * kQTile + lc;
  u32x4 o = u32x4{0u, 0u, 0u, 0u};
  if (r < R && c < C) {
    const u32x4 a = *reinterpret_cast<const u32x4*>(x + r * ldx + c);
    const u32x4 b = *reinterpret_cast<const u32x4*>(x + r * ldx + c + 8);
    o[0] = cvt4<FMT>(bf16_lo(a[0]) * s, bf16_hi(a[0]) * s, bf16_lo(a[1]) * s, bf16_hi(a[1]) * s);
    o[1] = cvt4<FMT>(bf16_lo(a[2]) * s, bf16_hi(a[2]) * s, bf16_lo(a[3]) * s, bf16_hi(a[3]) * s);
    o[2] = cvt4<FMT>(bf16_lo(b[0]) * s, bf16_hi(b[0]) * s, bf16_lo(b[1]) * s, bf16_hi(b[1]) * s);
    o[3] = cvt4<FMT>(bf16_lo(b[2]) * s, bf16_hi(b[2]) * s, bf16_lo(b[3]) * s, bf16_hi(b[3]) * s);
    *reinterpret_cast<u32x4*>(q + r * C + c) = o;
  }
  if constexpr (TR) {
    *reinterpret_cast<u32x4*>(tile + lr * kQTile + lc) = o;
    __syncthreads();
    const int tc = tid & 63, tg = tid >> 6;
    const int64_t r0 = rt * kQTile + 16 * tg;
    const int cc = ct * kQTile + tc;
    if (cc < C && r0 < R) {
      u32x4 t;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        unsigned v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) v |= (unsigned)tile[(16 * tg + 4 * w + j) * kQTile + tc] << (8 * j);
        t[w] = v;
      }
      *reinterpret_cast<u32x4*>(qt + (int64_t)cc * R + r0) = t;
    }
  }
}

int quant_rows(int64_t R, int64_t C) {
  // one partial per workgroup; 2 workgroups per CU saturate HBM on a streaming read (16 B per lane and trip)
  return stream_grid(R * (C / 8), kQThreads, 2 * kNumCU);
}

// ------------------------------------------------------------------------------------------------ K17
constexpr int kThreads = 512;
constexpr int kT = 256;                    // output tile (m and n)
constexpr int kBK = 128;                   // K step in bytes = fp8 elements
constexpr int kImage = kT * kBK;           // one operand image: 32 KiB
constexpr int kStage = 2 * kImage;         // A image, B image
constexpr int kLds = 2 * kStage;           // 128 KiB
constexpr int kPieces = 8;                 // LDS-DMA pieces (1 KiB = 8 rows) per wave and stage

typedef int i32x8 __attribute__((ext_vector_type(8)));

// what an out-of-range DMA lane reads instead of the operand
__device__ __attribute__((aligned(16))) unsigned g_zero16[4] = {0u, 0u, 0u, 0u};

struct Args {
  const uint8_t* a;
  const uint8_t* b;
  uint16_t* out;
  const uint16_t* res;   // [M][N] bf16 or null
  const void* bias;      // [N] fp32 (bias_f32) or bf16, or null
  const float* inv_a;
  const float* inv_b;
  int64_t lda, ldb;
  int64_t M, N, K;
  int m_tiles, n_tiles;
  int bias_f32;
};

__device__ __forceinline__ void barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// XOR term of the 128-B-row images (header: Swizzle)
__device__ __forceinline__ int swzf(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }

// the 32 k bytes of k step s (64 deep) that lane half hh holds of row `row`: chunks 4s + 2hh, + 1
__device__ __forceinline__ i32x8 frag(const uint8_t* img, int row, int s, int hh) {
  const int slot = (4 * s + 2 * hh) ^ swzf(row);
  const u32x4 lo = *reinterpret_cast<const u32x4*>(img + row * kBK + 16 * slot);
  const u32x4 hi = *reinterpret_cast<const u32x4*>(img + row * kBK + 16 * (slot ^ 1));
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// FA / FB: format flags of the A (m) and B (n) operand.  The builtin with both scale operands 0 lowers to the
// unscaled v_mfma_f32_32x32x64_f8f6f4 (cbsz: first operand's format, blgp: second's).
template <int FA, int FB>
__device__ __forceinline__ f32x16 mfma8(const i32x8& nfrag, const i32x8& mfrag, const f32x16& c) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(nfrag, mfrag, c, FB, FA, 0, 0, 0, 0);
}

template <int FA, int FB>
__global__ __launch_bounds__(kThreads) void gemm_kernel(const Args p) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[kLds];
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, l32 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  // XCD-grouped logical id (bijective remap), n tile fastest: an XCD's workgroups share A's row panel in L2
  const int wid = xcd_group_id(blockIdx.x, gridDim.x);
  const int nt = wid % p.n_tiles, mt = wid / p.n_tiles;
  const int64_t m0 = (int64_t)mt * kT, n0 = (int64_t)nt * kT;
  const int64_t K = p.K;
  const int nk = (int)((K + kBK - 1) / kBK);

  // DMA sources: waves 0..3 stream the A image, 4..7 the B image; piece e of wave w covers image rows
  // 64 (w & 3) + 8 e .. + 7, lane l of it row + (l >> 3), LDS slot l & 7 = chunk (l & 7) ^ f(row)
  const bool is_a = wave < 4;
  const uint8_t* const op = is_a ? p.a : p.b;
  const int64_t ld = is_a ? p.lda : p.ldb;
  const int64_t x0 = is_a ? m0 : n0, lim = is_a ? p.M : p.N;
  const uint8_t* src[kPieces];  // row start + chunk offset, or null for a row outside the operand
#pragma unroll
  for (int e = 0; e < kPieces; ++e) {
    const int row = 64 * (wave & 3) + 8 * e + (lane >> 3);
    const int kc = 16 * ((lane & 7) ^ swzf(row));
    src[e] = x0 + row < lim ? op + (x0 + row) * ld + kc : nullptr;
  }
  const int kc_even = 16 * ((lane & 7) ^ swzf(lane >> 3)), kc_odd = 16 * ((lane & 7) ^ swzf(8 + (lane >> 3)));
  uint8_t* const dma_dst = smem + (is_a ? 0 : kImage) + (wave & 3) * (kPieces * 1024);

  // K tile t -> stage t & 1; a lane whose row or chunk is outside reads the zero block
  auto stage = [&](int t) {
    const int64_t kb = (int64_t)t * kBK;
#pragma unroll
    for (int e = 0; e < kPieces; ++e) {
      const bool in = src[e] != nullptr && kb + ((e & 1) ? kc_odd : kc_even) < K;
      const void* s = in ? (const void*)(src[e] + kb) : (const void*)g_zero16;
      glds16(s, (lds_void*)(dma_dst + (t & 1) * kStage + e * 1024));
    }
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = zero16();

  stage(0);
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) {
      stage(t + 1);
      wait_vmcnt<kPieces>();  // K tile t's pieces: all but the 8 just issued
    } else {
      wait_vmcnt<0>();
    }
    barrier();
    const uint8_t* sa = smem + (t & 1) * kStage;
    const uint8_t* sb = sa + kImage;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      i32x8 nf[2], mf_[4];
#pragma unroll
      for (int b = 0; b < 2; ++b) nf[b] = frag(sb, wc * 64 + 32 * b + l32, s, hh);
#pragma unroll
      for (int a = 0; a < 4; ++a) mf_[a] = frag(sa, wr * 128 + 32 * a + l32, s, hh);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = mfma8<FA, FB>(nf[b], mf_[a], acc[a][b]);
    }
    wait_lgkmcnt0();  // this stage's last fragment reads, before the barrier that opens it for K tile t + 2
    barrier();
  }

  // ---- epilogue (header): two 128-row halves through LDS as fp32
  const float sc = p.inv_a[0] * p.inv_b[0];
  char* ot = reinterpret_cast<char*>(smem);
  const int c = tid & 31, rr = tid >> 5;
  const int64_t ng = n0 + 8 * c;
  float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (p.bias != nullptr && ng < p.N) {
    // element loads, once per lane: a bias that is a slice of a flat parameter buffer has any alignment
#pragma unroll
    for (int j = 0; j < 8; ++j)
      bv[j] = p.bias_f32 ? static_cast<const float*>(p.bias)[ng + j]
                         : bf16_to_f32(static_cast<const uint16_t*>(p.bias)[ng + j]);
  }
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    if (wr == half) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int ml = 32 * a + l32, ch = wc * 16 + 8 * b + 2 * g + hh;
            const f32x16& v = acc[a][b];
            *reinterpret_cast<f32x4*>(ot + ml * 1024 + 16 * (ch ^ (ml & 15))) =
                f32x4{v[4 * g] * sc, v[4 * g + 1] * sc, v[4 * g + 2] * sc, v[4 * g + 3] * sc};
          }
    }
    __syncthreads();
    if (ng < p.N) {
#pragma unroll 2
      for (int i = 0; i < 8; ++i) {
        const int ml = rr + 16 * i;
        const int64_t mg = m0 + 128 * half + ml;
        if (mg >= p.M) break;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(ot + ml * 1024 + 16 * ((2 * c) ^ (ml & 15)));
        const f32x4 hi = *reinterpret_cast<const f32x4*>(ot + ml * 1024 + 16 * ((2 * c + 1) ^ (ml & 15)));
        float v[8] = {lo[0] + bv[0], lo[1] + bv[1], lo[2] + bv[2], lo[3] + bv[3],
                      hi[0] + bv[4], hi[1] + bv[5], hi[2] + bv[6], hi[3] + bv[7]};
        if (p.res != nullptr) {
          float rv[8];
          load8<kBF16>(p.res, mg * p.N + ng, rv);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] += rv[j];
        }
        store8<kBF16>(p.out, mg * p.N + ng, v);
      }
    }
    __syncthreads();
  }
}

template <int FA, int FB>
hipError_t launch_gemm(const Args& p, int64_t grid, hipStream_t s) {
  hipLaunchKernelGGL((gemm_kernel<FA, FB>), dim3((unsigned)grid), dim3(kThreads), 0, s, p);
  return hipGetLastError();
}

// ----------------------------------------------------------------------------------------------- K17W
// fp8 weight gradient: dW[N][K] (bf16) = (sum_m dy8[m][n] x8[m][k]) inv_g inv_x.  Both operands have the
// reduction index (the token m) STRIDED: they are the row-major images the fp8 Linear already made (x8 in the
// forward, dy8 for the data gradient), so this GEMM costs no quantiser pass and the Linear saves x8, not x.
//
// Geometry (K17's): 256 (n) x 256 (k) output tile per 512-thread workgroup; 8 waves = 2 (wr: 128-row n half) x
// 4 (wc: 64-column k quarter); a wave owns 128 x 64 as 4 x 2 accumulators of 32 x 32.  A reduction step is 128
// tokens = two MFMA steps of 64.  LDS: 2 stages x (dy image [128 tokens][256 B of n] + x image [128][256 B of
// k]) = 2 x 64 KiB = 128 KiB.  Staging is K17's: LDS-DMA pieces of 1 KiB (here 4 token rows of 256 B), 8 per
// wave and stage -- waves 0..3 the dy image, 4..7 the x image -- counted vmcnt(8) waits, the two-barrier ring.
// A DMA lane whose token is past the workgroup's token range, or whose 16-B column chunk is past N (K), reads
// g_zero16: M is any positive number, N and K any multiples of 16, and no out-of-bounds address is formed.
//
// Fragments: the MFMA wants per lane one output row (an n, or a k) and 32 reduction bytes, which sit 256 B
// apart in the image.  ds_read_b64_tr_b8 gathers them: a 16-lane group reads an 8-token x 16-column block --
// lane i of the group ADDRESSES the 8 bytes at token i >> 1, columns 8 (i & 1) .. + 7, and RECEIVES the 8
// tokens of column i.  A fragment is four such reads (tokens 8q .. 8q + 7, q = 0..3, of the lane half's 32);
// lane groups 0 / 1 (2 / 3) take columns 0..15 / 16..31 of the 32-wide block, lane half hh tokens 32 hh .. + 31
// of the 64-deep MFMA step.  Which token lands in which byte of the 32 is the same for both operands (same map,
// same code), so a token meets itself; only the ownership of rows and columns has to be right, and
// tests/test_fp8_wgrad_gpu.py (exact on small integers) is the proof.
// Operand order: the MFMA's first operand is the x (k) fragment and its second the dy (n) fragment, so
// register r of lane l holds dW[n = l & 31][k = 8 (r >> 2) + 4 (l >> 5) + (r & 3)] of its block: the register
// quad runs along k, the contiguous output dimension.  cbsz carries x's format, blgp dy's.
//
// Swizzle: an image row is 256 B = all 64 banks, so unswizzled the 8 token rows of one transposed read would
// land on the same 4 banks (8-way conflict).  16-B slot s of token row r holds chunk s ^ 2 (r & 7), applied to
// the per-lane DMA source column and to the read address.  A 32-lane half of one read touches token rows
// r0 .. r0 + 7 (r0 % 8 == 0) and the chunk pair {c, c + 1}, c even: the slots are {c ^ 2j, (c ^ 2j) + 1} for
// j = 0..7 -- the XOR moves bits 1..3 only, so the eight pairs are the eight distinct aligned pairs of the 16
// slots: 256 B on 64 different banks, conflict-free whether the LDS serves the read 16 or 32 lanes at a time.
// The XOR term depends on the lane only (token row & 7 = (lane & 15) >> 1), so s, q and the stage are
// immediate offsets of one per-lane address per fragment.
//
// Split over tokens: a weight gradient has few tiles and a long reduction, so `splits` workgroups share a
// tile, each reducing a contiguous range of whole 128-token steps.  splits == 1: acc * (inv_g inv_x) through
// LDS as fp32 (K17's staging) and out as 16-B bf16 stores.  splits > 1: the same staging, raw fp32 partial sums
// to slab [split][N][K] in 1-KiB runs; wgrad8_reduce_kernel adds the slabs in split order, scales and rounds
// once.  No float atomics: results are deterministic.
constexpr int kWT = 128;                   // tokens per reduction step
constexpr int kWRow = 256;                 // bytes per image row (the n or k tile)
constexpr int kWImage = kWT * kWRow;       // 32 KiB
constexpr int kWStage = 2 * kWImage;       // dy image, x image
static_assert(2 * kWStage == kLds, "K17W uses K17's LDS budget");

typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) i32x2 lds_i32x2;

struct WArgs {
  const uint8_t* g;      // dy8 [M][N]
  const uint8_t* x;      // x8 [M][K]
  uint16_t* out;         // [N][K] bf16 (splits == 1)
  float* ws;             // [splits][N][K] fp32 (splits > 1)
  const float* inv_g;
  const float* inv_x;
  int64_t ldg, ldx;
  int64_t M, N, K;
  int n_tiles, k_tiles, splits;
  int steps_per;         // 128-token steps per split
};

// lane part of a fragment's read address for the 32 columns from c0 (header: Fragments, Swizzle)
__device__ __forceinline__ int tr_lane_off(int c0, int lane) {
  const int i = lane & 15, r7 = i >> 1;
  const int slot = ((c0 >> 4) + ((lane >> 4) & 1)) ^ (2 * r7);
  return (32 * (lane >> 5) + r7) * kWRow + 16 * slot + 8 * (i & 1);
}

// the 32 tokens of MFMA step s that this lane holds of its column: four ds_read_b64_tr_b8
__device__ __forceinline__ i32x8 frag_tr(const uint8_t* img, int lane_off, int s) {
  const uint8_t* p = img + lane_off + 64 * s * kWRow;
  const i32x2 q0 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(p));
  const i32x2 q1 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(p + 8 * kWRow));
  const i32x2 q2 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(p + 16 * kWRow));
  const i32x2 q3 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(p + 24 * kWRow));
  return i32x8{q0[0], q0[1], q1[0], q1[1], q2[0], q2[1], q3[0], q3[1]};
}

// FG / FX: format flags of dy8 and x8
template <int FG, int FX>
__global__ __launch_bounds__(kThreads) void wgrad_kernel(const WArgs p) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[kLds];
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, l32 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  // XCD-grouped logical id, tile fastest: an XCD's workgroups reduce the same tokens, whose rows they share in L2
  const int wid = xcd_group_id(blockIdx.x, gridDim.x);
  const int tiles = p.n_tiles * p.k_tiles;
  const int split = wid / tiles, tile = wid - split * tiles;
  const int64_t n0 = (int64_t)(tile / p.k_tiles) * kT, k0 = (int64_t)(tile % p.k_tiles) * kT;
  const int64_t mbeg = (int64_t)split * p.steps_per * kWT;
  int64_t mend = mbeg + (int64_t)p.steps_per * kWT;
  mend = mend < p.M ? mend : p.M;
  const int nk = mend > mbeg ? (int)((mend - mbeg + kWT - 1) / kWT) : 0;

  // DMA sources: piece e of wave w covers token rows 32 (w & 3) + 4 e .. + 3 of the step, lane l of it row
  // + (l >> 4), LDS slot l & 15 = chunk (l & 15) ^ 2 (row & 7), row & 7 = 4 (e & 1) + (l >> 4)
  const bool is_g = wave < 4;
  const uint8_t* const op = is_g ? p.g : p.x;
  const int64_t ld = is_g ? p.ldg : p.ldx;
  const int64_t c0 = is_g ? n0 : k0, clim = is_g ? p.N : p.K;
  const int64_t col_even = c0 + 16 * ((lane & 15) ^ (2 * (lane >> 4)));
  const int64_t col_odd = c0 + 16 * ((lane & 15) ^ (2 * (4 + (lane >> 4))));
  const bool ok_even = col_even < clim, ok_odd = col_odd < clim;
  const int row0 = 32 * (wave & 3) + (lane >> 4);
  uint8_t* const dma_dst = smem + (is_g ? 0 : kWImage) + (wave & 3) * (kPieces * 1024);

  // step t -> stage t & 1; a lane whose token or column chunk is outside reads the zero block
  auto stage = [&](int t) {
    const int64_t mb = mbeg + (int64_t)t * kWT + row0;
#pragma unroll
    for (int e = 0; e < kPieces; ++e) {
      const int64_t m = mb + 4 * e;
      const bool in = m < mend && ((e & 1) ? ok_odd : ok_even);
      const void* s = in ? (const void*)(op + m * ld + ((e & 1) ? col_odd : col_even)) : (const void*)g_zero16;
      glds16(s, (lds_void*)(dma_dst + (t & 1) * kWStage + e * 1024));
    }
  };

  int goff[4], xoff[2];
#pragma unroll
  for (int a = 0; a < 4; ++a) goff[a] = tr_lane_off(wr * 128 + 32 * a, lane);
#pragma unroll
  for (int b = 0; b < 2; ++b) xoff[b] = tr_lane_off(wc * 64 + 32 * b, lane);

  f32x16 acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = zero16();

  if (nk > 0) stage(0);
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) {
      stage(t + 1);
      wait_vmcnt<kPieces>();  // step t's pieces: all but the 8 just issued
    } else {
      wait_vmcnt<0>();
    }
    barrier();
    const uint8_t* sg = smem + (t & 1) * kWStage;
    const uint8_t* sx = sg + kWImage;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      i32x8 xf[2], gf[4];
#pragma unroll
      for (int b = 0; b < 2; ++b) xf[b] = frag_tr(sx, xoff[b], s);
#pragma unroll
      for (int a = 0; a < 4; ++a) gf[a] = frag_tr(sg, goff[a], s);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = mfma8<FG, FX>(xf[b], gf[a], acc[a][b]);
    }
    wait_lgkmcnt0();  // this stage's last fragment reads, before the barrier that opens it for step t + 2
    barrier();
  }

  // ---- epilogue (header): two 128-row n halves through LDS as fp32, then rows of 8 k per lane
  const bool slab = p.splits > 1;
  const float sc = slab ? 1.f : p.inv_g[0] * p.inv_x[0];
  char* ot = reinterpret_cast<char*>(smem);
  const int c = tid & 31, rr = tid >> 5;
  const int64_t kg = k0 + 8 * c;
  float* const ws = slab ? p.ws + (int64_t)split * p.N * p.K : nullptr;
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    if (wr == half) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int nl = 32 * a + l32, ch = wc * 16 + 8 * b + 2 * g + hh;
            const f32x16& v = acc[a][b];
            *reinterpret_cast<f32x4*>(ot + nl * 1024 + 16 * (ch ^ (nl & 15))) =
                f32x4{v[4 * g] * sc, v[4 * g + 1] * sc, v[4 * g + 2] * sc, v[4 * g + 3] * sc};
          }
    }
    __syncthreads();
    if (kg < p.K) {
#pragma unroll 2
      for (int i = 0; i < 8; ++i) {
        const int nl = rr + 16 * i;
        const int64_t ng = n0 + 128 * half + nl;
        if (ng >= p.N) break;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(ot + nl * 1024 + 16 * ((2 * c) ^ (nl & 15)));
        const f32x4 hi = *reinterpret_cast<const f32x4*>(ot + nl * 1024 + 16 * ((2 * c + 1) ^ (nl & 15)));
        if (slab) {
          *reinterpret_cast<f32x4*>(ws + ng * p.K + kg) = lo;
          *reinterpret_cast<f32x4*>(ws + ng * p.K + kg + 4) = hi;
        } else {
          const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          store8<kBF16>(p.out, ng * p.K + kg, v);
        }
      }
    }
    __syncthreads();
  }
}

// out[e] = bf16((sum_s ws[s][e]) inv_g inv_x), slabs added in split order; 8 elements per lane, 16-B accesses
__global__ __launch_bounds__(256) void wgrad8_reduce_kernel(const float* __restrict__ ws, uint16_t* __restrict__ out,
                                                            int splits, int64_t n, const float* __restrict__ inv_g,
                                                            const float* __restrict__ inv_x) {
  const float sc = inv_g[0] * inv_x[0];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 8;
  for (int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8; e < n; e += stride) {
    f32x4 lo = *reinterpret_cast<const f32x4*>(ws + e), hi = *reinterpret_cast<const f32x4*>(ws + e + 4);
    for (int q = 1; q < splits; ++q) {
      lo += *reinterpret_cast<const f32x4*>(ws + (int64_t)q * n + e);
      hi += *reinterpret_cast<const f32x4*>(ws + (int64_t)q * n + e + 4);
    }
    const float v[8] = {lo[0] * sc, lo[1] * sc, lo[2] * sc, lo[3] * sc, hi[0] * sc, hi[1] * sc, hi[2] * sc, hi[3] * sc};
    store8<kBF16>(out, e, v);
  }
}

template <int FG, int FX>
hipError_t launch_wgrad(const WArgs& p, hipStream_t s) {
  const int64_t grid = (int64_t)p.n_tiles * p.k_tiles * p.splits;
  hipLaunchKernelGGL((wgrad_kernel<FG, FX>), dim3((unsigned)grid), dim3(kThreads), 0, s, p);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------- MX quantiser, K17X
// OCP MX block scaling: every 32 consecutive elements along the reduction dimension of the GEMM that consumes
// an image share one E8M0 scale byte e (value 2^(e - 127)); the elements are e4m3fn or e5m2.
//   e = clamp(floor(log2 amax_block) + 127 - EMAX, 0, 254), EMAX = 8 (e4m3) / 15 (e5m2); all-zero block: e = 127.
// floor(log2 amax) + 127 is the exponent field E of the block's bf16 amax (the max is taken on the bit patterns,
// as in the per-tensor quantiser), so e = max(E - EMAX, 0): no division, no log; a subnormal amax has E = 0 and
// meets the clamp at 0; a finite bf16 has E <= 254, so e <= 246 and the upper clamp never binds.
// Elements: x * 2^(127 - e).  That factor has the fp32 exponent field 254 - e, in [8, 254] for every e the
// quantiser forms: always a normal fp32 number, and a power of two, so the product is exact in fp32 (|x| <
// 2^(e - 127 + EMAX + 1) keeps it below 2^(EMAX + 1); a bf16 subnormal times 2^127 is a normal fp32).  amax / X
// lies in [2^EMAX, 2^(EMAX + 1)) and FMAX is 1.75 * 2^EMAX, so the product is clamped to +-FMAX explicitly and
// only then cast (v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32, round to nearest even): the result does not depend on
// what the cast does on overflow.  Non-finite inputs: unspecified.
//
// Quantiser: ONE launch, one read of x, no amax pass (a block's scale is a function of that block alone), no
// atomics, no host sync.  A 256-thread workgroup takes a 64 x 64 bf16 tile.  Row image q [R][C] (blocks along
// C): lane (row tid / 4, columns 16 (tid & 3) .. + 15) loads 32 B, the two lanes of a block exchange their amax
// with one DPP shuffle, and each casts and stores 16 B; one lane in four stores the tile's two scale bytes of
// its row as one 16-bit word.  Transposed image qt [C][R] (blocks along R, R % 32 == 0) -- a second quantisation
// with its own scales, not a transpose of q: the data gradient needs W^T blocked along out-features.  The raw
// bf16 tile goes through LDS once (8 KiB; 16-B chunk c of row r at slot c ^ 2 (r >> 4): a wave's 16-bit column
// reads then touch 32 different banks, two lanes per word); lane (column tid / 4, rows 16 (tid & 3) .. + 15)
// gathers its 16 values, the lane pair of a block shuffles the amax, and 16 B leave down the column: 4 lanes
// write 64 contiguous bytes of qt.
//
// Scale layout (what K17X reads): uint8 [rows][ld], k-contiguous, ld % 4 == 0, ld >= 4 ceil(K / 128), base 4-B
// aligned -- so the 4 scale bytes of a row's 128-byte K step are ONE aligned 32-bit word, word t of the row.
// Bytes of a row past K / 32 need not hold anything in particular: K17X replaces them (below).  The quantiser
// writes 127 into the pad bytes its 16-bit stores cover and leaves the rest.
//
// K17X: C[M][N] (bf16) = sum_k (A[m][k] 2^(ea[m][k / 32] - 127)) (B[n][k] 2^(eb[n][k / 32] - 127)) (+ bias)
// (+ residual) on v_mfma_scale_f32_32x32x64_f8f6f4.  Geometry, data ring, swizzle, fragment reads and epilogue
// are K17's (its header above); the epilogue has no scale factor.  New are the k order of a fragment and the
// scale path.
// Which k a register byte is: the hardware's k index of the 32 operand bytes of lane l (row l & 31, half
// h = l >> 5) is 16 h .. + 15 for register bytes 0..15 and 32 + 16 h .. + 15 for bytes 16..31, and the scale of
// hardware k block j (k 32 j .. + 31) of a row is taken from the lane of that row in half j.  K17 need not care
// (both operands use one map, any bijection of k gives the same sum); here a block must meet its scale, so
// frag_mx reads 16-B chunks 4 s + h and 4 s + 2 + h of the row for MFMA s (K17: 4 s + 2 h and the next) -- still
// two ds_read_b128 with a chunk index that is uniform per 32-lane half, so K17's bank argument holds unchanged.
// tests/test_mx_gpu.py::test_scale_routing_exact (independent scales per row and block) is the proof.
// Scale path: lane (row, half h) supplies the scale of block h of the MFMA's 64 k in a VGPR; op_sel picks the
// byte.  MFMA s (0, 1) of a K step needs byte 2 s + h of the row's scale word.  op_sel is an immediate, so each
// word is permuted once per K step
// (v_perm_b32 with a per-lane selector) to hold byte (l >> 5) in byte 0 and byte 2 + (l >> 5) in byte 3, and the
// two MFMAs select bytes 0 and 3 (op_sel 0 and op_sel + op_sel_hi both set).
// The words travel through the same ring as the data: LDS holds 2 more KiB per stage (A words [256], B words
// [256]), wave w streams ONE extra piece per stage with glds4 -- lane l the word of row 64 (w & 3) + l of its
// image -- issued after its 8 data pieces.  Chosen over per-lane global loads because those would sit in the
// MFMA loop as 6 dependent VMEM loads per step that hipcc counts in vmcnt and would drain together with the
// uncounted DMA; through the ring they cost 6 conflict-free ds_read_b32 (32 consecutive words, both lane halves
// the same address).  Counted wait: a wave now has 9 loads per stage in flight, so K tile t is complete at
// vmcnt(9) after the 9 of K tile t + 1 were issued (loads retire in order); the RAW / WAR argument is K17's
// unchanged -- the barrier after the wait publishes stage t & 1 (data and words), lgkmcnt(0) + barrier after the
// last fragment and word read opens it for K tile t + 2 -- because the words live and die with their stage.
// Ragged shapes: any M, N % 8 == 0, K % 32 == 0 (K need not be a multiple of 128).  Data lanes outside the
// operand read the zero block as in K17.  A scale lane whose row is outside reads g_one_word (four bytes of 127)
// and never forms an address past the last row; inside, word t < ceil(K / 128) is within the row by the layout
// contract.  Bytes of the last word at or past K / 32 are replaced by 127 with one v_bfi per word (a uniform
// mask): a zero fragment times 2^(255 - 127) would be NaN, so no pad byte, next row or foreign byte reaches a
// result.
constexpr int kXScale = 2 * kT * 4;        // scale words of one stage: A [256], B [256]
constexpr int kXLds = kLds + 2 * kXScale;  // 132 KiB of the CU's 160

__device__ unsigned g_one_word = 0x7f7f7f7fu;  // what an out-of-range scale lane reads: 2^0 four times

// E8M0 byte of a block from the bit pattern of its bf16 amax (sign bit clear)
template <int FMT>
__device__ __forceinline__ unsigned mx_scale_byte(unsigned amax_bits) {
  constexpr int EMAX = FMT == kE5M2 ? 15 : 8;
  const int e = (int)(amax_bits >> 7) - EMAX;
  return amax_bits == 0 ? 127u : (unsigned)(e < 0 ? 0 : e);
}

__device__ __forceinline__ unsigned amax_word(unsigned m, unsigned w) {
  const unsigned lo = w & 0x7fffu, hi = (w >> 16) & 0x7fffu;
  m = m > lo ? m : lo;
  return m > hi ? m : hi;
}

template <int FMT>
__device__ __forceinline__ float mx_fit(float x, float f) {
  constexpr float FMAX = FMT == kE5M2 ? 57344.f : 448.f;
  return fminf(fmaxf(x * f, -FMAX), FMAX);
}

// four bf16 in two words -> four fp8 bytes of a block with factor f = 2^(127 - e)
template <int FMT>
__device__ __forceinline__ unsigned mx_cvt4(unsigned a, unsigned b, float f) {
  return cvt4<FMT>(mx_fit<FMT>(bf16_lo(a), f), mx_fit<FMT>(bf16_hi(a), f), mx_fit<FMT>(bf16_lo(b), f),
                   mx_fit<FMT>(bf16_hi(b), f));
}

template <int FMT, bool TR>
__global__ __launch_bounds__(kQThreads) void mx_quant_kernel(const uint16_t* __restrict__ x, int64_t ldx, int64_t R,
                                                             int C, uint8_t* __restrict__ q, uint8_t* __restrict__ e,
                                                             int64_t lde, uint8_t* __restrict__ qt,
                                                             uint8_t* __restrict__ et, int64_t ldet) {
  __shared__ __attribute__((aligned(16))) uint16_t tile[kQTile * kQTile];
  const int ctiles = (C + kQTile - 1) / kQTile;
  const int64_t rt = blockIdx.x / ctiles;
  const int ct = (int)(blockIdx.x - rt * ctiles);
  const int tid = threadIdx.x, lr = tid >> 2, lq = tid & 3;
  const int64_t r = rt * kQTile + lr;
  const int c = ct * kQTile + 16 * lq;
  const bool in = r < R && c < C;  // C % 32 == 0: a block is inside or outside as a whole
  u32x4 a = u32x4{0u, 0u, 0u, 0u}, b = a;
  if (in) {
    a = *reinterpret_cast<const u32x4*>(x + r * ldx + c);
    b = *reinterpret_cast<const u32x4*>(x + r * ldx + c + 8);
  }
  unsigned m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) m = amax_word(amax_word(m, a[i]), b[i]);
  const unsigned mo = (unsigned)__shfl_xor((int)m, 1, kWave);  // the block's other half
  const unsigned eb = mx_scale_byte<FMT>(m > mo ? m : mo);
  const unsigned eb2 = (unsigned)__shfl_xor((int)eb, 2, kWave);  // the row's other block of this tile
  if (in) {
    const float f = __uint_as_float((254u - eb) << 23);
    *reinterpret_cast<u32x4*>(q + r * C + c) = u32x4{mx_cvt4<FMT>(a[0], a[1], f), mx_cvt4<FMT>(a[2], a[3], f),
                                                     mx_cvt4<FMT>(b[0], b[1], f), mx_cvt4<FMT>(b[2], b[3], f)};
    // a block outside C has amax 0: its byte (127) lands in the row's padding, which lde covers
    if (lq == 0) *reinterpret_cast<uint16_t*>(e + r * lde + 2 * ct) = (uint16_t)(eb | (eb2 << 8));
  }
  if constexpr (TR) {
    u32x4* const trow = reinterpret_cast<u32x4*>(tile + lr * kQTile);
    const int fw = 2 * (lr >> 4);
    trow[(2 * lq) ^ fw] = a;
    trow[(2 * lq + 1) ^ fw] = b;
    __syncthreads();
    const int tc = tid >> 2, tg = tid & 3;
    const int64_t r0 = rt * kQTile + 16 * tg;
    const int cc = ct * kQTile + tc;
    const uint16_t* const col = tile + 16 * tg * kQTile + 8 * ((tc >> 3) ^ (2 * tg)) + (tc & 7);
    unsigned w[8];  // rows 2 j, 2 j + 1 of the lane's 16 as a bf16 pair
    unsigned mt = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      w[j] = (unsigned)col[2 * j * kQTile] | ((unsigned)col[(2 * j + 1) * kQTile] << 16);
      mt = amax_word(mt, w[j]);
    }
    const unsigned mto = (unsigned)__shfl_xor((int)mt, 1, kWave);
    const unsigned ebt = mx_scale_byte<FMT>(mt > mto ? mt : mto);
    const unsigned ebt2 = (unsigned)__shfl_xor((int)ebt, 2, kWave);
    if (cc < C && r0 < R) {  // R % 32 == 0: whole blocks
      const float f = __uint_as_float((254u - ebt) << 23);
      *reinterpret_cast<u32x4*>(qt + (int64_t)cc * R + r0) = u32x4{
          mx_cvt4<FMT>(w[0], w[1], f), mx_cvt4<FMT>(w[2], w[3], f), mx_cvt4<FMT>(w[4], w[5], f), mx_cvt4<FMT>(w[6], w[7], f)};
      if (tg == 0) *reinterpret_cast<uint16_t*>(et + (int64_t)cc * ldet + 2 * rt) = (uint16_t)(ebt | (ebt2 << 8));
    }
  }
}

struct XArgs {
  const uint8_t* a;
  const uint8_t* b;
  const uint8_t* ea;     // scale bytes [M][ldea] (header: Scale layout)
  const uint8_t* eb;     // [N][ldeb]
  uint16_t* out;
  const uint16_t* res;   // [M][N] bf16 or null
  const void* bias;      // [N] fp32 (bias_f32) or bf16, or null
  int64_t lda, ldb, ldea, ldeb;
  int64_t M, N, K;
  int m_tiles, n_tiles;
  int bias_f32;
};

// the 32 operand bytes of MFMA step s that lane half hh holds of row `row`: chunks 4s + hh and 4s + 2 + hh (header)
__device__ __forceinline__ i32x8 frag_mx(const uint8_t* img, int row, int s, int hh) {
  const int f = swzf(row);
  const u32x4 lo = *reinterpret_cast<const u32x4*>(img + row * kBK + 16 * ((4 * s + hh) ^ f));
  const u32x4 hi = *reinterpret_cast<const u32x4*>(img + row * kBK + 16 * ((4 * s + 2 + hh) ^ f));
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// OP: which byte of the lane's scale registers both operands use (0 or 3, header)
template <int FA, int FB, int OP>
__device__ __forceinline__ f32x16 mfmax(const i32x8& nfrag, const i32x8& mfrag, const f32x16& c, unsigned en,
                                        unsigned em) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(nfrag, mfrag, c, FB, FA, OP, (int)en, OP, (int)em);
}

template <int FA, int FB>
__global__ __launch_bounds__(kThreads) void mx_gemm_kernel(const XArgs p) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[kXLds];
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, l32 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  const int wid = xcd_group_id(blockIdx.x, gridDim.x);
  const int nt = wid % p.n_tiles, mt = wid / p.n_tiles;
  const int64_t m0 = (int64_t)mt * kT, n0 = (int64_t)nt * kT;
  const int64_t K = p.K;
  const int nk = (int)((K + kBK - 1) / kBK);
  const int kblocks = (int)(K >> 5);

  // DMA sources as K17: waves 0..3 stream the A image and A's scale words, 4..7 B's
  const bool is_a = wave < 4;
  const uint8_t* const op = is_a ? p.a : p.b;
  const int64_t ld = is_a ? p.lda : p.ldb;
  const int64_t x0 = is_a ? m0 : n0, lim = is_a ? p.M : p.N;
  const uint8_t* src[kPieces];
#pragma unroll
  for (int e = 0; e < kPieces; ++e) {
    const int row = 64 * (wave & 3) + 8 * e + (lane >> 3);
    const int kc = 16 * ((lane & 7) ^ swzf(row));
    src[e] = x0 + row < lim ? op + (x0 + row) * ld + kc : nullptr;
  }
  const int kc_even = 16 * ((lane & 7) ^ swzf(lane >> 3)), kc_odd = 16 * ((lane & 7) ^ swzf(8 + (lane >> 3)));
  uint8_t* const dma_dst = smem + (is_a ? 0 : kImage) + (wave & 3) * (kPieces * 1024);
  // scale piece: lane l the words of row 64 (wave & 3) + l, or the constant word for a row outside
  const int64_t erow = x0 + 64 * (wave & 3) + lane;
  const uint8_t* const esrc = erow < lim ? (is_a ? p.ea + erow * p.ldea : p.eb + erow * p.ldeb) : nullptr;
  uint8_t* const edst = smem + kLds + (is_a ? 0 : kT * 4) + (wave & 3) * 256;

  auto stage = [&](int t) {
    const int64_t kb = (int64_t)t * kBK;
#pragma unroll
    for (int e = 0; e < kPieces; ++e) {
      const bool in = src[e] != nullptr && kb + ((e & 1) ? kc_odd : kc_even) < K;
      const void* s = in ? (const void*)(src[e] + kb) : (const void*)g_zero16;
      glds16(s, (lds_void*)(dma_dst + (t & 1) * kStage + e * 1024));
    }
    const void* s = esrc != nullptr ? (const void*)(esrc + 4 * t) : (const void*)&g_one_word;
    glds4(s, (lds_void*)(edst + (t & 1) * kXScale));
  };

  // per-lane v_perm selector: byte 0 <- byte hh, byte 3 <- byte 2 + hh, bytes 1 and 2 <- 0 (header)
  const unsigned sel = (unsigned)hh | 0x000c0c00u | ((unsigned)(2 + hh) << 24);

  f32x16 acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = zero16();

  stage(0);
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) {
      stage(t + 1);
      wait_vmcnt<kPieces + 1>();  // K tile t's pieces: all but the 9 just issued
    } else {
      wait_vmcnt<0>();
    }
    barrier();
    const uint8_t* sa = smem + (t & 1) * kStage;
    const uint8_t* sb = sa + kImage;
    const unsigned* se = reinterpret_cast<const unsigned*>(smem + kLds + (t & 1) * kXScale);
    // bytes of this step's words that are scales of the operand; the others become 127
    const int nb = kblocks - 4 * t;
    const unsigned msk = nb >= 4 ? 0xffffffffu : (1u << (8 * nb)) - 1u;
    auto word = [&](int row) {
      const unsigned w = (se[row] & msk) | (0x7f7f7f7fu & ~msk);
      return __builtin_amdgcn_perm(w, w, sel);
    };
    unsigned en[2], em[4];
#pragma unroll
    for (int b = 0; b < 2; ++b) en[b] = word(kT + wc * 64 + 32 * b + l32);
#pragma unroll
    for (int a = 0; a < 4; ++a) em[a] = word(wr * 128 + 32 * a + l32);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      i32x8 nf[2], mf_[4];
#pragma unroll
      for (int b = 0; b < 2; ++b) nf[b] = frag_mx(sb, wc * 64 + 32 * b + l32, s, hh);
#pragma unroll
      for (int a = 0; a < 4; ++a) mf_[a] = frag_mx(sa, wr * 128 + 32 * a + l32, s, hh);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          acc[a][b] = s == 0 ? mfmax<FA, FB, 0>(nf[b], mf_[a], acc[a][b], en[b], em[a])
                             : mfmax<FA, FB, 3>(nf[b], mf_[a], acc[a][b], en[b], em[a]);
    }
    wait_lgkmcnt0();  // this stage's last fragment and word reads, before the barrier that opens it for K tile t + 2
    barrier();
  }

  // ---- epilogue: K17's, without a scale factor
  char* ot = reinterpret_cast<char*>(smem);
  const int c = tid & 31, rr = tid >> 5;
  const int64_t ng = n0 + 8 * c;
  float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (p.bias != nullptr && ng < p.N) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      bv[j] = p.bias_f32 ? static_cast<const float*>(p.bias)[ng + j]
                         : bf16_to_f32(static_cast<const uint16_t*>(p.bias)[ng + j]);
  }
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    if (wr == half) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int ml = 32 * a + l32, ch = wc * 16 + 8 * b + 2 * g + hh;
            const f32x16& v = acc[a][b];
            *reinterpret_cast<f32x4*>(ot + ml * 1024 + 16 * (ch ^ (ml & 15))) =
                f32x4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
          }
    }
    __syncthreads();
    if (ng < p.N) {
#pragma unroll 2
      for (int i = 0; i < 8; ++i) {
        const int ml = rr + 16 * i;
        const int64_t mg = m0 + 128 * half + ml;
        if (mg >= p.M) break;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(ot + ml * 1024 + 16 * ((2 * c) ^ (ml & 15)));
        const f32x4 hi = *reinterpret_cast<const f32x4*>(ot + ml * 1024 + 16 * ((2 * c + 1) ^ (ml & 15)));
        float v[8] = {lo[0] + bv[0], lo[1] + bv[1], lo[2] + bv[2], lo[3] + bv[3],
                      hi[0] + bv[4], hi[1] + bv[5], hi[2] + bv[6], hi[3] + bv[7]};
        if (p.res != nullptr) {
          float rv[8];
          load8<kBF16>(p.res, mg * p.N + ng, rv);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] += rv[j];
        }
        store8<kBF16>(p.out, mg * p.N + ng, v);
      }
    }
    __syncthreads();
  }
}

template <int FA, int FB>
hipError_t launch_mx_gemm(const XArgs& p, int64_t grid, hipStream_t s) {
  hipLaunchKernelGGL((mx_gemm_kernel<FA, FB>), dim3((unsigned)grid), dim3(kThreads), 0, s, p);
  return hipGetLastError();
}

template <int FMT>
hipError_t launch_mx_quant(const uint16_t* x, int64_t ldx, int64_t R, int C, uint8_t* q, uint8_t* e, int64_t lde,
                           uint8_t* qt, uint8_t* et, int64_t ldet, unsigned tiles, hipStream_t s) {
  if (qt != nullptr)
    hipLaunchKernelGGL((mx_quant_kernel<FMT, true>), dim3(tiles), dim3(kQThreads), 0, s, x, ldx, R, C, q, e, lde, qt, et, ldet);
  else
    hipLaunchKernelGGL((mx_quant_kernel<FMT, false>), dim3(tiles), dim3(kQThreads), 0, s, x, ldx, R, C, q, e, lde, qt, et, ldet);
  return hipGetLastError();
}

// ------------------------------------------------------------------ MX column-blocked quantiser, K17XW
// The weight gradient dW[n][k] = sum_m dy[m][n] x[m][k] reduces over the token m, so MX wants x and dy blocked
// along m: 32 tokens of ONE column share a scale byte.  mx_quant_cols_kernel writes, from the one read of its
// 64 x 64 tile, the row image (q, e: mx_quant_kernel's code, bit for bit) and the column-blocked image
//   qc [R][C] fp8, row-major as q;   ec [ceil(R / 32)][ldec] uint8, byte [B][c]: rows 32 B .. 32 B + 31 of column c.
// qc is a second quantisation with its own scales (same formula: mx_scale_byte of the block's bit-pattern amax,
// factor 2^(127 - e), explicit clamp, cast), not a copy of q.  R is any positive number: rows at or past R enter
// a block's amax as zeros and are not stored, the last block may be partial.  ldec % 4 == 0, ldec >= C, base 4-B
// aligned.
// Column amax -- chosen: shuffles plus a small LDS exchange (not the TR path's tile read by columns, which hands
// a lane a column, so the stores would run down columns; here a lane keeps its 16-B row run and the qc store is
// the q store).  A lane's 16 values are 8 words of two bit patterns; the maximum over the 16 rows of a wave is
// taken on the packed words (v_pk_max_u16, sign bits cleared) with xor-shuffles over the row lanes (offsets 4, 8,
// 16, 32), 8 words x 4 steps.  A 32-row block is two waves (rows 16 w .. + 15 are wave w): lanes 0..3 of each wave
// write its 64 column maxima (128 B) to LDS as two 16-B stores, and after one barrier every lane reads the partner
// wave's 32 B for its columns.  Banks: the four writing lanes cover 32 consecutive words; a wave's read is 4
// distinct 32-B runs of one 128-B row (the 16 lanes of a run read the same words: a broadcast), so neither
// conflicts.  Each of the 16 columns then has its own factor; 16 B of qc leave per lane, and the lanes of rows 0
// and 32 of the tile store their 16 scale bytes as four aligned words.
//
// K17XW: dW[N][K] (bf16) = sum_m (dy8[m][n] 2^(eg[m / 32][n] - 127)) (x8[m][k] 2^(ex[m / 32][k] - 127)) on
// v_mfma_scale_f32_32x32x64_f8f6f4, both operands row-major and token-strided with column-blocked scales (above).
// K17W's, unchanged: the 256 x 256 tile and 8 waves as 2 x 4, the 128-token step as two [128][256 B] images per
// stage and 2 stages, the 1-KiB DMA pieces with the s ^ 2 (token & 7) slot swizzle, ds_read_b64_tr_b8 fragments
// with x as the first operand (cbsz: x's format, blgp: dy's), the split over whole 128-token steps
// (madnn_fp8_wgrad_splits), the fp32 slabs added in split order, the two-half LDS epilogue.  No scale factor in
// the epilogue or the reduce.
// Block meets scale: the hardware takes the scale of k block j (k 32 j .. + 31 of the 64-deep MFMA) from the lane
// of that row in half j, and a lane of half h holds hardware k 16 h .. + 15 in register bytes 0..15 and
// 32 + 16 h .. + 15 in bytes 16..31 (K17X's header).  K17W gives half h tokens 32 h .. + 31, where a token only has
// to meet itself; here the four transposed reads of a fragment fetch tokens 16 h + 8 q .. + 7 (q = 0, 1: the MFMA
// step's first 32-token block) and 32 + 16 h + 8 (q - 2) .. + 7 (q = 2, 3: its second) -- tr_lane_off_mx /
// frag_tr_mx.  Inside a block every token of a column has the same scale, so the byte order inside one read does
// not matter as long as both operands share it (same code).  Bank argument: the eight token rows of one read are
// still r0 .. r0 + 7 with r0 % 8 == 0 (16 h, 8, 32 and 40 are multiples of 8), so the XOR term is still
// 2 ((lane & 15) >> 1) and K17W's argument holds unchanged; s, q and the stage stay immediate offsets.
// Scales ride the data ring (K17X): a 128-token step needs 4 block rows x 256 columns per operand = 1 KiB, ONE
// glds4 piece per wave and stage, issued after its 8 data pieces -- waves 0..3 dy's scales, 4..7 x's; wave w & 3
// takes block w & 3 of the step, lane l the word of columns 4 (l ^ 8 (w & 1)) .. + 3 of the tile.  LDS: 2 x 64 KiB
// + 2 x 2 KiB = kXLds.  Counted wait vmcnt(9); the RAW / WAR argument is K17X's (the bytes live and die with
// their stage).  MFMA s of a step: lane (column c, half h) supplies byte [2 s + h][c] of its operand's scale
// image with op_sel 0 -- one ds_read_u8 per accumulator row / column block, six per MFMA step and wave (4 dy,
// 2 x).  Conflicts: the 32 lanes of a half read 32 consecutive bytes = 8 words, four lanes a word (broadcast);
// the other half reads the next block row, 256 B = 64 banks further, i.e. the SAME banks -- hence the XOR 8 on the
// word index of odd block rows (applied to the DMA source column and as c ^ 32 h to the read), which puts it on
// the other 8 words of the aligned 16-word group: 16 different banks per read.
// Ragged: M any positive number, N and K multiples of 16.  Data lanes outside read g_zero16 as in K17W.  A scale
// lane whose token block is at or past ceil(M / 32), or whose column word is at or past N / K, reads g_one_word;
// no address past the tensors is formed.  The quantiser never writes 255, so zero data never meets a NaN scale.
// tests/test_mx_wgrad_gpu.py::test_scale_routing_exact (independent scales per token block and column) is the proof.
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

template <int FMT>
__global__ __launch_bounds__(kQThreads) void mx_quant_cols_kernel(const uint16_t* __restrict__ x, int64_t ldx, int64_t R,
                                                                  int C, uint8_t* __restrict__ q, uint8_t* __restrict__ e,
                                                                  int64_t lde, uint8_t* __restrict__ qc,
                                                                  uint8_t* __restrict__ ec, int64_t ldec) {
  __shared__ __attribute__((aligned(16))) unsigned cmax[kQThreads / kWave][kQTile / 2];
  const int ctiles = (C + kQTile - 1) / kQTile;
  const int64_t rt = blockIdx.x / ctiles;
  const int ct = (int)(blockIdx.x - rt * ctiles);
  const int tid = threadIdx.x, lr = tid >> 2, lq = tid & 3, wv = tid >> 6;
  const int64_t r = rt * kQTile + lr;
  const int c = ct * kQTile + 16 * lq;
  const bool in = r < R && c < C;
  u32x4 a = u32x4{0u, 0u, 0u, 0u}, b = a;
  if (in) {
    a = *reinterpret_cast<const u32x4*>(x + r * ldx + c);
    b = *reinterpret_cast<const u32x4*>(x + r * ldx + c + 8);
  }
  // ---- row image: mx_quant_kernel's
  unsigned m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) m = amax_word(amax_word(m, a[i]), b[i]);
  const unsigned mo = (unsigned)__shfl_xor((int)m, 1, kWave);
  const unsigned eb = mx_scale_byte<FMT>(m > mo ? m : mo);
  const unsigned eb2 = (unsigned)__shfl_xor((int)eb, 2, kWave);
  if (in) {
    const float f = __uint_as_float((254u - eb) << 23);
    *reinterpret_cast<u32x4*>(q + r * C + c) = u32x4{mx_cvt4<FMT>(a[0], a[1], f), mx_cvt4<FMT>(a[2], a[3], f),
                                                     mx_cvt4<FMT>(b[0], b[1], f), mx_cvt4<FMT>(b[2], b[3], f)};
    if (lq == 0) *reinterpret_cast<uint16_t*>(e + r * lde + 2 * ct) = (uint16_t)(eb | (eb2 << 8));
  }
  // ---- column image (header): amax of the wave's 16 rows per column, then the partner wave's
  unsigned w[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    w[i] = a[i] & 0x7fff7fffu;
    w[4 + i] = b[i] & 0x7fff7fffu;
  }
#pragma unroll
  for (int off = 4; off < kWave; off <<= 1)
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = pk_max_u16(w[i], (unsigned)__shfl_xor((int)w[i], off, kWave));
  if ((tid & 60) == 0) {
    *reinterpret_cast<u32x4*>(&cmax[wv][8 * lq]) = u32x4{w[0], w[1], w[2], w[3]};
    *reinterpret_cast<u32x4*>(&cmax[wv][8 * lq + 4]) = u32x4{w[4], w[5], w[6], w[7]};
  }
  __syncthreads();
  const u32x4 o0 = *reinterpret_cast<const u32x4*>(&cmax[wv ^ 1][8 * lq]);
  const u32x4 o1 = *reinterpret_cast<const u32x4*>(&cmax[wv ^ 1][8 * lq + 4]);
  u32x4 oq, oe;
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // output word j: columns 4 j .. 4 j + 3 = source words 2 j, 2 j + 1
    const unsigned m0 = pk_max_u16(w[2 * j], j < 2 ? o0[2 * j] : o1[2 * j - 4]);
    const unsigned m1 = pk_max_u16(w[2 * j + 1], j < 2 ? o0[2 * j + 1] : o1[2 * j - 3]);
    const unsigned e0 = mx_scale_byte<FMT>(m0 & 0xffffu), e1 = mx_scale_byte<FMT>(m0 >> 16);
    const unsigned e2 = mx_scale_byte<FMT>(m1 & 0xffffu), e3 = mx_scale_byte<FMT>(m1 >> 16);
    const unsigned s0 = j < 2 ? a[2 * j] : b[2 * j - 4], s1 = j < 2 ? a[2 * j + 1] : b[2 * j - 3];
    oq[j] = cvt4<FMT>(mx_fit<FMT>(bf16_lo(s0), __uint_as_float((254u - e0) << 23)),
                      mx_fit<FMT>(bf16_hi(s0), __uint_as_float((254u - e1) << 23)),
                      mx_fit<FMT>(bf16_lo(s1), __uint_as_float((254u - e2) << 23)),
                      mx_fit<FMT>(bf16_hi(s1), __uint_as_float((254u - e3) << 23)));
    oe[j] = e0 | (e1 << 8) | (e2 << 16) | (e3 << 24);
  }
  if (in) {
    *reinterpret_cast<u32x4*>(qc + r * C + c) = oq;
    if ((lr & 31) == 0) {  // the block's first row is inside, so the block exists; ldec % 4 == 0: aligned words
      unsigned* const ep = reinterpret_cast<unsigned*>(ec + (2 * rt + (lr >> 5)) * ldec + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) ep[j] = oe[j];
    }
  }
}

template <int FMT>
hipError_t launch_mx_quant_cols(const uint16_t* x, int64_t ldx, int64_t R, int C, uint8_t* q, uint8_t* e, int64_t lde,
                                uint8_t* qc, uint8_t* ec, int64_t ldec, unsigned tiles, hipStream_t s) {
  hipLaunchKernelGGL((mx_quant_cols_kernel<FMT>), dim3(tiles), dim3(kQThreads), 0, s, x, ldx, R, C, q, e, lde, qc, ec, ldec);
  return hipGetLastError();
}

constexpr int kXWScale = 2 * 4 * kWRow;    // scale bytes of one stage: dy [4 blocks][256], x [4][256]
static_assert(kLds + 2 * kXWScale == kXLds, "K17XW uses K17X's LDS budget");

struct XWArgs {
  const uint8_t* g;      // dy8 [M][N]
  const uint8_t* x;      // x8 [M][K]
  const uint8_t* eg;     // [ceil(M / 32)][ldeg]
  const uint8_t* ex;     // [ceil(M / 32)][ldex]
  uint16_t* out;         // [N][K] bf16 (splits == 1)
  float* ws;             // [splits][N][K] fp32 (splits > 1)
  int64_t ldg, ldx, ldeg, ldex;
  int64_t M, N, K;
  int n_tiles, k_tiles, splits;
  int steps_per;         // 128-token steps per split
};

// lane part of a fragment's read address for the 32 columns from c0: K17W's with half hh at tokens 16 hh (header)
__device__ __forceinline__ int tr_lane_off_mx(int c0, int lane) {
  const int i = lane & 15, r7 = i >> 1;
  const int slot = ((c0 >> 4) + ((lane >> 4) & 1)) ^ (2 * r7);
  return (16 * (lane >> 5) + r7) * kWRow + 16 * slot + 8 * (i & 1);
}

// tokens 16 hh .. + 15 and 32 + 16 hh .. + 15 of MFMA step s for this lane's column: four ds_read_b64_tr_b8
__device__ __forceinline__ i32x8 frag_tr_mx(const uint8_t* img, int lane_off, int s) {
  const uint8_t* p = img + lane_off + 64 * s * kWRow;
  const i32x2 q0 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(p));
  const i32x2 q1 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(p + 8 * kWRow));
  const i32x2 q2 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(p + 32 * kWRow));
  const i32x2 q3 = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)(p + 40 * kWRow));
  return i32x8{q0[0], q0[1], q1[0], q1[1], q2[0], q2[1], q3[0], q3[1]};
}

// FG / FX: format flags of dy8 and x8
template <int FG, int FX>
__global__ __launch_bounds__(kThreads) void mx_wgrad_kernel(const XWArgs p) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[kXLds];
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5, l32 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;

  const int wid = xcd_group_id(blockIdx.x, gridDim.x);
  const int tiles = p.n_tiles * p.k_tiles;
  const int split = wid / tiles, tile = wid - split * tiles;
  const int64_t n0 = (int64_t)(tile / p.k_tiles) * kT, k0 = (int64_t)(tile % p.k_tiles) * kT;
  const int64_t mbeg = (int64_t)split * p.steps_per * kWT;
  int64_t mend = mbeg + (int64_t)p.steps_per * kWT;
  mend = mend < p.M ? mend : p.M;
  const int nk = mend > mbeg ? (int)((mend - mbeg + kWT - 1) / kWT) : 0;

  // data DMA sources: K17W's
  const bool is_g = wave < 4;
  const uint8_t* const op = is_g ? p.g : p.x;
  const int64_t ld = is_g ? p.ldg : p.ldx;
  const int64_t c0 = is_g ? n0 : k0, clim = is_g ? p.N : p.K;
  const int64_t col_even = c0 + 16 * ((lane & 15) ^ (2 * (lane >> 4)));
  const int64_t col_odd = c0 + 16 * ((lane & 15) ^ (2 * (4 + (lane >> 4))));
  const bool ok_even = col_even < clim, ok_odd = col_odd < clim;
  const int row0 = 32 * (wave & 3) + (lane >> 4);
  uint8_t* const dma_dst = smem + (is_g ? 0 : kWImage) + (wave & 3) * (kPieces * 1024);
  // scale piece: block wave & 3 of the step, lane l the word of tile columns 4 (l ^ 8 (wave & 1)) .. + 3 (header)
  const uint8_t* const eop = is_g ? p.eg : p.ex;
  const int64_t lde = is_g ? p.ldeg : p.ldex;
  const int64_t ecol = c0 + 4 * (lane ^ (8 * (wave & 1)));
  const bool eok = ecol < clim;  // N, K % 16 == 0: a word is inside or outside as a whole
  const int64_t blocks = (p.M + 31) >> 5;
  uint8_t* const edst = smem + kLds + (is_g ? 0 : 4 * kWRow) + (wave & 3) * kWRow;

  auto stage = [&](int t) {
    const int64_t mb = mbeg + (int64_t)t * kWT + row0;
#pragma unroll
    for (int e = 0; e < kPieces; ++e) {
      const int64_t m = mb + 4 * e;
      const bool in = m < mend && ((e & 1) ? ok_odd : ok_even);
      const void* s = in ? (const void*)(op + m * ld + ((e & 1) ? col_odd : col_even)) : (const void*)g_zero16;
      glds16(s, (lds_void*)(dma_dst + (t & 1) * kWStage + e * 1024));
    }
    const int64_t blk = ((mbeg + (int64_t)t * kWT) >> 5) + (wave & 3);
    const void* s = eok && blk < blocks ? (const void*)(eop + blk * lde + ecol) : (const void*)&g_one_word;
    glds4(s, (lds_void*)(edst + (t & 1) * kXWScale));
  };

  int goff[4], xoff[2];
#pragma unroll
  for (int a = 0; a < 4; ++a) goff[a] = tr_lane_off_mx(wr * 128 + 32 * a, lane);
#pragma unroll
  for (int b = 0; b < 2; ++b) xoff[b] = tr_lane_off_mx(wc * 64 + 32 * b, lane);
  // byte [2 s + hh][column ^ 32 hh] of a scale image: + 512 s; column block a (b) is 32 (a ^ hh) bytes along, so an
  // even and an odd block's offset per operand, + 64 for blocks 2 and 3
  const int egoff[2] = {hh * kWRow + wr * 128 + l32 + 32 * hh, hh * kWRow + wr * 128 + l32 + 32 * (1 - hh)};
  const int exoff[2] = {(4 + hh) * kWRow + wc * 64 + l32 + 32 * hh, (4 + hh) * kWRow + wc * 64 + l32 + 32 * (1 - hh)};

  f32x16 acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = zero16();

  if (nk > 0) stage(0);
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) {
      stage(t + 1);
      wait_vmcnt<kPieces + 1>();  // step t's pieces: all but the 9 just issued
    } else {
      wait_vmcnt<0>();
    }
    barrier();
    const uint8_t* sg = smem + (t & 1) * kWStage;
    const uint8_t* sx = sg + kWImage;
    const uint8_t* se = smem + kLds + (t & 1) * kXWScale;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      i32x8 xf[2], gf[4];
      unsigned ex[2], eg[4];
#pragma unroll
      for (int b = 0; b < 2; ++b) ex[b] = se[exoff[b] + 2 * kWRow * s];
#pragma unroll
      for (int a = 0; a < 4; ++a) eg[a] = se[egoff[a & 1] + 2 * kWRow * s + 64 * (a >> 1)];
#pragma unroll
      for (int b = 0; b < 2; ++b) xf[b] = frag_tr_mx(sx, xoff[b], s);
#pragma unroll
      for (int a = 0; a < 4; ++a) gf[a] = frag_tr_mx(sg, goff[a], s);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = mfmax<FG, FX, 0>(xf[b], gf[a], acc[a][b], ex[b], eg[a]);
    }
    wait_lgkmcnt0();  // this stage's last fragment and scale reads, before the barrier that opens it for step t + 2
    barrier();
  }

  // ---- epilogue: K17W's, without a scale factor
  const bool slab = p.splits > 1;
  char* ot = reinterpret_cast<char*>(smem);
  const int c = tid & 31, rr = tid >> 5;
  const int64_t kg = k0 + 8 * c;
  float* const ws = slab ? p.ws + (int64_t)split * p.N * p.K : nullptr;
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    if (wr == half) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int nl = 32 * a + l32, ch = wc * 16 + 8 * b + 2 * g + hh;
            const f32x16& v = acc[a][b];
            *reinterpret_cast<f32x4*>(ot + nl * 1024 + 16 * (ch ^ (nl & 15))) =
                f32x4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
          }
    }
    __syncthreads();
    if (kg < p.K) {
#pragma unroll 2
      for (int i = 0; i < 8; ++i) {
        const int nl = rr + 16 * i;
        const int64_t ng = n0 + 128 * half + nl;
        if (ng >= p.N) break;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(ot + nl * 1024 + 16 * ((2 * c) ^ (nl & 15)));
        const f32x4 hi = *reinterpret_cast<const f32x4*>(ot + nl * 1024 + 16 * ((2 * c + 1) ^ (nl & 15)));
        if (slab) {
          *reinterpret_cast<f32x4*>(ws + ng * p.K + kg) = lo;
          *reinterpret_cast<f32x4*>(ws + ng * p.K + kg + 4) = hi;
        } else {
          const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          store8<kBF16>(p.out, ng * p.K + kg, v);
        }
      }
    }
    __syncthreads();
  }
}

// out[e] = bf16(sum_s ws[s][e]), slabs added in split order (wgrad8_reduce_kernel without its scale pair)
__global__ __launch_bounds__(256) void mx_wgrad_reduce_kernel(const float* __restrict__ ws, uint16_t* __restrict__ out,
                                                              int splits, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 8;
  for (int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8; e < n; e += stride) {
    f32x4 lo = *reinterpret_cast<const f32x4*>(ws + e), hi = *reinterpret_cast<const f32x4*>(ws + e + 4);
    for (int q = 1; q < splits; ++q) {
      lo += *reinterpret_cast<const f32x4*>(ws + (int64_t)q * n + e);
      hi += *reinterpret_cast<const f32x4*>(ws + (int64_t)q * n + e + 4);
    }
    const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    store8<kBF16>(out, e, v);
  }
}

template <int FG, int FX>
hipError_t launch_mx_wgrad(const XWArgs& p, hipStream_t s) {
  const int64_t grid = (int64_t)p.n_tiles * p.k_tiles * p.splits;
  hipLaunchKernelGGL((mx_wgrad_kernel<FG, FX>), dim3((unsigned)grid), dim3(kThreads), 0, s, p);
  return hipGetLastError();
}

}  // namespace fp8
}  // namespace madnn

using namespace madnn;

extern "C" int madnn_fp8_quant_rows(int64_t R, int64_t C) {
  return fp8::quant_rows(R, C);
}

extern "C" hipError_t madnn_fp8_quant(const void* x, int64_t ldx, int64_t R, int64_t C, int fmt, void* q, void* qt,
                                      float* partial, float* scales, hipStream_t stream) {
  if (R <= 0 || C <= 0 || C % 16 || ldx % 8 || ldx < C || C > 0x7fffffff || (fmt != 0 && fmt != 1))
    return hipErrorInvalidValue;
  if (qt != nullptr && R % 16) return hipErrorInvalidValue;
  const int64_t tiles = ((R + fp8::kQTile - 1) / fp8::kQTile) * ((C + fp8::kQTile - 1) / fp8::kQTile);
  if (tiles > 0x7fffffff) return hipErrorInvalidValue;
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  const int G = fp8::quant_rows(R, C);
  hipLaunchKernelGGL(fp8::amax_partial_kernel, dim3(G), dim3(fp8::kQThreads), 0, stream, xp, ldx, R, (int)C, partial);
  uint8_t* qp = static_cast<uint8_t*>(q);
  uint8_t* qtp = static_cast<uint8_t*>(qt);
  const dim3 grid((unsigned)tiles), block(fp8::kQThreads);
  if (fmt == fp8::kE5M2) {
    hipLaunchKernelGGL(fp8::scale_finalize_kernel<1>, dim3(1), dim3(kWave), 0, stream, partial, G, scales);
    if (qt != nullptr) hipLaunchKernelGGL((fp8::cast_kernel<1, true>), grid, block, 0, stream, xp, ldx, R, (int)C, scales, qp, qtp);
    else hipLaunchKernelGGL((fp8::cast_kernel<1, false>), grid, block, 0, stream, xp, ldx, R, (int)C, scales, qp, qtp);
  } else {
    hipLaunchKernelGGL(fp8::scale_finalize_kernel<0>, dim3(1), dim3(kWave), 0, stream, partial, G, scales);
    if (qt != nullptr) hipLaunchKernelGGL((fp8::cast_kernel<0, true>), grid, block, 0, stream, xp, ldx, R, (int)C, scales, qp, qtp);
    else hipLaunchKernelGGL((fp8::cast_kernel<0, false>), grid, block, 0, stream, xp, ldx, R, (int)C, scales, qp, qtp);
  }
  return hipGetLastError();
}

extern "C" hipError_t madnn_fp8_gemm(const void* a, int fmt_a, const void* b, int fmt_b, const float* inv_a,
                                     const float* inv_b, const void* bias, int bias_f32, const void* res, void* out,
                                     int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, hipStream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 16 || N % 8 || lda % 16 || ldb % 16 || lda < K || ldb < K)
    return hipErrorInvalidValue;
  if ((fmt_a != 0 && fmt_a != 1) || (fmt_b != 0 && fmt_b != 1)) return hipErrorInvalidValue;
  fp8::Args p;
  p.a = static_cast<const uint8_t*>(a);
  p.b = static_cast<const uint8_t*>(b);
  p.out = static_cast<uint16_t*>(out);
  p.res = static_cast<const uint16_t*>(res);
  p.bias = bias;
  p.inv_a = inv_a;
  p.inv_b = inv_b;
  p.lda = lda;
  p.ldb = ldb;
  p.M = M;
  p.N = N;
  p.K = K;
  p.m_tiles = (int)((M + fp8::kT - 1) / fp8::kT);
  p.n_tiles = (int)((N + fp8::kT - 1) / fp8::kT);
  p.bias_f32 = bias_f32;
  const int64_t grid = (int64_t)p.m_tiles * p.n_tiles;
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  if (fmt_a == 0) return fmt_b == 0 ? fp8::launch_gemm<0, 0>(p, grid, stream) : fp8::launch_gemm<0, 1>(p, grid, stream);
  return fmt_b == 0 ? fp8::launch_gemm<1, 0>(p, grid, stream) : fp8::launch_gemm<1, 1>(p, grid, stream);
}

extern "C" hipError_t madnn_mx_quant(const void* x, int64_t ldx, int64_t R, int64_t C, int fmt, void* q, void* e,
                                     int64_t lde, void* qt, void* et, int64_t ldet, hipStream_t stream) {
  if (R <= 0 || C <= 0 || C % 32 || ldx % 8 || ldx < C || C > 0x7fffffff || (fmt != 0 && fmt != 1))
    return hipErrorInvalidValue;
  if (x == nullptr || q == nullptr || e == nullptr || lde % 4 || lde < 4 * ((C + 127) / 128)) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(qt)) % 16 ||
      (reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(et)) % 4)
    return hipErrorInvalidValue;
  if (qt != nullptr && (R % 32 || et == nullptr || ldet % 4 || ldet < 4 * ((R + 127) / 128))) return hipErrorInvalidValue;
  const int64_t tiles = ((R + fp8::kQTile - 1) / fp8::kQTile) * ((C + fp8::kQTile - 1) / fp8::kQTile);
  if (tiles > 0x7fffffff) return hipErrorInvalidValue;
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  uint8_t* qp = static_cast<uint8_t*>(q);
  uint8_t* ep = static_cast<uint8_t*>(e);
  uint8_t* qtp = static_cast<uint8_t*>(qt);
  uint8_t* etp = static_cast<uint8_t*>(et);
  if (fmt == fp8::kE5M2)
    return fp8::launch_mx_quant<1>(xp, ldx, R, (int)C, qp, ep, lde, qtp, etp, ldet, (unsigned)tiles, stream);
  return fp8::launch_mx_quant<0>(xp, ldx, R, (int)C, qp, ep, lde, qtp, etp, ldet, (unsigned)tiles, stream);
}

extern "C" hipError_t madnn_mx_gemm(const void* a, int fmt_a, const void* ea, int64_t ldea, const void* b, int fmt_b,
                                    const void* eb, int64_t ldeb, const void* bias, int bias_f32, const void* res,
                                    void* out, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                                    hipStream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 32 || N % 8 || lda % 16 || ldb % 16 || lda < K || ldb < K)
    return hipErrorInvalidValue;
  if ((fmt_a != 0 && fmt_a != 1) || (fmt_b != 0 && fmt_b != 1)) return hipErrorInvalidValue;
  const int64_t ldmin = 4 * ((K + fp8::kBK - 1) / fp8::kBK);  // whole scale words per row
  if (ea == nullptr || eb == nullptr || ldea % 4 || ldeb % 4 || ldea < ldmin || ldeb < ldmin ||
      (reinterpret_cast<uintptr_t>(ea) | reinterpret_cast<uintptr_t>(eb)) % 4)
    return hipErrorInvalidValue;
  fp8::XArgs p;
  p.a = static_cast<const uint8_t*>(a);
  p.b = static_cast<const uint8_t*>(b);
  p.ea = static_cast<const uint8_t*>(ea);
  p.eb = static_cast<const uint8_t*>(eb);
  p.out = static_cast<uint16_t*>(out);
  p.res = static_cast<const uint16_t*>(res);
  p.bias = bias;
  p.lda = lda;
  p.ldb = ldb;
  p.ldea = ldea;
  p.ldeb = ldeb;
  p.M = M;
  p.N = N;
  p.K = K;
  p.m_tiles = (int)((M + fp8::kT - 1) / fp8::kT);
  p.n_tiles = (int)((N + fp8::kT - 1) / fp8::kT);
  p.bias_f32 = bias_f32;
  const int64_t grid = (int64_t)p.m_tiles * p.n_tiles;
  if (grid > 0x7fffffff) return hipErrorInvalidValue;
  if (fmt_a == 0) return fmt_b == 0 ? fp8::launch_mx_gemm<0, 0>(p, grid, stream) : fp8::launch_mx_gemm<0, 1>(p, grid, stream);
  return fmt_b == 0 ? fp8::launch_mx_gemm<1, 0>(p, grid, stream) : fp8::launch_mx_gemm<1, 1>(p, grid, stream);
}

// Workgroups per output tile for K17W: 256 CUs, one 128-KiB-LDS workgroup per CU.  Model, as madnn_wgrad_splits:
// rounds of 256 workgroups x 128-token steps per split + the fp32 slab round trip (splits x N x K x 8 B);
// a split keeps >= 4 steps.  The constants are UNMEASURED estimates: 1.8 us per 256^2 x 128 step (twice the
// bf16 MFMA rate, ~2.4 PF/s) and ~5 TB/s for the slabs (bench/fp8_linear_ab.py records what they give).
extern "C" int madnn_fp8_wgrad_splits(int64_t M, int64_t N, int64_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 1;
  const int64_t tiles = ((N + fp8::kT - 1) / fp8::kT) * ((K + fp8::kT - 1) / fp8::kT);
  const int64_t steps = (M + fp8::kWT - 1) / fp8::kWT;
  int best = 1;
  double best_t = 1e30;
  for (int sp = 1; sp <= 256; ++sp) {
    if (sp > 1 && steps / sp < 4) break;
    const int64_t per = (steps + sp - 1) / sp;
    const int64_t rounds = (tiles * sp + kNumCU - 1) / kNumCU;
    const double t = rounds * per * 1.8 + (sp > 1 ? sp * (double)N * K * 8.0 / 5.0e6 : 0.0);
    if (t < best_t * 0.98) {
      best_t = t;
      best = sp;
    }
  }
  return best;
}

extern "C" hipError_t madnn_fp8_wgrad(const void* dy8, int fmt_g, const void* x8, int fmt_x, const float* inv_g,
                                      const float* inv_x, void* dw, float* ws, int splits, int64_t M, int64_t N,
                                      int64_t K, int64_t ldg, int64_t ldx, hipStream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || N % 16 || K % 16 || ldg % 16 || ldx % 16 || ldg < N || ldx < K)
    return hipErrorInvalidValue;
  if ((fmt_g != 0 && fmt_g != 1) || (fmt_x != 0 && fmt_x != 1) || splits < 1) return hipErrorInvalidValue;
  if (dy8 == nullptr || x8 == nullptr || dw == nullptr || inv_g == nullptr || inv_x == nullptr) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(dy8) | reinterpret_cast<uintptr_t>(x8) | reinterpret_cast<uintptr_t>(dw) |
       reinterpret_cast<uintptr_t>(ws)) % 16)
    return hipErrorInvalidValue;
  if (splits > 1 && ws == nullptr) return hipErrorInvalidValue;
  const int64_t steps = (M + fp8::kWT - 1) / fp8::kWT;
  fp8::WArgs p;
  p.g = static_cast<const uint8_t*>(dy8);
  p.x = static_cast<const uint8_t*>(x8);
  p.out = static_cast<uint16_t*>(dw);
  p.inv_g = inv_g;
  p.inv_x = inv_x;
  p.ldg = ldg;
  p.ldx = ldx;
  p.M = M;
  p.N = N;
  p.K = K;
  p.n_tiles = (int)((N + fp8::kT - 1) / fp8::kT);
  p.k_tiles = (int)((K + fp8::kT - 1) / fp8::kT);
  p.splits = (int)(splits < steps ? splits : steps);  // no split without a step; the slabs beyond stay unused
  p.steps_per = (int)((steps + p.splits - 1) / p.splits);
  p.splits = (int)((steps + p.steps_per - 1) / p.steps_per);
  p.ws = p.splits > 1 ? ws : nullptr;
  if ((int64_t)p.n_tiles * p.k_tiles * p.splits > 0x7fffffff) return hipErrorInvalidValue;
  hipError_t e;
  if (fmt_g == 0) e = fmt_x == 0 ? fp8::launch_wgrad<0, 0>(p, stream) : fp8::launch_wgrad<0, 1>(p, stream);
  else e = fmt_x == 0 ? fp8::launch_wgrad<1, 0>(p, stream) : fp8::launch_wgrad<1, 1>(p, stream);
  if (e != hipSuccess || p.splits == 1) return e;
  const int64_t n = N * K;
  hipLaunchKernelGGL(fp8::wgrad8_reduce_kernel, dim3((unsigned)stream_grid(n / 8, 256, 2048)), dim3(256), 0, stream,
                     p.ws, p.out, p.splits, n, inv_g, inv_x);
  return hipGetLastError();
}

extern "C" hipError_t madnn_mx_quant_cols(const void* x, int64_t ldx, int64_t R, int64_t C, int fmt, void* q, void* e,
                                          int64_t lde, void* qc, void* ec, int64_t ldec, hipStream_t stream) {
  if (R <= 0 || C <= 0 || C % 32 || ldx % 8 || ldx < C || C > 0x7fffffff || (fmt != 0 && fmt != 1))
    return hipErrorInvalidValue;
  if (x == nullptr || q == nullptr || e == nullptr || lde % 4 || lde < 4 * ((C + 127) / 128)) return hipErrorInvalidValue;
  if (qc == nullptr || ec == nullptr || ldec % 4 || ldec < C) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(qc)) % 16 ||
      (reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(ec)) % 4)
    return hipErrorInvalidValue;
  const int64_t tiles = ((R + fp8::kQTile - 1) / fp8::kQTile) * ((C + fp8::kQTile - 1) / fp8::kQTile);
  if (tiles > 0x7fffffff) return hipErrorInvalidValue;
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  uint8_t* qp = static_cast<uint8_t*>(q);
  uint8_t* ep = static_cast<uint8_t*>(e);
  uint8_t* qcp = static_cast<uint8_t*>(qc);
  uint8_t* ecp = static_cast<uint8_t*>(ec);
  if (fmt == fp8::kE5M2)
    return fp8::launch_mx_quant_cols<1>(xp, ldx, R, (int)C, qp, ep, lde, qcp, ecp, ldec, (unsigned)tiles, stream);
  return fp8::launch_mx_quant_cols<0>(xp, ldx, R, (int)C, qp, ep, lde, qcp, ecp, ldec, (unsigned)tiles, stream);
}

extern "C" hipError_t madnn_mx_wgrad(const void* dy8, int fmt_g, const void* eg, int64_t ldeg, const void* x8, int fmt_x,
                                     const void* ex, int64_t ldex, void* dw, float* ws, int splits, int64_t M, int64_t N,
                                     int64_t K, int64_t ldg, int64_t ldx, hipStream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || N % 16 || K % 16 || ldg % 16 || ldx % 16 || ldg < N || ldx < K)
    return hipErrorInvalidValue;
  if ((fmt_g != 0 && fmt_g != 1) || (fmt_x != 0 && fmt_x != 1) || splits < 1) return hipErrorInvalidValue;
  if (dy8 == nullptr || x8 == nullptr || dw == nullptr || eg == nullptr || ex == nullptr) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(dy8) | reinterpret_cast<uintptr_t>(x8) | reinterpret_cast<uintptr_t>(dw) |
       reinterpret_cast<uintptr_t>(ws)) % 16)
    return hipErrorInvalidValue;
  if (ldeg % 4 || ldex % 4 || ldeg < N || ldex < K ||
      (reinterpret_cast<uintptr_t>(eg) | reinterpret_cast<uintptr_t>(ex)) % 4)
    return hipErrorInvalidValue;
  if (splits > 1 && ws == nullptr) return hipErrorInvalidValue;
  const int64_t steps = (M + fp8::kWT - 1) / fp8::kWT;
  fp8::XWArgs p;
  p.g = static_cast<const uint8_t*>(dy8);
  p.x = static_cast<const uint8_t*>(x8);
  p.eg = static_cast<const uint8_t*>(eg);
  p.ex = static_cast<const uint8_t*>(ex);
  p.out = static_cast<uint16_t*>(dw);
  p.ldg = ldg;
  p.ldx = ldx;
  p.ldeg = ldeg;
  p.ldex = ldex;
  p.M = M;
  p.N = N;
  p.K = K;
  p.n_tiles = (int)((N + fp8::kT - 1) / fp8::kT);
  p.k_tiles = (int)((K + fp8::kT - 1) / fp8::kT);
  p.splits = (int)(splits < steps ? splits : steps);  // as madnn_fp8_wgrad
  p.steps_per = (int)((steps + p.splits - 1) / p.splits);
  p.splits = (int)((steps + p.steps_per - 1) / p.steps_per);
  p.ws = p.splits > 1 ? ws : nullptr;
  if ((int64_t)p.n_tiles * p.k_tiles * p.splits > 0x7fffffff) return hipErrorInvalidValue;
  hipError_t e;
  if (fmt_g == 0) e = fmt_x == 0 ? fp8::launch_mx_wgrad<0, 0>(p, stream) : fp8::launch_mx_wgrad<0, 1>(p, stream);
  else e = fmt_x == 0 ? fp8::launch_mx_wgrad<1, 0>(p, stream) : fp8::launch_mx_wgrad<1, 1>(p, stream);
  if (e != hipSuccess || p.splits == 1) return e;
  const int64_t n = N * K;
  hipLaunchKernelGGL(fp8::mx_wgrad_reduce_kernel, dim3((unsigned)stream_grid(n / 8, 256, 2048)), dim3(256), 0, stream,
                     p.ws, p.out, p.splits, n);
  return hipGetLastError();
}
