// K17 -- fp8 GEMM on v_mfma_f32_32x32x64_f8f6f4 for gfx950, and the per-tensor quantiser that feeds it:
// the forward and the data gradient of an opt-in FP8 Linear (ops.linear(fp8=True), madnn.nn.Fp8Linear).
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
