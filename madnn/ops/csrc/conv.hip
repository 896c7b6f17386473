// K9 — NHWC 1x1 convolution (stride 1) as bf16 MFMA GEMMs for gfx950: forward (+ the
// following BatchNorm's batch statistics), data gradient and weight gradient.
//
// Why: 36 of ResNet-50's 53 convolutions are bottleneck 1x1s.  The MIOpen solvers that the
// shipped MI355X find-db picks for them (madnn/tuning/miopen, batch 512) reach 35-60 % of
// the HBM / MFMA bound outside layer1 and ~50 % on the data gradient inside it, and the
// BatchNorm after each one re-reads its whole output for the statistics.
//
// An NHWC activation is a dense [M = N*H*W, C] matrix and a 1x1 weight a [Cout, Cin]
// matrix, so the three passes are plain GEMMs:
//   forward   Y[m][co]   = sum_ci X[m][ci]  W[co][ci]
//   dgrad     dX[m][ci]  = sum_co dY[m][co] W[co][ci]
//   wgrad     dW[co][ci] = sum_m  dY[m][co] X[m][ci]
// One template computes D[i][j] = sum_k A(i, k) B(k, j) with j on the MFMA lane.  Each
// operand is staged from "row" memory (k contiguous: a [R][64] LDS tile read with
// ds_read_b128) or from "column" memory (k strided: a [64][C] tile read with the gfx950
// transpose read ds_read_b64_tr_b16), see mfma.h:
//   forward : i = co (A = W, row),     j = m  (B = X, row)    -> Y[j][i]
//   dgrad   : i = ci (A = W, column),  j = m  (B = dY, row)   -> dX[j][i]
//   wgrad   : i = co (A = dY, column), j = ci (B = X, column), the m reduction split over
//             workgroups; each split stores its fp32 partial [Cout][Cin] slab (one accumulator
//             register = two 128-B row segments per wave instruction) and one streaming pass sums
//             the slabs in split order -- deterministic, unlike float atomics (no -munsafe-fp-atomics
//             result that depends on arrival order).
// In the store epilogue a lane owns 4 consecutive i of one j: one 8-byte store.
//
// CDNA4 mapping: v_mfma_f32_32x32x16_bf16; 4 waves per workgroup, each owning a 64x64
// (64x32, 32x32) block of D; 64-deep k steps staged global -> VGPR -> LDS, double
// buffered with one barrier per step, so the next step's global loads are in flight
// during this step's MFMAs; 64 KiB of LDS and <= 256 VGPRs: 2 workgroups (8 waves) per
// CU.  Forward / dgrad workgroups are persistent: a workgroup keeps its i tile and walks
// its j tiles, so loading tile t+1 overlaps tile t's MFMAs and epilogue.
// Where the workgroup's weight slice fits 32 KiB, forward and data grad run ring_kernel instead: the slice stays
// in LDS for the whole walk and the activation rows arrive by LDS-DMA through a 3-stage ring (below; the
// register-staged gemm_kernel remains for the other shapes, the weight grad and as MADNN_K9_RING=0).
//
// Fused BatchNorm statistics (forward): the workgroup accumulates, per output channel,
// the sum and sum of squares of the bf16-rounded outputs it stores, in registers across
// all its tiles, and writes one [2][Cout] partial row.  That slab is the input format of
// bn.hip's finalize kernel, so the BatchNorm forward skips its statistics pass over Y.
//
// (A BatchNorm apply + ReLU prologue on the X operand, a BN-reduction epilogue over a residual
// ReLU's bit mask and a stride-2 residual epilogue were measured, lost their A/Bs and were removed
// in round 6: docs/PERF.md.)
#include <cstdlib>

#include "mfma.h"

// K12P (gemmp.hip): the deep forwards and the deep plain data grad run there (use_deep)
extern "C" {
int madnn_gemmp_supported(int64_t I, int64_t J, int64_t K, int has_bias);
int madnn_conv1x1_fwd_p_rows(int64_t M, int64_t cout);
hipError_t madnn_conv1x1_fwd_p(const void* x, const void* w, void* y, float* stats, int64_t M, int64_t cin,
                               int64_t cout, hipStream_t s);
hipError_t madnn_linear_dgrad_p(const void* dy, const void* w, const void* pre, void* dx, float* colsum, int64_t M,
                                int64_t N, int64_t K, int gelu_kind, hipStream_t s);
}

namespace madnn {
namespace conv {

using namespace mf;

constexpr int kThreads = 256;
constexpr int kBK = 64;                // reduction depth of one pipeline step
constexpr int kTargetWG = 2 * kNumCU;  // resident workgroups: 2 per CU

// run-time tunables (swept through madnn_conv1x1_tune, profiles/r1_k9_tune.json)
struct Tune {
  int fwd_wg = kTargetWG;  // forward / dgrad persistent grid target
  int wgrad_wg = 2 * kNumCU;  // weight-grad workgroups (tiles x m splits)
  int xcd = 1;             // XCD-aware workgroup remap
  int ring = ring_default();  // store-mode main loop: 0 register-staged, 1 LDS-DMA ring where it applies (use_ring)
  static int ring_default() {
    const char* e = getenv("MADNN_K9_RING");
    return e != nullptr && *e != 0 ? atoi(e) : 1;
  }
  int deep = deep_default();  // deep forwards / the deep plain data grad on K12P (gemmp.hip) where use_deep says so
  static int deep_default() {
    const char* e = getenv("MADNN_K9_DEEP");
    return e != nullptr && *e != 0 ? atoi(e) : 1;
  }
};
inline Tune& tune() {
  static Tune t;
  return t;
}

enum Mode : int { kStoreT = 0, kSplit = 1 };

struct GemmArgs {
  const uint16_t* a;
  const uint16_t* b;
  void* out;
  const uint16_t* res;  // store epilogue: out = D + res (same layout as out), or null
  const unsigned char* resmask;  // with res: res element e counts only where bit e of resmask is set
                                 // (a ReLU bit mask over the same [J][I] elements, 8 per byte), or null
  float* stats;
  const uint16_t* bny;  // BNB epilogue (data grad): BN input y [J][I] whose backward sums are taken,
  const float* bnsc;    //   with its forward scale / shift (ReLU mask = y * sc + sh > 0)
  const float* bnsh;
  int64_t lda, ldb, ldo;
  int64_t I, J, K;                       // D is I x J, reduction length K
  int i_tiles, j_tiles, j_groups, k_chunk;
  int xcd;  // 1: remap workgroup ids so consecutive logical ids share an XCD (and its L2)
};

// One operand's 64-deep slice, register-staged: R rows of "row" memory ([x][ld], k
// contiguous) or 64 k-rows of "column" memory ([k][ld], R contiguous x).  Rows past the
// end load a valid row and are zeroed by a mask (no per-load branch).
template <bool COL, int R>
struct Stage {
  static constexpr int PER = R / 32;  // 16-B chunks per thread
  u32x4 r[PER];

  __device__ __forceinline__ void load(const uint16_t* __restrict__ base, int64_t ld, int64_t x0, int64_t xlim,
                                       int64_t k0, int64_t klim, int tid) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = tid + kThreads * i;
      int64_t row, lim, col;
      if constexpr (COL) {
        row = k0 + c / (R / 8);
        lim = klim;
        col = x0 + (c % (R / 8)) * 8;
      } else {
        row = x0 + (c >> 3);
        lim = xlim;
        col = k0 + (c & 7) * 8;
      }
      const bool ok = row < lim;
      const u32x4 v = *reinterpret_cast<const u32x4*>(base + (ok ? row : lim - 1) * ld + col);
      const unsigned keep = ok ? 0xffffffffu : 0u;
      r[i] = v & keep;
    }
  }

  __device__ __forceinline__ void store(uint16_t* tile, int tid) const {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int c = tid + kThreads * i;
      int boff;
      if constexpr (COL) {
        boff = swz<R>(c / (R / 8), c % (R / 8));
      } else {
        boff = swz<64>(c >> 3, c & 7);
      }
      *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(tile) + boff) = r[i];
    }
  }

  // MFMA operand for k16 step s of the extent block starting at x (lane -> x + (lane & 31))
  static __device__ __forceinline__ bf16x8 frag(const uint16_t* tile, int s, int x, int lane) {
    if constexpr (COL) {
      return lds_col<R>(tile, 16 * s, x, lane);
    } else {
      return lds_row(tile, x + (lane & 31), 2 * s + (lane >> 5));
    }
  }
};

// BNB (store mode): besides the output D, accumulate per output channel the BatchNorm backward sums
// sum g and sum g*y, g = D * [y * sc + sh > 0], into the same [groups][2][I] partial rows STATS writes
// (the data grad of conv3 whose input was relu(bn2(y)): bn2's backward skips its reduction pass).
template <bool A_COL, bool B_COL, int BI, int BJ, int MODE, bool STATS, bool BNB = false>
__global__ __launch_bounds__(kThreads, 2) void gemm_kernel(const GemmArgs p) {
  static_assert(!(STATS && BNB), "one statistics epilogue per launch");
  constexpr int NI = (BI == 64 && BJ == 64) ? 1 : 2;  // 32-row i blocks per wave
  constexpr int WI = BI / (32 * NI), WJ = 4 / WI, NJ = BJ / (32 * WJ);
  static_assert(WI * WJ == 4 && NJ >= 1, "four waves tile the workgroup");
  constexpr int AE = BI * kBK, BE = BJ * kBK, SE = AE + BE;  // one pipeline buffer: [A | B]
  static_assert(SE >= BI * BJ, "a pipeline buffer holds the bf16 output tile");
  // output tile (store epilogue): [BJ][BI] bf16, 16-B chunks XOR-swizzled per row
  constexpr int CPR = BI / 8;               // 16-B chunks per output row
  constexpr int RPP = kThreads / CPR;       // rows per pass of the 256 threads
  __shared__ __attribute__((aligned(16))) uint16_t smem[2 * SE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l32 = lane & 31, hh = lane >> 5;
  const int wi = wave / WJ, wj = wave % WJ;
  // logical id: consecutive ids share the B (j) panel.  The dispatcher deals ids round-robin
  // over the 8 XCDs; the bijective remap of cdna_hip_programming.md T1 gives each XCD a
  // contiguous range of logical ids so the shared panels hit in that XCD's L2.
  int wid = blockIdx.x;
  if (p.xcd) wid = xcd_group_id(wid, gridDim.x);
  const int it = wid % p.i_tiles;
  const int grp = wid / p.i_tiles;
  const int64_t i0 = (int64_t)it * BI;
  const int nk = (int)((p.K + kBK - 1) / kBK);
  int jt, kbeg, kend, jstride;
  if constexpr (MODE == kSplit) {  // one j tile, k steps [kbeg, kend)
    jt = grp % p.j_tiles;
    kbeg = (grp / p.j_tiles) * p.k_chunk;
    kend = min(kbeg + p.k_chunk, nk);
    jstride = p.j_tiles;
  } else {  // persistent: j tiles grp, grp + j_groups, ...; all k
    jt = grp;
    kbeg = 0;
    kend = nk;
    jstride = p.j_groups;
  }
  if (jt >= p.j_tiles || kbeg >= kend) return;

  Stage<A_COL, BI> sta;
  Stage<B_COL, BJ> stb;
  f32x16 acc[NI][NJ];
#pragma unroll
  for (int a = 0; a < NI; ++a)
#pragma unroll
    for (int b = 0; b < NJ; ++b) acc[a][b] = zero16();
  // statistics: this thread's 8 output channels (chunk tid % CPR), summed over its rows of every tile
  float ssum[8], ssq[8], bs[8], bh[8];
  if constexpr (STATS || BNB) {
#pragma unroll
    for (int e = 0; e < 8; ++e) ssum[e] = ssq[e] = 0.f;
  }
  if constexpr (BNB) {  // this thread's 8 output channels (chunk tid % CPR of the i tile) are fixed
    const int cc = tid % (BI / 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      bs[e] = p.bnsc[i0 + 8 * cc + e];
      bh[e] = p.bnsh[i0 + 8 * cc + e];
    }
  }
  // byte offset of 16-B chunk c of output row r: rows of 256 B (BI = 128) or 128 B (BI = 64)
  auto out_off = [](int r, int c) {
    if constexpr (BI == 128) return r * 256 + 16 * (c ^ (r & 15));
    else return r * 128 + 16 * (c ^ ((r >> 1) & 7));
  };

  sta.load(p.a, p.lda, i0, p.I, (int64_t)kbeg * kBK, p.K, tid);
  stb.load(p.b, p.ldb, (int64_t)jt * BJ, p.J, (int64_t)kbeg * kBK, p.K, tid);
  sta.store(smem, tid);
  stb.store(smem + AE, tid);
  __syncthreads();
  int cur = 0, ks = kbeg;
  for (;;) {
    int njt = jt, nks = ks + 1;
    if (nks == kend) {
      nks = kbeg;
      njt = jt + jstride;
    }
    const bool more = njt < p.j_tiles;
    if (more) {
      sta.load(p.a, p.lda, i0, p.I, (int64_t)nks * kBK, p.K, tid);
      stb.load(p.b, p.ldb, (int64_t)njt * BJ, p.J, (int64_t)nks * kBK, p.K, tid);
    }
    uint16_t* buf = smem + cur * SE;
#pragma unroll
    for (int s = 0; s < kBK / 16; ++s) {
      bf16x8 af[NI], bv[NJ];
#pragma unroll
      for (int a = 0; a < NI; ++a) af[a] = Stage<A_COL, BI>::frag(buf, s, (wi * NI + a) * 32, lane);
#pragma unroll
      for (int b = 0; b < NJ; ++b) bv[b] = Stage<B_COL, BJ>::frag(buf + AE, s, (wj * NJ + b) * 32, lane);
#pragma unroll
      for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int b = 0; b < NJ; ++b) acc[a][b] = mfma(af[a], bv[b], acc[a][b]);
    }
    if (more) {  // the other buffer was last read before the previous barrier
      sta.store(smem + (cur ^ 1) * SE, tid);
      stb.store(smem + (cur ^ 1) * SE + AE, tid);
    }
    if (ks == kend - 1) {  // tile done: epilogue
      if constexpr (MODE == kStoreT) {
        // D[i][j] (4 consecutive i per lane) -> LDS tile [j][i] -> full-row 16-B global stores
        __syncthreads();  // every wave is done reading buf
        char* ot = reinterpret_cast<char*>(buf);
#pragma unroll
        for (int b = 0; b < NJ; ++b) {
          const int jr = (wj * NJ + b) * 32 + l32;
#pragma unroll
          for (int a = 0; a < NI; ++a)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int ic = (wi * NI + a) * 32 + 8 * g + 4 * hh;  // first of the 4 i
              const unsigned lo = pack_bf16x2(acc[a][b][4 * g], acc[a][b][4 * g + 1]);
              const unsigned hi = pack_bf16x2(acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]);
              *reinterpret_cast<u32x2*>(ot + out_off(jr, ic >> 3) + 8 * ((ic >> 2) & 1)) = u32x2{lo, hi};
            }
        }
        __syncthreads();
        uint16_t* out = static_cast<uint16_t*>(p.out);
        const int c = tid % CPR;
#pragma unroll
        for (int u = 0; u < BJ / RPP; ++u) {
          const int r = tid / CPR + RPP * u;
          const int64_t j = (int64_t)jt * BJ + r;
          if (j < p.J) {
            u32x4 v = *reinterpret_cast<const u32x4*>(ot + out_off(r, c));
            if (p.res != nullptr) {  // fused residual-gradient accumulation (fp32 add, one rounding)
              u32x4 rv = *reinterpret_cast<const u32x4*>(p.res + j * p.ldo + i0 + 8 * c);
              if (p.resmask != nullptr) {
                const unsigned bits = p.resmask[(j * p.ldo + i0 + 8 * c) >> 3];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  rv[e] &= ((bits >> (2 * e)) & 1u ? 0xffffu : 0u) | ((bits >> (2 * e + 1)) & 1u ? 0xffff0000u : 0u);
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float lo = bf16_lo(v[e]) + bf16_lo(rv[e]);
                const float hi = bf16_hi(v[e]) + bf16_hi(rv[e]);
                v[e] = pack_bf16x2(lo, hi);
              }
            }
            *reinterpret_cast<u32x4*>(out + j * p.ldo + i0 + 8 * c) = v;
            if constexpr (BNB) {
              const u32x4 yv = *reinterpret_cast<const u32x4*>(p.bny + j * p.ldo + i0 + 8 * c);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                  const int k = 2 * e + hf;
                  const float g = hf ? bf16_hi(v[e]) : bf16_lo(v[e]);
                  const float yy = hf ? bf16_hi(yv[e]) : bf16_lo(yv[e]);
                  const bool on = yy * bs[k] + bh[k] > 0.f;
                  const float gm = on ? g : 0.f;
                  ssum[k] += gm;
                  ssq[k] += gm * yy;
                }
              }
            }
            if constexpr (STATS) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float x0 = bf16_lo(v[e]);
                const float x1 = bf16_hi(v[e]);
                ssum[2 * e] += x0;
                ssq[2 * e] += x0 * x0;
                ssum[2 * e + 1] += x1;
                ssq[2 * e + 1] += x1 * x1;
              }
            }
          }
        }
      } else {
        // this split's partial slab (split = grp / j_tiles)
        const int64_t jw = (int64_t)jt * BJ + wj * NJ * 32 + l32;
        float* out = static_cast<float*>(p.out) + (int64_t)(grp / p.j_tiles) * p.I * p.ldo;
#pragma unroll
        for (int a = 0; a < NI; ++a)
#pragma unroll
          for (int b = 0; b < NJ; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int64_t i = i0 + (wi * NI + a) * 32 + acc_row(r, hh);
              out[i * p.ldo + jw + b * 32] = acc[a][b][r];
            }
      }
#pragma unroll
      for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int b = 0; b < NJ; ++b) acc[a][b] = zero16();
    }
    if (!more) break;
    __syncthreads();  // next buffer filled; this one (or its output tile) fully consumed
    cur ^= 1;
    jt = njt;
    ks = nks;
  }

  if constexpr (STATS || BNB) {
    __syncthreads();  // smem is free
    float* red = reinterpret_cast<float*>(smem);  // [RPP][2][BI]
    const int c = tid % CPR, rg = tid / CPR;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[(rg * 2) * BI + 8 * c + e] = ssum[e];
      red[(rg * 2 + 1) * BI + 8 * c + e] = ssq[e];
    }
    __syncthreads();
    for (int k = tid; k < 2 * BI; k += kThreads) {
      const int which = k / BI, ii = k % BI;
      float v = 0.f;
      for (int g = 0; g < RPP; ++g) v += red[(g * 2 + which) * BI + ii];
      p.stats[((int64_t)grp * 2 + which) * p.I + i0 + ii] = v;
    }
  }
}

template <bool A_COL, bool B_COL, int BI, int BJ, int MODE, bool STATS, bool BNB = false>
hipError_t launch(const GemmArgs& p, int grid, hipStream_t s) {
  hipLaunchKernelGGL((gemm_kernel<A_COL, B_COL, BI, BJ, MODE, STATS, BNB>), dim3(grid), dim3(kThreads), 0, s, p);
  return hipGetLastError();
}

// ---- K9 ring: the store-mode main loop with LDS-DMA operands (docs/ARCHITECTURE.md "K9 ring schedule") ----
// The workgroup's weight slice A [BI][K] is loaded once and stays in LDS for the whole persistent walk (the
// register-staged loop loads it again in every k step of every tile); the B operand (activation rows) streams
// through a ring of kRingStages 64-deep stages, written by global_load_lds_dwordx4 straight into the swz<64>
// row image Stage::frag reads.  While step u's MFMAs issue, steps u+1 and u+2 are in flight, across tile
// boundaries and through the epilogue; waits are counted vmcnt(N) (wait_vm below), never a drain inside a walk.
// Same MFMA instruction, same ascending k, same epilogue arithmetic and thread map as gemm_kernel: bitwise the
// same outputs and partial rows.
constexpr int kRingStages = 3;
constexpr int kBStage = 128 * kBK;  // bf16 elements of one B stage: [128 j][64 k], 16 KiB

// LDS-DMA from a wave-uniform base plus a 32-bit per-lane byte offset (no 64-bit per-lane address); M0 is set
// and restored inside the statement (common.h glds16), and the leading s_nop covers a base that was formed
// with v_readfirstlane
__device__ __forceinline__ void glds16_off(const void* base, unsigned voff, unsigned lds_byte) {
  const unsigned lds = __builtin_amdgcn_readfirstlane(lds_byte);
  unsigned keep;
  asm volatile(
      "s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(base), "s"(lds)
      : "memory");
}

// LDS accesses retired, then the barrier (a raw s_barrier: __syncthreads' fences would drain vmcnt)
__device__ __forceinline__ void ring_bar() {
  wait_lgkmcnt0();
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// Wait until this wave's DMA of step u has landed.  VMEM operations retire in issue order on one counter; the
// operations a wave has issued after step u's 4 DMA instructions are, in order: the epilogue of step u-2 (if
// it ended a tile), the 4 DMA instructions of step u+1 (if the stream has one: `next`), the epilogue of step
// u-1 (if it ended a tile).  An epilogue followed by another step belongs to a full tile (the partial tile is
// the last of the walk), so it has issued exactly EST global stores per wave, plus its res / mask / bny loads,
// which are left out of the count: a count below the true number only waits longer.
template <int EST>
__device__ __forceinline__ void wait_vm(bool next, int epilogues) {
  if (next) {
    if (epilogues == 0) wait_vmcnt<4>();
    else if (epilogues == 1) wait_vmcnt<4 + EST>();
    else wait_vmcnt<4 + 2 * EST>();
  } else {
    if (epilogues == 0) wait_vmcnt<0>();
    else if (epilogues == 1) wait_vmcnt<EST>();
    else wait_vmcnt<2 * EST>();
  }
}

// LDS: 32 KiB of resident weight slice (AK k steps: K <= 128 at BI = 128, K <= 256 at BI = 64) + 3 x 16 KiB of
// B stages = 80 KiB: two workgroups per CU, as gemm_kernel.
template <bool A_COL, int BI, bool STATS, bool BNB>
__global__ __launch_bounds__(kThreads, 2) void ring_kernel(const GemmArgs p) {
  static_assert(!(STATS && BNB), "one statistics epilogue per launch");
  static_assert(!A_COL || BI == 128, "the column image of the weight slice is 128 wide");
  constexpr int BJ = 128, NS = kRingStages, AK = 256 / BI;
  constexpr int NI = 2, WI = BI / 64, WJ = 4 / WI, NJ = BJ / (32 * WJ);
  constexpr int AE = BI * kBK;          // one k step of the resident slice
  constexpr int CPR = BI / 8;           // 16-B chunks per output row
  constexpr int RPP = kThreads / CPR;   // rows per pass of the 256 threads
  constexpr int EST = BJ / RPP;         // global stores per thread and full tile
  constexpr int PR = kBStage / BI;      // output rows one B stage holds as [PR][BI] bf16
  constexpr int NP = BJ / PR;           // staging passes per tile (2 at BI = 128: wave row wj writes pass wj)
  static_assert(NP == 1 || NP == WJ, "a staging pass is the j rows of one wave row");
  __shared__ __attribute__((aligned(16))) uint16_t smem[AK * AE + NS * kBStage];
  uint16_t* const ares = smem;
  uint16_t* const bring = smem + AK * AE;
  const unsigned lds_a = (unsigned)(size_t)(lds_void*)smem, lds_b = lds_a + 2u * AK * AE;  // LDS byte addresses
  const int tid = threadIdx.x, lane = tid & 63, l32 = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave / WJ, wj = wave % WJ;
  int wid = blockIdx.x;
  if (p.xcd) wid = xcd_group_id(wid, gridDim.x);
  const int it = wid % p.i_tiles;
  const int grp = wid / p.i_tiles;
  const int64_t i0 = (int64_t)it * BI;
  const int nk = (int)(p.K / kBK);  // <= AK (launcher)
  const int jstride = p.j_groups, jtiles = p.j_tiles;
  int jt = grp;
  if (jt >= jtiles) return;
  const int total = ((jtiles - grp + jstride - 1) / jstride) * nk;  // k steps of this workgroup's stream
  // kernel-argument fields as scalars (a lambda capturing the struct by reference sends it to scratch)
  const uint16_t* const pb = p.b;
  const int64_t J = p.J, ldb = p.ldb;

  // resident weight slice: nk images, [BI][64] swz<64> (row memory) or [64][128] swz<128> (column memory)
  for (int t = 0; t < nk; ++t) {
#pragma unroll
    for (int q = 0; q < BI / 32; ++q) {
      const int inst = wave * (BI / 32) + q;  // 1 KiB of the image per instruction
      unsigned off;
      if constexpr (A_COL) {
        const int r = inst * 4 + (lane >> 4);
        const int ch = (lane & 15) ^ (((r & 3) << 2) | ((r >> 2) & 3));
        off = (unsigned)((t * kBK + r) * (int)p.lda + (int)i0 + 8 * ch) * 2u;
      } else {
        const int r = inst * 8 + (lane >> 3);
        const int ch = (lane & 7) ^ ((((r >> 1) & 1) << 2) | ((r >> 2) & 3));
        off = (unsigned)(((int)i0 + r) * (int)p.lda + t * kBK + 8 * ch) * 2u;
      }
      glds16_off(p.a, off, lds_a + 2u * (unsigned)(t * AE + inst * 512));
    }
  }

  // B stage: this wave's 4 DMA instructions cover rows 32 wave + 8 q + (lane >> 3); slot lane & 7 of row r
  // holds chunk (lane & 7) ^ f(r) (swz<64>).  Rows past J load the last valid row; their outputs are skipped.
  const int rq0 = wave * 32 + (lane >> 3);
  unsigned colb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = rq0 + 8 * q;
    colb[q] = 16u * (unsigned)((lane & 7) ^ ((((r >> 1) & 1) << 2) | ((r >> 2) & 3)));
  }
  int ijt = grp, ikt = 0, istage = 0;  // DMA cursor: j tile, k step and stage of the next step to issue
  auto issue_b = [&]() {
    const int64_t j0 = (int64_t)ijt * BJ;
    const int valid = (int)min((int64_t)BJ, J - j0);
    const uint16_t* base = pb + j0 * ldb + (int64_t)ikt * kBK;
    const unsigned dst = lds_b + 2u * (unsigned)(istage * kBStage + wave * 2048);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = min(rq0 + 8 * q, valid - 1);
      glds16_off(base, (unsigned)(row * (int)ldb) * 2u + colb[q], dst + 1024u * q);
    }
    istage = istage + 1 == NS ? 0 : istage + 1;
    if (++ikt == nk) {
      ikt = 0;
      ijt += jstride;
    }
  };
  issue_b();
  if (total > 1) issue_b();

  f32x16 acc[NI][NJ];
#pragma unroll
  for (int a = 0; a < NI; ++a)
#pragma unroll
    for (int b = 0; b < NJ; ++b) acc[a][b] = zero16();
  float ssum[8], ssq[8], bs[8], bh[8];
  if constexpr (STATS || BNB) {
#pragma unroll
    for (int e = 0; e < 8; ++e) ssum[e] = ssq[e] = 0.f;
  }
  if constexpr (BNB) {
    const int cc = tid % (BI / 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      bs[e] = p.bnsc[i0 + 8 * cc + e];
      bh[e] = p.bnsh[i0 + 8 * cc + e];
    }
  }
  // byte offset of 16-B chunk c of staged output row r (gemm_kernel's images)
  auto out_off = [](int r, int c) {
    if constexpr (BI == 128) return r * 256 + 16 * (c ^ (r & 15));
    else return r * 128 + 16 * (c ^ ((r >> 1) & 7));
  };

  int u = 0, t = 0, st = 0;     // stream step, its k step and its stage
  int l1 = 0, l2 = 0;           // 1: step u-1 / u-2 ended a tile
  for (;;) {
    wait_vm<EST>(u + 1 < total, l1 + l2);
    ring_bar();  // step u landed in every wave; stage (u - 1) % NS (operands or staged output) fully consumed
    if (u + 2 < total) issue_b();  // into that stage
    const uint16_t* abuf = ares + t * AE;
    uint16_t* bbuf = bring + st * kBStage;
#pragma unroll
    for (int s = 0; s < kBK / 16; ++s) {
      bf16x8 af[NI], bv[NJ];
#pragma unroll
      for (int a = 0; a < NI; ++a) af[a] = Stage<A_COL, BI>::frag(abuf, s, (wi * NI + a) * 32, lane);
#pragma unroll
      for (int b = 0; b < NJ; ++b) bv[b] = Stage<false, BJ>::frag(bbuf, s, (wj * NJ + b) * 32, lane);
#pragma unroll
      for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int b = 0; b < NJ; ++b) acc[a][b] = mfma(af[a], bv[b], acc[a][b]);
    }
    const bool last = t == nk - 1;
    if (last) {
      // epilogue (gemm_kernel's, staged through the stage just consumed in NP passes of PR rows): the next
      // steps' DMA stays in flight in the other two stages
      ring_bar();  // every wave is done reading bbuf
      char* ot = reinterpret_cast<char*>(bbuf);
      uint16_t* out = static_cast<uint16_t*>(p.out);
      const int c = tid % CPR;
#pragma unroll
      for (int h = 0; h < NP; ++h) {
        if (NP == 1 || wj == h) {
#pragma unroll
          for (int b = 0; b < NJ; ++b) {
            const int jr = (wj * NJ + b) * 32 + l32 - h * PR;
#pragma unroll
            for (int a = 0; a < NI; ++a)
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                const int ic = (wi * NI + a) * 32 + 8 * g + 4 * hh;  // first of the 4 i
                const unsigned lo = pack_bf16x2(acc[a][b][4 * g], acc[a][b][4 * g + 1]);
                const unsigned hi = pack_bf16x2(acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]);
                *reinterpret_cast<u32x2*>(ot + out_off(jr, ic >> 3) + 8 * ((ic >> 2) & 1)) = u32x2{lo, hi};
              }
          }
        }
        ring_bar();
#pragma unroll
        for (int uu = 0; uu < EST / NP; ++uu) {
          const int r = tid / CPR + RPP * (h * (EST / NP) + uu);
          const int64_t j = (int64_t)jt * BJ + r;
          if (j < p.J) {
            u32x4 v = *reinterpret_cast<const u32x4*>(ot + out_off(r - h * PR, c));
            if (p.res != nullptr) {  // fused residual-gradient accumulation (fp32 add, one rounding)
              u32x4 rv = *reinterpret_cast<const u32x4*>(p.res + j * p.ldo + i0 + 8 * c);
              if (p.resmask != nullptr) {
                const unsigned bits = p.resmask[(j * p.ldo + i0 + 8 * c) >> 3];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  rv[e] &= ((bits >> (2 * e)) & 1u ? 0xffffu : 0u) | ((bits >> (2 * e + 1)) & 1u ? 0xffff0000u : 0u);
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float lo = bf16_lo(v[e]) + bf16_lo(rv[e]);
                const float hi = bf16_hi(v[e]) + bf16_hi(rv[e]);
                v[e] = pack_bf16x2(lo, hi);
              }
            }
            *reinterpret_cast<u32x4*>(out + j * p.ldo + i0 + 8 * c) = v;
            if constexpr (BNB) {
              const u32x4 yv = *reinterpret_cast<const u32x4*>(p.bny + j * p.ldo + i0 + 8 * c);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                  const int k = 2 * e + hf;
                  const float g = hf ? bf16_hi(v[e]) : bf16_lo(v[e]);
                  const float yy = hf ? bf16_hi(yv[e]) : bf16_lo(yv[e]);
                  const bool on = yy * bs[k] + bh[k] > 0.f;
                  const float gm = on ? g : 0.f;
                  ssum[k] += gm;
                  ssq[k] += gm * yy;
                }
              }
            }
            if constexpr (STATS) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float x0 = bf16_lo(v[e]);
                const float x1 = bf16_hi(v[e]);
                ssum[2 * e] += x0;
                ssq[2 * e] += x0 * x0;
                ssum[2 * e + 1] += x1;
                ssq[2 * e + 1] += x1 * x1;
              }
            }
          }
        }
        if (h + 1 < NP) ring_bar();  // pass h read back before pass h + 1 overwrites it
      }
#pragma unroll
      for (int a = 0; a < NI; ++a)
#pragma unroll
        for (int b = 0; b < NJ; ++b) acc[a][b] = zero16();
    }
    if (++u == total) break;
    l2 = l1;
    l1 = last ? 1 : 0;
    st = st + 1 == NS ? 0 : st + 1;
    if (last) {
      t = 0;
      jt += jstride;
    } else {
      ++t;
    }
  }

  if constexpr (STATS || BNB) {
    ring_bar();  // the stream is over (the last wait was a drain): the stages are free
    float* red = reinterpret_cast<float*>(bring);  // [RPP][2][BI]: one stage
    const int c = tid % CPR, rg = tid / CPR;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[(rg * 2) * BI + 8 * c + e] = ssum[e];
      red[(rg * 2 + 1) * BI + 8 * c + e] = ssq[e];
    }
    ring_bar();
    for (int k = tid; k < 2 * BI; k += kThreads) {
      const int which = k / BI, ii = k % BI;
      float v = 0.f;
      for (int g = 0; g < RPP; ++g) v += red[(g * 2 + which) * BI + ii];
      p.stats[((int64_t)grp * 2 + which) * p.I + i0 + ii] = v;
    }
  }
}

template <bool A_COL, int BI, bool STATS, bool BNB = false>
hipError_t launch_ring(const GemmArgs& p, int grid, hipStream_t s) {
  hipLaunchKernelGGL((ring_kernel<A_COL, BI, STATS, BNB>), dim3(grid), dim3(kThreads), 0, s, p);
  return hipGetLastError();
}

// Does a store-mode launch take the ring?  Where the weight slice fits its 32 KiB, except the shapes whose
// per-shape A/B the ring lost (docs/PERF.md round 12): BI = 64 at K = 64, where the register-staged loop already
// runs above 5.7 TB/s.  Everything else (K > 128 at BI = 128, the BI = 64 data grad) runs gemm_kernel.
inline bool use_ring(bool a_col, int bi, int64_t K) {
  if (tune().ring <= 0 || (a_col && bi != 128)) return false;
  const int64_t nk = K / kBK;
  return bi == 128 ? nk <= 2 : (nk >= 2 && nk <= 4);
}

// Does the forward (or, with dgrad, the plain data grad: no residual, no BN sums) run on K12P, the persistent
// 256x256-tile 8-wave GEMM of gemmp.hip, instead of K9?  Where K12P takes the shape (M and the output channels
// multiples of 256, the reduction a multiple of 64) and both channel counts are deep: Cin >= 256 with Cout >= Cin.
// Measured: the five such channel pairs of the ResNet-50 step (256 -> 512, 256 -> 1024, 512 -> 1024, 512 -> 2048,
// 1024 -> 2048) and the 256 -> 512 data grad, at M = 25088 .. 1605632, each 1.2-2.0x faster than K9 by more than
// both arms' spreads at 2048 and at 512 images (profiles/r14_k12p_plain_vs_k9.json); K9's four waves per workgroup
// cannot keep the MFMAs fed there (docs/PERF.md rounds 12, 14).  With the BatchNorm consumer counted
// (profiles/r14_k12p_deep_kernel_ab_b512.json) 256 -> 1024 at M = 100352 is even, not faster: its M / 64 partial
// rows cross the consumer's prereduce threshold.  Not measured, and on K12P by extension only: other pairs the
// rule admits (square ones such as 256 -> 256, 512 -> 512) and small M, where K12P has (M / 256) * (Cout / 256)
// tiles for 256 CUs.  The rule has no bound on M because the small shapes of tests/test_conv1x1_deep_gpu.py must
// reach the kernel.  Shallower or contracting shapes were not measured and stay on K9.
inline bool use_deep(int64_t M, int64_t cin, int64_t cout, bool dgrad = false) {
  if (tune().deep <= 0 || cin < 256 || cout < cin) return false;
  return (dgrad ? madnn_gemmp_supported(cin, M, cout, 0) : madnn_gemmp_supported(cout, M, cin, 0)) != 0;
}

// i-tile width of the forward: 128 where Cout allows, except that with the ring on K = 192 / 256 take 64-wide
// tiles, whose weight slice fits the ring's 32 KiB (measured faster than 128-wide register-staged tiles:
// docs/PERF.md round 12).  The plan, and with it the number of partial rows, follows the width.
inline int fwd_bi(int64_t cin, int64_t cout) {
  if (cout % 128 != 0) return 64;
  const int64_t nk = cin / kBK;
  return (tune().ring > 0 && nk >= 3 && nk <= 4) ? 64 : 128;
}

// forward / dgrad: i tiles x j groups, each workgroup walking an equal share of the j tiles.
// Shallow reductions (K < 512: one tile is a few k steps, HBM-bound) stay persistent so the next
// tile's loads overlap this tile's epilogue; deep ones get one tile per workgroup (measured
// faster: profiles/r1_k9_tune.json).
inline void plan_persistent(GemmArgs& p, int64_t J, int BI, int64_t I, int64_t K) {
  p.i_tiles = (int)(I / BI);
  p.j_tiles = (int)((J + 127) / 128);
  const int64_t total = (int64_t)p.i_tiles * p.j_tiles;
  const int64_t per = K >= 8 * kBK ? 1 : (total + tune().fwd_wg - 1) / tune().fwd_wg;
  p.j_groups = (int)((p.j_tiles + per - 1) / per);
  p.k_chunk = 0;
}

// dw[i] = sum over splits of slab[s][i], in split order (deterministic), fp32 or bf16; n % 4 == 0
template <bool BF16>
__global__ __launch_bounds__(256) void split_reduce_kernel(const float* __restrict__ slab, int splits, int64_t n,
                                                           void* __restrict__ dw) {
  const int64_t n4 = n / 4;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n4; v += (int64_t)gridDim.x * 256) {
    f32x4 acc = reinterpret_cast<const f32x4*>(slab)[v];
    for (int s = 1; s < splits; ++s) acc += reinterpret_cast<const f32x4*>(slab + (int64_t)s * n)[v];
    if constexpr (BF16) {
      const unsigned lo = pack_bf16x2(acc[0], acc[1]);
      const unsigned hi = pack_bf16x2(acc[2], acc[3]);
      reinterpret_cast<u32x2*>(dw)[v] = u32x2{lo, hi};
    } else {
      reinterpret_cast<f32x4*>(dw)[v] = acc;
    }
  }
}

// workgroup tiles and m splits of the weight gradient (shared by the launcher and the workspace size)
inline void wgrad_split(int64_t M, int64_t cin, int64_t cout, int& bi, int& bj, int64_t& tiles, int& k_chunk,
                        int64_t& splits) {
  bi = cout % 128 == 0 ? 128 : 64;
  bj = cin % 128 == 0 ? 128 : 64;
  tiles = (cout / bi) * (cin / bj);
  const int64_t nk = (M + kBK - 1) / kBK;
  splits = (tune().wgrad_wg + tiles - 1) / tiles;
  splits = splits < 1 ? 1 : (splits > nk ? nk : splits);
  k_chunk = (int)((nk + splits - 1) / splits);
  splits = (nk + k_chunk - 1) / k_chunk;
}

// K9F — backward of relu(bn3(conv3(a2)) + idt) behind bn3's reduction, for C = 64 -> 4C = 256 (ResNet
// layer 1): bn3's apply, conv3's data grad (+ bn2's backward sums, the BNB epilogue) and conv3's weight
// grad in one kernel, so dy3 = ca g + cb y3 + cc (g = dout under bn3's ReLU bit mask) is formed in
// registers and never reaches HBM.  Workgroups are persistent over 128-row m tiles.  Per 64-channel co
// step the bf16-rounded dy3 tile [128 m][64 co] is stored to LDS once and read twice: with row reads as
// the data grad's B operand (da2[m][ci] += dy3[m][co] W3[co][ci]) and with transpose reads as the weight
// grad's A operand (dW3[co][ci] += dy3[m][co] a2[m][ci]).  W3 stays in LDS for the whole walk, the
// 256 x 64 dW3 accumulators in registers (64 per lane); each workgroup stores one fp32 slab and
// split_reduce_kernel sums the slabs in workgroup order (deterministic).
// LDS: W3 32 KiB + dy3 2 x 16 KiB + a2 16 KiB = 80 KiB: two workgroups per CU.
// The layer-1 downsample block, relu(bn3(conv3(a2)) + bn_ds(conv_ds(xf))), runs the kernel twice behind the
// dual reduction: once as above, and once with (yd, bn_ds's coefficients, W_ds, xf) in the place of
// (y3, bn3's, W3, a2) and without the BNB epilogue (template parameter BNB below).
constexpr int kFC = 64, kFC4 = 256, kFBM = 128;
constexpr int kFW = kFC4 * kFC, kFT = kFBM * 64;  // LDS elements: W3 image, one [128][64] tile

struct FusedArgs {
  const uint16_t* dout;       // [M][4C]
  const uint16_t* y;          // [M][4C] the BatchNorm's input: y3 (bn3) or yd (the downsample BatchNorm)
  const unsigned char* mask;  // the block's ReLU bit mask over [M][4C], 8 per byte
  const float* coef;          // that BatchNorm's backward coefficients ca | cb | cc, [3][4C]
  const uint16_t* w;          // [4C][C]: W3 or W_ds
  const uint16_t* a;          // [M][C] the convolution's input: a2 = relu(bn2(y2)), or xf
  const uint16_t* y2;         // [M][C]                      (BNB only)
  const float* sc2;           // bn2's forward scale / shift (BNB only)
  const float* sh2;
  uint16_t* da;               // [M][C] the data gradient
  float* partial;             // [grid][2][C] bn2's backward sums (BNB only)
  float* slabs;               // [grid][4C][C]
  int64_t M;
  int m_tiles;
};

// BNB: the data gradient is d relu(bn2(y2)) and the epilogue also takes bn2's backward sums over it (conv3).
// Without it the data gradient is stored plainly: no y2 / sc2 / sh2 reads, no sums, no partial row (the
// downsample convolution, whose input xf has no BatchNorm of this block in front of it).
template <bool BNB>
__global__ __launch_bounds__(kThreads, 2) void bn3_conv3_bwd_kernel(const FusedArgs p) {
  __shared__ __attribute__((aligned(16))) uint16_t smem[kFW + 3 * kFT];
  uint16_t* const wt = smem;             // [256 co][64 ci], swz<64>
  uint16_t* const dyt = smem + kFW;      // 2 x [128 m][64 co]
  uint16_t* const at = dyt + 2 * kFT;    // [128 m][64 ci]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l32 = lane & 31, hh = lane >> 5;
  const int G = gridDim.x;
  // staging and the store epilogue share one thread map: 16-B chunk c8 of the 64-channel rows r8 + 32 i
  const int c8 = tid & 7, r8 = tid >> 3;

  {
    Stage<false, kFBM> sw;
#pragma unroll
    for (int h = 0; h < kFC4 / kFBM; ++h) {
      sw.load(p.w, kFC, h * kFBM, kFC4, 0, kFC, tid);
      sw.store(wt + h * kFT, tid);
    }
  }
  float ssum[BNB ? 8 : 1], ssq[BNB ? 8 : 1];
#pragma unroll
  for (int e = 0; e < (BNB ? 8 : 1); ++e) ssum[e] = ssq[e] = 0.f;
  f32x16 accw[kFC4 / 64], accd[2];
#pragma unroll
  for (int q = 0; q < kFC4 / 64; ++q) accw[q] = zero16();
  accd[0] = accd[1] = zero16();

  // Register stage of one step.  Addresses are a uniform tile base plus a 32-bit per-thread offset; rows
  // past M load the last valid row (in bounds) and are zeroed in convert_store, after the affine step: a
  // zeroed load would still yield cc.  (a2's rows past M then meet zero dy3 rows.)
  u32x4 sd[4], sy[4], sa[4];
  unsigned mk[4];
  // a 32-bit offset the compiler must take as it is: uniform base + this offset is one load, whereas a
  // 64-bit per-thread address hoisted out of the walk costs two registers for every load of a step
  auto opaque = [](unsigned v) {
    asm volatile("" : "+v"(v));
    return v;
  };
  auto row_of = [&](int tile, int i) {  // row r8 + 32 i of the tile, clamped to the rows that exist
    const int valid = (int)min((int64_t)kFBM, p.M - (int64_t)tile * kFBM);
    return min(r8 + 32 * i, valid - 1);
  };
  auto load_step = [&](int tile, int q) {
    const int64_t m0 = (int64_t)tile * kFBM;
    const char* bd = reinterpret_cast<const char*>(p.dout + m0 * kFC4 + q * 64);
    const char* by = reinterpret_cast<const char*>(p.y + m0 * kFC4 + q * 64);
    const unsigned char* bm = p.mask + m0 * (kFC4 / 8) + q * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned r = (unsigned)row_of(tile, i);
      const unsigned vo = opaque((r * kFC4 + 8 * c8) * 2u), vm = opaque(r * (kFC4 / 8) + c8);
      sd[i] = *reinterpret_cast<const u32x4*>(bd + vo);
      sy[i] = *reinterpret_cast<const u32x4*>(by + vo);
      mk[i] = (unsigned)(int)reinterpret_cast<const signed char*>(bm)[vm];  // bits 0..7 are used; no zero-extend to wait for
    }
  };
  auto load_a2 = [&](int tile) {
    const char* ba = reinterpret_cast<const char*>(p.a + (int64_t)tile * kFBM * kFC);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      sa[i] = *reinterpret_cast<const u32x4*>(ba + opaque(((unsigned)row_of(tile, i) * kFC + 8 * c8) * 2u));
  };
  auto store_a2 = [&]() {
    // rows 32 apart share the swizzle term: one offset, formed here, plus 4 KiB steps
    char* a0 = reinterpret_cast<char*>(at) + opaque((unsigned)swz<64>(r8, c8));
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(a0 + 4096 * i) = sa[i];
  };
  // dy3 of the staged step, rounded to bf16, into an LDS tile.  The coefficient loads (cache hits) are
  // issued first and fenced, so their latency runs under the wait for the staged data, not after it.
  auto convert_store = [&](uint16_t* tile_lds, int tile, int q) {
    const float* cf = p.coef + q * 64 + 8 * c8;
    f32x4 ca[2], cb[2], cc[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      ca[h] = *reinterpret_cast<const f32x4*>(cf + 4 * h);
      cb[h] = *reinterpret_cast<const f32x4*>(cf + kFC4 + 4 * h);
      cc[h] = *reinterpret_cast<const f32x4*>(cf + 2 * kFC4 + 4 * h);
    }
    __builtin_amdgcn_sched_barrier(0);
    const int valid = (int)min((int64_t)kFBM, p.M - (int64_t)tile * kFBM);
    unsigned mb[4];  // taken here, so that nothing derived from a mask byte is scheduled (and waited for) earlier
#pragma unroll
    for (int i = 0; i < 4; ++i) mb[i] = opaque(mk[i]);
    u32x4 o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned keep = r8 + 32 * i < valid ? 0xffffffffu : 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int k = 2 * e + hf;
          const float d = hf ? bf16_hi(sd[i][e]) : bf16_lo(sd[i][e]);
          const float y = hf ? bf16_hi(sy[i][e]) : bf16_lo(sy[i][e]);
          const float g = ((mb[i] >> k) & 1u) ? d : 0.f;
          v[hf] = ca[k >> 2][k & 3] * g + cb[k >> 2][k & 3] * y + cc[k >> 2][k & 3];
        }
        o[i][e] = pack_bf16x2(v[0], v[1]) & keep;
      }
    }
    char* t0 = reinterpret_cast<char*>(tile_lds) + opaque((unsigned)swz<64>(r8, c8));  // as in store_a2
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(t0 + 4096 * i) = o[i];
  };
  // da2 tile in LDS: [128 m][64 ci] bf16, 16-B chunks XOR-swizzled per row (gemm_kernel's BI = 64 image)
  auto out_off = [](int r, int c) { return r * 128 + 16 * (c ^ ((r >> 1) & 7)); };

  int tile = blockIdx.x;  // the launcher keeps grid <= m_tiles
  load_step(tile, 0);
  load_a2(tile);
  convert_store(dyt, tile, 0);
  store_a2();
  __syncthreads();
  int cur = 0;
  for (;;) {
    const int ntile = tile + G;
    const bool more = ntile < p.m_tiles;
#pragma unroll
    for (int q = 0; q < kFC4 / 64; ++q) {
      const bool last = q == kFC4 / 64 - 1;
      const int nq = last ? 0 : q + 1;
      const int nt = last ? ntile : tile;
      const bool go = !last || more;
      if (go) {  // the next step's global loads are in flight during this step's MFMAs
        load_step(nt, nq);
        if (last) load_a2(nt);
      }
      uint16_t* buf = dyt + cur * kFT;
      // data grad: i = ci (W3, column memory), j = m (dy3, row memory); wave w owns m rows 32 w .. +31
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bf16x8 bv = lds_row(buf, wave * 32 + l32, 2 * s + hh);
#pragma unroll
        for (int a = 0; a < 2; ++a) accd[a] = mfma(lds_col<64>(wt, q * 64 + 16 * s, a * 32, lane), bv, accd[a]);
        // scheduling fences: at most two k steps of operand fragments live (the kernel sits at the 256-VGPR budget)
        if (s & 1) __builtin_amdgcn_sched_barrier(0);
      }
      // weight grad: i = co (dy3, column memory), j = ci (a2, column memory), m the reduction;
      // wave w owns co block w >> 1 of this step and ci block w & 1
#pragma unroll
      for (int s = 0; s < kFBM / 16; ++s) {
        accw[q] = mfma(lds_col<64>(buf, 16 * s, (wave >> 1) * 32, lane), lds_col<64>(at, 16 * s, (wave & 1) * 32, lane),
                       accw[q]);
        if (s & 1) __builtin_amdgcn_sched_barrier(0);
      }
      if (go) convert_store(dyt + (cur ^ 1) * kFT, nt, nq);  // the other buffer was last read before the previous barrier
      if (last) {
        __syncthreads();  // every wave is done reading buf and the a2 tile
        if (more) store_a2();
        char* ot = reinterpret_cast<char*>(buf);
        const int jr = (int)opaque((unsigned)(wave * 32 + l32));  // the 8 swizzled offsets are formed here, not held
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int ic = a * 32 + 8 * g + 4 * hh;  // first of the lane's 4 consecutive ci
            const unsigned lo = pack_bf16x2(accd[a][4 * g], accd[a][4 * g + 1]);
            const unsigned hi = pack_bf16x2(accd[a][4 * g + 2], accd[a][4 * g + 3]);
            *reinterpret_cast<u32x2*>(ot + out_off(jr, ic >> 3) + 8 * ((ic >> 2) & 1)) = u32x2{lo, hi};
          }
        accd[0] = accd[1] = zero16();
        __syncthreads();
        // full-row 16-B stores of da2, and bn2's backward sums over what is stored (BNB); bn2's scale and
        // shift are reloaded per tile (cache hits) instead of held in 16 registers across the walk
        if constexpr (BNB) {
          float bs[8], bh[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            bs[e] = p.sc2[8 * c8 + e];
            bh[e] = p.sh2[8 * c8 + e];
          }
          const int64_t m0 = (int64_t)tile * kFBM;
          const int valid = (int)min((int64_t)kFBM, p.M - m0);
          char* bo = reinterpret_cast<char*>(p.da + m0 * kFC);
          const char* by2 = reinterpret_cast<const char*>(p.y2 + m0 * kFC);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int r = r8 + 32 * u;
            if (r < valid) {
              const unsigned off = opaque(((unsigned)r * kFC + 8 * c8) * 2u);
              const u32x4 v = *reinterpret_cast<const u32x4*>(ot + opaque((unsigned)out_off(r8, c8)) + 4096 * u);
              *reinterpret_cast<u32x4*>(bo + off) = v;
              const u32x4 yv = *reinterpret_cast<const u32x4*>(by2 + off);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                  const int k = 2 * e + hf;
                  const float g = hf ? bf16_hi(v[e]) : bf16_lo(v[e]);
                  const float yy = hf ? bf16_hi(yv[e]) : bf16_lo(yv[e]);
                  const float gm = yy * bs[k] + bh[k] > 0.f ? g : 0.f;
                  ssum[k] += gm;
                  ssq[k] += gm * yy;
                }
              }
            }
          }
        } else {
          const int64_t m0 = (int64_t)tile * kFBM;
          const int valid = (int)min((int64_t)kFBM, p.M - m0);
          char* bo = reinterpret_cast<char*>(p.da + m0 * kFC);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int r = r8 + 32 * u;
            if (r < valid)
              *reinterpret_cast<u32x4*>(bo + opaque(((unsigned)r * kFC + 8 * c8) * 2u)) =
                  *reinterpret_cast<const u32x4*>(ot + opaque((unsigned)out_off(r8, c8)) + 4096 * u);
          }
        }
      }
      if (!go) break;
      __syncthreads();  // next buffer filled; this one (or the da2 tile in it) fully consumed
      cur ^= 1;
    }
    if (!more) break;
    tile = ntile;
  }

  // this workgroup's dW3 slab (the thread indices are formed again, not carried in registers through the walk)
  const int t2 = (int)opaque(threadIdx.x), w2 = t2 >> 6, col2 = t2 & 31, h2 = (t2 >> 5) & 1;
  float* slab = p.slabs + (int64_t)blockIdx.x * kFW;
#pragma unroll
  for (int q = 0; q < kFC4 / 64; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      slab[(q * 64 + (w2 >> 1) * 32 + acc_row(r, h2)) * kFC + (w2 & 1) * 32 + col2] = accw[q][r];
  if constexpr (BNB) {
    // bn2's partial row: sum the 32 row groups through LDS
    __syncthreads();
    float* red = reinterpret_cast<float*>(dyt);  // [32][2][64]
    const int rg = t2 >> 3, cg = t2 & 7;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[(rg * 2) * kFC + 8 * cg + e] = ssum[e];
      red[(rg * 2 + 1) * kFC + 8 * cg + e] = ssq[e];
    }
    __syncthreads();
    if (t2 < 2 * kFC) {
      const int which = t2 / kFC, ii = t2 % kFC;
      float v = 0.f;
      for (int g = 0; g < 32; ++g) v += red[(g * 2 + which) * kFC + ii];
      p.partial[((int64_t)blockIdx.x * 2 + which) * kFC + ii] = v;
    }
  }
}

inline int fused_groups(int64_t M) {
  const int64_t tiles = (M + kFBM - 1) / kFBM;
  const int64_t want = tune().fwd_wg < 1 ? 1 : tune().fwd_wg;
  return (int)(tiles < want ? tiles : want);
}

}  // namespace conv
}  // namespace madnn

using namespace madnn::conv;

extern "C" {

// key 0: forward/dgrad grid target, 1: weight-grad workgroups, 2: XCD remap (0/1), 3: ring main loop (0/1),
// 4: deep forwards / plain data grad on K12P (0/1); returns the old value (value < 0: query only)
int madnn_conv1x1_tune(int key, int value) {
  int* f = key == 0   ? &tune().fwd_wg
           : key == 1 ? &tune().wgrad_wg
           : key == 2 ? &tune().xcd
           : key == 3 ? &tune().ring
           : key == 4 ? &tune().deep
                      : nullptr;
  if (f == nullptr) return -1;
  const int old = *f;
  if (value >= 0) *f = value;
  return old;
}

int madnn_conv1x1_supported(int64_t cin, int64_t cout) {
  return (cin % 64 == 0 && cout % 64 == 0 && cin >= 64 && cout >= 64 && cin <= 16384 && cout <= 16384) ? 1 : 0;
}

// partial-statistics rows the forward writes ([rows][2][cout] fp32)
int madnn_conv1x1_stat_rows(int64_t M, int64_t cin, int64_t cout) {
  if (!madnn_conv1x1_supported(cin, cout) || M <= 0) return 0;
  if (use_deep(M, cin, cout)) return madnn_conv1x1_fwd_p_rows(M, cout);
  GemmArgs p{};
  plan_persistent(p, M, fwd_bi(cin, cout), cout, cin);
  return p.j_groups;
}

// partial rows the BNB data grad writes ([rows][2][cin] fp32)
int madnn_conv1x1_dgrad_rows(int64_t M, int64_t cin, int64_t cout) {
  if (!madnn_conv1x1_supported(cin, cout) || M <= 0) return 0;
  GemmArgs p{};
  plan_persistent(p, M, cin % 128 == 0 ? 128 : 64, cin, cout);
  return p.j_groups;
}

hipError_t madnn_conv1x1_fwd(const void* x, const void* w, void* y, float* stats, int64_t M, int64_t cin,
                             int64_t cout, hipStream_t s) {
  if (!madnn_conv1x1_supported(cin, cout)) return hipErrorInvalidValue;
  if (M <= 0) return hipSuccess;
  if (use_deep(M, cin, cout)) return madnn_conv1x1_fwd_p(x, w, y, stats, M, cin, cout, s);
  GemmArgs p{};
  p.a = static_cast<const uint16_t*>(w);
  p.lda = cin;
  p.b = static_cast<const uint16_t*>(x);
  p.ldb = cin;
  p.out = y;
  p.ldo = cout;
  p.stats = stats;
  p.xcd = tune().xcd;
  p.I = cout;
  p.J = M;
  p.K = cin;
  const bool wide = fwd_bi(cin, cout) == 128;
  plan_persistent(p, M, wide ? 128 : 64, cout, cin);
  const int grid = p.i_tiles * p.j_groups;
  const bool ring = use_ring(false, wide ? 128 : 64, cin);
  if (wide) {
    if (ring) return stats ? launch_ring<false, 128, true>(p, grid, s) : launch_ring<false, 128, false>(p, grid, s);
    return stats ? launch<false, false, 128, 128, kStoreT, true>(p, grid, s)
                 : launch<false, false, 128, 128, kStoreT, false>(p, grid, s);
  }
  if (ring) return stats ? launch_ring<false, 64, true>(p, grid, s) : launch_ring<false, 64, false>(p, grid, s);
  return stats ? launch<false, false, 64, 128, kStoreT, true>(p, grid, s)
               : launch<false, false, 64, 128, kStoreT, false>(p, grid, s);
}

// dx = dY W (+ res: an accumulated gradient of the same layout, added in the epilogue)
// bny/bnsc/bnsh/partial (optional, all or none): dx is d relu(bn(bny)); the epilogue also writes bn's
// backward sums as partial [madnn_conv1x1_dgrad_rows][2][cin] (see BNB)
// resmask (with res): res counts only where its ReLU bit is set
hipError_t madnn_conv1x1_dgrad(const void* dy, const void* w, void* dx, const void* res, int64_t M, int64_t cin,
                               int64_t cout, const void* bny, const float* bnsc, const float* bnsh, float* partial,
                               hipStream_t s, const unsigned char* resmask) {
  if (!madnn_conv1x1_supported(cin, cout)) return hipErrorInvalidValue;
  if (M <= 0) return hipSuccess;
  if (res == nullptr && bny == nullptr && use_deep(M, cin, cout, true))
    return madnn_linear_dgrad_p(dy, w, nullptr, dx, nullptr, M, cout, cin, 1, s);
  GemmArgs p{};
  p.a = static_cast<const uint16_t*>(w);  // A[i = ci][k = co] = W[co][ci]: column memory
  p.lda = cin;
  p.b = static_cast<const uint16_t*>(dy);  // B[k = co][j = m] = dY[m][co]: row memory
  p.ldb = cout;
  p.out = dx;
  p.res = static_cast<const uint16_t*>(res);
  p.resmask = res != nullptr ? resmask : nullptr;
  p.xcd = tune().xcd;
  p.ldo = cin;
  p.I = cin;
  p.J = M;
  p.K = cout;
  const bool wide = cin % 128 == 0;
  plan_persistent(p, M, wide ? 128 : 64, cin, cout);
  const int grid = p.i_tiles * p.j_groups;
  const bool ring = use_ring(true, wide ? 128 : 64, cout);
  if (bny != nullptr) {
    if (partial == nullptr || bnsc == nullptr || bnsh == nullptr || res != nullptr) return hipErrorInvalidValue;
    p.bny = static_cast<const uint16_t*>(bny);
    p.bnsc = bnsc;
    p.bnsh = bnsh;
    p.stats = partial;
    if (ring) return launch_ring<true, 128, false, true>(p, grid, s);
    return wide ? launch<true, false, 128, 128, kStoreT, false, true>(p, grid, s)
                : launch<true, false, 64, 128, kStoreT, false, true>(p, grid, s);
  }
  if (ring) return launch_ring<true, 128, false>(p, grid, s);
  return wide ? launch<true, false, 128, 128, kStoreT, false>(p, grid, s)
              : launch<true, false, 64, 128, kStoreT, false>(p, grid, s);
}

// fp32 floats of workspace madnn_conv1x1_wgrad needs (the per-split partial slabs)
int64_t madnn_conv1x1_wgrad_ws(int64_t M, int64_t cin, int64_t cout) {
  int bi, bj, kc;
  int64_t tiles, splits;
  wgrad_split(M, cin, cout, bi, bj, tiles, kc, splits);
  return splits * cin * cout;
}

// dw: [cout][cin] fp32 or (dw_bf16) bf16; ws: madnn_conv1x1_wgrad_ws floats (the per-split partial
// slabs, summed in split order into dw -- one pass that also casts)
hipError_t madnn_conv1x1_wgrad(const void* dy, const void* x, void* dw, int dw_bf16, float* ws, int64_t M, int64_t cin,
                               int64_t cout, hipStream_t s) {
  if (!madnn_conv1x1_supported(cin, cout)) return hipErrorInvalidValue;
  if (M <= 0) return hipMemsetAsync(dw, 0, (size_t)(cin * cout) * (dw_bf16 ? 2 : 4), s);
  GemmArgs p{};
  p.a = static_cast<const uint16_t*>(dy);  // A[i = co][k = m] = dY[m][co]: column memory
  p.lda = cout;
  p.b = static_cast<const uint16_t*>(x);  // B[k = m][j = ci] = X[m][ci]: column memory
  p.ldb = cin;
  p.xcd = tune().xcd;
  p.ldo = cin;
  p.I = cout;
  p.J = cin;
  p.K = M;
  int bi, bj;
  int64_t tiles, splits;
  wgrad_split(M, cin, cout, bi, bj, tiles, p.k_chunk, splits);
  if (ws == nullptr) return hipErrorInvalidValue;
  p.out = ws;
  p.i_tiles = (int)(cout / bi);
  p.j_tiles = (int)(cin / bj);
  const int grid = (int)(tiles * splits);
  p.j_groups = 0;
  hipError_t e;
  if (bi == 128 && bj == 128) e = launch<true, true, 128, 128, kSplit, false>(p, grid, s);
  else if (bi == 128) e = launch<true, true, 128, 64, kSplit, false>(p, grid, s);
  else if (bj == 128) e = launch<true, true, 64, 128, kSplit, false>(p, grid, s);
  else e = launch<true, true, 64, 64, kSplit, false>(p, grid, s);
  if (e != hipSuccess) return e;
  const int64_t n = cin * cout;
  const int64_t blocks = (n / 4 + 255) / 256;
  const dim3 grid_r((unsigned)(blocks < 4 * madnn::kNumCU ? blocks : 4 * madnn::kNumCU));
  if (dw_bf16) {
    hipLaunchKernelGGL(split_reduce_kernel<true>, grid_r, dim3(256), 0, s, ws, (int)splits, n, dw);
  } else {
    hipLaunchKernelGGL(split_reduce_kernel<false>, grid_r, dim3(256), 0, s, ws, (int)splits, n, dw);
  }
  return hipGetLastError();
}

// K9F (bn3_conv3_bwd_kernel): the shapes it is built for
int madnn_bn3_conv3_bwd_supported(int64_t c, int64_t c4) { return (c == kFC && c4 == kFC4) ? 1 : 0; }

// workgroups = bn2 partial rows ([rows][2][C]) = dW3 slabs ([rows][4C][C] fp32 of workspace)
int madnn_bn3_conv3_bwd_groups(int64_t M) { return M > 0 ? fused_groups(M) : 0; }

// K9F launch.  y / coef / w / a: the BatchNorm input, its ca | cb | cc ([3][4C], bn_bwd_finalize_kernel), the
// weight and the convolution input -- bn3's set (y3, W3, a2) or the downsample path's (yd, W_ds, xf).
// y2 / sc2 / sh2 / partial all given: da is d relu(bn2(y2)) and partial gets bn2's backward sums (BNB); all
// null: da is stored plainly.  partial / slabs: madnn_bn3_conv3_bwd_groups rows;
// dw: [4C][C] fp32 or (dw_bf16) bf16, the slabs summed in workgroup order
hipError_t madnn_bn3_conv3_bwd(const void* dout, const void* y, const unsigned char* mask, const float* coef,
                               const void* w, const void* a, const void* y2, const float* sc2, const float* sh2,
                               void* da, float* partial, float* slabs, void* dw, int dw_bf16, int64_t M, int64_t c,
                               int64_t c4, hipStream_t s) {
  if (!madnn_bn3_conv3_bwd_supported(c, c4) || M <= 0) return hipErrorInvalidValue;
  const bool bnb = y2 != nullptr;
  if (bnb != (sc2 != nullptr) || bnb != (sh2 != nullptr) || bnb != (partial != nullptr)) return hipErrorInvalidValue;
  FusedArgs p{};
  p.dout = static_cast<const uint16_t*>(dout);
  p.y = static_cast<const uint16_t*>(y);
  p.mask = mask;
  p.coef = coef;
  p.w = static_cast<const uint16_t*>(w);
  p.a = static_cast<const uint16_t*>(a);
  p.y2 = static_cast<const uint16_t*>(y2);
  p.sc2 = sc2;
  p.sh2 = sh2;
  p.da = static_cast<uint16_t*>(da);
  p.partial = partial;
  p.slabs = slabs;
  p.M = M;
  p.m_tiles = (int)((M + kFBM - 1) / kFBM);
  const int grid = fused_groups(M);
  if (bnb) {
    hipLaunchKernelGGL(bn3_conv3_bwd_kernel<true>, dim3(grid), dim3(kThreads), 0, s, p);
  } else {
    hipLaunchKernelGGL(bn3_conv3_bwd_kernel<false>, dim3(grid), dim3(kThreads), 0, s, p);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t n = kFW;
  const dim3 grid_r((unsigned)((n / 4 + 255) / 256));
  if (dw_bf16) {
    hipLaunchKernelGGL(split_reduce_kernel<true>, grid_r, dim3(256), 0, s, slabs, grid, n, dw);
  } else {
    hipLaunchKernelGGL(split_reduce_kernel<false>, grid_r, dim3(256), 0, s, slabs, grid, n, dw);
  }
  return hipGetLastError();
}

}  // extern "C"
