// W8A8 projection: block-scaled OCP e4m3 weights x per-(token, 128-column group) e4m3 activations on the FP8 matrix
// instruction (v_mfma_f32_16x16x128_f8f6f4: one instruction contracts exactly one 128-k scale block), both scale grids
// applied in fp32.  This is how the published FP8 checkpoints define inference (activation_scheme "dynamic",
// weight_block_size [128, 128]):
//     sx[m, b]  = max(amax_{k in block b} |x[m, k]|, FLT_MIN) / 448                (fp32, correctly rounded division)
//     xq[m, k]  = e4m3_rne(float(x[m, k]) / sx[m, k / 128])                        (fp32 division, round to nearest even)
//     out[m, n] = round_bf16( sum_b sx[m, b] * sw[n / 128, b] * sum_{k in block b} float(xq[m, k]) * float(q[n, k]) )
// The inner sum of a block is ONE MFMA that starts from zero (exact products, fp32 sum); it enters the running fp32 sum
// through one FMA with the combined scale sx * sw.  No operand is ever rounded after scaling.
//
// msgl_a8_quant (a8_quant_kernel): 16 lanes own one 128-column group.  A lane reads 16 B (8 bf16), the amax goes over the
// 16 lanes by DPP, one IEEE division per element, v_cvt_pk_fp8_f32 (round to nearest even) after a clamp to +-448 (the
// quotient can exceed 448 by an ulp; the NaN encoding is never produced), 8 B stored per lane, lane 0 of the group stores sx.
//
// msgl_w8a8_gemm_nt (w8a8_gemm_kernel): the work split of gemm_w8_tall.hip with both operands at one byte per element.
//   * grid = (N / 128) x ceil(M / TM) x k_slices, workgroup = 4 waves, TM = 128 or 256;
//   * weights never pass through LDS and are never converted: wave w owns weight rows [32 w, 32 w + 32) as two 16-row units.
//     Per block, lane (r = l & 15, kg = l >> 4) loads q[n0 + 16 i + r, 128 b + 32 kg .. + 31] (two 16-B loads: whole 128-B
//     lines) and those 8 dwords ARE the MFMA A operand; the loads of block b + 1 are issued before the MFMAs of block b;
//   * xq goes global -> LDS by DMA (global_load_lds_dwordx4) into two stages of TM rows x 128 B (one block).  A wave
//     instruction fills 1 KB = 8 rows lane-linearly, so the swizzle is on the SOURCE side: the lane that lands on 16-B slot
//     s of row r fetches column s ^ ((r >> 1) & 7).  Two neighbouring rows fill one 256-B bank span, so the 16 rows of a
//     fragment read (lane (r, kg), h = 0, 1: row 16 t + r, column 2 kg + h, one 16-B LDS load each) fall into 16 different
//     bank groups.  The B operand of lane (r, kg) is bytes 32 kg .. 32 kg + 31 of its row: the same k -> (lane, byte) mapping
//     as the weights, so the instruction's own k order does not matter;
//   * sx of the stage's rows and block rides along (global_load_lds_dword, TM x 4 B per stage); lane (r, kg) needs one value
//     per 16-row tile: s = sx * sw (sw: one scalar load per block for the workgroup), then acc = fma(s, part, acc);
//   * x is the B operand, so an accumulator lane (r, kg) holds out[m0 + 16 t + r, n0 + 16 i + 4 kg .. + 3] and its sx value is
//     the same for all four; M tiles are taken in pairs: four independent MFMAs (2 tiles x 2 units) in flight;
//   * rows at or above M issue no DMA, their LDS rows are zeroed once; M tiles wholly at or above M are skipped;
//   * one barrier per block, as in the tall kernel; LDS = 2 x TM x 132 B.  TM = 128: 33 KB, two workgroups per CU (two
//     waves per SIMD); TM = 256: 66 KB, and its 128 accumulator registers leave room for one workgroup per CU;
//   * k_slices > 1: slice s takes blocks [s nblk / S, (s + 1) nblk / S) and writes an fp32 slab [M][N] into the caller's
//     workspace; w8a8_reduce_kernel adds the slabs in slice order and rounds.  Deterministic, no atomics.
#include <float.h>

#include "common.h"

namespace msgl {

typedef int a8_i8 __attribute__((ext_vector_type(8)));
typedef float a8_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t a8_u4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void a8_lds_t;
typedef __attribute__((address_space(1))) const void a8_glb_t;

constexpr int kA8TileN = 128;    // weight rows per workgroup = one scale row group
constexpr int kA8Block = 128;    // k per scale block = bytes of one weight line = bytes of one staged xq row
constexpr int kA8Waves = 4;
constexpr int kA8MaxSlices = 64;
constexpr float kA8Max = 448.0f;  // largest finite e4m3

// ---------------------------------------------------------------------------- activation quantiser
__global__ __launch_bounds__(256) void a8_quant_kernel(uint8_t* __restrict__ xq, float* __restrict__ sx,
                                                       const uint16_t* __restrict__ x, uint32_t groups, uint32_t nblk,
                                                       int64_t ldx, int64_t ldxq) {
  const uint32_t g = (blockIdx.x * 256u + threadIdx.x) >> 4;  // the 128-column group of these 16 lanes
  const bool live = g < groups;                               // whole groups: the DPP rows below never mix live and dead
  const uint32_t gg = live ? g : 0u;
  const uint32_t m = gg / nblk, b = gg - m * nblk;
  const int sub = threadIdx.x & 15;
  const int64_t col = (int64_t)b * kA8Block + sub * 8;
  float f[8];
  unpack8<BF16>(ldg16(x + (int64_t)m * ldx + col), f);
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) a = fmaxf(a, fabsf(f[i]));
  a = fmaxf(a, dpp_mov<kDppXor1>(a));
  a = fmaxf(a, dpp_mov<kDppXor2>(a));
  a = fmaxf(a, dpp_mov<kDppHalfMirror>(a));
  a = fmaxf(a, dpp_mov<kDppRowMirror>(a));
  const float s = fmaxf(a, FLT_MIN) / kA8Max;
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = __builtin_amdgcn_fmed3f(f[i] / s, -kA8Max, kA8Max);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
  if (live) {
    *reinterpret_cast<uint2*>(xq + (int64_t)m * ldxq + col) = uint2{(uint32_t)lo, (uint32_t)hi};
    if (sub == 0) sx[g] = s;
  }
}

// ---------------------------------------------------------------------------- FP8 x FP8 GEMM
// SLABS: write fp32 into part[blockIdx.z][M][N] instead of bf16 into out.
template <int TM, bool SLABS>
__global__ __launch_bounds__(64 * kA8Waves, TM == 128 ? 2 : 1) void w8a8_gemm_kernel(
    uint16_t* __restrict__ out, float* __restrict__ part, const uint8_t* __restrict__ xq, const float* __restrict__ sx,
    const uint8_t* __restrict__ q, const float* __restrict__ sw, int M, int N, int nblk, int64_t ldxq, int64_t ldq,
    int64_t ldo) {
  constexpr int kStage = TM * kA8Block;          // xq bytes of one stage
  constexpr int kPieces = TM / (8 * kA8Waves);   // DMA instructions (8 rows each) per wave per block
  constexpr int kPairs = TM / 32;                // pairs of 16-row M tiles
  __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * kStage];
  __shared__ __attribute__((aligned(256))) float ssx[2 * TM];
  const int lane = threadIdx.x & 63, wave = sgpr(threadIdx.x >> 6);
  const int r = lane & 15, kg = lane >> 4;
  const int m0 = blockIdx.y * TM;
  const int live = M - m0;  // rows of this M tile that exist (>= 1)
  const int S = gridDim.z, slice = blockIdx.z;
  const int b0 = (int)((int64_t)slice * nblk / S), b1 = (int)((int64_t)(slice + 1) * nblk / S);

  // weights: lane (r, kg) of unit i reads q[n0 + 32 wave + 16 i + r, 128 b + 32 kg .. + 31]
  const int64_t n0 = (int64_t)blockIdx.x * kA8TileN + wave * 32;
  const uint8_t* qp = q + (n0 + r) * ldq + kg * 32;
  const float* sp = sw + (int64_t)blockIdx.x * nblk;

  // xq DMA: piece i of this wave = stage rows 32 i + 8 wave + (0 .. 7); this lane lands on slot (lane & 7) of row
  // drow + 32 i and fetches column (lane & 7) ^ ((row >> 1) & 7), (row >> 1) & 7 = (drow >> 1) & 7
  const int drow = 8 * wave + (lane >> 3);
  const uint8_t* xsrc = xq + ((int64_t)m0 + drow) * ldxq + (((lane & 7) ^ ((drow >> 1) & 7)) * 16);
  const int64_t xstep = 32 * ldxq;  // bytes from piece i to piece i + 1
  // sx DMA: wave w brings the scales of stage rows 64 w + lane (one dword per lane)
  const int srow = 64 * wave + lane;
  const float* ssrc = sx + ((int64_t)m0 + srow) * nblk;

  // fragment read offsets within a stage: row r of M tile 0, column 2 kg + h at slot (2 kg + h) ^ ((r >> 1) & 7)
  int fo[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) fo[h] = r * kA8Block + (((2 * kg + h) ^ ((r >> 1) & 7)) * 16);

  // rows at or above M are never written by the DMA: zero them once, in both stages
#pragma unroll
  for (int i = 0; i < kPieces; ++i) {
    if (drow + 32 * i >= live) {
      const int off = (drow + 32 * i) * kA8Block + (lane & 7) * 16;
      *reinterpret_cast<a8_u4*>(smem + off) = a8_u4{0u, 0u, 0u, 0u};
      *reinterpret_cast<a8_u4*>(smem + kStage + off) = a8_u4{0u, 0u, 0u, 0u};
    }
  }
  if ((int)threadIdx.x < TM && (int)threadIdx.x >= live) ssx[threadIdx.x] = ssx[TM + threadIdx.x] = 0.f;

  auto load_w = [&](a8_u4 (&raw)[2][2], int b) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint8_t* p = qp + (int64_t)i * 16 * ldq + (int64_t)b * kA8Block;
      raw[i][0] = *reinterpret_cast<const a8_u4*>(p);
      raw[i][1] = *reinterpret_cast<const a8_u4*>(p + 16);
    }
  };
  auto issue_x = [&](int b, int buf) __attribute__((always_inline)) {
    unsigned char* sb = smem + buf * kStage + 8 * wave * kA8Block;
    const uint8_t* src = xsrc + (int64_t)b * kA8Block;
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      if (32 * i + 8 * wave < live) {  // wave-uniform: pieces wholly at or above M issue nothing
        if (drow + 32 * i < live)
          __builtin_amdgcn_global_load_lds((a8_glb_t*)(src + i * xstep), (a8_lds_t*)(sb + i * 32 * kA8Block), 16, 0, 0);
      }
    }
    if (64 * wave < TM && 64 * wave < live) {  // wave-uniform
      if (srow < live) __builtin_amdgcn_global_load_lds((a8_glb_t*)(ssrc + b), (a8_lds_t*)(ssx + buf * TM + 64 * wave), 4, 0, 0);
    }
  };

  a8_f32x4 acc[2][TM / 16];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < TM / 16; ++t) acc[i][t] = a8_f32x4{0.f, 0.f, 0.f, 0.f};

  a8_u4 raw[2][2], nxt[2][2];
  load_w(raw, b0);
  issue_x(b0, 0);
  int buf = 0;
  for (int b = b0; b < b1; ++b) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of block b (and its weight lines) have landed
    __syncthreads();                                  // stage buf is whole; every wave is done with stage buf ^ 1
    if (b + 1 < b1) {                                 // wave-uniform
      load_w(nxt, b + 1);
      issue_x(b + 1, buf ^ 1);
    }
    const float sc = sp[b];
    a8_i8 a[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
      a[i] = a8_i8{(int)raw[i][0].x, (int)raw[i][0].y, (int)raw[i][0].z, (int)raw[i][0].w,
                   (int)raw[i][1].x, (int)raw[i][1].y, (int)raw[i][1].z, (int)raw[i][1].w};
    const unsigned char* sb = smem + buf * kStage;
    const float* sxs = ssx + buf * TM + r;
#pragma unroll
    for (int tp = 0; tp < kPairs; ++tp) {
      if (tp * 32 >= live) break;  // wave-uniform
      a8_i8 bv[2];
      float s[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const unsigned char* row = sb + (2 * tp + u) * 16 * kA8Block;
        const a8_u4 v0 = *reinterpret_cast<const a8_u4*>(row + fo[0]);
        const a8_u4 v1 = *reinterpret_cast<const a8_u4*>(row + fo[1]);
        bv[u] = a8_i8{(int)v0.x, (int)v0.y, (int)v0.z, (int)v0.w, (int)v1.x, (int)v1.y, (int)v1.z, (int)v1.w};
        s[u] = sxs[(2 * tp + u) * 16] * sc;
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          // both formats e4m3 (cbsz = blgp = 0); all-zero scale operands select the unscaled instruction
          const a8_f32x4 pr = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], bv[u], a8_f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0,
                                                                                0, 0, 0, 0);
          a8_f32x4& c = acc[i][2 * tp + u];
          c.x = fmaf(s[u], pr.x, c.x);
          c.y = fmaf(s[u], pr.y, c.y);
          c.z = fmaf(s[u], pr.z, c.z);
          c.w = fmaf(s[u], pr.w, c.w);
        }
    }
    if (b + 1 < b1) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        raw[i][0] = nxt[i][0];
        raw[i][1] = nxt[i][1];
      }
    }
    buf ^= 1;
  }

  // lane (r, kg) holds out[m0 + 16 t + r, n0 + 16 i + 4 kg .. + 3]
#pragma unroll
  for (int t = 0; t < TM / 16; ++t) {
    const int m = t * 16 + r;
    if (m < live) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const a8_f32x4 v = acc[i][t];
        const int64_t col = n0 + i * 16 + kg * 4;
        if (SLABS) {
          *reinterpret_cast<a8_f32x4*>(part + ((int64_t)slice * M + m0 + m) * N + col) = v;
        } else {
          uint2 pk;
          pk.x = Elem<BF16>::pack(v.x, v.y);
          pk.y = Elem<BF16>::pack(v.z, v.w);
          *reinterpret_cast<uint2*>(out + ((int64_t)m0 + m) * ldo + col) = pk;
        }
      }
    }
  }
}

// out[m][c] = round_bf16(sum_s part[s][m][c]), slabs added in slice order; 4 columns per thread
__global__ __launch_bounds__(256) void w8a8_reduce_kernel(uint16_t* __restrict__ out, const float* __restrict__ part, int M,
                                                          int N, int S, int64_t ldo) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per_row = N >> 2;
  if (gid >= (int64_t)M * per_row) return;
  const int m = (int)(gid / per_row), c = (int)(gid - (int64_t)m * per_row) * 4;
  const float* p = part + (int64_t)m * N + c;
  float4 v = *reinterpret_cast<const float4*>(p);
  for (int s = 1; s < S; ++s) {
    const float4 o = *reinterpret_cast<const float4*>(p + (int64_t)s * M * N);
    v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
  }
  uint2 pk;
  pk.x = Elem<BF16>::pack(v.x, v.y);
  pk.y = Elem<BF16>::pack(v.z, v.w);
  *reinterpret_cast<uint2*>(out + (int64_t)m * ldo + c) = pk;
}

template <int TM>
static void launch_w8a8(uint16_t* out, float* part, const uint8_t* xq, const float* sx, const uint8_t* q, const float* sw,
                        int M, int N, int K, int64_t ldxq, int64_t ldq, int64_t ldo, int k_slices, hipStream_t st) {
  const dim3 grid((unsigned)(N / kA8TileN), (unsigned)((M + TM - 1) / TM), (unsigned)k_slices), block(64 * kA8Waves);
  if (k_slices == 1) {
    w8a8_gemm_kernel<TM, false><<<grid, block, 0, st>>>(out, part, xq, sx, q, sw, M, N, K / kA8Block, ldxq, ldq, ldo);
  } else {
    w8a8_gemm_kernel<TM, true><<<grid, block, 0, st>>>(out, part, xq, sx, q, sw, M, N, K / kA8Block, ldxq, ldq, ldo);
    const int64_t threads = (int64_t)M * (N / 4);
    w8a8_reduce_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(out, part, M, N, k_slices, ldo);
  }
}

}  // namespace msgl

using namespace msgl;

extern "C" int msgl_a8_quant(void* xq, float* sx, const void* x, int M, int K, int64_t ldx, int64_t ldxq, int dtype,
                             void* stream) {
  MSGL_REQUIRE(xq && sx && x, "a8_quant: null pointer");
  MSGL_REQUIRE(dtype == MSGL_BF16, "a8_quant: activations must be bf16 (dtype code %d)", dtype);
  MSGL_REQUIRE(M >= 1 && K >= 128 && K % 128 == 0, "a8_quant: M = %d, K = %d (K a multiple of the 128-column group)", M, K);
  MSGL_REQUIRE(ldx >= K && ldxq >= K && ldx % 8 == 0 && ldxq % 16 == 0, "a8_quant: leading dimensions (%lld, %lld)",
               (long long)ldx, (long long)ldxq);
  MSGL_REQUIRE(aligned16(x) && aligned16(xq) && (reinterpret_cast<uintptr_t>(sx) & 3u) == 0,
               "a8_quant: x, xq must be 16-byte and sx 4-byte aligned");
  const int64_t groups = (int64_t)M * (K / 128);
  MSGL_REQUIRE(groups <= 0x0fffffffll, "a8_quant: M x K = %d x %d is more than 2^28 - 1 groups", M, K);
  a8_quant_kernel<<<dim3((unsigned)((groups + 15) / 16)), dim3(256), 0, static_cast<hipStream_t>(stream)>>>(
      (uint8_t*)xq, sx, (const uint16_t*)x, (uint32_t)groups, (uint32_t)(K / 128), ldx, ldxq);
  MSGL_CHECK_LAUNCH("a8_quant");
  return MSGL_OK;
}

extern "C" int64_t msgl_w8a8_workspace_bytes(int M, int N, int k_slices) {
  if (M < 1 || N < kA8TileN || N % kA8TileN || k_slices < 1 || k_slices > kA8MaxSlices) return MSGL_EINVAL;
  if (k_slices == 1) return 0;
  return (int64_t)k_slices * M * (int64_t)N * (int64_t)sizeof(float);
}

extern "C" int msgl_w8a8_gemm_nt(void* out, const void* xq, const float* sx, const void* q, const float* scales, int M, int N,
                                 int K, int64_t ldxq, int64_t ldq, int64_t ldo, int dtype, int tm, int k_slices,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  MSGL_REQUIRE(out && xq && sx && q && scales, "w8a8_gemm_nt: null pointer");
  MSGL_REQUIRE(dtype == MSGL_BF16, "w8a8_gemm_nt: the output must be bf16 (dtype code %d)", dtype);
  MSGL_REQUIRE(M >= 1, "w8a8_gemm_nt: M = %d", M);
  MSGL_REQUIRE(N >= 128 && N % 128 == 0 && K >= 128 && K % 128 == 0,
               "w8a8_gemm_nt: N = %d and K = %d must be multiples of the 128 x 128 scale block", N, K);
  MSGL_REQUIRE(tm == 128 || tm == 256, "w8a8_gemm_nt: tm %d (128, 256)", tm);
  MSGL_REQUIRE(k_slices >= 1 && k_slices <= K / 128 && k_slices <= kA8MaxSlices,
               "w8a8_gemm_nt: %d k-slices outside [1, min(K / 128 = %d, %d)]", k_slices, K / 128, kA8MaxSlices);
  MSGL_REQUIRE((M + tm - 1) / tm <= 65535, "w8a8_gemm_nt: M = %d is more than 65535 tiles of %d rows", M, tm);
  MSGL_REQUIRE(ldxq >= K && ldq >= K && ldo >= N && ldxq % 16 == 0 && ldq % 16 == 0 && ldo % 4 == 0,
               "w8a8_gemm_nt: leading dimensions (%lld, %lld, %lld)", (long long)ldxq, (long long)ldq, (long long)ldo);
  MSGL_REQUIRE(aligned16(xq) && aligned16(q) && (reinterpret_cast<uintptr_t>(out) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(sx) & 3u) == 0 && (reinterpret_cast<uintptr_t>(scales) & 3u) == 0,
               "w8a8_gemm_nt: xq, q must be 16-byte, out 8-byte and sx, scales 4-byte aligned");
  const int64_t need = msgl_w8a8_workspace_bytes(M, N, k_slices);
  if (need > 0) {
    MSGL_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= need,
                 "w8a8_gemm_nt: %d k-slices need %lld bytes of 16-byte aligned workspace (got %lld)", k_slices,
                 (long long)need, (long long)workspace_bytes);
    MSGL_REQUIRE((int64_t)M * (N / 4) <= 0x7fffffffll * 256, "w8a8_gemm_nt: M x N = %d x %d is too large to k-slice", M, N);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (tm == 128)
    launch_w8a8<128>((uint16_t*)out, (float*)workspace, (const uint8_t*)xq, sx, (const uint8_t*)q, scales, M, N, K, ldxq, ldq,
                     ldo, k_slices, s);
  else
    launch_w8a8<256>((uint16_t*)out, (float*)workspace, (const uint8_t*)xq, sx, (const uint8_t*)q, scales, M, N, K, ldxq, ldq,
                     ldo, k_slices, s);
  MSGL_CHECK_LAUNCH("w8a8_gemm_nt");
  return MSGL_OK;
}
