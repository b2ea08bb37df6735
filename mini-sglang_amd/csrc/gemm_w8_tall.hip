// Tall-tile W8A16 projection GEMM: block-scaled OCP e4m3 weights, bf16 activations, fp32 accumulate, any M >= 1:
//     out[m, n] = round_bf16( sum_b s[n / 128, b] * sum_{k in block b} x[m, k] * float(q[n, k]) )
// The contract and the numerics of csrc/gemm_w8.hip (exact e4m3 -> bf16, the MFMAs of a block start from zero, one fp32 FMA
// with the block scale, a scaled weight is never rounded); the work split is the opposite one.  There every workgroup
// restages all of x for 16 - 64 weight rows; here a workgroup owns 128 weight rows (one scale row group) x TM rows of x, so a
// staged activation byte meets 128 weight rows and a weight byte meets TM activation rows.
//
// Layout and work split
//   * grid = (N / 128) x ceil(M / TM) x k_slices, workgroup = 4 waves (one per SIMD), TM = 128 or 256;
//   * weights never pass through LDS: wave w owns weight rows [32 w, 32 w + 32) of the tile as two 16-row units.  Per 128-k
//     block, lane (r = l & 15, kg = l >> 4) loads q[n0 + 16 i + r, 128 b + 32 kg .. + 31] (two 16-B loads per unit: whole 128-B
//     lines), converts them once with v_cvt_scalef32_pk_bf16_fp8 (scale 1.0) into four MFMA A operands per unit and keeps them
//     while it walks all TM / 16 M tiles.  The loads of block b + 1 are issued before the MFMAs of block b;
//   * x goes global -> LDS by DMA (global_load_lds_dwordx4: no staging registers, no ds_write) into TWO stages of TM rows x
//     256 B (one 128-k block): 2 x 64 KB at TM = 256 (one workgroup per CU), 2 x 32 KB at TM = 128 (two per CU).  A wave
//     instruction fills 1 KB = 4 rows lane-linearly, so the swizzle is applied on the SOURCE side: the lane that lands on
//     16-B slot s of row r fetches column s ^ (r & 15).  A fragment read (lane (r, kg), step h: row 16 t + r, column 4 kg + h)
//     is one 16-B LDS load; the 16 rows of a lane group fall into 16 different bank groups;
//   * rows at or above M: their lanes issue no DMA and their LDS rows are zeroed once before the loop (zero columns of the B
//     operand); M tiles that lie wholly at or above M are skipped; nothing is stored for m >= M;
//   * one barrier per block: wait for the own DMA pieces of block b, barrier (stage b & 1 is visible, stage (b + 1) & 1 is
//     free), issue weight loads and DMA of block b + 1, then the MFMAs of block b;
//   * accumulators: 2 units x TM / 16 tiles x 4 fp32.  The per-block partial sums are transient: M tiles are taken in pairs,
//     four independent MFMA chains (2 tiles x 2 units) of four v_mfma_f32_16x16x32_bf16 each, every x fragment feeds two
//     MFMAs, then acc = fma(scale, part, acc).  The scale is one scalar load per block for the whole workgroup;
//   * k_slices > 1 (small tile grids): slice s takes blocks [s nblk / S, (s + 1) nblk / S) and writes an fp32 slab [M][N] into
//     the caller's workspace; w8_tall_reduce_kernel adds the slabs in slice order and rounds.  Deterministic, no atomics.
#include "common.h"

namespace msgl {

typedef __bf16 w8t_bf16x8 __attribute__((ext_vector_type(8)));
typedef float w8t_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t w8t_u4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void w8t_lds_t;
typedef __attribute__((address_space(1))) const void w8t_glb_t;

constexpr int kW8TTileN = 128;    // weight rows per workgroup = one scale row group
constexpr int kW8TBlock = 128;    // k per scale block = bytes of one weight line
constexpr int kW8TRowBytes = 256; // one staged x row: 128 k of bf16 = 16 columns of 16 B
constexpr int kW8TWaves = 4;
constexpr int kW8TMaxSlices = 64;

// four e4m3 bytes -> four bf16 (exact)
__device__ __forceinline__ void w8t_cvt4(uint32_t v, uint32_t& lo, uint32_t& hi) {
  lo = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v, 1.0f, false));
  hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v, 1.0f, true));
}

// SLABS: write fp32 into part[blockIdx.z][M][N] instead of bf16 into out.
template <int TM, bool SLABS>
__global__ __launch_bounds__(64 * kW8TWaves) void w8_tall_gemm_kernel(
    uint16_t* __restrict__ out, float* __restrict__ part, const uint16_t* __restrict__ x, const uint8_t* __restrict__ q,
    const float* __restrict__ scales, int M, int N, int nblk, int64_t ldx, int64_t ldq, int64_t ldo) {
  constexpr int kStage = TM * kW8TRowBytes;
  constexpr int kPieces = TM / (4 * kW8TWaves);  // DMA instructions (4 rows each) per wave per block
  constexpr int kPairs = TM / 32;                // pairs of 16-row M tiles
  __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * kStage];
  const int lane = threadIdx.x & 63, wave = sgpr(threadIdx.x >> 6);
  const int r = lane & 15, kg = lane >> 4;
  const int m0 = blockIdx.y * TM;
  const int live = M - m0;  // rows of this M tile that exist (>= 1)
  const int S = gridDim.z, slice = blockIdx.z;
  const int b0 = (int)((int64_t)slice * nblk / S), b1 = (int)((int64_t)(slice + 1) * nblk / S);

  // weights: lane (r, kg) of unit i reads q[n0 + 32 wave + 16 i + r, 128 b + 32 kg .. + 31]
  const int64_t n0 = (int64_t)blockIdx.x * kW8TTileN + wave * 32;
  const uint8_t* qp = q + (n0 + r) * ldq + kg * 32;
  const float* sp = scales + (int64_t)blockIdx.x * nblk;

  // x DMA: piece i of this wave = stage rows 16 i + 4 wave + (0 .. 3); this lane lands on slot (lane & 15) of row
  // drow + 16 i and fetches column (lane & 15) ^ (row & 15), row & 15 = drow
  const int drow = 4 * wave + kg;
  const unsigned char* xsrc = reinterpret_cast<const unsigned char*>(x) + ((int64_t)m0 + drow) * ldx * 2 + ((r ^ drow) * 16);
  const int64_t xstep = 16 * ldx * 2;  // bytes from piece i to piece i + 1

  // fragment read offsets within a stage: row r of M tile 0, column 4 kg + h at slot (4 kg + h) ^ r
  int fo[4];
#pragma unroll
  for (int h = 0; h < 4; ++h) fo[h] = r * kW8TRowBytes + (((4 * kg + h) ^ r) * 16);

  // rows at or above M are never written by the DMA: zero them once, in both stages
#pragma unroll
  for (int i = 0; i < kPieces; ++i) {
    if (drow + 16 * i >= live) {
      const int off = (drow + 16 * i) * kW8TRowBytes + r * 16;
      *reinterpret_cast<w8t_u4*>(smem + off) = w8t_u4{0u, 0u, 0u, 0u};
      *reinterpret_cast<w8t_u4*>(smem + kStage + off) = w8t_u4{0u, 0u, 0u, 0u};
    }
  }

  auto load_w = [&](w8t_u4 (&raw)[2][2], int b) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint8_t* p = qp + (int64_t)i * 16 * ldq + (int64_t)b * kW8TBlock;
      raw[i][0] = *reinterpret_cast<const w8t_u4*>(p);
      raw[i][1] = *reinterpret_cast<const w8t_u4*>(p + 16);
    }
  };
  auto issue_x = [&](int b, int buf) __attribute__((always_inline)) {
    unsigned char* sb = smem + buf * kStage + 4 * wave * kW8TRowBytes;
    const unsigned char* src = xsrc + (int64_t)b * kW8TRowBytes;
#pragma unroll
    for (int i = 0; i < kPieces; ++i) {
      if (16 * i + 4 * wave < live) {  // wave-uniform: pieces wholly at or above M issue nothing
        if (drow + 16 * i < live)
          __builtin_amdgcn_global_load_lds((w8t_glb_t*)(src + i * xstep), (w8t_lds_t*)(sb + i * 16 * kW8TRowBytes), 16, 0, 0);
      }
    }
  };

  w8t_f32x4 acc[2][TM / 16];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int t = 0; t < TM / 16; ++t) acc[i][t] = w8t_f32x4{0.f, 0.f, 0.f, 0.f};

  w8t_u4 raw[2][2], nxt[2][2];
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
    uint32_t a[2][8][2];  // [unit][dword of the lane's 32 bytes] -> 4 bf16
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int d = 0; d < 8; ++d) w8t_cvt4(raw[i][d >> 2][d & 3], a[i][d][0], a[i][d][1]);
    const unsigned char* sb = smem + buf * kStage;
#pragma unroll
    for (int tp = 0; tp < kPairs; ++tp) {
      if (tp * 32 >= live) break;  // wave-uniform
      w8t_f32x4 pr[2][2];          // [tile of the pair][unit]
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 2; ++i) pr[u][i] = w8t_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < 4; ++h) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const w8t_u4 bv = *reinterpret_cast<const w8t_u4*>(sb + (2 * tp + u) * 16 * kW8TRowBytes + fo[h]);
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const w8t_u4 av = {a[i][2 * h][0], a[i][2 * h][1], a[i][2 * h + 1][0], a[i][2 * h + 1][1]};
            pr[u][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(w8t_bf16x8, av),
                                                               __builtin_bit_cast(w8t_bf16x8, bv), pr[u][i], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          w8t_f32x4& c = acc[i][2 * tp + u];
          c.x = fmaf(sc, pr[u][i].x, c.x);
          c.y = fmaf(sc, pr[u][i].y, c.y);
          c.z = fmaf(sc, pr[u][i].z, c.z);
          c.w = fmaf(sc, pr[u][i].w, c.w);
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
        const w8t_f32x4 v = acc[i][t];
        const int64_t col = n0 + i * 16 + kg * 4;
        if (SLABS) {
          *reinterpret_cast<w8t_f32x4*>(part + ((int64_t)slice * M + m0 + m) * N + col) = v;
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
__global__ __launch_bounds__(256) void w8_tall_reduce_kernel(uint16_t* __restrict__ out, const float* __restrict__ part,
                                                             int M, int N, int S, int64_t ldo) {
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
static void launch_w8_tall(uint16_t* out, float* part, const uint16_t* x, const uint8_t* q, const float* scales, int M, int N,
                           int K, int64_t ldx, int64_t ldq, int64_t ldo, int k_slices, hipStream_t st) {
  const dim3 grid((unsigned)(N / kW8TTileN), (unsigned)((M + TM - 1) / TM), (unsigned)k_slices), block(64 * kW8TWaves);
  if (k_slices == 1) {
    w8_tall_gemm_kernel<TM, false><<<grid, block, 0, st>>>(out, part, x, q, scales, M, N, K / kW8TBlock, ldx, ldq, ldo);
  } else {
    w8_tall_gemm_kernel<TM, true><<<grid, block, 0, st>>>(out, part, x, q, scales, M, N, K / kW8TBlock, ldx, ldq, ldo);
    const int64_t threads = (int64_t)M * (N / 4);
    w8_tall_reduce_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st>>>(out, part, M, N, k_slices, ldo);
  }
}

}  // namespace msgl

using namespace msgl;

extern "C" int64_t msgl_w8_tall_workspace_bytes(int M, int N, int k_slices) {
  if (M < 1 || N < kW8TTileN || N % kW8TTileN || k_slices < 1 || k_slices > kW8TMaxSlices) return MSGL_EINVAL;
  if (k_slices == 1) return 0;
  return (int64_t)k_slices * M * (int64_t)N * (int64_t)sizeof(float);
}

extern "C" int msgl_w8_tall_gemm_nt(void* out, const void* x, const void* q, const float* scales, int M, int N, int K,
                                    int64_t ldx, int64_t ldq, int64_t ldo, int dtype, int tm, int k_slices, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  MSGL_REQUIRE(out && x && q && scales, "w8_tall_gemm_nt: null pointer");
  MSGL_REQUIRE(dtype == MSGL_BF16, "w8_tall_gemm_nt: activations must be bf16 (dtype code %d)", dtype);
  MSGL_REQUIRE(M >= 1, "w8_tall_gemm_nt: M = %d", M);
  MSGL_REQUIRE(N >= 128 && N % 128 == 0 && K >= 128 && K % 128 == 0,
               "w8_tall_gemm_nt: N = %d and K = %d must be multiples of the 128 x 128 scale block", N, K);
  MSGL_REQUIRE(tm == 128 || tm == 256, "w8_tall_gemm_nt: tm %d (128, 256)", tm);
  MSGL_REQUIRE(k_slices >= 1 && k_slices <= K / 128 && k_slices <= kW8TMaxSlices,
               "w8_tall_gemm_nt: %d k-slices outside [1, min(K / 128 = %d, %d)]", k_slices, K / 128, kW8TMaxSlices);
  MSGL_REQUIRE((M + tm - 1) / tm <= 65535, "w8_tall_gemm_nt: M = %d is more than 65535 tiles of %d rows", M, tm);
  MSGL_REQUIRE(ldx >= K && ldq >= K && ldo >= N && ldx % 8 == 0 && ldq % 16 == 0 && ldo % 4 == 0,
               "w8_tall_gemm_nt: leading dimensions (%lld, %lld, %lld)", (long long)ldx, (long long)ldq, (long long)ldo);
  MSGL_REQUIRE(aligned16(x) && aligned16(q) && (reinterpret_cast<uintptr_t>(out) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(scales) & 3u) == 0,
               "w8_tall_gemm_nt: x, q must be 16-byte, out 8-byte and scales 4-byte aligned");
  const int64_t need = msgl_w8_tall_workspace_bytes(M, N, k_slices);
  if (need > 0) {
    MSGL_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= need,
                 "w8_tall_gemm_nt: %d k-slices need %lld bytes of 16-byte aligned workspace (got %lld)", k_slices,
                 (long long)need, (long long)workspace_bytes);
    MSGL_REQUIRE((int64_t)M * (N / 4) <= 0x7fffffffll * 256, "w8_tall_gemm_nt: M x N = %d x %d is too large to k-slice", M, N);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (tm == 128)
    launch_w8_tall<128>((uint16_t*)out, (float*)workspace, (const uint16_t*)x, (const uint8_t*)q, scales, M, N, K, ldx, ldq,
                        ldo, k_slices, s);
  else
    launch_w8_tall<256>((uint16_t*)out, (float*)workspace, (const uint16_t*)x, (const uint8_t*)q, scales, M, N, K, ldx, ldq,
                        ldo, k_slices, s);
  MSGL_CHECK_LAUNCH("w8_tall_gemm_nt");
  return MSGL_OK;
}
