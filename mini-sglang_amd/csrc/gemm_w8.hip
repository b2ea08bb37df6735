// W8A16 projection GEMM: block-scaled OCP e4m3 weights, bf16 activations, fp32 accumulate (1 <= M <= 256):
//     out[m, n] = round_bf16( sum_b s[n / 128, b] * sum_{k in block b} x[m, k] * float(q[n, k]) )
// q [N, K] are the checkpoint's float8_e4m3fn bytes, s [N / 128, K / 128] its fp32 `weight_scale_inv` grid.  A decode
// step is a stream of the projection weights; this family streams half the bytes of the 16-bit kernels.
//
// Layout and work split
//   * the unit of work is 16 weight rows x 128 k = one scale block's worth of 16 whole 128-B lines.  A wave reads it
//     with two 16-B loads per lane: lane (r = l & 15, kg = l >> 4) holds q[n0 + r, 128 b + 32 kg .. + 31], so every
//     128-B line of a weight row is read whole, by one wave, once per launch (whatever M is);
//   * the 32 bytes of a lane become four v_mfma_f32_16x16x32_bf16 A operands (8 consecutive k each) through
//     v_cvt_scalef32_pk_bf16_fp8 with scale 1.0: e4m3 -> bf16 is exact, the block scale never touches a bf16 value;
//   * x is the B operand, staged through LDS in chunks of S J 128-k blocks (all of M x K does not fit at M = 256,
//     K = 5120) and read back in the matching k order: lane (r, kg), step j reads x[16 t + r, 128 b + 32 kg + 8 j .. + 7]
//     as one 16-B LDS load.  The 16-B columns of a row are XOR-swizzled with the row (r & 15), so the 16 rows of a
//     k-group fall into 16 different bank groups;
//   * the four MFMAs of a block start from zero; their sum is added to the running sum multiplied by the block's
//     scale (fp32 FMA).  The scale is uniform over the wave's rows: one scalar load per block;
//   * a workgroup is U x S waves: U row groups (row_tiles) share the staged x chunk, S k-slices split each chunk's
//     blocks (slice s takes blocks s J .. s J + J - 1 of the chunk).  At 64 < M <= 128 a wave takes two 16-row units, so an x
//     fragment read from LDS feeds two MFMAs.  Grid = N / (16 units-per-wave U): a function of the arguments only;
//   * S > 1 (small N at small M: o_proj): the slices' sums meet in LDS (the x area, reused) and wave s = 0 of each row
//     group adds them in slice order -- deterministic, no atomics, no workspace.
// The weight loads of a chunk are issued before the barrier and the staging pass, so they are in flight while x arrives.
//
// msgl_w8_dequant writes round_bf16(float(q) * s) (product in fp32) for batches above 256 rows: the 16-bit GEMM paths
// then run on the scratch copy.
#include "common.h"

namespace msgl {

typedef __bf16 w8_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 w8_bf16x2 __attribute__((ext_vector_type(2)));
typedef float w8_f32x4 __attribute__((ext_vector_type(4)));
typedef float w8_f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t w8_u4 __attribute__((ext_vector_type(4)));

constexpr int kW8Block = 128;             // k per scale block = bytes of one weight line
constexpr int kW8LdsBytes = 64 * 1024;    // no more than the default dynamic LDS limit
constexpr int kW8MaxWaves = 8;

// 16-row units per wave: at 65 .. 128 rows an x fragment read from LDS feeds two MFMAs (at 16 M tiles the accumulators of two
// units no longer fit the register file)
__host__ __device__ constexpr int w8_units_per_wave(int MT) { return MT == 8 ? 2 : 1; }
__host__ __device__ constexpr int w8_max_blocks_per_wave(int MT) { return MT >= 8 ? 1 : 4; }

// four e4m3 bytes -> four bf16 (exact)
__device__ __forceinline__ void w8_cvt4(uint32_t v, uint32_t& lo, uint32_t& hi) {
  lo = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v, 1.0f, false));
  hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v, 1.0f, true));
}

// byte offset of 16-B column `c` of row `row` in the staged chunk (row pitch = 16 kcb columns of 16 B per block)
__device__ __forceinline__ int w8_lds_off(int row, int c, int cols) {
  return (row * cols + ((c & ~15) | ((c ^ row) & 15))) * 16;
}

// MT = 16-row M tiles the kernel is unrolled for (tiles at or above M are skipped), J = 128-k blocks per wave per chunk.
// blockDim = 64 U S, grid = N / (16 NT U), dynamic LDS = max(rows * S J 256, S > 1 ? U S NT MT 1024 : 0) bytes.
template <int MT, int J>
__global__ __launch_bounds__(64 * kW8MaxWaves) void w8_gemm_kernel(
    uint16_t* __restrict__ out, const uint16_t* __restrict__ x, const uint8_t* __restrict__ q,
    const float* __restrict__ scales, int M, int nblk, int64_t ldx, int64_t ldq, int64_t ldo, int S) {
  constexpr int NT = w8_units_per_wave(MT);
  extern __shared__ __attribute__((aligned(16))) unsigned char w8_lds[];
  const int lane = threadIdx.x & 63, wave = sgpr(threadIdx.x >> 6);  // uniform: the scale is one scalar load
  const int r = lane & 15, kg = lane >> 4;
  const int s = wave % S, u = wave / S, U = (int)(blockDim.x >> 6) / S;
  const int64_t n0 = ((int64_t)blockIdx.x * U + u) * (16 * NT);  // NT units of one wave share a 128-row scale group
  const int rows = (M + 15) & ~15;
  const int kcb = S * J, cols = kcb * 16;  // blocks / 16-B columns per staged chunk
  const uint8_t* qp = q + (n0 + r) * ldq + kg * 32;
  const float* sp = scales + (n0 >> 7) * nblk;

  w8_f32x4 acc[NT][MT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[i][t] = w8_f32x4{0.f, 0.f, 0.f, 0.f};

  for (int cb = 0; cb < nblk; cb += kcb) {
    // this wave's blocks of the chunk: weights HBM -> VGPR, issued ahead of the barrier and the staging pass
    w8_u4 raw[J][NT][2];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int kb = cb + s * J + j;
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        raw[j][i][0] = raw[j][i][1] = w8_u4{0u, 0u, 0u, 0u};
        if (kb < nblk) {
          const uint8_t* p = qp + (int64_t)i * 16 * ldq + (int64_t)kb * kW8Block;
          raw[j][i][0] = *reinterpret_cast<const w8_u4*>(p);
          raw[j][i][1] = *reinterpret_cast<const w8_u4*>(p + 16);
        }
      }
    }
    __syncthreads();  // every wave is done with the previous chunk
    for (int p = threadIdx.x; p < rows * cols; p += blockDim.x) {
      const int row = p / cols, c = p - row * cols;
      w8_u4 v = {0u, 0u, 0u, 0u};  // rows at or above M: zero columns of the B operand
      if (row < M && cb * 16 + c < nblk * 16) v = *reinterpret_cast<const w8_u4*>(x + row * ldx + ((int64_t)cb * 16 + c) * 8);
      *reinterpret_cast<w8_u4*>(w8_lds + w8_lds_off(row, c, cols)) = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int kb = cb + s * J + j;
      if (kb >= nblk) break;  // wave-uniform
      const float sc = sp[kb];
      uint32_t a[NT][8][2];  // [unit][dword of the lane's 32 bytes] -> 4 bf16
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int d = 0; d < 8; ++d) w8_cvt4(raw[j][i][d >> 2][d & 3], a[i][d][0], a[i][d][1]);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        if (t * 16 >= M) break;  // wave-uniform
        w8_f32x4 part[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) part[i] = w8_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const int c = (s * J + j) * 16 + kg * 4 + h;
          const w8_u4 b = *reinterpret_cast<const w8_u4*>(w8_lds + w8_lds_off(t * 16 + r, c, cols));
#pragma unroll
          for (int i = 0; i < NT; ++i) {
            const w8_u4 av = {a[i][2 * h][0], a[i][2 * h][1], a[i][2 * h + 1][0], a[i][2 * h + 1][1]};
            part[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(w8_bf16x8, av),
                                                              __builtin_bit_cast(w8_bf16x8, b), part[i], 0, 0, 0);
          }
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          acc[i][t].x = fmaf(sc, part[i].x, acc[i][t].x);
          acc[i][t].y = fmaf(sc, part[i].y, acc[i][t].y);
          acc[i][t].z = fmaf(sc, part[i].z, acc[i][t].z);
          acc[i][t].w = fmaf(sc, part[i].w, acc[i][t].w);
        }
      }
    }
  }

  // lane (r, kg) holds out[16 t + r, n0 + 16 i + 4 kg .. + 3]
  w8_f32x4* red = reinterpret_cast<w8_f32x4*>(w8_lds);  // [U][S][NT][MT][64]
  if (S > 1) {
    __syncthreads();  // the x area is free
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int t = 0; t < MT; ++t) red[(((u * S + s) * NT + i) * MT + t) * 64 + lane] = acc[i][t];
    __syncthreads();
    if (s != 0) return;
  }
#pragma unroll
  for (int i = 0; i < NT; ++i) {
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      w8_f32x4 v = acc[i][t];
      for (int j = 1; j < S; ++j) {  // slice order
        const w8_f32x4 o = red[(((u * S + j) * NT + i) * MT + t) * 64 + lane];
        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
      }
      const int m = t * 16 + r;
      if (m < M) {
        uint2 pk;
        pk.x = Elem<BF16>::pack(v.x, v.y);
        pk.y = Elem<BF16>::pack(v.z, v.w);
        *reinterpret_cast<uint2*>(out + (int64_t)m * ldo + n0 + i * 16 + kg * 4) = pk;
      }
    }
  }
}

// one thread: 16 weight bytes of one row (inside one scale block) -> 16 bf16
__global__ __launch_bounds__(256) void w8_dequant_kernel(uint16_t* __restrict__ out, const uint8_t* __restrict__ q,
                                                         const float* __restrict__ scales, int64_t pieces, int kp,
                                                         int64_t ldq, int64_t ldo) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pieces) return;
  const int64_t n = p / kp;
  const int c = (int)(p - n * kp);  // 16-element column of the row
  const float sc = scales[(n >> 7) * (kp >> 3) + (c >> 3)];
  const w8_u4 v = *reinterpret_cast<const w8_u4*>(q + n * ldq + (int64_t)c * 16);
  w8_u4 o[2];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const w8_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[d], false);
    const w8_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[d], true);
    o[d >> 1][(d & 1) * 2] = Elem<BF16>::pack(lo.x * sc, lo.y * sc);
    o[d >> 1][(d & 1) * 2 + 1] = Elem<BF16>::pack(hi.x * sc, hi.y * sc);
  }
  w8_u4* op = reinterpret_cast<w8_u4*>(out + n * ldo + (int64_t)c * 16);
  op[0] = o[0];
  op[1] = o[1];
}

template <int MT>
static int launch_w8(uint16_t* out, const uint16_t* x, const uint8_t* q, const float* scales, int M, int N, int K,
                     int64_t ldx, int64_t ldq, int64_t ldo, int S, int U, hipStream_t st) {
  constexpr int NT = w8_units_per_wave(MT);
  const int rows = (M + 15) & ~15, nblk = K / kW8Block;
  const size_t red = S > 1 ? (size_t)U * S * NT * MT * 64 * sizeof(w8_f32x4) : 0;
  // blocks per wave per chunk: as many as the LDS limit and K allow (a choice of the shape and the knobs only)
  int J = w8_max_blocks_per_wave(MT);
  while (J > 1 && ((size_t)rows * S * J * 256 > (size_t)kW8LdsBytes || S * J > nblk)) J >>= 1;
  const size_t stage = (size_t)rows * S * J * 256;
  if (stage > (size_t)kW8LdsBytes || red > (size_t)kW8LdsBytes) {
    set_error("w8_gemm_nt: M = %d with %d k-slices x %d row tiles needs %zu bytes of LDS (limit %d)", M, S, U,
              stage > red ? stage : red, kW8LdsBytes);
    return MSGL_EINVAL;
  }
  const dim3 grid((unsigned)(N / (16 * NT * U))), block(64 * U * S);
  const size_t lds = stage > red ? stage : red;
#define MSGL_W8(J_)                                         \
  if constexpr (J_ <= w8_max_blocks_per_wave(MT))           \
    if (J == J_) w8_gemm_kernel<MT, J_><<<grid, block, lds, st>>>(out, x, q, scales, M, nblk, ldx, ldq, ldo, S)
  MSGL_W8(1); MSGL_W8(2); MSGL_W8(4);
#undef MSGL_W8
  return MSGL_OK;
}

}  // namespace msgl

using namespace msgl;

extern "C" int msgl_w8_gemm_nt(void* out, const void* x, const void* q, const float* scales, int M, int N, int K,
                               int64_t ldx, int64_t ldq, int64_t ldo, int dtype, int slices, int row_tiles, void* stream) {
  MSGL_REQUIRE(out && x && q && scales, "w8_gemm_nt: null pointer");
  MSGL_REQUIRE(dtype == MSGL_BF16, "w8_gemm_nt: activations must be bf16 (dtype code %d)", dtype);
  MSGL_REQUIRE(M >= 1 && M <= 256, "w8_gemm_nt: M = %d outside [1, 256]", M);
  MSGL_REQUIRE(N >= 128 && N % 128 == 0 && K >= 128 && K % 128 == 0,
               "w8_gemm_nt: N = %d and K = %d must be multiples of the 128 x 128 scale block", N, K);
  MSGL_REQUIRE(row_tiles == 1 || row_tiles == 2 || row_tiles == 4, "w8_gemm_nt: row_tiles %d (1, 2, 4)", row_tiles);
  MSGL_REQUIRE(slices >= 1 && slices <= kW8MaxWaves && slices * row_tiles <= kW8MaxWaves && slices <= K / 128,
               "w8_gemm_nt: %d k-slices x %d row tiles outside [1, %d waves] or above K / 128", slices, row_tiles, kW8MaxWaves);
  MSGL_REQUIRE(ldx >= K && ldq >= K && ldo >= N && ldx % 8 == 0 && ldq % 16 == 0 && ldo % 4 == 0,
               "w8_gemm_nt: leading dimensions (%lld, %lld, %lld)", (long long)ldx, (long long)ldq, (long long)ldo);
  MSGL_REQUIRE(aligned16(x) && aligned16(q) && (reinterpret_cast<uintptr_t>(out) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(scales) & 3u) == 0,
               "w8_gemm_nt: x, q must be 16-byte, out 8-byte and scales 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int MT = M <= 16 ? 1 : M <= 32 ? 2 : M <= 64 ? 4 : M <= 128 ? 8 : 16;
  int rc = MSGL_EINVAL;
#define MSGL_W8_MT(MT_) \
  if (MT == MT_) rc = launch_w8<MT_>((uint16_t*)out, (const uint16_t*)x, (const uint8_t*)q, scales, M, N, K, ldx, ldq, ldo, slices, row_tiles, s)
  MSGL_W8_MT(1); MSGL_W8_MT(2); MSGL_W8_MT(4); MSGL_W8_MT(8); MSGL_W8_MT(16);
#undef MSGL_W8_MT
  if (rc != MSGL_OK) return rc;
  MSGL_CHECK_LAUNCH("w8_gemm_nt");
  return MSGL_OK;
}

extern "C" int msgl_w8_dequant(void* out, const void* q, const float* scales, int N, int K, int64_t ldq, int64_t ldo,
                               void* stream) {
  MSGL_REQUIRE(out && q && scales, "w8_dequant: null pointer");
  MSGL_REQUIRE(N >= 128 && N % 128 == 0 && K >= 128 && K % 128 == 0,
               "w8_dequant: N = %d and K = %d must be multiples of the 128 x 128 scale block", N, K);
  MSGL_REQUIRE(ldq >= K && ldo >= K && ldq % 16 == 0 && ldo % 8 == 0, "w8_dequant: leading dimensions (%lld, %lld)",
               (long long)ldq, (long long)ldo);
  MSGL_REQUIRE(aligned16(out) && aligned16(q) && (reinterpret_cast<uintptr_t>(scales) & 3u) == 0,
               "w8_dequant: out, q must be 16-byte and scales 4-byte aligned");
  const int64_t pieces = (int64_t)N * (K / 16);
  const int64_t blocks = (pieces + 255) / 256;
  MSGL_REQUIRE(blocks <= 0x7fffffff, "w8_dequant: N x K = %d x %d is too large for one launch", N, K);
  w8_dequant_kernel<<<dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream)>>>(
      (uint16_t*)out, (const uint8_t*)q, scales, pieces, K / 16, ldq, ldo);
  MSGL_CHECK_LAUNCH("w8_dequant");
  return MSGL_OK;
}
