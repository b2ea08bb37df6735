// Mixture-of-experts MLP with block-scaled FP8 expert weights (W8A16): the pipeline of moe.hip -- route, align, gate_up,
// down, slot-ordered sum -- with the two grouped GEMMs reading OCP e4m3 bytes and one fp32 scale per 128 x 128 block, the
// layout of the FP8 checkpoints (`weight`, `weight_scale_inv`).  The align and sum kernels, the work-item tables and the
// workspace layout are moe.hip's (moe_tables.h); grids depend on (T, k, E, shape) only, a workgroup past the device-side
// item count exits, nothing is allocated, no float atomics, and a token's row is independent of the rest of the batch.
//
//   gemm 1   act[pos, f] = silu(x[token] . W1[e][f]) * (x[token] . W1[e][I + f]),   W1 = q1 * s1.   Workgroup = (64 features, item)
//   gemm 2   partial[pair, c] = (act[pos] . W2[e][c]) * weight[pair], fp32,          W2 = q2 * s2.   Workgroup = (128 columns, item)
//
// Numerics, those of gemm_w8.hip: e4m3 -> bf16 is exact (v_cvt_scalef32_pk_bf16_fp8 with scale 1.0); the four
// v_mfma_f32_16x16x32_bf16 of a 128-k block start from zero; the block's partial sum enters the running fp32 sum through
// one fma(scale, part, acc).  A scaled weight is never rounded.  The epilogues are moe.hip's: SiLU.mul on the accumulators
// -> bf16 act; x routing weight -> fp32 partial per pair; slots added in order.
//
// Work split.  An item is <= 64 rows of one expert, a workgroup four waves.  A wave owns two 16-row weight tiles: the gate
// and the up rows of 16 features (gate_up; two different scale row groups, I_l rows apart) or 32 consecutive columns
// (down; one scale row group, 32 | 128).  Weights go HBM -> VGPR, never through LDS: lane (r = l & 15, kg = l >> 4) loads
// the 32 contiguous bytes q[row0 + r, 128 b + 32 kg ..], so four lanes cover a whole 128-B line and every line is read
// once per item; MFMA j of the block takes bytes 8 j .. 8 j + 7 of each lane.  The matching activation fragment is one
// 16-B LDS read at k = 128 b + 32 kg + 8 j.  The k loop is outermost and all four row blocks' accumulators stay live (32
// fp32 registers, plus 8 transient per row block for the block partial sums), so an expert with <= 64 rows has each
// weight byte read from HBM once per launch.  Block scales are wave-uniform: one scalar load per (tile, block).
//
// The item's rows are staged through LDS per chunk of NB blocks (gathered by token in gemm 1, act rows in gemm 2, pad rows
// zero); the chunk's weight loads are issued before the rows are staged.  NB is a compile-time choice
// (MSGL_MOE_W8_CHUNK_BLOCKS): 2 blocks = 256 k is the bf16 kernel's chunk with half its weight bytes in flight (33 KB of
// LDS, 159 / 134 VGPRs, three waves per SIMD); 4 blocks = 512 k has the bf16 kernel's sixteen 1-KB requests per wave in
// flight but 65 KB of LDS and 256 VGPRs + 52 AGPRs (gate_up): one wave per SIMD.  Measured on Qwen3-30B-A3B
// (profiles/moe_w8_bench.json): 256 k is faster at every batch (T = 64: 151 vs 236 us), so 2 is kept;
// occupancy, not bytes in flight per wave, is what the stream needs.  Both compile without scratch.
//
// LDS image: row pitch = 256 NB + 16 bytes.  A fragment read has the 16 lanes r = 0 .. 15 of a lane group at the same k
// offset in 16 consecutive rows: byte address = r (256 NB + 16) + c.  The LDS has 64 four-byte banks, 256 bytes per turn;
// 256 NB is a whole number of turns, so the address is 16 r + c (mod 256): sixteen different 16-byte bank groups, every
// bank used once per 16 lanes.
#include "moe_tables.h"

#ifndef MSGL_MOE_W8_CHUNK_BLOCKS
#define MSGL_MOE_W8_CHUNK_BLOCKS 2
#endif

namespace msgl {

typedef __attribute__((ext_vector_type(4))) float mw8_f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 mw8_bf16x8;

constexpr int kMoeW8Block = 128;  // k per scale block = bytes of one weight line
constexpr int kMoeW8ChunkBlocks = MSGL_MOE_W8_CHUNK_BLOCKS;
static_assert(kMoeW8ChunkBlocks == 2 || kMoeW8ChunkBlocks == 4, "the staged chunk is 256 or 512 k");

__host__ __device__ constexpr int moe_w8_pitch(int NB) { return NB * 256 + 16; }
__host__ __device__ constexpr int moe_w8_lds_bytes(int NB) { return kMoeItemRows * moe_w8_pitch(NB) + kMoeItemRows * 4; }

// four e4m3 bytes -> four bf16 (exact)
__device__ __forceinline__ void moe_w8_cvt4(uint32_t v, uint32_t& lo, uint32_t& hi) {
  lo = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v, 1.0f, false));
  hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v, 1.0f, true));
}

enum { MOE_W8_GATE_UP = 1, MOE_W8_DOWN = 2 };

struct MoeW8Params {
  const uint16_t* a;   // GATE_UP: x [T, K]; DOWN: act [cap, K]
  const uint8_t* q;    // GATE_UP: q1 [E, 2 N, K]; DOWN: q2 [E, N, K]
  const float* s;      // GATE_UP: s1 [E, 2 N / 128, K / 128]; DOWN: s2 [E, N / 128, K / 128]
  MoeTables tb;
  uint16_t* act;       // GATE_UP out: [cap, N]
  float* partial;      // DOWN out: [P, N]
  const float* topk_w; // [P]
  int K, N, topk;
};

template <int MODE, int NB>
__global__ __launch_bounds__(256) void moe_w8_gemm_kernel(const MoeW8Params p) {
  constexpr int kPitch = moe_w8_pitch(NB), kCols = NB * 16;  // 16-B columns of a staged row
  extern __shared__ __attribute__((aligned(16))) unsigned char mw8_lds[];
  unsigned char* xs = mw8_lds;
  int* rowsrc = reinterpret_cast<int*>(mw8_lds + kMoeItemRows * kPitch);
  const int item = blockIdx.y;
  if (item >= *p.tb.n_items) return;
  const int e = sgpr(p.tb.item_expert[item]), pos0 = sgpr(p.tb.item_pos[item]), nrb = sgpr(p.tb.item_blocks[item]);
  const int tid = threadIdx.x, lane = tid & 63, wv = sgpr(tid >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int K = p.K, N = p.N, nblk = K / kMoeW8Block;
  if (tid < kMoeItemRows) {  // source row of each staged row: the pair's token (gate_up) / its own act row (down); -1 = zeros
    const int pair = tid < kMoeBM * nrb ? p.tb.sorted[pos0 + tid] : -1;
    rowsrc[tid] = pair < 0 ? -1 : MODE == MOE_W8_GATE_UP ? pair / p.topk : pos0 + tid;
  }
  // this wave's two tiles of 16 weight rows, and the scale rows of their 128-row groups (wave-uniform).  N % 128 == 0:
  // every wave of the grid has columns
  const int col = MODE == MOE_W8_GATE_UP ? 64 * blockIdx.x + 16 * wv : 128 * blockIdx.x + 32 * wv;
  const uint8_t* qrow[2];
  const float* sp[2];
  if (MODE == MOE_W8_GATE_UP) {
    qrow[0] = p.q + ((int64_t)e * 2 * N + col + r16) * K + 32 * q4;
    qrow[1] = qrow[0] + (int64_t)N * K;
    sp[0] = p.s + ((int64_t)e * (2 * N / kMoeW8Block) + col / kMoeW8Block) * nblk;
    sp[1] = sp[0] + (int64_t)(N / kMoeW8Block) * nblk;
  } else {
    qrow[0] = p.q + ((int64_t)e * N + col + r16) * K + 32 * q4;
    qrow[1] = qrow[0] + (int64_t)16 * K;
    sp[0] = sp[1] = p.s + ((int64_t)e * (N / kMoeW8Block) + col / kMoeW8Block) * nblk;
  }
  mw8_f32x4 acc[kMoeItemBlocks][2];
#pragma unroll
  for (int rb = 0; rb < kMoeItemBlocks; ++rb) acc[rb][0] = acc[rb][1] = mw8_f32x4{0.f, 0.f, 0.f, 0.f};

  for (int cb = 0; cb < nblk; cb += NB) {
    const int nb = sgpr(min(NB, nblk - cb));
    // the chunk's weight bytes first: they travel while the rows are staged
    U4 raw[NB][2][2];
#pragma unroll
    for (int j = 0; j < NB; ++j)
      if (j < nb) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const uint8_t* src = qrow[u] + (int64_t)(cb + j) * kMoeW8Block;
          raw[j][u][0] = ldg16(src);
          raw[j][u][1] = ldg16(src + 16);
        }
      }
    __syncthreads();  // the previous chunk has been read (first pass: rowsrc is written)
#pragma unroll 8  // eight 16-B pieces in flight per thread: all sixteen of a 512-k chunk would not fit the register file
    for (int i = 0; i < kMoeItemRows * kCols / 256; ++i) {
      const int piece = tid + 256 * i, row = piece / kCols, c = piece % kCols;
      if (row < kMoeBM * nrb && c < 16 * nb) {
        const int src = rowsrc[row];
        U4 v = {0u, 0u, 0u, 0u};
        if (src >= 0) v = ldg16(p.a + (int64_t)src * K + (int64_t)cb * kMoeW8Block + 8 * c);
        *reinterpret_cast<U4*>(xs + row * kPitch + 16 * c) = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NB; ++j)
      if (j < nb) {
        const float sc0 = sp[0][cb + j], sc1 = sp[1][cb + j];
        uint32_t a[2][8][2];  // [tile][dword of the lane's 32 bytes] -> 4 bf16
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int d = 0; d < 8; ++d) {
            const U4& w = raw[j][u][d >> 2];
            moe_w8_cvt4((d & 3) == 0 ? w.x : (d & 3) == 1 ? w.y : (d & 3) == 2 ? w.z : w.w, a[u][d][0], a[u][d][1]);
          }
#pragma unroll
        for (int rb = 0; rb < kMoeItemBlocks; ++rb)
          if (rb < nrb) {
            mw8_f32x4 part0 = {0.f, 0.f, 0.f, 0.f}, part1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int h = 0; h < 4; ++h) {
              const U4 b = *reinterpret_cast<const U4*>(xs + (kMoeBM * rb + r16) * kPitch + (128 * j + 32 * q4 + 8 * h) * 2);
              const U4 a0 = {a[0][2 * h][0], a[0][2 * h][1], a[0][2 * h + 1][0], a[0][2 * h + 1][1]};
              const U4 a1 = {a[1][2 * h][0], a[1][2 * h][1], a[1][2 * h + 1][0], a[1][2 * h + 1][1]};
              part0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mw8_bf16x8, a0),
                                                              __builtin_bit_cast(mw8_bf16x8, b), part0, 0, 0, 0);
              part1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mw8_bf16x8, a1),
                                                              __builtin_bit_cast(mw8_bf16x8, b), part1, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              acc[rb][0][i] = fmaf(sc0, part0[i], acc[rb][0][i]);
              acc[rb][1][i] = fmaf(sc1, part1[i], acc[rb][1][i]);
            }
          }
      }
  }
  // lane holds D[weight row 4 q4 + i][token row r16] in register i of each tile
#pragma unroll
  for (int rb = 0; rb < kMoeItemBlocks; ++rb)
    if (rb < nrb) {
      const int pos = pos0 + kMoeBM * rb + r16;
      const int pair = p.tb.sorted[pos];
      if (pair < 0) continue;
      if (MODE == MOE_W8_GATE_UP) {
        uint2 pk;
        pk.x = Elem<BF16>::pack(silu_mul_f32(acc[rb][0][0], acc[rb][1][0]), silu_mul_f32(acc[rb][0][1], acc[rb][1][1]));
        pk.y = Elem<BF16>::pack(silu_mul_f32(acc[rb][0][2], acc[rb][1][2]), silu_mul_f32(acc[rb][0][3], acc[rb][1][3]));
        *reinterpret_cast<uint2*>(p.act + (int64_t)pos * N + col + 4 * q4) = pk;
      } else {
        const float wgt = p.topk_w[pair];
        float* dst = p.partial + (int64_t)pair * N + col + 4 * q4;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          float4 v;
          v.x = acc[rb][u][0] * wgt; v.y = acc[rb][u][1] * wgt; v.z = acc[rb][u][2] * wgt; v.w = acc[rb][u][3] * wgt;
          *reinterpret_cast<float4*>(dst + 16 * u) = v;
        }
      }
    }
}

template <int MODE>
static int moe_w8_launch(const MoeW8Params& g, unsigned tiles, unsigned items, hipStream_t s) {
  constexpr int kLds = moe_w8_lds_bytes(kMoeW8ChunkBlocks);
  auto* kernel = &moe_w8_gemm_kernel<MODE, kMoeW8ChunkBlocks>;
  static PerDeviceOnce lds_attr;  // per instantiation and device: more than 64 KB of dynamic LDS has to be requested
  if (kLds > 65536 && !lds_attr.ensure([&] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLds) ==
               hipSuccess;
      })) {
    set_error("moe_w8_forward: cannot reserve %d bytes of LDS: %s", kLds, hipGetErrorString(hipGetLastError()));
    return MSGL_ELAUNCH;
  }
  kernel<<<dim3(tiles, items), dim3(256), kLds, s>>>(g);
  return MSGL_OK;
}

static int moe_w8_check_shape(const char* who, int64_t T, int64_t E, int64_t k, int64_t hidden, int64_t I) {
  const int rc = moe_check_shape(who, T, E, k, hidden, I);
  if (rc != MSGL_OK) return rc;
  MSGL_REQUIRE(hidden % kMoeW8Block == 0 && I % kMoeW8Block == 0,
               "%s: hidden = %lld and the expert intermediate size %lld must be multiples of the 128 x 128 scale block", who,
               (long long)hidden, (long long)I);
  return MSGL_OK;
}

}  // namespace msgl

using namespace msgl;

extern "C" int64_t msgl_moe_w8_workspace_bytes(int T, int E, int k, int hidden, int I_l) {
  const int rc = moe_w8_check_shape("moe_w8_workspace_bytes", T, E, k, hidden, I_l);
  if (rc != MSGL_OK) return rc;
  return moe_layout(T, E, k, hidden, I_l).bytes;
}

extern "C" int msgl_moe_w8_forward(const void* x, const void* q1, const float* s1, const void* q2, const float* s2,
                                   const float* topk_weights, const int32_t* topk_ids, void* workspace,
                                   int64_t workspace_bytes, void* out, int T, int E, int k, int hidden, int I_l, void* stream) {
  MSGL_REQUIRE(x && q1 && s1 && q2 && s2 && topk_weights && topk_ids && out, "moe_w8_forward: null pointer");
  const int rc = moe_w8_check_shape("moe_w8_forward", T, E, k, hidden, I_l);
  if (rc != MSGL_OK) return rc;
  const MoeLayout L = moe_layout(T, E, k, hidden, I_l);
  MSGL_REQUIRE(L.max_items <= kMoeMaxGridY, "moe_w8_forward: %lld work items exceed one launch; split the tokens",
               (long long)L.max_items);
  MSGL_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0 && workspace_bytes >= L.bytes,
               "moe_w8_forward: needs %lld workspace bytes, 256-byte aligned", (long long)L.bytes);
  MSGL_REQUIRE(aligned16(x) && aligned16(q1) && aligned16(q2) && aligned16(out),
               "moe_w8_forward: x, q1, q2 and out must be 16-byte aligned");
  MSGL_REQUIRE(((reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2)) & 3u) == 0,
               "moe_w8_forward: the scale grids must be 4-byte aligned");
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const MoeTables tb = moe_tables(ws, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  moe_launch_align(tb, topk_ids, T * k, E, s);
  MSGL_CHECK_LAUNCH("moe_w8_forward(align)");

  MoeW8Params g;
  g.tb = tb;
  g.act = reinterpret_cast<uint16_t*>(ws + L.o_act);
  g.partial = reinterpret_cast<float*>(ws + L.o_partial);
  g.topk_w = topk_weights;
  g.topk = k;
  g.a = static_cast<const uint16_t*>(x); g.q = static_cast<const uint8_t*>(q1); g.s = s1; g.K = hidden; g.N = I_l;
  int lrc = moe_w8_launch<MOE_W8_GATE_UP>(g, (unsigned)(I_l / 64), (unsigned)L.max_items, s);
  if (lrc != MSGL_OK) return lrc;
  MSGL_CHECK_LAUNCH("moe_w8_forward(gate_up)");
  g.a = g.act; g.q = static_cast<const uint8_t*>(q2); g.s = s2; g.K = I_l; g.N = hidden;
  lrc = moe_w8_launch<MOE_W8_DOWN>(g, (unsigned)(hidden / 128), (unsigned)L.max_items, s);
  if (lrc != MSGL_OK) return lrc;
  MSGL_CHECK_LAUNCH("moe_w8_forward(down)");
  moe_launch_sum(static_cast<uint16_t*>(out), g.partial, topk_ids, T, k, E, hidden, s);
  MSGL_CHECK_LAUNCH("moe_w8_forward(sum)");
  return MSGL_OK;
}
