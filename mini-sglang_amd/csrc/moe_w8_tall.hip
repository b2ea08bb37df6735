// The expert MLP with block-scaled FP8 expert weights (csrc/moe_w8.hip, W8A16) for prefill-sized batches: the 256-row work
// items, the three-launch align, the column slabs and the slab sum of csrc/moe_tall.hip (moe_tall_tables.h), with the two
// grouped GEMMs reading OCP e4m3 bytes and one fp32 scale per 128 x 128 block straight from the checkpoint layout.
//
// Numerics: those of moe_w8.hip, bit for bit.  e4m3 -> bf16 is exact (v_cvt_scalef32_pk_bf16_fp8 with scale 1.0); lane
// (r = l & 15, kg = l >> 4) holds the 32 bytes q[row0 + r, 128 b + 32 kg ..] and MFMA h of the block takes bytes 8 h .. 8 h + 7;
// the four v_mfma_f32_16x16x32_bf16 of a 128-k block start from zero, in h order; one fmaf(scale, part, acc) per block, blocks
// ascending; silu_mul_f32 on the fp32 accumulators -> bf16 act; x routing weight -> fp32 partial per pair; slots added in
// order and rounded once.  An accumulator belongs to one (pair, column), so the order in which row blocks are visited
// changes nothing.
//
// Work split and data movement (the movement of gemm_w8_tall.hip under the tables of moe_tall.hip)
//   * workgroup = 128 weight rows x one item of <= 256 rows, 4 waves (one per SIMD); grid = (column tile, item), x fastest,
//     grid.y = the shape's upper bound on items, a workgroup past the device-side item count exits (graph capture);
//   * weights never pass through LDS.  Wave w owns two 16-row units: the gate rows and the up rows of the 16 features
//     f0 + 16 w (gate_up: two scale row groups, I_l rows apart, SiLU.mul stays on the accumulators) or 32 consecutive columns
//     of the slab (down: one scale row group).  Per 128-k block a lane loads its 2 x 32 bytes (four lanes = one 128-B line),
//     converts them once into four MFMA A operands per unit and keeps them while the wave walks every live 16-row block of
//     the item; the lines of block b + 1 are requested before the MFMAs of block b.  A weight byte is read once per item, by
//     one wave.  Block scales are wave-uniform: one scalar load per (unit, block);
//   * activations go global -> LDS by DMA (global_load_lds_dwordx4: no staging registers, no ds_write) into TWO stages of
//     256 rows x 256 B (one 128-k block): 2 x 64 KB, one workgroup per CU.  A DMA lane supplies its own global address, so the
//     gather by token (gate_up: x[sorted[pos] / topk]; down: the item's own act rows) costs nothing.  A wave instruction fills
//     1 KB = 4 rows lane-linearly, so the XOR swizzle is applied on the SOURCE side: the lane landing on 16-B slot s of row r
//     fetches column s ^ (r & 15).  A fragment read (lane (r, kg), MFMA h: row 16 t + r, column 4 kg + h) is one 16-B LDS
//     load and the 16 rows of a lane group fall into 16 different bank groups;
//   * pad rows (sorted == -1) and rows past the item issue no DMA; they are zeroed once, in both stages, before the loop.
//     16-row blocks at or past item_blocks are skipped (taken in pairs: the odd last block's partner is zero rows);
//   * one barrier per block: wait for the wave's own DMA pieces of block b, barrier (stage b & 1 is whole, stage (b + 1) & 1
//     is free), issue weight loads and DMA of block b + 1, then the MFMAs of block b;
//   * accumulators: 2 units x 16 row blocks x 4 fp32 = 128 registers.  The per-block partial sums are transient: row blocks in
//     pairs, 2 x 2 independent chains of four MFMAs, every x fragment feeds two MFMAs, then acc = fma(scale, part, acc).
#include "moe_tall_tables.h"

namespace msgl {

typedef __bf16 mw8t_bf16x8 __attribute__((ext_vector_type(8)));
typedef float mw8t_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t mw8t_u4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void mw8t_lds_t;
typedef __attribute__((address_space(1))) const void mw8t_glb_t;

constexpr int kMoeW8TBlock = 128;     // k per scale block = bytes of one weight line
constexpr int kMoeW8TRowBytes = 256;  // one staged row: 128 k of bf16 = 16 columns of 16 B
constexpr int kMoeW8TStage = kTallItemRows * kMoeW8TRowBytes;
constexpr int kMoeW8TWaves = 4;
constexpr int kMoeW8TPieces = kTallItemRows / (4 * kMoeW8TWaves);  // DMA instructions (4 rows each) per wave per block
static_assert(kMoeW8TPieces == kTallItemBlocks, "piece i of a wave lies in row block i");

// four e4m3 bytes -> four bf16 (exact)
__device__ __forceinline__ void mw8t_cvt4(uint32_t v, uint32_t& lo, uint32_t& hi) {
  lo = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v, 1.0f, false));
  hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)v, 1.0f, true));
}

enum { MW8T_GATE_UP = 1, MW8T_DOWN = 2 };

struct MoeW8TallParams {
  const uint16_t* a;    // GATE_UP: x [T, K]; DOWN: act [cap, K]
  const uint8_t* q;     // GATE_UP: q1 [E, 2 N, K]; DOWN: q2 [E, N, K]
  const float* s;       // GATE_UP: s1 [E, 2 N / 128, K / 128]; DOWN: s2 [E, N / 128, K / 128]
  TallTables tb;
  uint16_t* act;        // GATE_UP out: [cap, N]
  float* partial;       // DOWN out: [P, W], the slab's columns
  const float* topk_w;  // [P]
  int K, N, topk;
  int c0, W;            // DOWN: the slab starts at column c0 of N (a multiple of 128); row pitch of `partial`
};

template <int MODE>
__global__ __launch_bounds__(64 * kMoeW8TWaves) void moe_w8_tall_gemm_kernel(const MoeW8TallParams p) {
  __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * kMoeW8TStage];
  const int item = blockIdx.y;
  if (item >= *p.tb.n_items) return;
  const int e = sgpr(p.tb.item_expert[item]), pos0 = sgpr(p.tb.item_pos[item]), nrb = sgpr(p.tb.item_blocks[item]);
  const int lane = threadIdx.x & 63, wave = sgpr(threadIdx.x >> 6);
  const int r = lane & 15, kg = lane >> 4;
  const int K = p.K, N = p.N, nblk = K / kMoeW8TBlock;

  // weights: lane (r, kg) of unit u reads q[row(u) + r, 128 b + 32 kg .. + 31]; the scale rows of the units' 128-row groups
  const int col = MODE == MW8T_GATE_UP ? 64 * (int)blockIdx.x + 16 * wave : p.c0 + 128 * (int)blockIdx.x + 32 * wave;
  const uint8_t* qp[2];
  const float* sp[2];
  if (MODE == MW8T_GATE_UP) {
    qp[0] = p.q + ((int64_t)e * 2 * N + col + r) * K + 32 * kg;
    qp[1] = qp[0] + (int64_t)N * K;
    sp[0] = p.s + ((int64_t)e * (2 * N / kMoeW8TBlock) + col / kMoeW8TBlock) * nblk;
    sp[1] = sp[0] + (int64_t)(N / kMoeW8TBlock) * nblk;
  } else {
    qp[0] = p.q + ((int64_t)e * N + col + r) * K + 32 * kg;
    qp[1] = qp[0] + (int64_t)16 * K;
    sp[0] = sp[1] = p.s + ((int64_t)e * (N / kMoeW8TBlock) + col / kMoeW8TBlock) * nblk;
  }

  // activation DMA: piece i of this wave = stage rows 16 i + 4 wave + (0 .. 3); this lane lands on slot r of row drow + 16 i
  // and fetches column r ^ (row & 15), row & 15 = drow.  xsrc[i] = the source row's first byte of that column, or null
  // (pad row, row past the item): no DMA, zeros in both stages
  const int drow = 4 * wave + kg;
  const unsigned char* xsrc[kMoeW8TPieces];
#pragma unroll
  for (int i = 0; i < kMoeW8TPieces; ++i) {
    const int row = drow + 16 * i;
    const int pair = i < nrb ? p.tb.sorted[pos0 + row] : -1;
    xsrc[i] = nullptr;
    if (pair >= 0)
      xsrc[i] = reinterpret_cast<const unsigned char*>(p.a) +
                (int64_t)(MODE == MW8T_GATE_UP ? pair / p.topk : pos0 + row) * K * 2 + ((r ^ drow) * 16);
    else {
      const int off = row * kMoeW8TRowBytes + r * 16;
      *reinterpret_cast<mw8t_u4*>(smem + off) = mw8t_u4{0u, 0u, 0u, 0u};
      *reinterpret_cast<mw8t_u4*>(smem + kMoeW8TStage + off) = mw8t_u4{0u, 0u, 0u, 0u};
    }
  }

  // fragment read offsets within a stage: row r of row block 0, column 4 kg + h at slot (4 kg + h) ^ r
  int fo[4];
#pragma unroll
  for (int h = 0; h < 4; ++h) fo[h] = r * kMoeW8TRowBytes + (((4 * kg + h) ^ r) * 16);

  auto load_w = [&](mw8t_u4 (&raw)[2][2], int b) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint8_t* src = qp[u] + (int64_t)b * kMoeW8TBlock;
      raw[u][0] = *reinterpret_cast<const mw8t_u4*>(src);
      raw[u][1] = *reinterpret_cast<const mw8t_u4*>(src + 16);
    }
  };
  auto issue_x = [&](int b, int buf) __attribute__((always_inline)) {
    unsigned char* sb = smem + buf * kMoeW8TStage + 4 * wave * kMoeW8TRowBytes;
#pragma unroll
    for (int i = 0; i < kMoeW8TPieces; ++i) {
      if (i < nrb) {  // wave-uniform: pieces of row blocks past the item issue nothing
        if (xsrc[i])
          __builtin_amdgcn_global_load_lds((mw8t_glb_t*)(xsrc[i] + (int64_t)b * kMoeW8TRowBytes),
                                           (mw8t_lds_t*)(sb + i * 16 * kMoeW8TRowBytes), 16, 0, 0);
      }
    }
  };

  mw8t_f32x4 acc[2][kTallItemBlocks];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int t = 0; t < kTallItemBlocks; ++t) acc[u][t] = mw8t_f32x4{0.f, 0.f, 0.f, 0.f};

  mw8t_u4 raw[2][2], nxt[2][2];
  load_w(raw, 0);
  issue_x(0, 0);
  int buf = 0;
  for (int b = 0; b < nblk; ++b) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of block b (and its weight lines) have landed
    __syncthreads();                                  // stage buf is whole; every wave is done with stage buf ^ 1
    if (b + 1 < nblk) {
      load_w(nxt, b + 1);
      issue_x(b + 1, buf ^ 1);
    }
    const float sc[2] = {sp[0][b], sp[1][b]};
    uint32_t a[2][8][2];  // [unit][dword of the lane's 32 bytes] -> 4 bf16
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int d = 0; d < 8; ++d) mw8t_cvt4(raw[u][d >> 2][d & 3], a[u][d][0], a[u][d][1]);
    const unsigned char* sb = smem + buf * kMoeW8TStage;
#pragma unroll
    for (int tp = 0; tp < kTallItemBlocks / 2; ++tp) {
      if (2 * tp >= nrb) break;  // wave-uniform
      mw8t_f32x4 pr[2][2];       // [row block of the pair][unit]
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) pr[t][u] = mw8t_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < 4; ++h) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const mw8t_u4 bv = *reinterpret_cast<const mw8t_u4*>(sb + (2 * tp + t) * 16 * kMoeW8TRowBytes + fo[h]);
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const mw8t_u4 av = {a[u][2 * h][0], a[u][2 * h][1], a[u][2 * h + 1][0], a[u][2 * h + 1][1]};
            pr[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mw8t_bf16x8, av),
                                                               __builtin_bit_cast(mw8t_bf16x8, bv), pr[t][u], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          mw8t_f32x4& c = acc[u][2 * tp + t];
          c.x = fmaf(sc[u], pr[t][u].x, c.x);
          c.y = fmaf(sc[u], pr[t][u].y, c.y);
          c.z = fmaf(sc[u], pr[t][u].z, c.z);
          c.w = fmaf(sc[u], pr[t][u].w, c.w);
        }
    }
    if (b + 1 < nblk) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        raw[u][0] = nxt[u][0];
        raw[u][1] = nxt[u][1];
      }
    }
    buf ^= 1;
  }

  // lane holds D[weight row 4 kg + i][token row r] in register i of each tile
#pragma unroll
  for (int t = 0; t < kTallItemBlocks; ++t)
    if (t < nrb) {
      const int pos = pos0 + kTallBM * t + r;
      const int pair = p.tb.sorted[pos];
      if (pair < 0) continue;
      if (MODE == MW8T_GATE_UP) {
        uint2 pk;
        pk.x = Elem<BF16>::pack(silu_mul_f32(acc[0][t].x, acc[1][t].x), silu_mul_f32(acc[0][t].y, acc[1][t].y));
        pk.y = Elem<BF16>::pack(silu_mul_f32(acc[0][t].z, acc[1][t].z), silu_mul_f32(acc[0][t].w, acc[1][t].w));
        *reinterpret_cast<uint2*>(p.act + (int64_t)pos * N + col + 4 * kg) = pk;
      } else {
        const float wgt = p.topk_w[pair];
        float* dst = p.partial + (int64_t)pair * p.W + (col - p.c0) + 4 * kg;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          float4 v;
          v.x = acc[u][t].x * wgt; v.y = acc[u][t].y * wgt; v.z = acc[u][t].z * wgt; v.w = acc[u][t].w * wgt;
          *reinterpret_cast<float4*>(dst + 16 * u) = v;
        }
      }
    }
}

}  // namespace msgl

using namespace msgl;

extern "C" int msgl_moe_w8_forward_tall(const void* x, const void* q1, const float* s1, const void* q2, const float* s2,
                                        const float* topk_weights, const int32_t* topk_ids, void* workspace,
                                        int64_t workspace_bytes, void* out, int T, int E, int k, int hidden, int I_l,
                                        void* stream) {
  MSGL_REQUIRE(x && q1 && s1 && q2 && s2 && topk_weights && topk_ids && out, "moe_w8_forward_tall: null pointer");
  int rc = tall_check_shape("moe_w8_forward_tall", T, E, k, hidden, I_l);
  if (rc != MSGL_OK) return rc;
  MSGL_REQUIRE(hidden % kMoeW8TBlock == 0 && I_l % kMoeW8TBlock == 0,
               "moe_w8_forward_tall: hidden = %d and the expert intermediate size %d must be multiples of the 128 x 128 scale "
               "block", hidden, I_l);
  const TallLayout L = tall_layout(T, E, k, I_l);
  MSGL_REQUIRE(L.max_items <= kTallMaxGridY, "moe_w8_forward_tall: %lld work items exceed one launch; split the tokens",
               (long long)L.max_items);
  int64_t W = tall_slab_room(L, workspace_bytes);
  MSGL_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0 && W >= 128,
               "moe_w8_forward_tall: needs %lld workspace bytes, 256-byte aligned", (long long)tall_min_bytes(L));
  if (W >= hidden) W = hidden;
  MSGL_REQUIRE(aligned16(x) && aligned16(q1) && aligned16(q2) && aligned16(out),
               "moe_w8_forward_tall: x, q1, q2 and out must be 16-byte aligned");
  MSGL_REQUIRE(((reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2)) & 3u) == 0,
               "moe_w8_forward_tall: the scale grids must be 4-byte aligned");
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const TallTables tb = tall_tables(ws, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  rc = tall_launch_align("moe_w8_forward_tall(align)", tb, L, topk_ids, E, s);
  if (rc != MSGL_OK) return rc;

  MoeW8TallParams g;
  g.tb = tb;
  g.act = reinterpret_cast<uint16_t*>(ws + L.o_act);
  g.partial = reinterpret_cast<float*>(ws + L.o_partial);
  g.topk_w = topk_weights;
  g.topk = k;
  g.c0 = 0; g.W = 0;
  g.a = static_cast<const uint16_t*>(x); g.q = static_cast<const uint8_t*>(q1); g.s = s1; g.K = hidden; g.N = I_l;
  const dim3 block(64 * kMoeW8TWaves);
  moe_w8_tall_gemm_kernel<MW8T_GATE_UP><<<dim3((unsigned)(I_l / 64), (unsigned)L.max_items), block, 0, s>>>(g);
  MSGL_CHECK_LAUNCH("moe_w8_forward_tall(gate_up)");
  g.a = g.act; g.q = static_cast<const uint8_t*>(q2); g.s = s2; g.K = I_l; g.N = hidden; g.W = (int)W;
  for (int c0 = 0; c0 < hidden; c0 += (int)W) {  // W and hidden are multiples of 128: so is every slab
    const int wcols = hidden - c0 < (int)W ? hidden - c0 : (int)W;
    g.c0 = c0;
    moe_w8_tall_gemm_kernel<MW8T_DOWN><<<dim3((unsigned)(wcols / 128), (unsigned)L.max_items), block, 0, s>>>(g);
    MSGL_CHECK_LAUNCH("moe_w8_forward_tall(down)");
    rc = tall_launch_sum("moe_w8_forward_tall(sum)", static_cast<uint16_t*>(out), g.partial, topk_ids, T, k, E, hidden, c0,
                         wcols, (int)W, s);
    if (rc != MSGL_OK) return rc;
  }
  return MSGL_OK;
}
