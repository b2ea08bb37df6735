// The expert MLP of csrc/moe.hip for prefill-sized batches, where an expert's run of (token, slot) pairs is hundreds of rows
// long.  Same arithmetic, bit for bit (v_mfma_f32_16x16x32_bf16 with weights as A and tokens as B, one accumulator per
// (pair, column), k ascending in 32 J-wide steps with the in-step permutation of moe_gemm_kernel, silu_mul_f32 on the fp32
// accumulators, fp32 partial x routing weight, slot-ordered sum rounded once), different data movement:
//
//   align    the three-launch align and the 256-row item tables of moe_tall_tables.h.
//   GEMMs    workgroup = 128 weight rows x one item, four waves as 2 (weight halves of 64 rows) x 2 (token halves of 128 rows),
//            4 x 8 accumulator tiles = 128 registers per lane.  BOTH operands pass through LDS in 32 J-k steps, double
//            buffered: a step's 384 rows (256 token rows gathered by token / act rows, 128 weight rows) are fetched into
//            registers two steps ahead of their MFMAs and written to the other buffer one step ahead, one barrier per
//            step.  A weight byte is fetched once per item instead of once per wave: 48 KB per 64-k step for 4.2 MFLOP,
//            about 115 B/ns per CU at the full MFMA rate against 150 B/ns for a 128 x 128 tile.  In the gate/up GEMM a wave's
//            64 weight rows are the gate rows and the up rows of the same 32 features, so SiLU.mul stays on the accumulators.
//   grid     (column tile, item), x fastest: the workgroups of an item, then of the expert's next item, are adjacent in
//            launch order, so the ~250 workgroups in flight cover about ten experts and an expert's second and later items
//            find its weights in L2 or the Infinity Cache.  grid.y is the shape's upper bound on items; a workgroup past
//            the device-side item count exits (graph capture).
//   partials the down GEMM and the sum run per COLUMN SLAB of `hidden`, W columns (a multiple of 128, the last slab may be
//            narrower), W the widest that fits the caller's workspace: scratch = tables + act + P x W x 4 bytes.
#include "moe_tall_tables.h"

namespace msgl {

typedef __attribute__((ext_vector_type(4))) float tall_f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 tall_bf16x8;

constexpr int kTallWRows = 128;      // weight rows per workgroup
constexpr int kTallRows = kTallItemRows + kTallWRows;  // LDS rows per stage

// ---------------------------------------------------------------------------------------------------------------- GEMMs
enum { TALL_GATE_UP = 1, TALL_DOWN = 2 };

struct TallGemmParams {
  const uint16_t* a;    // TALL_GATE_UP: x [T, K]; TALL_DOWN: act [cap, K]
  const uint16_t* w;    // TALL_GATE_UP: w1 [E, 2 N, K]; TALL_DOWN: w2 [E, N, K]
  TallTables tb;
  uint16_t* act;        // TALL_GATE_UP out: [cap, N]
  float* partial;       // TALL_DOWN out: [P, W], the slab's columns
  const float* topk_w;  // [P]
  int K, N, topk;
  int c0, c_end, W;     // TALL_DOWN: the slab is columns [c0, c_end) of N (multiples of 64); row pitch of `partial`
};

template <int J>
struct TallGeom {
  static constexpr int kStepK = 32 * J;
  static constexpr int kRowBytes = 2 * kStepK + 16;  // +16: consecutive rows start four banks apart
  static constexpr int kStageBytes = kTallRows * kRowBytes;
  static constexpr int kPiecesPerRow = 4 * J;        // 16-byte pieces
  static constexpr int kRowStep = 256 / kPiecesPerRow;  // rows between two pieces of one thread
  static constexpr int kPieces = kTallRows / kRowStep;  // per thread and step: 12 (J = 2) / 6 (J = 1)
  static constexpr int kTokenPieces = kTallItemRows / kRowStep;
  static constexpr int kLdsBytes = 2 * kStageBytes;
};

template <int MODE, int J>
__global__ __launch_bounds__(256) void moe_tall_gemm_kernel(const TallGemmParams p) {
  using G = TallGeom<J>;
  extern __shared__ __attribute__((aligned(16))) unsigned char tall_lds[];
  const int item = blockIdx.y;
  if (item >= *p.tb.n_items) return;
  const int e = sgpr(p.tb.item_expert[item]), pos0 = sgpr(p.tb.item_pos[item]), nrb = sgpr(p.tb.item_blocks[item]);
  const int tid = threadIdx.x, lane = tid & 63, wv = sgpr(tid >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int wr = wv & 1, tc = wv >> 1;  // weight half (64 rows), token half (128 rows)
  const int K = p.K, N = p.N;

  // the sources of this thread's pieces: LDS row prow + kRowStep i, bytes 16 pc ..; rows 0 .. 255 are the item's token rows,
  // rows 256 .. 383 the weight rows (wave half wr: tiles 0, 1 = gate and 2, 3 = up rows of 32 features / 64 columns)
  const int prow = tid / G::kPiecesPerRow, pc = tid % G::kPiecesPerRow;
  const uint16_t* src[G::kPieces];
#pragma unroll
  for (int i = 0; i < G::kPieces; ++i) {
    const int row = prow + G::kRowStep * i;
    src[i] = nullptr;  // zeros: pad rows, rows past the item, weight rows past the matrix
    if (i < G::kTokenPieces) {
      const int pair = row < kTallBM * nrb ? p.tb.sorted[pos0 + row] : -1;
      if (pair >= 0) src[i] = p.a + (int64_t)(MODE == TALL_GATE_UP ? pair / p.topk : pos0 + row) * K + 8 * pc;
    } else {
      const int r = row - kTallItemRows;
      if (MODE == TALL_GATE_UP) {
        const int f = 64 * blockIdx.x + 32 * (r >> 6) + 16 * ((r >> 4) & 1) + (r & 15);
        if (f < N) src[i] = p.w + ((int64_t)e * 2 * N + (int64_t)((r >> 5) & 1) * N + f) * K + 8 * pc;
      } else {
        const int c = p.c0 + 128 * blockIdx.x + r;
        if (c < p.c_end) src[i] = p.w + ((int64_t)e * N + c) * K + 8 * pc;
      }
    }
  }
  const bool active = MODE == TALL_GATE_UP ? 64 * (int)blockIdx.x + 32 * wr < N : p.c0 + 128 * (int)blockIdx.x + 64 * wr < p.c_end;
  const int nlive = sgpr(min(8, max(0, nrb - 8 * tc)));  // this wave's live 16-row blocks

  tall_f32x4 acc[4][8];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[t][b] = tall_f32x4{0.f, 0.f, 0.f, 0.f};

  // two steps are in flight: while step s is multiplied, step s + 1 sits in registers and step s + 2 is on its way from
  // memory (one wave per SIMD: nothing else hides that latency).  Register set and LDS buffer of step s = s & 1.
  U4 st[2][G::kPieces];
  auto fetch = [&](U4 (&r)[G::kPieces], int step) {
#pragma unroll
    for (int i = 0; i < G::kPieces; ++i) {
      r[i] = U4{0u, 0u, 0u, 0u};
      if (src[i]) r[i] = ldg16(src[i] + step * G::kStepK);
    }
  };
  auto stage = [&](const U4 (&r)[G::kPieces], int buf) {
    unsigned char* dst = tall_lds + buf * G::kStageBytes + prow * G::kRowBytes + 16 * pc;
#pragma unroll
    for (int i = 0; i < G::kPieces; ++i) *reinterpret_cast<U4*>(dst + G::kRowStep * i * G::kRowBytes) = r[i];
  };
  auto multiply = [&](int buf) {
    if (!active) return;
    const unsigned char* base = tall_lds + buf * G::kStageBytes + r16 * G::kRowBytes + q4 * 16 * J;
    U4 a[4][J];  // lane group q holds k = 8 J q + 8 j + 0..7 of the step for MFMA j
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int j = 0; j < J; ++j)
        a[t][j] = *reinterpret_cast<const U4*>(base + (kTallItemRows + 64 * wr + 16 * t) * G::kRowBytes + 16 * j);
#pragma unroll
    for (int b = 0; b < 8; ++b)
      if (b < nlive) {
#pragma unroll
        for (int j = 0; j < J; ++j) {
          const U4 bf = *reinterpret_cast<const U4*>(base + (128 * tc + 16 * b) * G::kRowBytes + 16 * j);
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc[t][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(tall_bf16x8, a[t][j]),
                                                                __builtin_bit_cast(tall_bf16x8, bf), acc[t][b], 0, 0, 0);
        }
      }
  };

  const int nsteps = K / G::kStepK;
  fetch(st[0], 0);
  if (nsteps > 1) fetch(st[1], 1);
  stage(st[0], 0);
  if (nsteps > 2) fetch(st[0], 2);
  __syncthreads();
  for (int s = 0; s < nsteps; s += 2) {
    multiply(0);
    if (s + 1 < nsteps) stage(st[1], 1);  // buffer 1 was last read in step s - 1, before the previous barrier
    if (s + 3 < nsteps) fetch(st[1], s + 3);
    __syncthreads();
    if (s + 1 < nsteps) {
      multiply(1);
      if (s + 2 < nsteps) stage(st[0], 0);
      if (s + 4 < nsteps) fetch(st[0], s + 4);
      __syncthreads();
    }
  }
  if (!active) return;
  // lane holds D[weight row 4 q4 + i][token row r16] in register i of each tile
#pragma unroll
  for (int b = 0; b < 8; ++b)
    if (b < nlive) {
      const int pos = pos0 + 128 * tc + kTallBM * b + r16;
      const int pair = p.tb.sorted[pos];
      if (pair < 0) continue;
      if (MODE == TALL_GATE_UP) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          uint2 pk;
          pk.x = Elem<BF16>::pack(silu_mul_f32(acc[t][b][0], acc[t + 2][b][0]), silu_mul_f32(acc[t][b][1], acc[t + 2][b][1]));
          pk.y = Elem<BF16>::pack(silu_mul_f32(acc[t][b][2], acc[t + 2][b][2]), silu_mul_f32(acc[t][b][3], acc[t + 2][b][3]));
          *reinterpret_cast<uint2*>(p.act + (int64_t)pos * N + 64 * blockIdx.x + 32 * wr + 16 * t + 4 * q4) = pk;
        }
      } else {
        const float wgt = p.topk_w[pair];
        float* dst = p.partial + (int64_t)pair * p.W + 128 * blockIdx.x + 64 * wr + 4 * q4;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          float4 v;
          v.x = acc[t][b][0] * wgt; v.y = acc[t][b][1] * wgt; v.z = acc[t][b][2] * wgt; v.w = acc[t][b][3] * wgt;
          *reinterpret_cast<float4*>(dst + 16 * t) = v;
        }
      }
    }
}

// ---------------------------------------------------------------------------------------------------------------- host
template <int MODE, int J>
static int tall_launch_gemm(const TallGemmParams& g, unsigned tiles, unsigned items, hipStream_t s) {
  auto* kernel = &moe_tall_gemm_kernel<MODE, J>;
  static PerDeviceOnce lds_attr;  // per instantiation and device: more than 64 KB of dynamic LDS has to be requested
  if (TallGeom<J>::kLdsBytes > 65536 && !lds_attr.ensure([&] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   TallGeom<J>::kLdsBytes) == hipSuccess;
      })) {
    set_error("moe_forward_tall: cannot reserve %d bytes of LDS: %s", TallGeom<J>::kLdsBytes,
              hipGetErrorString(hipGetLastError()));
    return MSGL_ELAUNCH;
  }
  kernel<<<dim3(tiles, items), dim3(256), TallGeom<J>::kLdsBytes, s>>>(g);
  MSGL_CHECK_LAUNCH("moe_forward_tall(gemm)");
  return MSGL_OK;
}

}  // namespace msgl

using namespace msgl;

extern "C" int64_t msgl_moe_workspace_bytes_tall(int T, int E, int k, int hidden, int I_l) {
  const int rc = tall_check_shape("moe_workspace_bytes_tall", T, E, k, hidden, I_l);
  if (rc != MSGL_OK) return rc;
  return tall_min_bytes(tall_layout(T, E, k, I_l));
}

extern "C" int msgl_moe_forward_tall(const void* x, const void* w1, const void* w2, const float* topk_weights,
                                     const int32_t* topk_ids, void* workspace, int64_t workspace_bytes, void* out, int T,
                                     int E, int k, int hidden, int I_l, void* stream) {
  MSGL_REQUIRE(x && w1 && w2 && topk_weights && topk_ids && out, "moe_forward_tall: null pointer");
  int rc = tall_check_shape("moe_forward_tall", T, E, k, hidden, I_l);
  if (rc != MSGL_OK) return rc;
  const TallLayout L = tall_layout(T, E, k, I_l);
  MSGL_REQUIRE(L.max_items <= kTallMaxGridY, "moe_forward_tall: %lld work items exceed one launch; split the tokens",
               (long long)L.max_items);
  int64_t W = tall_slab_room(L, workspace_bytes);
  MSGL_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0 && W >= 128,
               "moe_forward_tall: needs %lld workspace bytes, 256-byte aligned", (long long)tall_min_bytes(L));
  if (W >= hidden) W = hidden;
  MSGL_REQUIRE(aligned16(x) && aligned16(w1) && aligned16(w2) && aligned16(out),
               "moe_forward_tall: pointers must be 16-byte aligned");
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const TallTables tb = tall_tables(ws, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  rc = tall_launch_align("moe_forward_tall(align)", tb, L, topk_ids, E, s);
  if (rc != MSGL_OK) return rc;

  TallGemmParams g;
  g.tb = tb;
  g.act = reinterpret_cast<uint16_t*>(ws + L.o_act);
  g.partial = reinterpret_cast<float*>(ws + L.o_partial);
  g.topk_w = topk_weights;
  g.topk = k;
  g.c0 = 0; g.c_end = 0; g.W = 0;
  g.a = static_cast<const uint16_t*>(x); g.w = static_cast<const uint16_t*>(w1); g.K = hidden; g.N = I_l;
  rc = tall_launch_gemm<TALL_GATE_UP, 2>(g, (unsigned)((I_l + 63) / 64), (unsigned)L.max_items, s);
  if (rc != MSGL_OK) return rc;
  g.a = g.act; g.w = static_cast<const uint16_t*>(w2); g.K = I_l; g.N = hidden; g.W = (int)W;
  for (int c0 = 0; c0 < hidden; c0 += (int)W) {
    const int wcols = hidden - c0 < (int)W ? hidden - c0 : (int)W;
    g.c0 = c0; g.c_end = c0 + wcols;
    const unsigned tiles = (unsigned)((wcols + 127) / 128);
    rc = I_l % 64 == 0 ? tall_launch_gemm<TALL_DOWN, 2>(g, tiles, (unsigned)L.max_items, s)
                       : tall_launch_gemm<TALL_DOWN, 1>(g, tiles, (unsigned)L.max_items, s);
    if (rc != MSGL_OK) return rc;
    rc = tall_launch_sum("moe_forward_tall(sum)", static_cast<uint16_t*>(out), g.partial, topk_ids, T, k, E, hidden, c0, wcols,
                         (int)W, s);
    if (rc != MSGL_OK) return rc;
  }
  return MSGL_OK;
}
