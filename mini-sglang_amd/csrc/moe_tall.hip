// The expert MLP of csrc/moe.hip for prefill-sized batches, where an expert's run of (token, slot) pairs is hundreds of rows
// long.  Same arithmetic, bit for bit (v_mfma_f32_16x16x32_bf16 with weights as A and tokens as B, one accumulator per
// (pair, column), k ascending in 32 J-wide steps with the in-step permutation of moe_gemm_kernel, silu_mul_f32 on the fp32
// accumulators, fp32 partial x routing weight, slot-ordered sum rounded once), different data movement:
//
//   align    three launches over SEGMENTS of 1024 pairs (four waves x 256 pairs): count (a wave ranks its pairs among
//            those of the same expert with ballots and writes its per-expert counts), scan (one workgroup: per expert an
//            exclusive prefix over all wave segments, then over experts the padded run offsets and the item tables), scatter
//            (sorted[off[e] + prefix[wave segment][e] + rank] = pair).  Stable in pair index, runs padded to 16 with -1:
//            the `sorted` of moe_align_kernel.  No atomics; every table entry has exactly one writer.
//   items    an expert's run is cut into items of up to 256 rows (sixteen 16-row blocks).
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
#include "common.h"

namespace msgl {

typedef __attribute__((ext_vector_type(4))) float tall_f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 tall_bf16x8;

constexpr int kTallMaxExperts = 256;
constexpr int kTallMaxTopk = 8;
constexpr int kTallBM = 16;          // row-block height, as kMoeBM
constexpr int kTallItemBlocks = 16;  // row blocks per item
constexpr int kTallItemRows = kTallBM * kTallItemBlocks;
constexpr int kTallWRows = 128;      // weight rows per workgroup
constexpr int kTallRows = kTallItemRows + kTallWRows;  // LDS rows per stage
constexpr int kTallSegWaves = 4;
constexpr int kTallWavePairs = 256;  // pairs per wave segment
constexpr int kTallMaxGridY = 65535;

struct TallTables {
  int32_t* sorted;       // [cap]  as MoeTables::sorted
  int32_t* lpos;         // [P]    a pair's rank among its wave segment's pairs of the same expert
  int32_t* cnt;          // [wave segments, E]  count, then exclusive prefix over wave segments
  int32_t* off;          // [256]  first position of an expert's run
  int32_t* item_expert;  // [max_items]
  int32_t* item_pos;     // [max_items]
  int32_t* item_blocks;  // [max_items]  1 .. 16 row blocks
  int32_t* n_items;      // [1]
};

// ---------------------------------------------------------------------------------------------------------------- align
__global__ __launch_bounds__(64 * kTallSegWaves) void moe_tall_count_kernel(const TallTables tb, const int32_t* __restrict__ ids,
                                                                            int P, int E) {
  __shared__ int cnt[kTallSegWaves][kTallMaxExperts];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < kTallSegWaves * kTallMaxExperts; i += blockDim.x) (&cnt[0][0])[i] = 0;
  __syncthreads();
  const int sub = blockIdx.x * kTallSegWaves + wv;
  const int lo = sub * kTallWavePairs, hi = min(P, lo + kTallWavePairs);
  for (int base = lo; base < hi; base += 64) {
    const int i = base + lane;
    int e = i < hi ? ids[i] : -1;
    if (e < 0 || e >= E) e = -1;
    bool todo = e >= 0;
    int lp = 0;
    while (true) {  // one round per distinct expert among the 64 pairs, in order of first appearance
      const unsigned long long m = __ballot(todo);
      if (!m) break;
      const int le = __shfl(e, __ffsll(m) - 1, 64);
      const bool mine = todo && e == le;
      const unsigned long long same = __ballot(mine);
      const int before = cnt[wv][le];
      if (mine) {
        lp = before + __popcll(same & ((1ull << lane) - 1ull));
        todo = false;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      if (lane == 0) cnt[wv][le] = before + __popcll(same);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    if (e >= 0) tb.lpos[i] = lp;
  }
  __syncthreads();
  for (int e = lane; e < E; e += 64) tb.cnt[(int64_t)sub * E + e] = cnt[wv][e];
}

// one workgroup of sixteen waves: wave w scans experts w, w + 16, ... over the wave segments (64 per round, wave prefix sum)
__global__ __launch_bounds__(1024) void moe_tall_scan_kernel(const TallTables tb, int nsub, int E) {
  __shared__ int num[kTallMaxExperts], off[kTallMaxExperts], ioff[kTallMaxExperts];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid < kTallMaxExperts) num[tid] = 0;
  __syncthreads();
  for (int e = wv; e < E; e += 16) {
    int run = 0;
    for (int s0 = 0; s0 < nsub; s0 += 64) {
      const int s = s0 + lane;
      const int c = s < nsub ? tb.cnt[(int64_t)s * E + e] : 0;
      int inc = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int a = __shfl_up(inc, d, 64);
        if (lane >= d) inc += a;
      }
      if (s < nsub) tb.cnt[(int64_t)s * E + e] = run + inc - c;
      run += __shfl(inc, 63, 64);
    }
    if (lane == 0) num[e] = run;
  }
  __syncthreads();
  if (wv == 0) {  // exclusive scans over experts (four per lane) of the padded run lengths and of the item counts
    int pad[4], its[4], ps = 0, is = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = num[4 * lane + j];
      pad[j] = (n + kTallBM - 1) / kTallBM * kTallBM;
      its[j] = (n + kTallItemRows - 1) / kTallItemRows;
      ps += pad[j];
      is += its[j];
    }
    int pi = ps, ii = is;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int a = __shfl_up(pi, d, 64), b = __shfl_up(ii, d, 64);
      if (lane >= d) {
        pi += a;
        ii += b;
      }
    }
    int po = pi - ps, io = ii - is;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      off[4 * lane + j] = po;
      ioff[4 * lane + j] = io;
      po += pad[j];
      io += its[j];
    }
    if (lane == 63) *tb.n_items = ii;
  }
  __syncthreads();
  if (tid < E) {
    const int n = num[tid], padded = (n + kTallBM - 1) / kTallBM * kTallBM;
    tb.off[tid] = off[tid];
    for (int q = 0; q * kTallItemRows < n; ++q) {
      tb.item_expert[ioff[tid] + q] = tid;
      tb.item_pos[ioff[tid] + q] = off[tid] + q * kTallItemRows;
      tb.item_blocks[ioff[tid] + q] = min(kTallItemBlocks, (padded - q * kTallItemRows) / kTallBM);
    }
    for (int i = n; i < padded; ++i) tb.sorted[off[tid] + i] = -1;
  }
}

__global__ __launch_bounds__(64 * kTallSegWaves) void moe_tall_scatter_kernel(const TallTables tb,
                                                                              const int32_t* __restrict__ ids, int P, int E) {
  const int lane = threadIdx.x & 63;
  const int sub = blockIdx.x * kTallSegWaves + (threadIdx.x >> 6);
  const int lo = sub * kTallWavePairs, hi = min(P, lo + kTallWavePairs);
  for (int i = lo + lane; i < hi; i += 64) {
    const int e = ids[i];
    if (e >= 0 && e < E) tb.sorted[tb.off[e] + tb.cnt[(int64_t)sub * E + e] + tb.lpos[i]] = i;
  }
}

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

// out[t][c0 + c] = bf16(sum over slots, in slot order, of partial[t k + slot][c]) for the slab's columns; eight per thread
__global__ __launch_bounds__(256) void moe_tall_sum_kernel(uint16_t* __restrict__ out, const float* __restrict__ partial,
                                                           const int32_t* __restrict__ ids, int T, int k, int E, int hidden,
                                                           int c0, int wcols, int W) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per_row = wcols >> 3;
  if (gid >= (int64_t)T * per_row) return;
  const int t = (int)(gid / per_row), c = (int)(gid - (int64_t)t * per_row) * 8;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int slot = 0; slot < k; ++slot) {
    const int64_t pair = (int64_t)t * k + slot;
    const int e = ids[pair];
    if (e < 0 || e >= E) continue;
    const float* q = partial + pair * W + c;
    const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 4);
    s[0] += a.x; s[1] += a.y; s[2] += a.z; s[3] += a.w;
    s[4] += b.x; s[5] += b.y; s[6] += b.z; s[7] += b.w;
  }
  stg16(out + (int64_t)t * hidden + c0 + c, pack8<BF16>(s));
}

// ---------------------------------------------------------------------------------------------------------------- host
static inline int64_t tall_up256(int64_t n) { return (n + 255) / 256 * 256; }

struct TallLayout {
  int64_t P, cap, max_items, nseg;
  int64_t o_sorted, o_lpos, o_cnt, o_off, o_iexp, o_ipos, o_iblk, o_nitems, o_act, o_partial;  // o_partial = the fixed part
};

// a pure function of the shapes: positions <= P + 15 min(E, P); every item but an expert's last holds 256 pairs
static TallLayout tall_layout(int64_t T, int64_t E, int64_t k, int64_t I) {
  TallLayout L;
  const int64_t P = T * k, ne = E < P ? E : P;
  L.P = P;
  L.cap = P + (kTallBM - 1) * ne;
  L.max_items = ne + P / kTallItemRows;
  L.nseg = (P + kTallSegWaves * kTallWavePairs - 1) / (kTallSegWaves * kTallWavePairs);
  int64_t o = 0;
  L.o_sorted = o; o += tall_up256(L.cap * 4);
  L.o_lpos = o; o += tall_up256(P * 4);
  L.o_cnt = o; o += tall_up256(L.nseg * kTallSegWaves * E * 4);
  L.o_off = o; o += tall_up256(kTallMaxExperts * 4);
  L.o_iexp = o; o += tall_up256(L.max_items * 4);
  L.o_ipos = o; o += tall_up256(L.max_items * 4);
  L.o_iblk = o; o += tall_up256(L.max_items * 4);
  L.o_nitems = o; o += 256;
  L.o_act = o; o += tall_up256(L.cap * I * 2);
  L.o_partial = o;
  return L;
}

static int tall_check_shape(const char* who, int64_t T, int64_t E, int64_t k, int64_t hidden, int64_t I) {
  MSGL_REQUIRE(T >= 1 && T * k < (1ll << 30), "%s: T = %lld outside [1, 2^30 / k)", who, (long long)T);
  MSGL_REQUIRE(E >= 1 && E <= kTallMaxExperts, "%s: E = %lld outside [1, %d]", who, (long long)E, kTallMaxExperts);
  MSGL_REQUIRE(k >= 1 && k <= kTallMaxTopk && k <= E, "%s: k = %lld outside [1, min(%d, E)]", who, (long long)k, kTallMaxTopk);
  MSGL_REQUIRE(hidden >= 64 && hidden % 64 == 0, "%s: hidden = %lld must be a multiple of 64", who, (long long)hidden);
  MSGL_REQUIRE(I >= 32 && I % 32 == 0, "%s: the expert intermediate size %lld must be a multiple of 32", who, (long long)I);
  return MSGL_OK;
}

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
  const TallLayout L = tall_layout(T, E, k, I_l);
  return L.o_partial + tall_up256(L.P * 128 * 4);
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
  // the widest column slab whose fp32 partials fit behind the tables and act: a multiple of 128, or all of hidden
  const int64_t room = workspace_bytes - L.o_partial;
  int64_t W = room > 0 ? room / (L.P * 4) / 128 * 128 : 0;
  MSGL_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0 && W >= 128,
               "moe_forward_tall: needs %lld workspace bytes, 256-byte aligned",
               (long long)(L.o_partial + tall_up256(L.P * 128 * 4)));
  if (W >= hidden) W = hidden;
  MSGL_REQUIRE(aligned16(x) && aligned16(w1) && aligned16(w2) && aligned16(out),
               "moe_forward_tall: pointers must be 16-byte aligned");
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  TallTables tb;
  tb.sorted = reinterpret_cast<int32_t*>(ws + L.o_sorted);
  tb.lpos = reinterpret_cast<int32_t*>(ws + L.o_lpos);
  tb.cnt = reinterpret_cast<int32_t*>(ws + L.o_cnt);
  tb.off = reinterpret_cast<int32_t*>(ws + L.o_off);
  tb.item_expert = reinterpret_cast<int32_t*>(ws + L.o_iexp);
  tb.item_pos = reinterpret_cast<int32_t*>(ws + L.o_ipos);
  tb.item_blocks = reinterpret_cast<int32_t*>(ws + L.o_iblk);
  tb.n_items = reinterpret_cast<int32_t*>(ws + L.o_nitems);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int P = T * k;
  const dim3 seg_grid((unsigned)L.nseg), seg_block(64 * kTallSegWaves);
  moe_tall_count_kernel<<<seg_grid, seg_block, 0, s>>>(tb, topk_ids, P, E);
  MSGL_CHECK_LAUNCH("moe_forward_tall(count)");
  moe_tall_scan_kernel<<<dim3(1), dim3(1024), 0, s>>>(tb, (int)(L.nseg * kTallSegWaves), E);
  MSGL_CHECK_LAUNCH("moe_forward_tall(scan)");
  moe_tall_scatter_kernel<<<seg_grid, seg_block, 0, s>>>(tb, topk_ids, P, E);
  MSGL_CHECK_LAUNCH("moe_forward_tall(scatter)");

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
    const int64_t threads = (int64_t)T * (wcols / 8);
    moe_tall_sum_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(
        static_cast<uint16_t*>(out), g.partial, topk_ids, T, k, E, hidden, c0, wcols, (int)W);
    MSGL_CHECK_LAUNCH("moe_forward_tall(sum)");
  }
  return MSGL_OK;
}
