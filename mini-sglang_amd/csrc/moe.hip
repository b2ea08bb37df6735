// Mixture-of-experts MLP (Qwen3-MoE), bf16 with fp32 accumulation: the reference's FusedMoe.forward (P/moe/fused.py:230-256,
// activation "silu", router weight applied to the OUTPUT) as five launches whose grids depend on (T, k, E, shape) only:
//
//   route    fp32 softmax over E, the k largest probabilities (ties: lowest expert), optional renormalisation.  One wave per
//            token, four experts per lane, wave reductions, no LDS.                                  (P/moe/fused.py:9-28)
//   align    ONE workgroup sorts the T k (token, slot) pairs by expert, stable in pair index, every expert's run padded to
//            the row-block height 16 (pad entries = -1), and cuts the runs into ITEMS of up to four row blocks (64 rows):
//            item -> (expert, first position, row blocks), plus the item count, all in device memory.  Sixteen waves own
//            sixteen contiguous pair segments; a wave ranks the pairs of a 64-pair round with ballots and keeps its
//            per-expert counts in LDS, so the scatter needs no atomics and no order-dependent step.  (moe_align_block_size)
//   gemm 1   act[pos, f] = silu(x[token] . w1[e][f]) * (x[token] . w1[e][I + f]).  Workgroup = (64-feature tile, item).
//   gemm 2   partial[pair, c] = (act[pos] . w2[e][c]) * weight[pair], fp32.      Workgroup = (128-column tile, item).
//   sum      out[t] = bf16(partial[t k + 0] + ... + partial[t k + k - 1]) in slot order.
//
// The grouped GEMMs share one kernel.  grid = (column tiles, upper bound on items): a workgroup past the device-side item
// count exits, so the launch never depends on the routing (graph capture).  An item's rows are staged through LDS in
// 256-k chunks (gathered by token in gemm 1; pad rows are zeros), shared by the four waves; a wave owns 16 features
// (gemm 1: the gate AND the up row of each, so SiLU.mul happens on the accumulators and the [pairs, 2 I] intermediate never
// exists; w1 keeps the reference's [gate; up] row order) or 32 columns (gemm 2) and streams ITS weight rows from HBM
// straight into registers, a whole chunk (sixteen 1-KB loads per wave) requested before the chunk's rows are staged.  The k loop is
// outermost: all four row blocks' accumulators stay live, so an expert with <= 64 rows -- every decode batch -- has each
// weight byte read from HBM once per launch; longer runs are further items of the same kernel (their re-reads hit L2).
// MFMA v_mfma_f32_16x16x32_bf16 with weights as A and tokens as B, as gemm_ro.hip; the k index inside a 32 J-k step is
// permuted (lane group q holds k = 8 J q + 8 j + 0..7 for MFMA j) so that a lane loads 16 J contiguous bytes and four lanes a
// full 64 J-byte run of a weight row.  J = 2 where K % 64 == 0, else 1 (I_l = 96).
//
// A pair's result depends on its own row only: k in order, one accumulator per (pair, column), slots added in order.  Hence
// bit-repeatable and independent of the rest of the batch.  No float atomics anywhere.
#include "moe_tables.h"

namespace msgl {

typedef __attribute__((ext_vector_type(4))) float moe_f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 moe_bf16x8;

constexpr int kMoeChunkK = 256;        // k extent of one LDS stage
constexpr int kMoeRowBytes = kMoeChunkK * 2 + 16;  // +16: consecutive rows start four banks apart

// ---------------------------------------------------------------------------------------------------------------- route
template <bool kF32>
__global__ __launch_bounds__(256) void moe_route_kernel(float* __restrict__ weights, int32_t* __restrict__ ids,
                                                        const void* __restrict__ logits, int T, int E, int k, int renorm) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  float p[4];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = lane + 64 * j;
    float v = -INFINITY;
    if (e < E) {
      if (kF32)
        v = static_cast<const float*>(logits)[(int64_t)t * E + e];
      else
        v = __uint_as_float((uint32_t) static_cast<const uint16_t*>(logits)[(int64_t)t * E + e] << 16);
    }
    p[j] = v;
    mx = fmaxf(mx, v);
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    p[j] = lane + 64 * j < E ? expf(p[j] - mx) : 0.f;
    sum += p[j];
  }
  sum = __shfl(wave_sum(sum), 0, 64);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float q = p[j] / sum;
    p[j] = q >= 0.f ? q : 0.f;  // a NaN row still selects k valid experts
  }
  unsigned taken = 0;
  float wsel = 0.f, wsum = 0.f;  // lane i keeps selection i
  int isel = 0;
  for (int it = 0; it < k; ++it) {
    float bp = -1.f;
    int be = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = lane + 64 * j;
      if (e < E && !(taken & (1u << j)) && p[j] > bp) {  // ascending e: the lowest index wins a tie
        bp = p[j];
        be = e;
      }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float op = __shfl_xor(bp, d, 64);
      const int oe = __shfl_xor(be, d, 64);
      if (op > bp || (op == bp && oe < be)) {
        bp = op;
        be = oe;
      }
    }
    if ((be & 63) == lane) taken |= 1u << (be >> 6);
    if (lane == it) {
      wsel = bp;
      isel = be;
    }
    wsum += bp;  // selection order, the same on every lane
  }
  if (lane < k) {
    weights[(int64_t)t * k + lane] = renorm ? wsel / (wsum + 1e-8f) : wsel;
    ids[(int64_t)t * k + lane] = isel;
  }
}

// ---------------------------------------------------------------------------------------------------------------- align
__global__ __launch_bounds__(64 * kMoeAlignWaves) void moe_align_kernel(const MoeTables tb, const int32_t* __restrict__ ids,
                                                                        int P, int E) {
  __shared__ int cnt[kMoeAlignWaves][kMoeMaxExperts];  // per (wave segment, expert): count, then exclusive prefix over waves
  __shared__ int num[kMoeMaxExperts], off[kMoeMaxExperts], ioff[kMoeMaxExperts];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < kMoeAlignWaves * kMoeMaxExperts; i += blockDim.x) (&cnt[0][0])[i] = 0;
  __syncthreads();
  const int seg = ((P + kMoeAlignWaves - 1) / kMoeAlignWaves + 63) / 64 * 64;
  const int lo = wv * seg, hi = min(P, lo + seg);
  for (int base = lo; base < hi; base += 64) {
    const int i = base + lane;
    int e = i < hi ? ids[i] : -1;
    if (e < 0 || e >= E) e = -1;  // a pair with no valid expert contributes nothing (moe_sum_kernel skips it too)
    bool todo = e >= 0;
    int lp = 0;
    while (true) {
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
  if (tid < kMoeMaxExperts) {
    int run = 0;
    for (int w = 0; w < kMoeAlignWaves; ++w) {
      const int c = cnt[w][tid];
      cnt[w][tid] = run;
      run += c;
    }
    num[tid] = tid < E ? run : 0;
  }
  __syncthreads();
  if (wv == 0) {  // exclusive scans over experts (four per lane) of the padded run lengths and of the item counts
    int pad[4], its[4], ps = 0, is = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = num[4 * lane + j];
      pad[j] = (n + kMoeBM - 1) / kMoeBM * kMoeBM;
      its[j] = (n + kMoeItemRows - 1) / kMoeItemRows;
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
    const int n = num[tid], padded = (n + kMoeBM - 1) / kMoeBM * kMoeBM;
    for (int q = 0; q * kMoeItemRows < n; ++q) {
      tb.item_expert[ioff[tid] + q] = tid;
      tb.item_pos[ioff[tid] + q] = off[tid] + q * kMoeItemRows;
      tb.item_blocks[ioff[tid] + q] = min(kMoeItemBlocks, (padded - q * kMoeItemRows) / kMoeBM);
    }
    for (int i = n; i < padded; ++i) tb.sorted[off[tid] + i] = -1;
  }
  for (int i = lo + lane; i < hi; i += 64) {
    const int e = ids[i];
    if (e >= 0 && e < E) tb.sorted[off[e] + cnt[wv][e] + tb.lpos[i]] = i;
  }
}

// ---------------------------------------------------------------------------------------------------------------- GEMMs
enum { MOE_GATE_UP = 1, MOE_DOWN = 2 };

struct MoeGemmParams {
  const uint16_t* a;   // MOE_GATE_UP: x [T, K]; MOE_DOWN: act [cap, K]
  const uint16_t* w;   // MOE_GATE_UP: w1 [E, 2 N, K]; MOE_DOWN: w2 [E, N, K]
  MoeTables tb;
  uint16_t* act;       // MOE_GATE_UP out: [cap, N]
  float* partial;      // MOE_DOWN out: [P, N]
  const float* topk_w; // [P]
  int K, N, topk;
};

template <int MODE, int J>
__global__ __launch_bounds__(256, 3) void moe_gemm_kernel(const MoeGemmParams p) {
  __shared__ __attribute__((aligned(16))) unsigned char xs[kMoeItemRows * kMoeRowBytes];
  __shared__ int rowsrc[kMoeItemRows];
  const int item = blockIdx.y;
  if (item >= *p.tb.n_items) return;
  const int e = sgpr(p.tb.item_expert[item]), pos0 = sgpr(p.tb.item_pos[item]), nrb = sgpr(p.tb.item_blocks[item]);
  const int tid = threadIdx.x, lane = tid & 63, wv = sgpr(tid >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int K = p.K, N = p.N;
  if (tid < kMoeItemRows) {  // source row of each staged row: the pair's token (gate_up) / its own act row (down); -1 = zeros
    const int pair = tid < kMoeBM * nrb ? p.tb.sorted[pos0 + tid] : -1;
    rowsrc[tid] = pair < 0 ? -1 : MODE == MOE_GATE_UP ? pair / p.topk : pos0 + tid;
  }
  // this wave's two A tiles (16 weight rows each): gate and up rows of 16 features / 32 consecutive output columns
  const int col = MODE == MOE_GATE_UP ? 64 * blockIdx.x + 16 * wv : 128 * blockIdx.x + 32 * wv;
  const bool active = col < N;
  const uint16_t* wrow[2];
  if (MODE == MOE_GATE_UP) {
    wrow[0] = p.w + ((int64_t)e * 2 * N + col + r16) * K;
    wrow[1] = wrow[0] + (int64_t)N * K;
  } else {
    wrow[0] = p.w + ((int64_t)e * N + col + r16) * K;
    wrow[1] = wrow[0] + (int64_t)16 * K;
  }
  moe_f32x4 acc[kMoeItemBlocks][2];
#pragma unroll
  for (int rb = 0; rb < kMoeItemBlocks; ++rb) acc[rb][0] = acc[rb][1] = moe_f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kc0 = 0; kc0 < K; kc0 += kMoeChunkK) {
    const int kc_len = sgpr(min(kMoeChunkK, K - kc0));
    // the chunk's weight fragments first: they travel while the rows are staged.  Fragment a = (step a / J, MFMA a % J).
    U4 wa[2][8];
    if (active) {
#pragma unroll
      for (int a = 0; a < 8; ++a)
        if (32 * a < kc_len) {
          const int ko = kc0 + (a / J) * 32 * J + q4 * 8 * J + (a % J) * 8;
          wa[0][a] = ldg16(wrow[0] + ko);
          wa[1][a] = ldg16(wrow[1] + ko);
        }
    }
    __syncthreads();  // the previous chunk has been read (first pass: rowsrc is written)
#pragma unroll
    for (int i = 0; i < kMoeItemRows * (kMoeChunkK / 8) / 256; ++i) {
      const int piece = tid + 256 * i, row = piece >> 5, c = piece & 31;
      if (row < kMoeBM * nrb && 8 * c < kc_len) {
        const int src = rowsrc[row];
        U4 v = {0u, 0u, 0u, 0u};
        if (src >= 0) v = ldg16(p.a + (int64_t)src * K + kc0 + 8 * c);
        *reinterpret_cast<U4*>(xs + row * kMoeRowBytes + 16 * c) = v;
      }
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int a = 0; a < 8; ++a)
        if (32 * a < kc_len) {
          const int kb = ((a / J) * 32 * J + q4 * 8 * J + (a % J) * 8) * 2;
#pragma unroll
          for (int rb = 0; rb < kMoeItemBlocks; ++rb)
            if (rb < nrb) {
              const U4 b = *reinterpret_cast<const U4*>(xs + (kMoeBM * rb + r16) * kMoeRowBytes + kb);
              acc[rb][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(moe_bf16x8, wa[0][a]),
                                                                   __builtin_bit_cast(moe_bf16x8, b), acc[rb][0], 0, 0, 0);
              acc[rb][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(moe_bf16x8, wa[1][a]),
                                                                   __builtin_bit_cast(moe_bf16x8, b), acc[rb][1], 0, 0, 0);
            }
        }
    }
  }
  if (!active) return;
  // lane holds D[weight row 4 q4 + i][token row r16] in register i of each tile
#pragma unroll
  for (int rb = 0; rb < kMoeItemBlocks; ++rb)
    if (rb < nrb) {
      const int pos = pos0 + kMoeBM * rb + r16;
      const int pair = p.tb.sorted[pos];
      if (pair < 0) continue;
      if (MODE == MOE_GATE_UP) {
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

// out[t][c] = bf16(sum over slots, in slot order, of partial[t k + slot][c]); eight columns per thread
__global__ __launch_bounds__(256) void moe_sum_kernel(uint16_t* __restrict__ out, const float* __restrict__ partial,
                                                      const int32_t* __restrict__ ids, int T, int k, int E, int hidden) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int per_row = hidden >> 3;
  if (gid >= (int64_t)T * per_row) return;
  const int t = (int)(gid / per_row), c = (int)(gid - (int64_t)t * per_row) * 8;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int slot = 0; slot < k; ++slot) {
    const int64_t pair = (int64_t)t * k + slot;
    const int e = ids[pair];
    if (e < 0 || e >= E) continue;
    const float* q = partial + pair * hidden + c;
    const float4 a = *reinterpret_cast<const float4*>(q), b = *reinterpret_cast<const float4*>(q + 4);
    s[0] += a.x; s[1] += a.y; s[2] += a.z; s[3] += a.w;
    s[4] += b.x; s[5] += b.y; s[6] += b.z; s[7] += b.w;
  }
  stg16(out + (int64_t)t * hidden + c, pack8<BF16>(s));
}

// ---------------------------------------------------------------------------------------------------------------- host
void moe_launch_align(const MoeTables& tb, const int32_t* ids, int P, int E, hipStream_t s) {
  moe_align_kernel<<<dim3(1), dim3(64 * kMoeAlignWaves), 0, s>>>(tb, ids, P, E);
}

void moe_launch_sum(uint16_t* out, const float* partial, const int32_t* ids, int T, int k, int E, int hidden, hipStream_t s) {
  const int64_t threads = (int64_t)T * (hidden / 8);
  moe_sum_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(out, partial, ids, T, k, E, hidden);
}

}  // namespace msgl

using namespace msgl;

extern "C" int msgl_moe_route(float* topk_weights, int32_t* topk_ids, const void* logits, int T, int E, int k, int renormalize,
                              int logits_dtype, void* stream) {
  MSGL_REQUIRE(topk_weights && topk_ids && logits, "moe_route: null pointer");
  MSGL_REQUIRE(T >= 1, "moe_route: T = %d", T);
  MSGL_REQUIRE(E >= 1 && E <= kMoeMaxExperts, "moe_route: E = %d outside [1, %d]", E, kMoeMaxExperts);
  MSGL_REQUIRE(k >= 1 && k <= kMoeMaxTopk && k <= E, "moe_route: k = %d outside [1, min(%d, E)]", k, kMoeMaxTopk);
  MSGL_REQUIRE(logits_dtype == MSGL_BF16 || logits_dtype == MSGL_F32, "moe_route: logits must be bf16 or fp32 (dtype code %d)",
               logits_dtype);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 g((unsigned)((T + 3) / 4)), b(256);
  if (logits_dtype == MSGL_F32)
    moe_route_kernel<true><<<g, b, 0, s>>>(topk_weights, topk_ids, logits, T, E, k, renormalize);
  else
    moe_route_kernel<false><<<g, b, 0, s>>>(topk_weights, topk_ids, logits, T, E, k, renormalize);
  MSGL_CHECK_LAUNCH("moe_route");
  return MSGL_OK;
}

extern "C" int64_t msgl_moe_workspace_bytes(int T, int E, int k, int hidden, int I_l) {
  const int rc = moe_check_shape("moe_workspace_bytes", T, E, k, hidden, I_l);
  if (rc != MSGL_OK) return rc;
  return moe_layout(T, E, k, hidden, I_l).bytes;
}

extern "C" int msgl_moe_forward(const void* x, const void* w1, const void* w2, const float* topk_weights,
                                const int32_t* topk_ids, void* workspace, int64_t workspace_bytes, void* out, int T, int E,
                                int k, int hidden, int I_l, void* stream) {
  MSGL_REQUIRE(x && w1 && w2 && topk_weights && topk_ids && out, "moe_forward: null pointer");
  const int rc = moe_check_shape("moe_forward", T, E, k, hidden, I_l);
  if (rc != MSGL_OK) return rc;
  const MoeLayout L = moe_layout(T, E, k, hidden, I_l);
  MSGL_REQUIRE(L.max_items <= kMoeMaxGridY, "moe_forward: %lld work items exceed one launch; split the tokens",
               (long long)L.max_items);
  MSGL_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 255u) == 0 && workspace_bytes >= L.bytes,
               "moe_forward: needs %lld workspace bytes, 256-byte aligned", (long long)L.bytes);
  MSGL_REQUIRE(aligned16(x) && aligned16(w1) && aligned16(w2) && aligned16(out), "moe_forward: pointers must be 16-byte aligned");
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  const MoeTables tb = moe_tables(ws, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int P = T * k;
  moe_launch_align(tb, topk_ids, P, E, s);
  MSGL_CHECK_LAUNCH("moe_forward(align)");

  MoeGemmParams g;
  g.tb = tb;
  g.act = reinterpret_cast<uint16_t*>(ws + L.o_act);
  g.partial = reinterpret_cast<float*>(ws + L.o_partial);
  g.topk_w = topk_weights;
  g.topk = k;
  g.a = static_cast<const uint16_t*>(x); g.w = static_cast<const uint16_t*>(w1); g.K = hidden; g.N = I_l;
  moe_gemm_kernel<MOE_GATE_UP, 2><<<dim3((unsigned)((I_l + 63) / 64), (unsigned)L.max_items), dim3(256), 0, s>>>(g);
  MSGL_CHECK_LAUNCH("moe_forward(gate_up)");
  g.a = g.act; g.w = static_cast<const uint16_t*>(w2); g.K = I_l; g.N = hidden;
  const dim3 g2((unsigned)((hidden + 127) / 128), (unsigned)L.max_items);
  if (I_l % 64 == 0)
    moe_gemm_kernel<MOE_DOWN, 2><<<g2, dim3(256), 0, s>>>(g);
  else
    moe_gemm_kernel<MOE_DOWN, 1><<<g2, dim3(256), 0, s>>>(g);
  MSGL_CHECK_LAUNCH("moe_forward(down)");
  moe_launch_sum(static_cast<uint16_t*>(out), g.partial, topk_ids, T, k, E, hidden, s);
  MSGL_CHECK_LAUNCH("moe_forward(sum)");
  return MSGL_OK;
}
