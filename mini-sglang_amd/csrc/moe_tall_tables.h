// What the tall expert-MLP files share (moe_tall.hip: bf16 weights, moe_w8_tall.hip: block-scaled FP8 weights): the tables of
// 256-row work items, the three-launch align that writes them, the slab sum, the workspace layout and the shape contract.
// The kernels have internal linkage: each of the two files launches its own copy of the same code.
//
//   align    three launches over SEGMENTS of 1024 pairs (four waves x 256 pairs): count (a wave ranks its pairs among
//            those of the same expert with ballots and writes its per-expert counts), scan (one workgroup: per expert an
//            exclusive prefix over all wave segments, then over experts the padded run offsets and the item tables), scatter
//            (sorted[off[e] + prefix[wave segment][e] + rank] = pair).  Stable in pair index, runs padded to 16 with -1:
//            the `sorted` of moe_align_kernel.  No atomics; every table entry has exactly one writer.
//   items    an expert's run is cut into items of up to 256 rows (sixteen 16-row blocks).
#pragma once
#include "common.h"

namespace msgl {

constexpr int kTallMaxExperts = 256;
constexpr int kTallMaxTopk = 8;
constexpr int kTallBM = 16;          // row-block height, as kMoeBM
constexpr int kTallItemBlocks = 16;  // row blocks per item
constexpr int kTallItemRows = kTallBM * kTallItemBlocks;
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
static __global__ __launch_bounds__(64 * kTallSegWaves) void moe_tall_count_kernel(const TallTables tb,
                                                                                   const int32_t* __restrict__ ids, int P, int E) {
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
static __global__ __launch_bounds__(1024) void moe_tall_scan_kernel(const TallTables tb, int nsub, int E) {
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

static __global__ __launch_bounds__(64 * kTallSegWaves) void moe_tall_scatter_kernel(const TallTables tb,
                                                                                     const int32_t* __restrict__ ids, int P,
                                                                                     int E) {
  const int lane = threadIdx.x & 63;
  const int sub = blockIdx.x * kTallSegWaves + (threadIdx.x >> 6);
  const int lo = sub * kTallWavePairs, hi = min(P, lo + kTallWavePairs);
  for (int i = lo + lane; i < hi; i += 64) {
    const int e = ids[i];
    if (e >= 0 && e < E) tb.sorted[tb.off[e] + tb.cnt[(int64_t)sub * E + e] + tb.lpos[i]] = i;
  }
}

// ------------------------------------------------------------------------------------------------------------------ sum
// out[t][c0 + c] = bf16(sum over slots, in slot order, of partial[t k + slot][c]) for the slab's columns; eight per thread
static __global__ __launch_bounds__(256) void moe_tall_sum_kernel(uint16_t* __restrict__ out, const float* __restrict__ partial,
                                                                  const int32_t* __restrict__ ids, int T, int k, int E,
                                                                  int hidden, int c0, int wcols, int W) {
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
static inline TallLayout tall_layout(int64_t T, int64_t E, int64_t k, int64_t I) {
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

static inline TallTables tall_tables(unsigned char* ws, const TallLayout& L) {
  TallTables tb;
  tb.sorted = reinterpret_cast<int32_t*>(ws + L.o_sorted);
  tb.lpos = reinterpret_cast<int32_t*>(ws + L.o_lpos);
  tb.cnt = reinterpret_cast<int32_t*>(ws + L.o_cnt);
  tb.off = reinterpret_cast<int32_t*>(ws + L.o_off);
  tb.item_expert = reinterpret_cast<int32_t*>(ws + L.o_iexp);
  tb.item_pos = reinterpret_cast<int32_t*>(ws + L.o_ipos);
  tb.item_blocks = reinterpret_cast<int32_t*>(ws + L.o_iblk);
  tb.n_items = reinterpret_cast<int32_t*>(ws + L.o_nitems);
  return tb;
}

static inline int tall_check_shape(const char* who, int64_t T, int64_t E, int64_t k, int64_t hidden, int64_t I) {
  MSGL_REQUIRE(T >= 1 && T * k < (1ll << 30), "%s: T = %lld outside [1, 2^30 / k)", who, (long long)T);
  MSGL_REQUIRE(E >= 1 && E <= kTallMaxExperts, "%s: E = %lld outside [1, %d]", who, (long long)E, kTallMaxExperts);
  MSGL_REQUIRE(k >= 1 && k <= kTallMaxTopk && k <= E, "%s: k = %lld outside [1, min(%d, E)]", who, (long long)k, kTallMaxTopk);
  MSGL_REQUIRE(hidden >= 64 && hidden % 64 == 0, "%s: hidden = %lld must be a multiple of 64", who, (long long)hidden);
  MSGL_REQUIRE(I >= 32 && I % 32 == 0, "%s: the expert intermediate size %lld must be a multiple of 32", who, (long long)I);
  return MSGL_OK;
}

// the minimum scratch (one 128-column slab), and the columns whose fp32 partials fit behind the tables and act in
// workspace_bytes: a multiple of 128, below 128 = too small.  The slab width is that, or all of hidden if it is no wider
static inline int64_t tall_min_bytes(const TallLayout& L) { return L.o_partial + tall_up256(L.P * 128 * 4); }
static inline int64_t tall_slab_room(const TallLayout& L, int64_t workspace_bytes) {
  const int64_t room = workspace_bytes - L.o_partial;
  return room > 0 ? room / (L.P * 4) / 128 * 128 : 0;
}

// count, scan, scatter on `s`; `who` names the entry point in a launch error
static inline int tall_launch_align(const char* who, const TallTables& tb, const TallLayout& L, const int32_t* ids, int E,
                                    hipStream_t s) {
  const dim3 seg_grid((unsigned)L.nseg), seg_block(64 * kTallSegWaves);
  moe_tall_count_kernel<<<seg_grid, seg_block, 0, s>>>(tb, ids, (int)L.P, E);
  MSGL_CHECK_LAUNCH(who);
  moe_tall_scan_kernel<<<dim3(1), dim3(1024), 0, s>>>(tb, (int)(L.nseg * kTallSegWaves), E);
  MSGL_CHECK_LAUNCH(who);
  moe_tall_scatter_kernel<<<seg_grid, seg_block, 0, s>>>(tb, ids, (int)L.P, E);
  MSGL_CHECK_LAUNCH(who);
  return MSGL_OK;
}

// the slab [c0, c0 + wcols) of out from partial [P, W]
static inline int tall_launch_sum(const char* who, uint16_t* out, const float* partial, const int32_t* ids, int T, int k, int E,
                                  int hidden, int c0, int wcols, int W, hipStream_t s) {
  const int64_t threads = (int64_t)T * (wcols / 8);
  moe_tall_sum_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(out, partial, ids, T, k, E, hidden, c0, wcols,
                                                                                   W);
  MSGL_CHECK_LAUNCH(who);
  return MSGL_OK;
}

}  // namespace msgl
