// What the expert-MLP files share (moe.hip: bf16 weights, moe_w8.hip: block-scaled FP8 weights): the work-item tables that
// moe_align_kernel writes, the workspace layout, the shape contract, and host-side launchers of the align and sum kernels,
// which are defined once, in moe.hip.
#pragma once
#include "common.h"

namespace msgl {

constexpr int kMoeMaxExperts = 256;
constexpr int kMoeMaxTopk = 8;
constexpr int kMoeBM = 16;             // row-block height: every expert's run of pairs is padded to it
constexpr int kMoeItemBlocks = 4;      // row blocks per work item
constexpr int kMoeItemRows = kMoeBM * kMoeItemBlocks;
constexpr int kMoeAlignWaves = 16;
constexpr int kMoeMaxGridY = 65535;

struct MoeTables {
  int32_t* sorted;       // [cap]  pair index, or -1 (pad), grouped by expert, stable in pair index
  int32_t* lpos;         // [P]    scratch: a pair's rank among its wave segment's pairs of the same expert
  int32_t* item_expert;  // [max_items]
  int32_t* item_pos;     // [max_items]  first position in `sorted` (and row of `act`)
  int32_t* item_blocks;  // [max_items]  1 .. 4 row blocks
  int32_t* n_items;      // [1]
};

static inline int64_t up256(int64_t n) { return (n + 255) / 256 * 256; }

struct MoeLayout {
  int64_t cap, max_items;
  int64_t o_sorted, o_lpos, o_iexp, o_ipos, o_iblk, o_nitems, o_act, o_partial, bytes;
};

// a pure function of the arguments: positions after padding every expert's run to 16 <= P + 15 min(E, P); an item holds at
// least one pair and every item but an expert's last holds 64, so items <= min(E, P) + P / 64
static inline MoeLayout moe_layout(int64_t T, int64_t E, int64_t k, int64_t hidden, int64_t I) {
  MoeLayout L;
  const int64_t P = T * k, ne = E < P ? E : P;
  L.cap = P + (kMoeBM - 1) * ne;
  L.max_items = ne + P / kMoeItemRows;
  int64_t o = 0;
  L.o_sorted = o; o += up256(L.cap * 4);
  L.o_lpos = o; o += up256(P * 4);
  L.o_iexp = o; o += up256(L.max_items * 4);
  L.o_ipos = o; o += up256(L.max_items * 4);
  L.o_iblk = o; o += up256(L.max_items * 4);
  L.o_nitems = o; o += 256;
  L.o_act = o; o += up256(L.cap * I * 2);
  L.o_partial = o; o += up256(P * hidden * 4);
  L.bytes = o;
  return L;
}

static inline MoeTables moe_tables(unsigned char* ws, const MoeLayout& L) {
  MoeTables tb;
  tb.sorted = reinterpret_cast<int32_t*>(ws + L.o_sorted);
  tb.lpos = reinterpret_cast<int32_t*>(ws + L.o_lpos);
  tb.item_expert = reinterpret_cast<int32_t*>(ws + L.o_iexp);
  tb.item_pos = reinterpret_cast<int32_t*>(ws + L.o_ipos);
  tb.item_blocks = reinterpret_cast<int32_t*>(ws + L.o_iblk);
  tb.n_items = reinterpret_cast<int32_t*>(ws + L.o_nitems);
  return tb;
}

static inline int moe_check_shape(const char* who, int64_t T, int64_t E, int64_t k, int64_t hidden, int64_t I) {
  MSGL_REQUIRE(T >= 1 && T * k < (1ll << 30), "%s: T = %lld outside [1, 2^30 / k)", who, (long long)T);
  MSGL_REQUIRE(E >= 1 && E <= kMoeMaxExperts, "%s: E = %lld outside [1, %d]", who, (long long)E, kMoeMaxExperts);
  MSGL_REQUIRE(k >= 1 && k <= kMoeMaxTopk && k <= E, "%s: k = %lld outside [1, min(%d, E)]", who, (long long)k, kMoeMaxTopk);
  MSGL_REQUIRE(hidden >= 64 && hidden % 64 == 0, "%s: hidden = %lld must be a multiple of 64", who, (long long)hidden);
  MSGL_REQUIRE(I >= 32 && I % 32 == 0, "%s: the expert intermediate size %lld must be a multiple of 32", who, (long long)I);
  return MSGL_OK;
}

// moe.hip: the launches of moe_align_kernel (one workgroup) and moe_sum_kernel on `s`
void moe_launch_align(const MoeTables& tb, const int32_t* ids, int P, int E, hipStream_t s);
void moe_launch_sum(uint16_t* out, const float* partial, const int32_t* ids, int T, int k, int E, int hidden, hipStream_t s);

}  // namespace msgl
