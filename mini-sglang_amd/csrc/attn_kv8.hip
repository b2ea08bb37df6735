// FP8 (OCP e4m3fn) KV cache for head_dim 128 on gfx950: the quantising store, paged decode attention (partial + merge
// kernel) and varlen causal prefill attention over a pool of ONE byte per element, bf16 activations, fp32 accumulation.
// Entry points msgl_qk_norm_rope_store_kv8 / msgl_attn_decode_kv8 / msgl_attn_prefill_kv8 (include/msgl_hip.h).
//
// Numerics.  cache = e4m3_rne(clamp(float(x) / scale, -448, 448)), x the bf16 value the 16-bit store writes, scale one
// fp32 per tensor (k_scale, v_scale), IEEE division; the clamp keeps the NaN encoding out.  Attention multiplies exactly
// the stored values: e4m3 -> bf16 is exact (v_cvt_scalef32_pk_bf16_fp8, scale 1.0), the products run on the bf16 MFMAs,
// k_scale is folded into the exponent's scale (sm_scale * k_scale * log2 e) and v_scale into the final 1 / l (on the
// split-KV path into the partial sums before they are written: the merge arithmetic is that of the 16-bit kernels).
// P is rounded to bf16 before P.V as everywhere else.  No atomics: bit-repeatable.
//
// Geometry.  One kv head's token row is 128 B = one cache line, the byte geometry of csrc/attn_d64.hip: its wave-load
// coverage (8 token rows per 16-B-per-lane load), its 128-B LDS image rows and the source-side swizzles of
// global_load_lds_dwordx4 carry over in bytes.  What differs: the contraction is 128 deep, a conversion sits between LDS
// and the MFMA, and the V^T fragments come from 8-bit data.
//
// V^T fragments: ds_read_b64_tr_b8 on the BYTE image, then four conversions (decode and prefill alike).  A 16-lane group
// passes an [8 rows][16 B] block (lane j: row j >> 1, 8-byte half j & 1) and lane j receives column j = one d, eight
// tokens, in row order -- exactly one bf16 MFMA A operand after conversion, and two adjacent bytes are two adjacent
// contraction slots, which is what the packed conversion produces.  The alternative (convert before the LDS write, keep
// ds_read_b64_tr_b16 on a 256-B-row image) converts the same number of bytes but doubles the LDS image, its write
// traffic and the fragment reads (two per MFMA instead of one), and prefill cannot use it at all: its tiles arrive by
// DMA, which cannot convert.  One fragment path for both kernels.
//
// ---- store (qk_norm_rope_store_kv8_kernel) -----------------------------------------------------------------------------
// The row pass of qk_norm_rope_store_kernel (csrc/norm_rope_act.hip) at head_dim 128, bf16, same operations in the same
// order: 16 lanes own one (token, head), q and k are normalised and rotated in place in bf16 -- the same bits as the
// 16-bit entry point -- and only the scatter to the pool quantises: 8 elements -> 8 divisions, v_med3, two
// v_cvt_pk_fp8_f32 pairs, one 8-byte store per lane (a head row = 128 B = one line per 16 lanes).
//
// ---- decode (attn_decode_kv8_kernel) -----------------------------------------------------------------------------------
// One wave per (slot, virtual kv head) of the shared plan (msgl_attn_decode_plan, unchanged), 32-token steps.
//   * requests: lane = 8 * group + piece; lane group g owns tokens 4 g .. 4 g + 3 of the step and request j fetches token
//     4 g + j: every request is made of whole lines, 4 K + 4 V requests = 8 KB per step.  slot_run >= 16: one table entry
//     per 16-token tile; token-granular: one 16-byte table read per lane group and step.
//   * ring of register sets of one step (8 KB) each, sized as attn_d64.hip's: G >= 3 heads per wave: 3 sets (16 KB in flight
//     per wave) at two waves per SIMD; G <= 2: 2 sets at three waves per SIMD = 24 KB per SIMD.
//   * wave-private LDS images [32 tokens][128 B] for V and K (8 KB per wave).  Physical row = token ^ bit 2 of the token.
//     K: 16-byte pieces XORed by (token >> 1) & 7, read by ds_read_b128 (one piece = 16 dims = TWO MFMA steps); V: pieces
//     XORed by ((token >> 1) & 3) | (bit 4 of the token) << 2, so the 16 rows x 16 B of a 32-lane transposing read
//     (tokens 4 q .. 4 q + 3 of both tiles, q = 0, 1) fall on 64 distinct banks.
//   * S^T[16 tokens x 16 heads] = K . Q^T: FOUR v_mfma_f32_16x16x32_bf16 per 16-token tile.  The contraction order is
//     permuted to the byte layout: step (r, h), lane quarter q covers dims 64 r + 16 q + 8 h .. + 7, Q's fragments are
//     loaded in that order.
//   * O^T[128 d x 16 heads] += V^T . P^T over the step's 32 tokens: 8 MFMAs (one per 16-d block); S^T's result layout is
//     the B operand (contraction 8 q + i <-> tile A token 4 q + i, 8 q + 4 + i <-> tile B token 4 q + i) and ONE transposing
//     read per block returns the V^T fragment in that order.
//   * split-KV: pieces of a cut request write fp32 (v_scale * o, m, l) to the workspace in the head_dim 128 layout
//     ([piece][q head][128] | [piece][q head][2]); attn_decode_kv8_merge_kernel adds them in piece order.
//   hipcc --offload-arch=gfx950 resource report (no scratch, no spills):
//     3 sets: 189 VGPRs (runs of >= 16) / 197 (token-granular), 0 AGPRs, 64 KB LDS per 8-wave workgroup, two waves per
//     SIMD; 2 sets: 156 / 161 VGPRs, 0 AGPRs, 32 KB per 4-wave workgroup, three waves per SIMD; merge kernel 20 VGPRs, no
//     LDS; store kernel 48 VGPRs, no LDS, eight waves per SIMD.
//
// ---- prefill (attn_prefill_kv8_kernel) ---------------------------------------------------------------------------------
// One workgroup = 4 waves = one 128-row q tile of one (request, q head), 32 rows per wave, the swapped formulation
// S^T = K . Q^T, O^T += V^T . P^T on v_mfma_f32_32x32x16_bf16 with the online softmax lane-local (csrc/attn_prefill.hip).
//   * 64-key K / V tiles gathered through the token-granular table global -> LDS by global_load_lds_dwordx4 AS BYTES: 8 KB
//     per image, the double-buffered pair 32 KB per workgroup -- half the 16-bit head_dim 128 kernel's.  Where the saving
//     goes: NOWHERE yet.  Deeper (128-key) tiles would double the 32 score registers; a third resident workgroup needs
//     <= 168 registers and the kernel takes 169 VGPRs (0 AGPRs, no scratch, no spills; hipcc --offload-arch=gfx950 resource
//     report) -- under __launch_bounds__(256, 3) the compiler reaches 168 only by spilling two registers, which is not
//     accepted here.  So residency is what the 16-bit kernel has, two workgroups = two waves per SIMD, at 64 KB of LDS per
//     CU instead of 128 KB; a three-deep DMA ring in the free LDS is the open step (DESIGN.md 6e has the measurement).
//   * K image [64 keys][128 B], pieces XORed by (key >> 1) & 7 on the source side; a ds_read_b128 brings 16 dims = two
//     MFMA steps, converted on the fragment read; 8 steps per 32-key block.  V image row-major [64 keys][128 B], pieces
//     XORed by 2 * (bit 1 of the key | bit 3 of the key << 1); V^T fragments by ds_read_b64_tr_b8 (the lane's own eight
//     keys of the score registers, no cross-lane movement of P), one read + four conversions per MFMA.  One barrier per tile.
//   * bottom-right causal mask on tiles that cross a wave's diagonal only, tiles above it skipped; XCD-contiguous order of
//     (kv head, q tile, q head of the group), tile_order honoured.
#include <math.h>

#include <type_traits>

#include "attn_params.h"
#include "common.h"

namespace msgl {
namespace kv8 {

constexpr int kD = 128;
constexpr float kNegBig = -3.0e38f;
constexpr float kF8Max = 448.0f;  // largest finite e4m3

#define MSGL_KV8_PIN_MEM()                  \
  do {                                      \
    asm volatile("" ::: "memory");          \
    __builtin_amdgcn_sched_barrier(0);      \
  } while (0)

typedef uint32_t V4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((address_space(3))) i32x2 lds_i32x2;
typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) V4 lds_V4;
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void glb_void_t;

// eight e4m3 bytes -> eight bf16 (exact), byte order kept
__device__ __forceinline__ V4 cvt8(uint32_t lo, uint32_t hi) {
  V4 r;
  r.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)lo, 1.0f, false));
  r.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)lo, 1.0f, true));
  r.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)hi, 1.0f, false));
  r.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)hi, 1.0f, true));
  return r;
}
// the V^T fragment behind a transposing byte read (see the banner)
__device__ __forceinline__ V4 vt_frag(const lds_char* ptr) {
  const i32x2 r = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)ptr);
  return cvt8((uint32_t)r.x, (uint32_t)r.y);
}
__device__ __forceinline__ f32x4 mfma16(const V4& a, const V4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma32(const V4& a, const V4& b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// eight fp32 -> eight e4m3 bytes: IEEE division, clamp, round to nearest even
__device__ __forceinline__ uint2 quant8(const float (&f)[8], float scale) {
  float g[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) g[e] = __builtin_amdgcn_fmed3f(f[e] / scale, -kF8Max, kF8Max);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(g[0], g[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(g[2], g[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(g[4], g[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(g[6], g[7], hi, true);
  return uint2{(uint32_t)lo, (uint32_t)hi};
}

// over the four 16-lane groups of a wave (every lane ends with the result)
__device__ __forceinline__ float max_over_rows(float x) {
  const uint32_t u = __float_as_uint(x);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  x = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  const uint32_t w = __float_as_uint(x);
  const auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float sum_over_rows(float x) {
  const uint32_t u = __float_as_uint(x);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const uint32_t w = __float_as_uint(x);
  const auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// ---------------------------------------------------------------------------------------------------------------------
// store
// ---------------------------------------------------------------------------------------------------------------------
template <typename PosT, typename LocT>
__global__ __launch_bounds__(256) void qk_norm_rope_store_kv8_kernel(
    uint16_t* __restrict__ q, uint16_t* __restrict__ k, const uint16_t* __restrict__ v, const uint16_t* __restrict__ qw,
    const uint16_t* __restrict__ kw, float eps, const PosT* __restrict__ positions, const float* __restrict__ cache,
    uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, const LocT* __restrict__ out_loc, int64_t groups, int hq, int hk,
    int64_t qs, int64_t ks, int64_t vs, int64_t cs, float k_scale, float v_scale) {
  constexpr int LPR = kD / 8;
  using T = BF16;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t grp = gid / LPR;
  const int c = (int)(gid % LPR);
  const bool live = grp < groups;
  const int64_t g = live ? grp : 0;
  const int per_tok = hq + 2 * hk;
  const int64_t t = g / per_tok;
  const int head = (int)(g - t * per_tok);
  if (head >= hq + hk) {  // V head: quantise into the pool
    const int h = head - hq - hk;
    if (live) {
      float x[8];
      unpack8<T>(ldg16(v + t * vs + (int64_t)h * kD + c * 8), x);
      *reinterpret_cast<uint2*>(vc + (int64_t)out_loc[t] * cs + (int64_t)h * kD + c * 8) = quant8(x, v_scale);
    }
    return;  // whole 16-lane group leaves together; DPP below only spans such groups
  }
  const bool is_q = head < hq;
  uint16_t* p = is_q ? q + t * qs + (int64_t)head * kD + c * 8 : k + t * ks + (int64_t)(head - hq) * kD + c * 8;
  const uint16_t* w = is_q ? qw : kw;
  float x[8];
  unpack8<T>(ldg16(p), x);
  if (w != nullptr) {
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = fmaf(x[e], x[e], ss);
    ss = row16_sum(ss);
    const float inv = rsqrtf(ss / (float)kD + eps);
    float wf[8];
    unpack8<T>(ldg16(w + c * 8), wf);
    float y[8];  // rounded through bf16 before RoPE reads it, as the 16-bit pass does
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = __fmul_rn(__fmul_rn(x[e], inv), wf[e]);
    unpack8<T>(pack8<T>(y), x);
  }
  float o[8];  // partner lane holds the other half of the head (i <-> i + D / 2)
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = __shfl_xor(x[e], LPR / 2, 64);
  const int j = c & (LPR / 2 - 1);
  const float* csr = cache + (int64_t)positions[t] * kD + j * 8;
  float co[8], si[8];
  *reinterpret_cast<float4*>(co) = *reinterpret_cast<const float4*>(csr);
  *reinterpret_cast<float4*>(co + 4) = *reinterpret_cast<const float4*>(csr + 4);
  *reinterpret_cast<float4*>(si) = *reinterpret_cast<const float4*>(csr + kD / 2);
  *reinterpret_cast<float4*>(si + 4) = *reinterpret_cast<const float4*>(csr + kD / 2 + 4);
  const float sgn = c < LPR / 2 ? -1.f : 1.f;
  float y[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = fmaf(x[e], co[e], sgn * __fmul_rn(o[e], si[e]));
  const U4 outv = pack8<T>(y);
  if (live) {
    stg16(p, outv);
    if (!is_q) {  // the pool receives the quantised bf16 value, not the fp32 one
      float r[8];
      unpack8<T>(outv, r);
      *reinterpret_cast<uint2*>(kc + (int64_t)out_loc[t] * cs + (int64_t)(head - hq) * kD + c * 8) = quant8(r, k_scale);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------------------------------------------------
// per-wave images [32 tokens][128 B] (see the banner)
__device__ __forceinline__ int img_row(int tok) { return (tok ^ ((tok >> 2) & 1)) * 128; }
__device__ __forceinline__ int kimg_off(int tok, int piece) { return img_row(tok) + (((piece ^ (tok >> 1)) & 7) << 4); }
__device__ __forceinline__ int vimg_swz(int tok) { return ((tok >> 1) & 3) | (((tok >> 4) & 1) << 2); }
__device__ __forceinline__ int vimg_off(int tok, int piece) { return img_row(tok) + ((piece ^ vimg_swz(tok)) << 4); }
constexpr int kImgBytes = 32 * 128;  // one image; a wave owns V at 0 and K behind it

struct Step {  // 32 tokens of one kv head
  V4 k[4], v[4];
};
__device__ __forceinline__ void pin_step(Step& t) {  // nothing that consumes the step moves above this point
  asm volatile(""
               : "+v"(t.k[0]), "+v"(t.k[1]), "+v"(t.k[2]), "+v"(t.k[3]), "+v"(t.v[0]), "+v"(t.v[1]), "+v"(t.v[2]),
                 "+v"(t.v[3])
               :
               : "memory");
  __builtin_amdgcn_sched_barrier(0);
}

template <int kStages, int kWaves, int kMinW, bool kRun>
__global__ __launch_bounds__(64 * kWaves, kMinW) void attn_decode_kv8_kernel(const DecodeParams p, const float v_scale) {
  __shared__ __attribute__((aligned(16))) char lds[kWaves * 2 * kImgBytes];
  const int lane = threadIdx.x & 63;
  const int col = lane & 15;  // products: result column = q head of the group; A-operand row (token of a tile / d of a block)
  const int qd = lane >> 4;   // products: 8-wide quarter of a 32-deep contraction step; token quad of the results
  const int grp = lane >> 3;  // requests: token group (tokens 4 grp .. 4 grp + 3 of the step)
  const int pc = lane & 7;    // requests: 16-byte piece of the 128-B row
  const int wv = sgpr((int)(threadIdx.x >> 6));
  const int gw = sgpr((int)blockIdx.x * kWaves + wv);
  const int slot = gw / p.hv;
  const int h = gw - slot * p.hv;
  if (slot >= p.plan[3]) return;
  const int G = sgpr(p.hq / p.hv);
  const int* slot_first = p.plan + plan_off_slot_first(p.max_bs);
  const int4* items = reinterpret_cast<const int4*>(p.plan + plan_off_items(p.max_bs, p.capacity));
  const int4* items2 = reinterpret_cast<const int4*>(p.plan + plan_off_items2(p.max_bs, p.capacity));
  const int item_begin = sgpr(slot_first[slot]);
  const int item_end = sgpr(slot_first[slot + 1]);
  lds_char* img = (lds_char*)lds + wv * (2 * kImgBytes);

  int vwr[4], kwr[4], krd[2][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    vwr[j] = vimg_off(4 * grp + j, pc);
    kwr[j] = kImgBytes + kimg_off(4 * grp + j, pc);
  }
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int r = 0; r < 2; ++r) krd[t2][r] = kImgBytes + kimg_off(16 * t2 + col, 4 * r + qd);
  // V^T: lane j of a 16-lane group passes row j >> 1 of [tile A tokens 4 qd .. + 3 | tile B tokens 4 qd .. + 3], 8-byte half
  // j & 1 of the block's 16-byte piece, and receives column j.  Piece db of the row: XOR db << 4 (bits 4 .. 6 are the swizzle's)
  const int vtok = 4 * qd + (col >> 1) + ((col >> 1) < 4 ? 0 : 12);
  const int vrd = vimg_off(vtok, 0) + 8 * (col & 1);

  const int hq0 = h * G;
  const int kvh = hq0 / p.group;
  const uint32_t row_bytes = (uint32_t)p.kv_stride_tok;  // < 2^32: checked at launch
  const uint64_t head_bytes = (uint64_t)((int64_t)kvh * p.kv_stride_head);
  const uint64_t lane_bytes = head_bytes + pc * 16;
  const char* kbase = reinterpret_cast<const char*>(p.k);
  const char* vbase = reinterpret_cast<const char*>(p.v);

  for (int item = item_begin; item < item_end; ++item) {
    const int4 it = items[item], it2 = items2[item];
    const int b = sgpr(it.x);
    const int t0 = sgpr(it.y) * 16;
    const int t1 = min(sgpr(it2.x), sgpr(it.z) * 16);
    const bool single = sgpr(it2.y) == 1;
    const int row = p.req_rows ? sgpr(p.req_rows[b]) : b;
    const int* pt = p.page_table + (int64_t)row * p.pt_stride;
    const int nsteps = (t1 - t0 + 31) >> 5;
    if (nsteps <= 0) continue;  // (no plan makes an empty piece; a corrupt one must not index with garbage)
    const int s_first = sgpr(pt[t0]);  // position t0 < t1 is inside the request: what every masked token re-reads

    V4 qf[2][2];  // B operand of K . Q^T: column = head, dims 64 r + 16 qd + 8 hh ..
    {
      const uint16_t* qp = p.q + (int64_t)b * p.q_stride + (int64_t)(hq0 + col) * kD + qd * 16;
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          V4 z = {0u, 0u, 0u, 0u};
          if (col < G) z = *reinterpret_cast<const V4*>(qp + r * 64 + hh * 8);
          qf[r][hh] = z;
        }
    }
    float m = kNegBig, l = 0.f;
    f32x4 o[8];
#pragma unroll
    for (int db = 0; db < 8; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};

    // table entries of step min(si, last): with runs of >= 16 the first entry of each of its two tiles, else the lane
    // group's four.  Entries at or past t1 are read (inside the row) but never used as slots.
    auto slots_raw = [&](int si) -> int4 {
      const int tb = t0 + min(si, nsteps - 1) * 32;
      if constexpr (kRun) {
        int4 r = {pt[tb], pt[tb + 16 < t1 ? tb + 16 : tb], 0, 0};
        return r;
      } else {
        int tq = tb + 4 * grp;
        if (tq >= t1) tq = tb;
        return *reinterpret_cast<const int4*>(pt + tq);
      }
    };
    // request step si.  A token at or past t1 re-reads the piece's first row (finite data under P = 0: a table tail may
    // point at bytes that decode to NaN); a step past the piece's end still issues its eight requests -- the ring below
    // has no branch around them -- but every lane then asks for the same 16 bytes of that row.
    auto load_step = [&](const int4& sl, Step& t, int si) {
      const bool dead = si >= nsteps;
      const int tq = t0 + min(si, nsteps - 1) * 32 + 4 * grp;
      int s4[4];
      if constexpr (kRun) {
        const int base = (grp < 4 ? sl.x : sl.y) + ((4 * grp) & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) s4[i] = base + i;
      } else {
        s4[0] = sl.x; s4[1] = sl.y; s4[2] = sl.z; s4[3] = sl.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int s = tq + j < t1 ? s4[j] : s_first;
        const uint64_t off = dead ? (uint64_t)(uint32_t)s_first * row_bytes + head_bytes
                                  : (uint64_t)(uint32_t)s * row_bytes + lane_bytes;
        t.k[j] = __builtin_nontemporal_load(reinterpret_cast<const V4*>(kbase + off));
        t.v[j] = __builtin_nontemporal_load(reinterpret_cast<const V4*>(vbase + off));
      }
    };
    auto compute = [&](const Step& t, int tb) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        *(lds_V4*)(img + vwr[j]) = t.v[j];
        *(lds_V4*)(img + kwr[j]) = t.k[j];
      }
      f32x4 s[2];
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2) {
        s[t2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const V4 kb = *(lds_V4*)(img + krd[t2][r]);  // 16 dims of the lane's token: two contraction steps
          s[t2] = mfma16(cvt8(kb.x, kb.y), qf[r][0], s[t2]);
          s[t2] = mfma16(cvt8(kb.z, kb.w), qf[r][1], s[t2]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (tb + 16 * t2 + 4 * qd + i >= t1) s[t2][i] = -INFINITY;
      }
      float mx = fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])),
                       fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3])));
      mx = max_over_rows(mx) * p.scale_log2;
      if (__builtin_amdgcn_ballot_w64(mx > m) != 0) {  // some head's running max moved (wave-uniform branch)
        const float mn = fmaxf(m, mx);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        l *= alpha;
#pragma unroll
        for (int db = 0; db < 8; ++db)
#pragma unroll
          for (int i = 0; i < 4; ++i) o[db][i] *= alpha;
      }
      float pe[2][4];
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int i = 0; i < 4; ++i) pe[t2][i] = __builtin_amdgcn_exp2f(fmaf(s[t2][i], p.scale_log2, -m));
      l += ((pe[0][0] + pe[0][1]) + (pe[0][2] + pe[0][3])) + ((pe[1][0] + pe[1][1]) + (pe[1][2] + pe[1][3]));
      // P rounded to bf16 for the second product (as the 16-bit kernels do); l from the fp32 values
      const V4 pf = {Elem<BF16>::pack(pe[0][0], pe[0][1]), Elem<BF16>::pack(pe[0][2], pe[0][3]),
                     Elem<BF16>::pack(pe[1][0], pe[1][1]), Elem<BF16>::pack(pe[1][2], pe[1][3])};
#pragma unroll
      for (int db = 0; db < 8; ++db) o[db] = mfma16(vt_frag(img + (vrd ^ (db << 4))), pf, o[db]);
    };

    // kStages - 1 steps in flight, then per step: request step cur + kStages - 1, wait for step cur alone (pin_step),
    // consume it.  The table entries of a step are requested one step ahead of its K/V and BEFORE the K/V requests of the
    // running step, so waiting for them does not wait for those (vmcnt retires in order).
    Step ring[kStages];
#pragma unroll
    for (int st = 0; st < kStages - 1; ++st) {
      load_step(slots_raw(st), ring[st], st);
      MSGL_KV8_PIN_MEM();
    }
    int4 sn = slots_raw(kStages - 1);
    for (int c0 = 0; c0 < nsteps; c0 += kStages) {
#pragma unroll
      for (int st = 0; st < kStages; ++st) {
        const int cur = c0 + st;
        const int4 raw = slots_raw(cur + kStages);
        MSGL_KV8_PIN_MEM();
        load_step(sn, ring[(st + kStages - 1) % kStages], cur + kStages - 1);
        pin_step(ring[st]);
        if (cur < nsteps) compute(ring[st], t0 + cur * 32);
        MSGL_KV8_PIN_MEM();
        sn = raw;
      }
    }

    l = sum_over_rows(l);  // each lane summed its own eight tokens per step
    if (col < G) {
      const int hq = hq0 + col;
      if (single) {
        const float inv = v_scale / l;
        uint16_t* op = p.out + (int64_t)b * p.out_stride + (int64_t)hq * kD + 4 * qd;
#pragma unroll
        for (int db = 0; db < 8; ++db) {
          uint2 u;
          u.x = Elem<BF16>::pack(o[db][0] * inv, o[db][1] * inv);
          u.y = Elem<BF16>::pack(o[db][2] * inv, o[db][3] * inv);
          *reinterpret_cast<uint2*>(op + db * 16) = u;
        }
      } else {  // v_scale goes into the partial sums: the merge below is scale-free
        float* po = p.part_o + ((int64_t)item * p.hq + hq) * kD + 4 * qd;
#pragma unroll
        for (int db = 0; db < 8; ++db)
          *reinterpret_cast<float4*>(po + db * 16) =
              make_float4(o[db][0] * v_scale, o[db][1] * v_scale, o[db][2] * v_scale, o[db][3] * v_scale);
        if (qd == 0) *reinterpret_cast<float2*>(p.part_ml + ((int64_t)item * p.hq + hq) * 2) = make_float2(m, l);
      }
    }
  }
}

// merge the split-KV partial sums: one wave per (request, q head), two output dims per lane, pieces in index order.
// launched_slots: as in attn_decode_merge_kernel -- a plan with more slots than the launch in front had waves for means
// pieces were never computed: the output rows are NaN-poisoned instead of summed from uninitialised memory.
__global__ __launch_bounds__(256) void attn_decode_kv8_merge_kernel(const DecodeParams p, int batch, int launched_slots) {
  const int lane = threadIdx.x & 63;
  const int w = sgpr((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (w >= batch * p.hq) return;
  const int b = w / p.hq;
  const int hq = w - b * p.hq;
  uint32_t* op = reinterpret_cast<uint32_t*>(p.out + (int64_t)b * p.out_stride + (int64_t)hq * kD) + lane;
  if (p.plan[3] > launched_slots) {
    *op = 0xffffffffu;
    return;
  }
  const int n = sgpr(p.plan[plan_off_n_chunks(p.max_bs) + b]);
  if (n <= 1) return;  // single-piece requests were finished by the attention kernel
  const int i0 = sgpr(p.plan[plan_off_item_start() + b]);
  const float* pml = p.part_ml + ((int64_t)i0 * p.hq + hq) * 2;
  const float* po = p.part_o + ((int64_t)i0 * p.hq + hq) * kD + lane * 2;
  const int64_t ml_step = (int64_t)p.hq * 2, po_step = (int64_t)p.hq * kD;
  float mx = kNegBig;  // lanes fetch the pieces' maxima 64 at a time
  for (int j0 = 0; j0 < n; j0 += 64) mx = fmaxf(mx, j0 + lane < n ? pml[(j0 + lane) * ml_step] : kNegBig);
  mx = wave_max(mx);
  float acc0 = 0.f, acc1 = 0.f, den = 0.f;
  for (int j0 = 0; j0 < n; j0 += 4) {  // four pieces' loads in flight; the sums stay in piece order
    float2 ov[4], ml[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = min(j0 + u, n - 1);
      ov[u] = *reinterpret_cast<const float2*>(po + j * po_step);
      ml[u] = *reinterpret_cast<const float2*>(pml + j * ml_step);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (j0 + u < n) {
        const float wgt = __builtin_amdgcn_exp2f(ml[u].x - mx);
        acc0 = fmaf(wgt, ov[u].x, acc0);
        acc1 = fmaf(wgt, ov[u].y, acc1);
        den = fmaf(wgt, ml[u].y, den);
      }
    }
  }
  const float inv = 1.0f / den;
  *op = Elem<BF16>::pack(acc0 * inv, acc1 * inv);
}

template <bool kRun>
static void launch_decode_t(const DecodeParams& p, float v_scale, int batch, int64_t waves, hipStream_t s) {
  if (p.hq / p.hv <= 2)  // the plan counts three waves per SIMD for these groups: two register sets
    attn_decode_kv8_kernel<2, 4, 3, kRun><<<dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s>>>(p, v_scale);
  else  // two waves per SIMD, three register sets; 8 waves = the 8 kv heads of one slot at hv = 8
    attn_decode_kv8_kernel<3, 8, 2, kRun><<<dim3((unsigned)((waves + 7) / 8)), dim3(512), 0, s>>>(p, v_scale);
  const int64_t mblocks = ((int64_t)batch * p.hq + 3) / 4;
  attn_decode_kv8_merge_kernel<<<dim3((unsigned)mblocks), dim3(256), 0, s>>>(p, batch, (int)(waves / p.hv));
}

// ---------------------------------------------------------------------------------------------------------------------
// prefill
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kQTile = MSGL_PREFILL_QTILE;  // 128 query rows per workgroup
constexpr int kKTile = 64;                  // keys per tile
constexpr int kTileBytes = kKTile * kD;     // 8 KB: one K (or V) image

__device__ __forceinline__ int pk_off(int key, int piece) { return key * 128 + (((piece ^ (key >> 1)) & 7) << 4); }
__device__ __forceinline__ int pv_swz(int key) { return (((key >> 1) & 1) | (((key >> 3) & 1) << 1)) << 1; }

__global__ __launch_bounds__(256, 2) void attn_prefill_kv8_kernel(const PrefillParams p, int total_tiles, const float v_scale) {
  // two LDS objects: a tile's fragment reads cannot alias the DMA writes of the next tile
  __shared__ __attribute__((aligned(1024))) char lds_a[2 * kTileBytes];  // tiles 0, 2, ..: [K | V]
  __shared__ __attribute__((aligned(1024))) char lds_b[2 * kTileBytes];  // tiles 1, 3, ..
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5;

  // block -> (kv head, q tile, head of the group): each XCD owns a contiguous range
  const int n_per = (int)(gridDim.x >> 3);
  const int vidx = (int)(blockIdx.x & 7) * n_per + (int)(blockIdx.x >> 3);
  if (vidx >= total_tiles * p.hq) return;
  const int per_kv = total_tiles * p.group;
  const int kvh = vidx / per_kv;
  const int rem = vidx - kvh * per_kv;
  const int ti = rem / p.group;
  const int hq = kvh * p.group + (rem - ti * p.group);
  const int tile = p.tile_order ? p.tile_order[ti] : ti;

  const TileRequest rq = find_request(p, tile, lane);
  const int q_begin = rq.q_begin;
  const int q_len = rq.q_end - q_begin;
  const int k_len = rq.k_len;
  const int q0 = (tile - rq.tile_first) * kQTile;
  const int* pt = p.page_table + (int64_t)rq.row * p.pt_stride;
  const int diag = k_len - q_len;
  const int kend = min(k_len, diag + min(q0 + kQTile, q_len));
  const int ntiles = (kend + kKTile - 1) / kKTile;

  const int my_q = q0 + wave * 32 + (lane & 31);
  const bool q_valid = my_q < q_len;
  const int64_t q_tok = q_begin + (q_valid ? my_q : q_len - 1);
  V4 qf[4][2];  // B operand of K . Q^T: column = the lane's query row, dims 32 r + 16 hi + 8 hh ..
  {
    const uint16_t* qp = p.q + q_tok * p.q_stride + (int64_t)hq * kD + hi * 16;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) qf[r][hh] = *reinterpret_cast<const V4*>(qp + r * 32 + hh * 8);
  }
  const int my_qpos = diag + my_q;
  const int wave_min_qpos = diag + q0 + wave * 32;  // scalar

  f32x16 o[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[nb][r] = 0.f;
  float m_run = kNegBig, l_run = 0.f;

  // staging: DMA instruction i of this wave fills rows 32 i + 8 wave .. + 7 (1 KB) of an image; the lane lands on row
  // st_row + 32 i, 16-byte slot lane & 7, and fetches the piece the image's swizzle keeps there
  const int st_row = tid >> 3;
  const char* kbase = reinterpret_cast<const char*>(p.k);
  const char* vbase = reinterpret_cast<const char*>(p.v);
  const int64_t k_lane = (int64_t)kvh * p.kv_stride_head + ((((lane & 7) ^ (st_row >> 1)) & 7) << 4);
  const int64_t v_lane = (int64_t)kvh * p.kv_stride_head + (((lane & 7) ^ pv_swz(st_row)) << 4);
  int sl[2];
  auto load_slots = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) sl[i] = pt[min(kt * kKTile + st_row + 32 * i, k_len - 1)];  // never past the sequence
  };
  auto issue_dma = [&](char* buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t off = slot_offset(sl[i], p.kv_stride_tok);
      __builtin_amdgcn_global_load_lds((glb_void_t*)(kbase + off + k_lane), (lds_void_t*)(buf + (4 * i + wave) * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((glb_void_t*)(vbase + off + v_lane),
                                       (lds_void_t*)(buf + kTileBytes + (4 * i + wave) * 1024), 16, 0, 0);
    }
  };
  // per-lane LDS addresses.  K: the lane's key (lane & 31 of a 32-key block), piece 2 r + hi.  V^T of d block nb: the lane
  // passes row j >> 1 of its eight keys (4 hi + 0 .. 3 and 8 + 4 hi + 0 .. 3 of a 16-key group), 8-byte half j & 1 of piece
  // 2 nb + (the 16-lane group's d half), and receives column j.  Both swizzles are XORs of the piece index, and 2 r / 2 nb
  // touch bits the rest of it does not: ONE address register each, piece r / nb = that address ^ (r << 5) / (nb << 5)
  const int koff = pk_off(lane & 31, hi);
  int voff;
  {
    const int j = lane & 15;
    const int rho = j >> 1;
    const int key_l = 4 * hi + (rho < 4 ? rho : rho + 4);
    voff = kTileBytes + key_l * 128 + ((((lane >> 4) & 1) ^ pv_swz(key_l)) << 4) + 8 * (j & 1);
  }

  auto tile_body = [&](auto BUFC, const int kt) {
    constexpr int BUF = decltype(BUFC)::value;
    char* buf = BUF ? lds_b : lds_a;
    char* nxt = BUF ? lds_a : lds_b;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of tile kt (and the slots of tile kt + 1)
    __syncthreads();                                  // everyone's pieces; everyone done with the other buffer
    if (kt + 1 < ntiles) {
      issue_dma(nxt);
      if (kt + 2 < ntiles) load_slots(kt + 2);
    }
    const int key0 = kt * kKTile;
    if (key0 > wave_min_qpos + 31) return;  // whole tile above this wave's diagonal

    // S^T = K . Q^T: two 32-key blocks, eight k-steps each (a 16-byte read feeds two)
    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const V4 kk = *reinterpret_cast<const V4*>(buf + (koff ^ (r << 5)) + kb * 32 * 128);
        s[kb] = mfma32(cvt8(kk.x, kk.y), qf[r][0], s[kb]);
        s[kb] = mfma32(cvt8(kk.z, kk.w), qf[r][1], s[kb]);
      }
    }
    // causal mask (tiles crossing this wave's diagonal only): key0 + c + 4 hi > my_qpos  <=>  c > thr
    if (key0 + kKTile - 1 > wave_min_qpos) {
      const int thr = my_qpos - key0 - 4 * hi;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kb * 32 + (r & 3) + 8 * (r >> 2) > thr) s[kb][r] = -INFINITY;
    }
    // online softmax, lane-local row (+ lane ^ 32); the scale is folded into the exponent's fma
    float tmax = kNegBig;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[kb][r]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64)) * p.scale_log2;
    const float m_new = fmaxf(m_run, tmax);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    float rsum = 0.f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = __builtin_amdgcn_exp2f(fmaf(s[kb][r], p.scale_log2, -m_new));
        s[kb][r] = e;
        rsum += e;
      }
    rsum += __shfl_xor(rsum, 32, 64);
    l_run = fmaf(l_run, alpha, rsum);
    if (!__all(m_new == m_run)) {  // alpha == 1 on every row otherwise
#pragma unroll
      for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[nb][r] *= alpha;
    }
    m_run = m_new;
    // O^T += V^T . P^T: the lane's keys of (kb, half) are 4 hi + 0 .. 3 (contraction slots 0 .. 3) and 8 + 4 hi + 0 .. 3
    // (slots 4 .. 7) of the 16-key group -- its own score registers 8 half .. 8 half + 7, no cross-lane movement of P
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        V4 pf;
        pf.x = Elem<BF16>::pack(s[kb][8 * half + 0], s[kb][8 * half + 1]);
        pf.y = Elem<BF16>::pack(s[kb][8 * half + 2], s[kb][8 * half + 3]);
        pf.z = Elem<BF16>::pack(s[kb][8 * half + 4], s[kb][8 * half + 5]);
        pf.w = Elem<BF16>::pack(s[kb][8 * half + 6], s[kb][8 * half + 7]);
        const int gb = (kb * 32 + half * 16) * 128;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) o[nb] = mfma32(vt_frag((const lds_char*)(buf + (voff ^ (nb << 5)) + gb)), pf, o[nb]);
      }
    }
  };

  if (ntiles > 0) {
    load_slots(0);
    issue_dma(lds_a);
    if (ntiles > 1) load_slots(1);
  }
  for (int kt = 0; kt < ntiles; kt += 2) {
    tile_body(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < ntiles) tile_body(std::integral_constant<int, 1>{}, kt + 1);
  }

  if (q_valid) {  // O[q row][d] = v_scale * O^T / l
    const float inv = v_scale / l_run;
    uint16_t* op = p.out + (int64_t)(q_begin + my_q) * p.out_stride + (int64_t)hq * kD;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int d = nb * 32 + 8 * rg + 4 * hi;
        uint2 w;
        w.x = Elem<BF16>::pack(o[nb][4 * rg + 0] * inv, o[nb][4 * rg + 1] * inv);
        w.y = Elem<BF16>::pack(o[nb][4 * rg + 2] * inv, o[nb][4 * rg + 3] * inv);
        *reinterpret_cast<uint2*>(op + d) = w;
      }
    }
  }
}

// what the three entry points refuse alike, before anything is launched
static int check_common(const char* what, int head_dim, int dtype, float k_scale, float v_scale) {
  MSGL_REQUIRE(head_dim == kD, "%s: an FP8 KV cache needs head_dim 128, not %d", what, head_dim);
  MSGL_REQUIRE(dtype == MSGL_BF16, "%s: an FP8 KV cache needs bf16 activations (dtype code %d)", what, dtype);
  MSGL_REQUIRE(isfinite(k_scale) && isfinite(v_scale) && k_scale > 0.f && v_scale > 0.f,
               "%s: k_scale %g / v_scale %g must be finite and positive", what, (double)k_scale, (double)v_scale);
  return MSGL_OK;
}

}  // namespace kv8
}  // namespace msgl

using namespace msgl;

extern "C" int msgl_qk_norm_rope_store_kv8(void* q, void* k, const void* v, const void* q_norm_w, const void* k_norm_w,
                                           float eps, const void* positions, int positions_is_i64,
                                           const float* cos_sin_cache, void* k_cache, void* v_cache, const void* out_loc,
                                           int out_loc_is_i64, int64_t num_tokens, int num_q_heads, int num_k_heads,
                                           int head_dim, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                           int64_t cache_stride, int dtype, float k_scale, float v_scale, void* stream) {
  if (const int rc = kv8::check_common("qk_norm_rope_store_kv8", head_dim, dtype, k_scale, v_scale)) return rc;
  MSGL_REQUIRE(num_tokens >= 0, "qk_norm_rope_store_kv8: negative token count");
  if (num_tokens == 0) return MSGL_OK;
  MSGL_REQUIRE(q && k && v && positions && cos_sin_cache && k_cache && v_cache && out_loc,
               "qk_norm_rope_store_kv8: null pointer");
  MSGL_REQUIRE((q_norm_w == nullptr) == (k_norm_w == nullptr), "qk_norm_rope_store_kv8: need both or no norm weights");
  MSGL_REQUIRE(num_q_heads >= 1 && num_k_heads >= 1, "qk_norm_rope_store_kv8: %d q heads / %d k heads", num_q_heads, num_k_heads);
  MSGL_REQUIRE(q_stride % 8 == 0 && k_stride % 8 == 0 && v_stride % 8 == 0 && cache_stride % 16 == 0,
               "qk_norm_rope_store_kv8: q/k/v strides must be multiples of 8 elements, the cache stride of 16 bytes");
  MSGL_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(k_cache) && aligned16(v_cache) &&
                   aligned16(cos_sin_cache),
               "qk_norm_rope_store_kv8: pointers must be 16-byte aligned");
  MSGL_REQUIRE((positions_is_i64 == 0 || positions_is_i64 == 1) && (out_loc_is_i64 == 0 || out_loc_is_i64 == 1),
               "qk_norm_rope_store_kv8: bad index width flag");
  const int64_t groups = num_tokens * (num_q_heads + 2 * num_k_heads);
  const int64_t blocks = (groups * (kv8::kD / 8) + 255) / 256;
  MSGL_REQUIRE(blocks < (1ll << 31), "qk_norm_rope_store_kv8: too many tokens");
  hipStream_t s = static_cast<hipStream_t>(stream);
#define MSGL_KV8_STORE(PT, LT)                                                                                        \
  kv8::qk_norm_rope_store_kv8_kernel<PT, LT><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(                          \
      (uint16_t*)q, (uint16_t*)k, (const uint16_t*)v, (const uint16_t*)q_norm_w, (const uint16_t*)k_norm_w, eps,      \
      (const PT*)positions, cos_sin_cache, (uint8_t*)k_cache, (uint8_t*)v_cache, (const LT*)out_loc, groups,          \
      num_q_heads, num_k_heads, q_stride, k_stride, v_stride, cache_stride, k_scale, v_scale)
  if (positions_is_i64) {
    if (out_loc_is_i64) MSGL_KV8_STORE(int64_t, int64_t);
    else MSGL_KV8_STORE(int64_t, int32_t);
  } else {
    if (out_loc_is_i64) MSGL_KV8_STORE(int32_t, int64_t);
    else MSGL_KV8_STORE(int32_t, int32_t);
  }
#undef MSGL_KV8_STORE
  MSGL_CHECK_LAUNCH("qk_norm_rope_store_kv8");
  return MSGL_OK;
}

extern "C" int msgl_attn_decode_kv8(void* out, const void* q, const void* k_cache, const void* v_cache,
                                    const int32_t* page_table, int64_t pt_stride, const int32_t* req_rows,
                                    const int32_t* seq_lens, const int32_t* plan, void* workspace, int batch, int max_bs,
                                    int capacity, int num_q_heads, int num_kv_heads, int head_dim, int64_t q_stride_tok,
                                    int64_t kv_stride_tok, int64_t kv_stride_head, int64_t out_stride_tok, float sm_scale,
                                    int slot_run, int dtype, float k_scale, float v_scale, void* stream) {
  if (const int rc = kv8::check_common("attn_decode_kv8", head_dim, dtype, k_scale, v_scale)) return rc;
  MSGL_REQUIRE(out && q && k_cache && v_cache && page_table && seq_lens && plan && workspace,
               "attn_decode_kv8: null pointer");
  MSGL_REQUIRE(slot_run >= 1 && (slot_run & (slot_run - 1)) == 0, "attn_decode_kv8: slot_run %d must be a power of two",
               slot_run);
  MSGL_REQUIRE(batch >= 1 && batch <= max_bs && capacity >= max_bs, "attn_decode_kv8: bad batch/capacity");
  // one production kernel: the diagnosis / A-B codes name 16-bit head_dim 128 kernels only (the rule head_dim 64 follows)
  MSGL_REQUIRE(decode_select_code() == 0 || decode_select_code() == 71,
               "attn_decode_kv8: runs under select code 0 (or 71) only, not %d", decode_select_code());
  MSGL_REQUIRE(num_kv_heads >= 1 && num_q_heads >= num_kv_heads && num_q_heads % num_kv_heads == 0 &&
                   num_q_heads / num_kv_heads <= 16,
               "attn_decode_kv8: %d q heads / %d kv heads", num_q_heads, num_kv_heads);
  MSGL_REQUIRE(pt_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(page_table) & 15u) == 0,
               "attn_decode_kv8: page table rows must be 16-byte aligned");
  MSGL_REQUIRE(q_stride_tok % 8 == 0 && out_stride_tok % 8 == 0, "attn_decode_kv8: q / out strides must be multiples of 8 elements");
  MSGL_REQUIRE(kv_stride_tok > 0 && kv_stride_tok < (1ll << 32) && kv_stride_tok % 16 == 0 && kv_stride_head % 16 == 0,
               "attn_decode_kv8: cache rows must be 16-byte aligned (token stride %lld, head stride %lld bytes)",
               (long long)kv_stride_tok, (long long)kv_stride_head);
  MSGL_REQUIRE(aligned16(out) && aligned16(q) && aligned16(k_cache) && aligned16(v_cache) && aligned16(workspace) &&
                   aligned16(plan),
               "attn_decode_kv8: pointers must be 16-byte aligned");
  int G = 1;
  const int64_t waves = decode_plan_waves(num_q_heads, num_kv_heads, capacity, max_bs, &G);
  DecodeParams p;
  p.q = (const uint16_t*)q;
  p.k = (const uint16_t*)k_cache;  // bytes: the kernels index them as such
  p.v = (const uint16_t*)v_cache;
  p.page_table = page_table;
  p.req_rows = req_rows;
  p.seq_lens = seq_lens;
  p.plan = plan;
  p.out = (uint16_t*)out;
  p.part_o = (float*)workspace;
  p.part_ml = p.part_o + (int64_t)capacity * num_q_heads * head_dim;
  p.pt_stride = pt_stride;
  p.q_stride = q_stride_tok;
  p.kv_stride_tok = kv_stride_tok;
  p.kv_stride_head = kv_stride_head;
  p.out_stride = out_stride_tok;
  p.max_bs = max_bs;
  p.capacity = capacity;
  p.hq = num_q_heads;
  p.hv = num_q_heads / G;
  p.group = num_q_heads / num_kv_heads;
  p.slot_run = slot_run;
  p.scale_log2 = sm_scale * k_scale * 1.4426950408889634f;
  p.trace = nullptr;
  p.arrivals = nullptr;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (slot_run >= 16) kv8::launch_decode_t<true>(p, v_scale, batch, waves, s);
  else kv8::launch_decode_t<false>(p, v_scale, batch, waves, s);
  MSGL_CHECK_LAUNCH("attn_decode_kv8");
  return MSGL_OK;
}

extern "C" int msgl_attn_prefill_kv8(void* out, const void* q, const void* k_cache, const void* v_cache,
                                     const int32_t* page_table, int64_t pt_stride, const int32_t* req_rows,
                                     const int32_t* seq_lens, const int32_t* cu_seqlens_q, const int32_t* tile_cu, int batch,
                                     int total_tiles, int num_q_heads, int num_kv_heads, int head_dim, int64_t q_stride_tok,
                                     int64_t kv_stride_tok, int64_t kv_stride_head, int64_t out_stride_tok, float sm_scale,
                                     int dtype, const int32_t* tile_order, int impl, float k_scale, float v_scale,
                                     void* stream) {
  if (const int rc = kv8::check_common("attn_prefill_kv8", head_dim, dtype, k_scale, v_scale)) return rc;
  MSGL_REQUIRE(batch >= 0 && total_tiles >= 0, "attn_prefill_kv8: negative sizes");
  MSGL_REQUIRE(impl == 0 || impl == 4, "attn_prefill_kv8: the DMA-staged kernel only (impl 0 = 4), not impl %d", impl);
  if (batch == 0 || total_tiles == 0) return MSGL_OK;
  MSGL_REQUIRE(out && q && k_cache && v_cache && page_table && seq_lens && cu_seqlens_q && tile_cu,
               "attn_prefill_kv8: null pointer");
  MSGL_REQUIRE(num_kv_heads >= 1 && num_q_heads % num_kv_heads == 0 && num_q_heads <= 65535,
               "attn_prefill_kv8: %d q heads / %d kv heads", num_q_heads, num_kv_heads);
  MSGL_REQUIRE(kv_stride_tok > 0 && kv_stride_tok < (1ll << 32) && kv_stride_tok % 16 == 0 && kv_stride_head % 16 == 0,
               "attn_prefill_kv8: cache rows must be 16-byte aligned (token stride %lld, head stride %lld bytes)",
               (long long)kv_stride_tok, (long long)kv_stride_head);
  MSGL_REQUIRE(q_stride_tok % 8 == 0 && out_stride_tok % 4 == 0, "attn_prefill_kv8: q / out strides must be multiples of 8 / 4 elements");
  MSGL_REQUIRE(aligned16(q) && aligned16(k_cache) && aligned16(v_cache) && (reinterpret_cast<uintptr_t>(out) & 7u) == 0,
               "attn_prefill_kv8: pointers must be 16-byte aligned");
  PrefillParams p;
  p.q = (const uint16_t*)q;
  p.k = (const uint16_t*)k_cache;  // bytes
  p.v = (const uint16_t*)v_cache;
  p.page_table = page_table;
  p.req_rows = req_rows;
  p.seq_lens = seq_lens;
  p.cu_q = cu_seqlens_q;
  p.tile_cu = tile_cu;
  p.tile_order = tile_order;
  p.out = (uint16_t*)out;
  p.pt_stride = pt_stride;
  p.q_stride = q_stride_tok;
  p.kv_stride_tok = kv_stride_tok;
  p.kv_stride_head = kv_stride_head;
  p.out_stride = out_stride_tok;
  p.batch = batch;
  p.hq = num_q_heads;
  p.group = num_q_heads / num_kv_heads;
  p.scale_log2 = sm_scale * k_scale * 1.4426950408889634f;
  const int64_t total = (int64_t)total_tiles * num_q_heads;
  MSGL_REQUIRE(total < (1ll << 30), "attn_prefill_kv8: %lld workgroups", (long long)total);
  const unsigned blocks = (unsigned)((total + 7) / 8) * 8;  // 8 XCDs x n_per
  kv8::attn_prefill_kv8_kernel<<<dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream)>>>(p, total_tiles, v_scale);
  MSGL_CHECK_LAUNCH("attn_prefill_kv8");
  return MSGL_OK;
}
