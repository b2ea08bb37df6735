// Paged attention for head_dim 64 on gfx950: decode (partial + merge kernel) and varlen causal prefill, bf16 / fp16 with
// fp32 accumulation.  Reached through msgl_attn_decode / msgl_attn_prefill when head_dim == 64 (Llama-3.2-1B, TinyLlama,
// Qwen2.5-0.5B ...); work split, plan, workspace layout, tile units and scheduling order are those of the head_dim 128
// kernels, the kernels are not: a token row of one kv head is 128 B -- ONE cache line -- instead of 256 B, which changes how
// a wave's loads cover tokens, the LDS images and their swizzles, and the ratio of matrix work to softmax work.
//
// ---- decode (attn_decode_d64_kernel) ------------------------------------------------------------------------------------
// One wave per (slot, virtual kv head) of the shared plan; the wave walks its pieces in steps of 32 tokens = two plan tiles.
//   * load coverage: a 16-byte-per-lane wave load covers EIGHT token rows (lane = 8 * group + piece: token group, 16-byte
//     piece of the 128-B row), every request is made of whole lines.  Lane group g owns the step's tokens 4 g .. 4 g + 3 and
//     request j fetches token 4 g + j, so a token-granular table (slot_run < 16) costs one 16-byte table read per lane and
//     step; with slot_run >= 16 the step reads one table entry per 16-token tile.  4 K + 4 V requests = 8 KB per step.
//   * S^T[32 tokens x 16 heads] = K . Q^T: per 16-token tile two v_mfma_f32_16x16x32 steps (D = 64), the group's heads in the
//     16 result columns (padded with zero columns).  K reaches the A-operand layout through a wave-private LDS image.
//   * O^T[64 d x 16 heads] += V^T . P^T: the two tiles of a step fill ONE 32-deep contraction, so P.V is 4 v_mfma_f32_16x16x32
//     (one per 16-d block) per 32 tokens instead of 8 16x16x16: the result layout of S^T (one head, tokens 4 q + i of each
//     tile per lane) is the B-operand layout with contraction index 8 q + i <-> tile A token 4 q + i, 8 q + 4 + i <-> tile B
//     token 4 q + i, and the V^T fragments come in that order from two ds_read_b64_tr_b16.  A piece with an odd tile count
//     ends in a step whose second tile is masked (P = 0) and whose loads re-read one valid row.
//   * LDS images, per wave [32 tokens][128 B] for V and for K.  Physical row = token ^ bit 2 of the token (so the two token
//     groups of a 16-lane ds_write_b128 pass, tokens t and t + 4, fall into different 128-B halves of the 256-B bank span);
//     K: the row's eight 16-byte pieces XORed by (token >> 1) & 7 -- the 16 lanes of a ds_read_b128 pass (one piece index,
//     16 tokens) then cover all 64 banks; V: the row's four 32-byte d blocks XORed by (token >> 1) & 3 -- the 32 lanes of a
//     ds_read_b64_tr_b16 pass (8 tokens x 32 B) cover 32 distinct 8-byte bank pairs.
//   * bytes in flight: a ring of register sets of one step (8 KB) each.  G >= 3 heads per wave: 3 sets = 16 KB in flight per
//     wave at two waves per SIMD (the head_dim 128 default keeps 8 KB per wave there); G <= 2: 2 sets at three waves per SIMD
//     = 24 KB per SIMD, as the head_dim 128 default.  hipcc --offload-arch=gfx950 resource report, no spills: 3 sets 165 (runs
//     of >= 16) / 173 (token-granular) registers, 64 KB LDS per 8-wave workgroup = two waves per SIMD; 2 sets 132 / 137
//     registers, 32 KB per 4-wave workgroup = three waves per SIMD.
//   * split-KV: pieces of a cut request write fp32 (o, m, l) to the workspace ([piece][q head][64] | [piece][q head][2]) and
//     attn_decode_d64_merge_kernel adds them in piece order; a request with one piece writes its output directly.
//
// ---- prefill (attn_prefill_d64_kernel) ----------------------------------------------------------------------------------
// One workgroup = 4 waves = one 128-row q tile of one (request, q head), 32 rows per wave, the swapped formulation
// S^T = K . Q^T, O^T += V^T . P^T on v_mfma_f32_32x32x16 with the online softmax lane-local (see attn_prefill.hip).
//   * per 32-key block Q.K^T is 4 MFMA steps and O is two 16-register blocks per wave -- half the matrix work of head_dim
//     128 under the same 32 exponentials per lane, so the kernel is bound by the vector units.  The freed resources go to
//     residency: 64-key K/V tiles are 8 KB each, the double-buffered pair 32 KB per workgroup, and the kernel takes 114
//     registers (hipcc --offload-arch=gfx950 resource report, no spills), so FOUR workgroups share a CU (two at head_dim 128:
//     64 KB, <= 256 registers) and one group's softmax overlaps the others' MFMAs.
//   * K/V tiles gathered through the token-granular table, global -> LDS by global_load_lds_dwordx4: one wave instruction
//     fills 1 KB = 8 key rows lane-linearly, the swizzle is applied on the source side.  K image [64 keys][128 B], pieces
//     XORed by (key >> 1) & 7; V image row-major [64 keys][128 B], 64-B halves XORed by bit 1 of the key, read back
//     transposed by ds_read_b64_tr_b16.  One barrier per tile.
//   * bottom-right causal mask on tiles that cross a wave's diagonal only, tiles above it skipped; XCD-contiguous order of
//     (kv head, q tile, q head of the group), tile_order honoured.
#include <type_traits>

#include "attn_params.h"
#include "common.h"

namespace msgl {
namespace d64 {

constexpr int kD = 64;
constexpr float kNegBig = -3.0e38f;

#define MSGL_D64_PIN_MEM()                  \
  do {                                      \
    asm volatile("" ::: "memory");          \
    __builtin_amdgcn_sched_barrier(0);      \
  } while (0)

typedef uint32_t V4 __attribute__((ext_vector_type(4)));
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) V4 lds_V4;
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void glb_void_t;

template <typename T>
__device__ __forceinline__ f32x4 mfma16(const V4& a, const V4& b, f32x4 c) {
  if constexpr (std::is_same_v<T, BF16>)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <typename T>
__device__ __forceinline__ f32x16 mfma32(const U4& a, const U4& b, f32x16 c) {
  if constexpr (std::is_same_v<T, BF16>)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ uint2 tr_read(const lds_char* ptr) {
  return __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)ptr));
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
// decode
// ---------------------------------------------------------------------------------------------------------------------
// per-wave images [32 tokens][128 B] (see the banner)
__device__ __forceinline__ int img_row(int tok) { return (tok ^ ((tok >> 2) & 1)) * 128; }
__device__ __forceinline__ int kimg_off(int tok, int piece) { return img_row(tok) + (((piece ^ (tok >> 1)) & 7) << 4); }
__device__ __forceinline__ int vimg_off(int tok, int byte_in_row) {
  return img_row(tok) + (byte_in_row ^ (((tok >> 1) & 3) << 5));
}
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

template <typename T, int kStages, int kWaves, int kMinW, bool kRun>
__global__ __launch_bounds__(64 * kWaves, kMinW) void attn_decode_d64_kernel(const DecodeParams p) {
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

  int vwr[4], kwr[4], krd[2][2], vrd[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    vwr[j] = vimg_off(4 * grp + j, pc * 16);
    kwr[j] = kImgBytes + kimg_off(4 * grp + j, pc);
  }
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) krd[t2][kk] = kImgBytes + kimg_off(16 * t2 + col, 4 * kk + qd);
    // lane j of a 16-lane group passes row j >> 2, 8-byte chunk j & 3 of a [4 tokens][16 d] block and receives column j
#pragma unroll
    for (int db = 0; db < 4; ++db) vrd[db][t2] = vimg_off(16 * t2 + 4 * qd + (col >> 2), db * 32 + (col & 3) * 8);
  }

  const int hq0 = h * G;
  const int kvh = hq0 / p.group;
  const uint32_t row_bytes = (uint32_t)(p.kv_stride_tok * 2);  // < 2^32: checked at launch
  const uint64_t head_bytes = (uint64_t)((int64_t)kvh * p.kv_stride_head * 2);
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

    V4 qf[2];  // B operand of K . Q^T: column = head, dims 32 kk + 8 qd ..
    {
      const uint16_t* qp = p.q + (int64_t)b * p.q_stride + (int64_t)(hq0 + col) * kD + qd * 8;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        V4 z = {0u, 0u, 0u, 0u};
        if (col < G) z = *reinterpret_cast<const V4*>(qp + kk * 32);
        qf[kk] = z;
      }
    }
    float m = kNegBig, l = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};

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
    // request step si.  A token at or past t1 re-reads the piece's first row (finite data under P = 0); a step past the
    // piece's end still issues its eight requests -- the ring below has no branch around them -- but every lane then asks
    // for the same 16 bytes of that row.
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
        for (int kk = 0; kk < 2; ++kk) {
          const V4 kf = *(lds_V4*)(img + krd[t2][kk]);
          s[t2] = mfma16<T>(kf, qf[kk], s[t2]);
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
        for (int db = 0; db < 4; ++db)
#pragma unroll
          for (int i = 0; i < 4; ++i) o[db][i] *= alpha;
      }
      float pe[2][4];
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int i = 0; i < 4; ++i) pe[t2][i] = __builtin_amdgcn_exp2f(fmaf(s[t2][i], p.scale_log2, -m));
      l += ((pe[0][0] + pe[0][1]) + (pe[0][2] + pe[0][3])) + ((pe[1][0] + pe[1][1]) + (pe[1][2] + pe[1][3]));
      // P rounded to the 16-bit type for the second product (as the head_dim 128 kernels do); l from the fp32 values
      const V4 pf = {Elem<T>::pack(pe[0][0], pe[0][1]), Elem<T>::pack(pe[0][2], pe[0][3]),
                     Elem<T>::pack(pe[1][0], pe[1][1]), Elem<T>::pack(pe[1][2], pe[1][3])};
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        const uint2 va = tr_read(img + vrd[db][0]);
        const uint2 vb = tr_read(img + vrd[db][1]);
        const V4 vf = {va.x, va.y, vb.x, vb.y};
        o[db] = mfma16<T>(vf, pf, o[db]);
      }
    };

    // kStages - 1 steps in flight, then per step: request step cur + kStages - 1, wait for step cur alone (pin_step),
    // consume it.  The table entries of a step are requested one step ahead of its K/V and BEFORE the K/V requests of the
    // running step, so waiting for them does not wait for those (vmcnt retires in order).
    Step ring[kStages];
#pragma unroll
    for (int st = 0; st < kStages - 1; ++st) {
      load_step(slots_raw(st), ring[st], st);
      MSGL_D64_PIN_MEM();
    }
    int4 sn = slots_raw(kStages - 1);
    for (int c0 = 0; c0 < nsteps; c0 += kStages) {
#pragma unroll
      for (int st = 0; st < kStages; ++st) {
        const int cur = c0 + st;
        const int4 raw = slots_raw(cur + kStages);
        MSGL_D64_PIN_MEM();
        load_step(sn, ring[(st + kStages - 1) % kStages], cur + kStages - 1);
        pin_step(ring[st]);
        if (cur < nsteps) compute(ring[st], t0 + cur * 32);
        MSGL_D64_PIN_MEM();
        sn = raw;
      }
    }

    l = sum_over_rows(l);  // each lane summed its own eight tokens per step
    if (col < G) {
      const int hq = hq0 + col;
      if (single) {
        const float inv = 1.0f / l;
        uint16_t* op = p.out + (int64_t)b * p.out_stride + (int64_t)hq * kD + 4 * qd;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          uint2 u;
          u.x = Elem<T>::pack(o[db][0] * inv, o[db][1] * inv);
          u.y = Elem<T>::pack(o[db][2] * inv, o[db][3] * inv);
          *reinterpret_cast<uint2*>(op + db * 16) = u;
        }
      } else {
        float* po = p.part_o + ((int64_t)item * p.hq + hq) * kD + 4 * qd;
#pragma unroll
        for (int db = 0; db < 4; ++db)
          *reinterpret_cast<float4*>(po + db * 16) = make_float4(o[db][0], o[db][1], o[db][2], o[db][3]);
        if (qd == 0) *reinterpret_cast<float2*>(p.part_ml + ((int64_t)item * p.hq + hq) * 2) = make_float2(m, l);
      }
    }
  }
}

// merge the split-KV partial sums: one wave per (request, q head), one output dim per lane, pieces in index order.
// launched_slots: as in attn_decode_merge_kernel -- a plan with more slots than the launch in front had waves for means
// pieces were never computed: the output rows are NaN-poisoned instead of summed from uninitialised memory.
template <typename T>
__global__ __launch_bounds__(256) void attn_decode_d64_merge_kernel(const DecodeParams p, int batch, int launched_slots) {
  const int lane = threadIdx.x & 63;
  const int w = sgpr((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (w >= batch * p.hq) return;
  const int b = w / p.hq;
  const int hq = w - b * p.hq;
  uint16_t* op = p.out + (int64_t)b * p.out_stride + (int64_t)hq * kD + lane;
  if (p.plan[3] > launched_slots) {
    *op = 0xffffu;
    return;
  }
  const int n = sgpr(p.plan[plan_off_n_chunks(p.max_bs) + b]);
  if (n <= 1) return;  // single-piece requests were finished by the attention kernel
  const int i0 = sgpr(p.plan[plan_off_item_start() + b]);
  const float* pml = p.part_ml + ((int64_t)i0 * p.hq + hq) * 2;
  const float* po = p.part_o + ((int64_t)i0 * p.hq + hq) * kD + lane;
  const int64_t ml_step = (int64_t)p.hq * 2, po_step = (int64_t)p.hq * kD;
  float mx = kNegBig;  // lanes fetch the pieces' maxima 64 at a time
  for (int j0 = 0; j0 < n; j0 += 64) mx = fmaxf(mx, j0 + lane < n ? pml[(j0 + lane) * ml_step] : kNegBig);
  mx = wave_max(mx);
  float acc = 0.f, den = 0.f;
  for (int j0 = 0; j0 < n; j0 += 4) {  // four pieces' loads in flight; the sums stay in piece order
    float ov[4];
    float2 ml[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = min(j0 + u, n - 1);
      ov[u] = po[j * po_step];
      ml[u] = *reinterpret_cast<const float2*>(pml + j * ml_step);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (j0 + u < n) {
        const float wgt = __builtin_amdgcn_exp2f(ml[u].x - mx);
        acc = fmaf(wgt, ov[u], acc);
        den = fmaf(wgt, ml[u].y, den);
      }
    }
  }
  const float r = acc / den;
  *op = (uint16_t)(Elem<T>::pack(r, r) & 0xffffu);
}

template <typename T, bool kRun>
static void launch_decode_t(const DecodeParams& p, int batch, int64_t waves, hipStream_t s) {
  if (p.hq / p.hv <= 2)  // the plan counts three waves per SIMD for these groups: two register sets
    attn_decode_d64_kernel<T, 2, 4, 3, kRun><<<dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s>>>(p);
  else  // two waves per SIMD, three register sets; 8 waves = the 8 kv heads of one slot at hv = 8
    attn_decode_d64_kernel<T, 3, 8, 2, kRun><<<dim3((unsigned)((waves + 7) / 8)), dim3(512), 0, s>>>(p);
  const int64_t mblocks = ((int64_t)batch * p.hq + 3) / 4;
  attn_decode_d64_merge_kernel<T><<<dim3((unsigned)mblocks), dim3(256), 0, s>>>(p, batch, (int)(waves / p.hv));
}

// ---------------------------------------------------------------------------------------------------------------------
// prefill
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kQTile = MSGL_PREFILL_QTILE;  // 128 query rows per workgroup
constexpr int kKTile = 64;                  // keys per tile
constexpr int kTileBytes = kKTile * kD * 2;  // 8 KB: one K (or V) image
constexpr int kUnitBytes = 4 * kD * 2;       // four key rows of an image

__device__ __forceinline__ int pk_off(int key, int piece) { return key * 128 + (((piece ^ (key >> 1)) & 7) << 4); }

template <typename T>
__global__ __launch_bounds__(256, 4) void attn_prefill_d64_kernel(const PrefillParams p, int total_tiles) {
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
  U4 qf[4];  // B operand of K . Q^T: column = the lane's query row, dims 16 ks + 8 hi ..
  {
    const uint16_t* qp = p.q + q_tok * p.q_stride + (int64_t)hq * kD + hi * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = ldg16(qp + ks * 16);
  }
  const int my_qpos = diag + my_q;
  const int wave_min_qpos = diag + q0 + wave * 32;  // scalar

  f32x16 o[2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[nb][r] = 0.f;
  float m_run = kNegBig, l_run = 0.f;

  // staging: DMA instruction i of this wave fills rows 32 i + 8 wave .. + 7 (1 KB) of an image; the lane lands on row
  // st_row + 32 i, 16-byte slot lane & 7, and fetches the piece the image's swizzle keeps there
  const int st_row = tid >> 3;
  const int64_t k_lane = (int64_t)kvh * p.kv_stride_head + (((lane & 7) ^ ((st_row >> 1) & 7)) << 3);
  const int64_t v_lane = (int64_t)kvh * p.kv_stride_head + (((lane & 7) ^ (((st_row >> 1) & 1) << 2)) << 3);
  int sl[2];
  auto load_slots = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) sl[i] = pt[min(kt * kKTile + st_row + 32 * i, k_len - 1)];  // never past the sequence
  };
  auto issue_dma = [&](char* buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t off = slot_offset(sl[i], p.kv_stride_tok);
      __builtin_amdgcn_global_load_lds((glb_void_t*)(p.k + off + k_lane), (lds_void_t*)(buf + (4 * i + wave) * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((glb_void_t*)(p.v + off + v_lane),
                                       (lds_void_t*)(buf + kTileBytes + (4 * i + wave) * 1024), 16, 0, 0);
    }
  };
  // per-lane LDS addresses: K fragment of k-step ks (key lane & 31 of a 32-key block), V^T fragment of d block nb (the
  // lane's share of a [4 keys][16 d] block: row j >> 2, 8-byte chunk j & 3; the 64-B half swizzle depends on the row only)
  int koff[4], voff[2];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) koff[ks] = pk_off(lane & 31, 2 * ks + hi);
  {
    const int j = lane & 15;
    const int r4 = j >> 2;
    const int w = (16 * ((lane >> 4) & 1) + 4 * (j & 3)) * 2;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) voff[nb] = kTileBytes + hi * kUnitBytes + r4 * 128 + (((nb ^ (r4 >> 1)) & 1) << 6) + w;
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

    // S^T = K . Q^T: two 32-key blocks, four k-steps each
    f32x16 s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        s[kb] = mfma32<T>(*reinterpret_cast<const U4*>(buf + koff[ks] + kb * 32 * 128), qf[ks], s[kb]);
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
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[nb][r] *= alpha;
    }
    m_run = m_new;
    // O^T += V^T . P^T: the lane's keys of (kb, half) are the 4-key unit 8 kb + 4 half + hi (contraction slots 0..3) and
    // the unit two further (slots 4..7) -- its own score registers 8 half .. 8 half + 7, no cross-lane movement of P
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        U4 pf;
        pf.x = Elem<T>::pack(s[kb][8 * half + 0], s[kb][8 * half + 1]);
        pf.y = Elem<T>::pack(s[kb][8 * half + 2], s[kb][8 * half + 3]);
        pf.z = Elem<T>::pack(s[kb][8 * half + 4], s[kb][8 * half + 5]);
        pf.w = Elem<T>::pack(s[kb][8 * half + 6], s[kb][8 * half + 7]);
        const int ub = (kb * 8 + half * 4) * kUnitBytes;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          const uint2 v1 = tr_read((const lds_char*)(buf + voff[nb] + ub));
          const uint2 v2 = tr_read((const lds_char*)(buf + voff[nb] + ub + 2 * kUnitBytes));
          U4 vf;
          vf.x = v1.x; vf.y = v1.y; vf.z = v2.x; vf.w = v2.y;
          o[nb] = mfma32<T>(vf, pf, o[nb]);
        }
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

  if (q_valid) {  // O[q row][d] = O^T / l
    const float inv = 1.0f / l_run;
    uint16_t* op = p.out + (int64_t)(q_begin + my_q) * p.out_stride + (int64_t)hq * kD;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int d = nb * 32 + 8 * rg + 4 * hi;
        uint2 w;
        w.x = Elem<T>::pack(o[nb][4 * rg + 0] * inv, o[nb][4 * rg + 1] * inv);
        w.y = Elem<T>::pack(o[nb][4 * rg + 2] * inv, o[nb][4 * rg + 3] * inv);
        *reinterpret_cast<uint2*>(op + d) = w;
      }
    }
  }
}

}  // namespace d64

int launch_decode_d64(const DecodeParams& p, int batch, int64_t waves, int dtype, hipStream_t s) {
  MSGL_REQUIRE(dtype == MSGL_BF16 || dtype == MSGL_FP16, "attn_decode: unsupported dtype code %d", dtype);
  MSGL_REQUIRE(p.kv_stride_tok > 0 && p.kv_stride_tok * 2 < (1ll << 32), "attn_decode: kv token stride %lld",
               (long long)p.kv_stride_tok);
  MSGL_REQUIRE(p.hq / p.hv >= 1 && p.hq / p.hv <= 16 && waves >= 1, "attn_decode: %d heads per wave", p.hq / p.hv);
  const bool run = p.slot_run >= 16;
  if (dtype == MSGL_BF16) {
    if (run) d64::launch_decode_t<BF16, true>(p, batch, waves, s);
    else d64::launch_decode_t<BF16, false>(p, batch, waves, s);
  } else {
    if (run) d64::launch_decode_t<FP16, true>(p, batch, waves, s);
    else d64::launch_decode_t<FP16, false>(p, batch, waves, s);
  }
  return MSGL_OK;
}

int launch_prefill_d64(const PrefillParams& p, int total_tiles, int dtype, hipStream_t s) {
  const int64_t total = (int64_t)total_tiles * p.hq;
  const unsigned blocks = (unsigned)((total + 7) / 8) * 8;  // 8 XCDs x n_per
  if (dtype == MSGL_BF16) d64::attn_prefill_d64_kernel<BF16><<<dim3(blocks), dim3(256), 0, s>>>(p, total_tiles);
  else d64::attn_prefill_d64_kernel<FP16><<<dim3(blocks), dim3(256), 0, s>>>(p, total_tiles);
  return MSGL_OK;
}

}  // namespace msgl
