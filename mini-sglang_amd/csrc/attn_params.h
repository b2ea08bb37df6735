// What the attention files share: the decode plan's buffer layout, the two kernel parameter blocks, the prefill kernels' request lookup, and the launchers of
// the head_dim 64 kernels (csrc/attn_d64.hip) that the entry points in attn_decode.hip / attn_prefill.hip dispatch to.
// The plan layout, the parameter blocks and find_request were moved here from attn_decode.hip / attn_prefill.hip unchanged.
#pragma once
#include "common.h"

namespace msgl {

constexpr int kPlanHdr = 4;  // [0] n_items [1] tokens per slot [2] batch [3] n_slots

// plan buffer layout (int32 words):
//   hdr[4] | item_start[max_bs] | n_chunks[max_bs] | tile_start[max_bs] | slot_first[capacity + 1] |
//   items[4 * capacity] = (request, first tile, end tile, slot) |
//   items2[4 * capacity] = (seq_len, pieces of the request, its first piece, 0) | arrivals[max_bs * kTicketHeads]
// items2 repeats per piece what the kernels otherwise fetch by request AFTER the piece record arrived: with it a piece's
// scalars are two independent loads at an address known from the piece number alone (and are prefetched for piece i + 1
// while piece i streams).
// arrivals[b][kv head]: how many pieces of request b have published their partial sums in the running launch (matrix-core
// kernel under select code 72: the piece that arrives last combines them).  Zeroed by the plan kernel, left at zero by
// every launch.
constexpr int kTicketHeads = 64;
__host__ __device__ inline int64_t plan_off_item_start() { return kPlanHdr; }
__host__ __device__ inline int64_t plan_off_n_chunks(int max_bs) { return kPlanHdr + (int64_t)max_bs; }
__host__ __device__ inline int64_t plan_off_tile_start(int max_bs) { return kPlanHdr + 2ll * max_bs; }
__host__ __device__ inline int64_t plan_off_slot_first(int max_bs) { return kPlanHdr + 3ll * max_bs; }
__host__ __device__ inline int64_t plan_off_items(int max_bs, int capacity) {
  return ((kPlanHdr + 3ll * max_bs + capacity + 1 + 3) / 4) * 4;  // int4-aligned
}
__host__ __device__ inline int64_t plan_off_items2(int max_bs, int capacity) {
  return plan_off_items(max_bs, capacity) + 4ll * capacity;
}
__host__ __device__ inline int64_t plan_off_arrivals(int max_bs, int capacity) {
  return plan_off_items2(max_bs, capacity) + 4ll * capacity;
}

struct DecodeParams {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  const int* page_table;
  const int* req_rows;
  const int* seq_lens;
  const int* plan;
  uint16_t* out;
  float* part_o;
  float* part_ml;
  int64_t pt_stride, q_stride, kv_stride_tok, kv_stride_head, out_stride;
  int max_bs, capacity, hq, hv, group;  // hv = virtual kv heads (hq / G), group = hq / real kv heads
  int slot_run;               // aligned runs of this many positions map to consecutive slots (1: none)
  float scale_log2;
  unsigned long long* trace;  // diagnosis (msgl_attn_decode_trace): 16 clock stamps per wave, else nullptr
  int* arrivals;              // plan_off_arrivals: per (request, kv head) arrival counters of the matrix-core kernel
};

struct PrefillParams {
  const uint16_t* q;
  const uint16_t* k;
  const uint16_t* v;
  const int* page_table;
  const int* req_rows;
  const int* seq_lens;
  const int* cu_q;
  const int* tile_cu;
  const int* tile_order;  // optional [total_tiles]: launch order of the q tiles (heaviest first); tr kernel only
  uint16_t* out;
  int64_t pt_stride, q_stride, kv_stride_tok, kv_stride_head, out_stride;
  int batch, hq, group;
  float scale_log2;
};

// element offset of a pool slot: slot and the token stride are both < 2^32 (checked at launch), so ONE v_mad_u64_u32
// does it; the int64 x int64 product the types ask for costs two quarter-rate 32-bit multiplies and a carry chain more
__device__ __forceinline__ int64_t slot_offset(int slot, int64_t stride_tok) {
  return (int64_t)((uint64_t)(uint32_t)slot * (uint64_t)(uint32_t)stride_tok);
}

// The request a q tile belongs to and its scalars, in ONE memory latency for batches up to 64 requests (the bisection over
// tile_cu followed by the four scalar loads paid log2(B) + 1 dependent ones: ~2.5 us of a workgroup that computes for
// ~5 us on the benchmark's prefill chunks).  Lane i of a 64-request block loads request i's tile_cu, cu_q, cu_q[+1],
// seq_len and table row together; b = the last request with tile_cu[b] <= tile is counted with a ballot and its values are
// taken from that lane.
struct TileRequest {
  int b, q_begin, q_end, k_len, row, tile_first;
};
__device__ __forceinline__ TileRequest find_request(const PrefillParams& p, int tile, int lane) {
  TileRequest r;
  int base = 0;
  for (;;) {
    const int idx = min(base + lane, p.batch - 1);
    const int tc = base + lane < p.batch ? p.tile_cu[idx] : 0x7fffffff;
    const int cq0 = p.cu_q[idx], cq1 = p.cu_q[idx + 1], kl = p.seq_lens[idx];
    const int rr = p.req_rows ? p.req_rows[idx] : idx;
    const int cnt = __popcll(__ballot(tc <= tile));
    if (cnt > 0 && (cnt < 64 || base + 64 >= p.batch)) {
      const int l = cnt - 1;
      r.b = base + l;
      r.tile_first = __builtin_amdgcn_readlane(tc, l);
      r.q_begin = __builtin_amdgcn_readlane(cq0, l);
      r.q_end = __builtin_amdgcn_readlane(cq1, l);
      r.k_len = __builtin_amdgcn_readlane(kl, l);
      r.row = __builtin_amdgcn_readlane(rr, l);
      return r;
    }
    if (cnt == 0) {  // the last request of the previous block (more than 64 requests only)
      r.b = base - 1;
      r.tile_first = p.tile_cu[r.b];
      r.q_begin = p.cu_q[r.b];
      r.q_end = p.cu_q[r.b + 1];
      r.k_len = p.seq_lens[r.b];
      r.row = p.req_rows ? p.req_rows[r.b] : r.b;
      return r;
    }
    base += 64;
  }
}

// head_dim 64 (csrc/attn_d64.hip).  `waves`: the wave count the plan was made for (slots x virtual kv heads); the partial
// kernel is launched with at least that many, the merge kernel behind it.  Both return after queueing, MSGL_OK or an
// error code with the message set.
int launch_decode_d64(const DecodeParams& p, int batch, int64_t waves, int dtype, hipStream_t stream);
int launch_prefill_d64(const PrefillParams& p, int total_tiles, int dtype, hipStream_t stream);

// What the FP8-cache decode entry point (csrc/attn_kv8.hip) needs of attn_decode.hip: the running msgl_attn_decode_select
// code, and the wave count msgl_attn_decode_plan sizes the slots for with these head counts (*heads_per_wave = q heads
// packed per work unit), so that its grid covers every slot of a plan made by the unchanged plan kernel.
int decode_select_code();
int64_t decode_plan_waves(int num_q_heads, int num_kv_heads, int capacity, int max_bs, int* heads_per_wave);

}  // namespace msgl
