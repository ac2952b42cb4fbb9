// Front of the device-slot multi-row step (inference/kv_cache.py, the cell
// SpeculativeGreedyDecoder / SpeculativeSamplingDecoder verify their drafts in):
// RoPE of Q and K and the cache write of the sq new K / V rows of every
// sequence, in ONE launch per layer.  The torch form (LayerKV._write_multi after
// rope_k, and fp8_kv.quantize on e4m3 caches) is a dozen launches of index
// arithmetic per layer in a step made of 13-40 us kernels.
//
// Split: one wave per (row t, sequence m, KV group g), g fastest as the packed
// QKV output [sq, b, g, r + 2, hd] lies in memory, four waves per workgroup.
// The wave's item is a scalar (readfirstlane), so its cache slot, key count and
// page-table entry are scalar loads and the slot arithmetic runs once per wave
// on the scalar unit.  A head is hd / 8 lanes of 16 bytes, so a wave takes 4
// (hd 128) or 8 (hd 64) of the group's r + 2 heads per pass; a lane keeps its
// column of the head across passes, so the position's cos / sin (one float4
// each) are fetched once per lane.  Query heads: load, rotate (rope_rot8 of
// common.h, the function rope.hip calls), store in place.  The key
// head: the same, and the rotated vector, rounded to the model type as the
// 16-bit cache holds it, goes to the cache; the value head goes as it is.
// 16-bit caches take the 16-byte vector; e4m3 caches 8 clamped bytes
// (e4m3_pack8 of common.h, which kv_store_fp8_k calls too) in one 8-byte store,
// the scale of the head read from device memory.  No LDS, no cross-lane traffic.
//
// Slots (KvWriteMultiParams): slot[m] + t; paged, rows t >= 1 through the page
// table at logical position kv_len[m] - sq + t, so a page edge inside the sq
// rows lands on the sequence's next page.  A slot outside the cache (a sequence
// parked at the capacity, a table entry that names no page) is not stored.
#include "common.h"
#include "kernels.h"

namespace ema {
namespace {

static_assert((KV_PAGE & (KV_PAGE - 1)) == 0, "page arithmetic by shift and mask");

template <typename T, int HD, bool FP8>
__global__ __launch_bounds__(256) void kv_write_multi_k(const KvWriteMultiParams p) {
  constexpr int C8 = HD / 8, HPP = 64 / C8;  // 16-byte vectors per head, heads per pass
  const int lane = threadIdx.x & 63, d8 = lane % C8;
  const int item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  if (item >= p.sq * p.b * p.g) return;
  const int g = item % p.g, m = (item / p.g) % p.b, t = item / (p.g * p.b);
  int64_t slot = p.slot[m * p.slot_sb] + t;
  if (p.page_table && t > 0) {
    const int64_t lp = (int64_t)p.kv_len[m * p.kv_len_sb] - p.sq + t;  // (floor division, as torch's //)
    const int64_t pi = min(max(lp >> __builtin_ctz(KV_PAGE), (int64_t)0), (int64_t)p.pt_ld - 1);
    slot = (int64_t)p.page_table[(int64_t)m * p.pt_ld + pi] * KV_PAGE + (lp & (KV_PAGE - 1));
  }
  const bool store = slot >= 0 && slot < p.L;
  float c[4] = {1.f, 1.f, 1.f, 1.f}, sn[4] = {0.f, 0.f, 0.f, 0.f};
  if (p.cos) {
    const int64_t at = min(max(p.pos[(int64_t)m * p.pos_sb + t], (int64_t)0), p.max_pos - 1);
    const float4 cv = *reinterpret_cast<const float4*>(p.cos + at * (HD / 2) + d8 * 4);
    const float4 sv = *reinterpret_cast<const float4*>(p.sin + at * (HD / 2) + d8 * 4);
    c[0] = cv.x; c[1] = cv.y; c[2] = cv.z; c[3] = cv.w;
    sn[0] = sv.x; sn[1] = sv.y; sn[2] = sv.z; sn[3] = sv.w;
  }
  T* grp = (T*)p.qkv + (int64_t)t * p.q_ss + (int64_t)m * p.q_sb + (int64_t)g * p.q_sg + d8 * 8;
  const int64_t dst = slot * p.c_ss + (int64_t)m * p.c_sb + (int64_t)g * HD + d8 * 8;
  for (int h = lane / C8; h < p.r + 2; h += HPP) {  // 0..r-1 query heads, r the key, r + 1 the value
    T* ptr = grp + (int64_t)h * p.q_sh;
    V16<T> v = ld16(ptr);
    if (h <= p.r && p.cos) {
      rope_rot8(v, c, sn);
      st16(ptr, v);
    }
    if (h < p.r || !store) continue;
    const bool isv = h > p.r;
    if constexpr (FP8) {
      float f[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = to_f(v.v[e]);
      *reinterpret_cast<uint2*>((uint8_t*)(isv ? p.vcache : p.kcache) + dst) =
          e4m3_pack8(f, 1.0f / p.scales[(isv ? p.g : 0) + g]);
    } else {
      st16((T*)(isv ? p.vcache : p.kcache) + dst, v);
    }
  }
}

template <typename T>
void launch(const KvWriteMultiParams& p, hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)p.sq * p.b * p.g + 3) / 4));
  if (p.hd == 128) {
    if (p.scales) hipLaunchKernelGGL((kv_write_multi_k<T, 128, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((kv_write_multi_k<T, 128, false>), grid, dim3(256), 0, s, p);
  } else {
    if (p.scales) hipLaunchKernelGGL((kv_write_multi_k<T, 64, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((kv_write_multi_k<T, 64, false>), grid, dim3(256), 0, s, p);
  }
}

}  // namespace

void kv_write_multi(const KvWriteMultiParams& p, int dt, hipStream_t s) {
  if ((int64_t)p.sq * p.b * p.g == 0) return;
  if (dt == DT_BF16) launch<bf16>(p, s);
  else launch<fp16>(p, s);
}

}  // namespace ema
