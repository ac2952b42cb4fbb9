// Shared pieces of the decode weight-streaming GEMMs (skinny_gemm.hip: <= 32
// rows, X in registers; wide_gemm.hip: 33-64 rows, X through LDS): the MFMA
// wrapper, the e4m3 / MXFP4 piece expansions, and the fused epilogues with
// their prefetched operands.  Every function is internal to the including
// translation unit.
#pragma once
#include <type_traits>

#include "act_math.h"
#include "common.h"
#include "fa_common.h"
#include "kernels.h"

namespace ema {
namespace {

typedef __attribute__((ext_vector_type(4))) float f4;
typedef __attribute__((ext_vector_type(2))) float f2;
typedef __attribute__((ext_vector_type(4))) int i4;
typedef __attribute__((ext_vector_type(2))) int i2;

enum { EPI_PLAIN = 0, EPI_RES = 1, EPI_GLU = 2, EPI_QKV = 3, EPI_ACT = 4 };
// norm prologue of the skinny kernels (SkinnyArgs::norm_w / norm_b)
enum { NORM_NONE = 0, NORM_RMS = 1, NORM_LN = 2 };

template <typename T>
__device__ __forceinline__ f4 mfma16x16x32(typename fa::MT<T>::x8 a, typename fa::MT<T>::x8 b, f4 c) {
  if constexpr (__is_same(T, bf16)) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// 8 e4m3fn bytes (k order: lo bytes 0-3, hi bytes 0-3) -> one A fragment of T;
// every e4m3 value is exact in bf16 and fp16
template <typename T>
__device__ __forceinline__ typename fa::MT<T>::x8 fp8x8(int lo, int hi) {
  typename fa::MT<T>::x8 o;
  const f2 c0 = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false), c1 = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true);
  const f2 c2 = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false), c3 = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
  o[0] = (T)c0[0]; o[1] = (T)c0[1]; o[2] = (T)c1[0]; o[3] = (T)c1[1];
  o[4] = (T)c2[0]; o[5] = (T)c2[1]; o[6] = (T)c3[0]; o[7] = (T)c3[1];
  return o;
}

// W4 ring slot: the lane's 8 e2m1 nibbles of each of four k-steps and the four
// e8m0 bytes (byte h = k-step h) of its W row
struct W4Slot {
  i4 v;
  int sc;
};

// 8 e2m1 nibbles (k order: byte 0 low, byte 0 high, byte 1 low, ...) times
// 2^(e8m0 byte h of sc - 127) -> one A fragment of T.  The quantiser keeps
// every product a normal number of T, so the conversion is exact and the byte
// is never the zero / NaN encoding.
template <typename T>
__device__ __forceinline__ typename fa::MT<T>::x8 fp4x8(int v, int sc, int h) {
  typename fa::MT<T>::x8 o;
  const float s = __builtin_bit_cast(float, ((sc >> (8 * h)) & 0xff) << 23);
  if constexpr (__is_same(T, bf16)) {
    const auto c0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, s, 0);
    const auto c1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, s, 1);
    const auto c2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, s, 2);
    const auto c3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, s, 3);
    o[0] = c0[0]; o[1] = c0[1]; o[2] = c1[0]; o[3] = c1[1];
    o[4] = c2[0]; o[5] = c2[1]; o[6] = c3[0]; o[7] = c3[1];
  } else {
    const auto c0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, s, 0);
    const auto c1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, s, 1);
    const auto c2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, s, 2);
    const auto c3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, s, 3);
    o[0] = c0[0]; o[1] = c0[1]; o[2] = c1[0]; o[3] = c1[1];
    o[4] = c2[0]; o[5] = c2[1]; o[6] = c3[0]; o[7] = c3[1];
  }
  return o;
}

// W row fed to MFMA row r of workgroup n-block `blk`
template <int EPI>
__device__ __forceinline__ int64_t w_row(int blk, int r, int N) {
  if constexpr (EPI == EPI_GLU) return r < 8 ? (int64_t)blk * 8 + r : (int64_t)N + blk * 8 + (r - 8);
  else return (int64_t)blk * 16 + r;
}

// Output of one 16-feature block (t = the block's reduced fp32 tile; lane
// holds column m = lane & 15, features 4 (lane >> 4) + i).
// The epilogue's global operands for one block, loaded ahead (before the
// block's k-loop) by the wave that runs the epilogue, so the epilogue does not
// wait out load round trips while the other waves stream the next block: the
// residual tile (EPI_RES) or the rotary cos / sin pairs (EPI_QKV; the token
// positions and the cache slot once per workgroup).
template <typename T, int EPI>
struct EpiPre {
  typename fa::MT<T>::x4 rv{};
  float c[2] = {0.f, 0.f}, s[2] = {0.f, 0.f};
  int pos = 0;       // (32-bit: two row blocks' 64-bit positions and slots spilled)
  int64_t slot = 0;  // uniform: scalar registers
  f4 sc = {1.f, 1.f, 1.f, 1.f};  // W8: the scales of the lane's 4 W rows (epi_scale)
  float kvr = 1.f;  // FP8 KV cache: 1 / scale of the lane's k / v head (kv_rscale)
};

// FP8 KV cache: the reciprocal scale of the k (h == r) or v (h == r + 1) head
// of group g; q heads store no cache value
__device__ __forceinline__ float kv_rscale(const SkinnyArgs& p, int n) {
  const int per_g = (p.r + 2) * p.hd, g = n / per_g, h = (n - g * per_g) / p.hd;
  if (h < p.r) return 1.f;
  const int ng = p.N / per_g;
  return 1.0f / p.kv_scale[(h - p.r) * ng + g];
}

// W8: the reduced fp32 tile times the row scales, in front of the epilogue's
// first rounding.  The product is handed on as an opaque value so that the
// epilogue compiles from the same expressions as in the 16-bit forms: fused
// with the multiply, hipcc contracted other products of the rotary rotation
// into FMAs than it does there, and a q element that cancels to ~1e-5 of its
// terms came out one ulp apart.
__device__ __forceinline__ f4 scale_tile(f4 t, const f4& sc) {
  t *= sc;
  asm volatile("" : "+v"(t));
  return t;
}

// W8: the fp32 scales of the 4 W rows whose sums this lane holds (MFMA rows
// 4 (lane >> 4) + i: consecutive W rows in every form, 16-B aligned)
template <int EPI>
__device__ __forceinline__ f4 epi_scale(const SkinnyArgs& p, int blk, int half, int lane) {
  const int nr = 4 * (lane >> 4);
  int64_t row;
  if constexpr (EPI == EPI_GLU) {
    // half unit: MFMA rows 0-3 / 8-11 (4-7 / 12-15 duplicate them) = features 8 blk + 4 half ..
    if (half < 0) row = w_row<EPI>(blk, nr, p.N);
    else row = (nr < 8 ? 0 : (int64_t)p.N) + (int64_t)blk * 8 + 4 * half;
  } else {
    row = (int64_t)blk * 16 + nr;
  }
  return *reinterpret_cast<const f4*>(p.w_scale + row);
}

// EPI_QKV: which geometry of SkinnyArgs the call has.  GEOM -1: read at run
// time (p.seqs, a wave-uniform branch); 0 / 1: the kernel was compiled for one
// row per sequence / for the multi-row geometry.  The persistent forms take
// it as a template argument: beside their k-loop's registers the run-time
// branch cost them 1-4 VGPRs and put 12 B of scratch into a form that had
// none (profiles/r23b_fused_multirow_isa.txt).
template <int GEOM>
__device__ __forceinline__ bool qkv_multi(const SkinnyArgs& p) {
  if constexpr (GEOM < 0) return p.seqs != 0;
  else return GEOM == 1;
}

// EPI_QKV: the rotary position of GEMM row i.  One row per sequence: pos[i *
// pos_sb].  Multi-row geometry: row i is token t = i / seqs of sequence m = i %
// seqs, its position pos[m * pos_sb + t] of the [b, sq] ids as the decoders
// hold them, clamped to the tables as kv_write_multi_k clamps it.
template <int GEOM>
__device__ __forceinline__ int64_t qkv_pos(const SkinnyArgs& p, int i) {
  if (qkv_multi<GEOM>(p)) {
    const int t = (i * p.seqs_mul) >> 16, m = i - t * p.seqs;
    return min(max(p.pos[(int64_t)m * p.pos_sb + t], (int64_t)0), (int64_t)p.max_pos - 1);
  }
  return p.pos[(int64_t)i * p.pos_sb];
}

// EPI_QKV, multi-row geometry: the cache slot of GEMM row i (uniform: scalar
// loads of the sequence's slot, key count and table entry, scalar arithmetic),
// or -1 for a row that is not stored; col receives its cache column m.
__device__ __forceinline__ int64_t multi_slot(const SkinnyArgs& p, int i, int& col) {
  static_assert((KV_PAGE & (KV_PAGE - 1)) == 0, "page arithmetic by shift and mask");
  const int t = (i * p.seqs_mul) >> 16, m = i - t * p.seqs;
  col = m;
  int64_t slot = p.slot_ptr[m * p.slot_sb] + t;
  if (p.page_table && t > 0) {
    const int sq = (p.M * p.seqs_mul) >> 16;
    const int64_t lp = (int64_t)p.kv_len[m * p.kv_len_sb] - sq + t;  // (floor division, as torch's //)
    const int64_t pi = min(max(lp >> __builtin_ctz(KV_PAGE), (int64_t)0), (int64_t)p.pt_ld - 1);
    slot = (int64_t)p.page_table[(int64_t)m * p.pt_ld + pi] * KV_PAGE + (lp & (KV_PAGE - 1));
  }
  return slot >= 0 && slot < p.L ? slot : -1;
}

// EPI_QKV: the lane's 4 rotated k or v values (head h of group g, dims d ..
// d + 3, feature n) to cache row `sl`, column `col`.  e4m3 cache: as rounded to
// T, scaled, clamped (the convert alone turns an overflow into NaN), packed and
// stored as one dword.
template <typename T, int EPI>
__device__ __forceinline__ void kv_put(const SkinnyArgs& p, const typename fa::MT<T>::x4& o, int h,
                                       int n, int g, int d, int64_t sl, int col,
                                       const EpiPre<T, EPI>& pre, bool use_pre) {
  const int hd = p.hd;
  if (p.kv_scale) {
    const float inv = use_pre ? pre.kvr : kv_rscale(p, n);
    float f[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = fminf(fmaxf((float)o[e] * inv, -448.f), 448.f);
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w, true);
    uint8_t* c8 = (uint8_t*)(h == p.r ? p.kcache : p.vcache);
    *reinterpret_cast<int*>(c8 + sl * p.c_ss + (int64_t)col * p.c_sb + (int64_t)g * hd + d) = w;
  } else {
    T* cache = (T*)(h == p.r ? p.kcache : p.vcache);
    *reinterpret_cast<typename fa::MT<T>::x4*>(cache + sl * p.c_ss + (int64_t)col * p.c_sb +
                                               (int64_t)g * hd + d) = o;
  }
}

template <typename T, int EPI, int GEOM = -1>
__device__ __forceinline__ void epi_init(const SkinnyArgs& p, int lane, EpiPre<T, EPI>& e,
                                         int moff = 0) {
  if constexpr (EPI == EPI_QKV) {
    const int m = (lane & 15) + moff;
    e.pos = m < p.M ? (int)qkv_pos<GEOM>(p, m) : 0;
    const int64_t sl = p.slot_ptr ? *p.slot_ptr : p.slot;
    e.slot = (int64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(sl & 0xffffffffll)) |
             ((int64_t)__builtin_amdgcn_readfirstlane((int)(sl >> 32)) << 32);
  }
}

template <typename T, int EPI>
__device__ __forceinline__ void epi_prefetch(const SkinnyArgs& p, int blk, int lane, EpiPre<T, EPI>& e,
                                             int moff = 0) {
  const int m = (lane & 15) + moff, n = blk * 16 + 4 * (lane >> 4);
  if (m >= p.M) return;
  if constexpr (EPI == EPI_RES) {
    e.rv = *reinterpret_cast<const typename fa::MT<T>::x4*>((const T*)p.res + (int64_t)m * p.ldr + n);
  }
  if constexpr (EPI == EPI_QKV) {
    const int hd = p.hd, per_g = (p.r + 2) * hd;
    const int d = (n - (n / per_g) * per_g) % hd;
    const float* cr = p.cos + (int64_t)e.pos * (hd / 2) + d / 2;
    const float* sr = p.sin + (int64_t)e.pos * (hd / 2) + d / 2;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      e.c[j] = cr[j];
      e.s[j] = sr[j];
    }
    if (p.kv_scale) e.kvr = kv_rscale(p, n);
  }
}

template <typename T, int EPI, int ACT, int GEOM = -1>
__device__ __forceinline__ void epilogue(const SkinnyArgs& p, int blk, const f4& t, int lane,
                                         int half, const EpiPre<T, EPI>& pre, bool use_pre,
                                         int moff = 0) {
  const int M = p.M;
  // D layout: lane holds column m = lane & 15 (+ moff: the row block), rows
  // (features) 4 (lane >> 4) + i
  const int m = (lane & 15) + moff, nr = 4 * (lane >> 4);
  typename fa::MT<T>::x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (T)t[i];
  T* __restrict__ y = (T*)p.y;
  if constexpr (EPI == EPI_GLU) {
    // lanes 0-31 hold up rows 0-7, lanes 32-63 the gate rows of the same f
    typename fa::MT<T>::x4 gt;
#pragma unroll
    for (int i = 0; i < 4; ++i) gt[i] = (T)__shfl_xor((float)o[i], 32, 64);
    // half block (half >= 0): features 4 half .. 4 half + 3 only, in MFMA
    // rows 0-3 / 8-11 (rows 4-7 / 12-15 duplicate them and are not stored)
    if ((half < 0 ? lane < 32 : lane < 16) && m < M) {
      typename fa::MT<T>::x4 out;
#pragma unroll
      for (int i = 0; i < 4; ++i) out[i] = (T)((float)o[i] * act<ACT>((float)gt[i]));
      const int f = blk * 8 + (half < 0 ? nr : 4 * half);
      *reinterpret_cast<typename fa::MT<T>::x4*>(y + (int64_t)m * p.ldy + f) = out;
    }
    return;
  }
  if (m >= M) return;
  const int n = blk * 16 + nr;
  if constexpr (EPI == EPI_RES) {
    const typename fa::MT<T>::x4 rv = use_pre ? pre.rv :
        *reinterpret_cast<const typename fa::MT<T>::x4*>((const T*)p.res + (int64_t)m * p.ldr + n);
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (T)((float)o[i] + (float)rv[i]);
  }
  if constexpr (EPI == EPI_QKV) {
    const int hd = p.hd, per_g = (p.r + 2) * hd;
    const int g = n / per_g, rem = n - g * per_g, h = rem / hd, d = rem - h * hd;
    if (h <= p.r) {  // q heads and the k head: rotate pairs (d, d+1), (d+2, d+3)
      const int64_t pos = use_pre ? 0 : qkv_pos<GEOM>(p, m);
      const float* cr = p.cos + pos * (hd / 2) + d / 2;
      const float* sr = p.sin + pos * (hd / 2) + d / 2;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const float x0 = (float)o[2 * j], x1 = (float)o[2 * j + 1];
        const float c = use_pre ? pre.c[j] : cr[j], sn = use_pre ? pre.s[j] : sr[j];
        o[2 * j] = (T)(x0 * c - x1 * sn);
        o[2 * j + 1] = (T)(x0 * sn + x1 * c);
      }
    }
    T* dst;
    if (h < p.r) {
      dst = y + (int64_t)m * p.ldy + (int64_t)(g * p.r + h) * hd + d;
    } else {
      if (qkv_multi<GEOM>(p)) {
        // multi-row geometry (the verify step of the speculative decoders): the
        // block's rows are tokens of several
        // sequences and a sequence's rows straddle blocks, so the walk is the
        // per-row one below, four rows' slots resolved per round on the scalar
        // unit (multi_slot) before the lanes of each row store.
        const int rows = min(16, M - moff);
#pragma unroll 1
        for (int i0 = 0; i0 < rows; i0 += 4) {
          int64_t sl4[4];
          int col4[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) sl4[u] = multi_slot(p, moff + min(i0 + u, rows - 1), col4[u]);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (m != moff + i0 + u || sl4[u] < 0) continue;
            kv_put<T, EPI>(p, o, h, n, g, d, sl4[u], col4[u], pre, use_pre);
          }
        }
        return;
      }
      if (p.slot_sb) {
        // per-row slots (ragged decode; a wave-uniform branch): one pass per
        // row of the block, the row's slot a scalar load as in the scalar
        // form, the lanes of that row store; four slots fetched per round
        // (indices clamped to the block's last row).  No per-lane slot: the
        // persistent forms have no VGPRs to spare beside the k-loop's
        // (profiles/r15a_ragged_isa.txt).  Rows m >= M have returned above.
        const int rows = min(16, M - moff);
#pragma unroll 1
        for (int i0 = 0; i0 < rows; i0 += 4) {
          int64_t sl4[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) sl4[u] = p.slot_ptr[moff + min(i0 + u, rows - 1)];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (m != moff + i0 + u) continue;
            const int64_t sl = sl4[u];
            if (p.kv_scale) {
              const float inv = use_pre ? pre.kvr : kv_rscale(p, n);
              float f[4];
#pragma unroll
              for (int e = 0; e < 4; ++e) f[e] = fminf(fmaxf((float)o[e] * inv, -448.f), 448.f);
              int w = 0;
              w = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w, false);
              w = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w, true);
              uint8_t* c8 = (uint8_t*)(h == p.r ? p.kcache : p.vcache);
              *reinterpret_cast<int*>(c8 + sl * p.c_ss + (int64_t)m * p.c_sb + (int64_t)g * hd + d) = w;
            } else {
              T* cache = (T*)(h == p.r ? p.kcache : p.vcache);
              *reinterpret_cast<typename fa::MT<T>::x4*>(cache + sl * p.c_ss + (int64_t)m * p.c_sb +
                                                         (int64_t)g * hd + d) = o;
            }
          }
        }
        return;
      }
      const int64_t slot = use_pre ? pre.slot : p.slot_ptr ? *p.slot_ptr : p.slot;
      if (p.kv_scale) {
        // e4m3 cache: the lane's 4 consecutive dims of one token and head, as
        // rounded to T above, scaled, clamped (the convert alone turns an
        // overflow into NaN), packed and stored as one dword
        const float inv = use_pre ? pre.kvr : kv_rscale(p, n);
        float f[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = fminf(fmaxf((float)o[i] * inv, -448.f), 448.f);
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w, true);
        uint8_t* c8 = (uint8_t*)(h == p.r ? p.kcache : p.vcache);
        *reinterpret_cast<int*>(c8 + slot * p.c_ss + (int64_t)m * p.c_sb + (int64_t)g * hd + d) = w;
        return;
      }
      T* cache = (T*)(h == p.r ? p.kcache : p.vcache);
      dst = cache + slot * p.c_ss + (int64_t)m * p.c_sb + (int64_t)g * hd + d;
    }
    *reinterpret_cast<typename fa::MT<T>::x4*>(dst) = o;
    return;
  }
  if constexpr (EPI == EPI_ACT) {  // gelu_fwd_k on the rounded product
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (T)gelu_erf((float)o[i]);
  }
  *reinterpret_cast<typename fa::MT<T>::x4*>(y + (int64_t)m * p.ldy + n) = o;
}

}  // namespace
}  // namespace ema
