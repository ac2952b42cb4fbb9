// Multi-row decode attention for gfx950: 2-16 new query tokens per sequence
// against a long KV cache whose length lives on the device (a speculative
// verify step, a small piece of a chunked prefill, any multi-token step
// inside a captured graph).
//
// flash_decode.hip serves one query row per sequence and scores on the VALU
// (lane = key); the FlashAttention forward takes a host key count and walks
// the whole cache serially, one workgroup per (sequence, head).  Here the
// (query head of a KV group, token) pairs that share every K/V byte are packed
// into the N dimension of a matrix instruction, and the KEYS are split over
// the grid as in flash_decode.hip:
//
//   grid = key chunks x (KV groups x head slices) x batch, 256 threads.  A
//   workgroup takes one chunk (128 or 256 keys, flash_decode_mq_chunk) of one
//   KV group of one sequence and the packed rows of hps = min(r, 32 / sq) whole
//   heads (at most 32 rows; row = head * sq + token).  Two forms: up to 16
//   packed rows run v_mfma_f32_16x16x32, 17-32 run v_mfma_f32_32x32x16.
//   Each wave owns 32 keys of every 128 of the chunk and never meets the
//   others before the end:
//     * scores, swapped: S^T = K Q^T (keys = M, packed rows = N, head dim = K).
//       The Q fragments are loaded once and stay in registers.  A lane's K
//       fragment is 8 consecutive dims of one key: one 16-B global load (KV8: an
//       8-B load expanded with v_cvt_pk_f32_fp8, exact) straight to registers.
//     * mask and softmax in registers in the log2 domain, one bound pair (lo,
//       e) per packed row = per lane; only a wave tile that straddles a bound
//       compares.  A row's keys lie in the registers of 64 / N lanes: two or
//       four lane-xor steps finish its max and its sum.
//     * P.V: O^T = V^T P^T.  In the swapped form the score accumulator of a lane
//       already is its B-operand fragment (fa_common.h), so P crosses with no
//       LDS and no permute: a rounding to T.  V is token-major: the wave writes
//       its 32 V rows to its own LDS image (image (a) of fa_common.h, the
//       forward kernel's) and reads V^T fragments with ds_read_b64_tr_b16.  KV8:
//       V bytes are expanded before the LDS write.
//     * the four waves' (m, l, O) meet once per workgroup: (m, l) through LDS,
//       then each wave rescales its O and the waves add into one fp32 LDS tile
//       in wave order.
//   Partials (unnormalised fp32 O, (m, l) per row) go to the workspace with
//   agent-scope write-through stores; the last workgroup of a (sequence, group,
//   slice) to arrive combines them in chunk order and re-arms the counter: the
//   protocol of decode_attn_k, one launch, deterministic.  A chunk past the
//   sequence's length or below every row's window writes only (-inf, 0).
//
// Where this departs from the outline it was built to:
//   * all loads of a wave TILE (32 keys: its K fragments and its V rows), not
//     of the whole chunk, are issued before the first wait: at 256 keys per
//     chunk the second tile's fragments would not fit beside the first's;
//   * V is staged per wave, not per chunk: no workgroup barrier inside the key
//     loop, 8 KiB of LDS per wave at hd 128;
//   * chunks are 128 or 256 keys (a wave tile is 32 keys in both MFMA forms), so
//     nothing smaller than 128 keys per workgroup widens a small grid;
//   * the tile image is the forward kernel's, whose transposed reads are
//     conflict-free; its 16-B row writes were not measured.
//
// FP8 (KV8): the K scale folds into the score scale and the V scale into the
// final normalisation, so with power-of-two scales the result is bitwise that
// of the 16-bit form over the dequantised cache.  Paged: a chunk never
// straddles a page (KV_PAGE % chunk == 0): one uniform table load per
// workgroup, bitwise the contiguous result.
#include <type_traits>

#include "common.h"
#include "fa_common.h"
#include "kernels.h"

namespace ema {
namespace {

typedef __attribute__((ext_vector_type(2))) float f2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
using fa::f32x16;

// The two MFMA forms.  32 rows: fa_common.h's maps.  16 rows (16x16x32):
//   A[row = lane&15][k = 8*(lane>>4) + j], B[k = 8*(lane>>4) + j][col = lane&15],
//   C/D: col = lane&15, row = 4*(lane>>4) + reg, reg = 0..3.
template <typename T, bool R32>
struct Mma;
template <typename T>
struct Mma<T, true> {
  typedef f32x16 acc;
  static constexpr int AR = 16;
  static __device__ __forceinline__ acc mfma(typename fa::MT<T>::x8 a, typename fa::MT<T>::x8 b, acc c) {
    return fa::MT<T>::mfma(a, b, c);
  }
};
template <typename T>
struct Mma<T, false> {
  typedef f32x4 acc;
  static constexpr int AR = 4;
  static __device__ __forceinline__ acc mfma(typename fa::MT<T>::x8 a, typename fa::MT<T>::x8 b, acc c) {
    if constexpr (__is_same(T, bf16)) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};

// 8 e4m3fn bytes -> 8 values of T (v_cvt_pk_f32_fp8, then a rounding that is
// exact: e4m3 fits bf16 and fp16)
template <typename T>
__device__ __forceinline__ typename fa::MT<T>::x8 e4m3x8(uint2 w) {
  typename fa::MT<T>::x8 r;
  const f2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, false);
  const f2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.x, true);
  const f2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, false);
  const f2 d = __builtin_amdgcn_cvt_pk_f32_fp8((int)w.y, true);
  r[0] = (T)a[0]; r[1] = (T)a[1]; r[2] = (T)b[0]; r[3] = (T)b[1];
  r[4] = (T)c[0]; r[5] = (T)c[1]; r[6] = (T)d[0]; r[7] = (T)d[1];
  return r;
}

template <typename T, int HD, bool KV8, bool PAGED, bool R32>
__global__ __launch_bounds__(256) void decode_attn_mq_k(const DecodeMqParams p) {
  typedef Mma<T, R32> M;
  typedef typename M::acc acc_t;
  typedef typename fa::MT<T>::x8 x8;
  typedef typename fa::MT<T>::x4 x4;
  typedef std::conditional_t<KV8, uint8_t, T> KT;     // cache element
  typedef std::conditional_t<KV8, uint2, x8> kpiece;  // 8 dims of one K / V row
  constexpr int NR = R32 ? 32 : 16;  // packed rows: the MFMA's N
  constexpr int AR = M::AR;          // accumulator registers
  constexpr int NST = R32 ? 1 : 2;   // score tiles per 32-key wave tile
  constexpr int KW = R32 ? 16 : 32;  // head dims per score k-step
  constexpr int KS = HD / KW;
  constexpr int DT = HD / NR;        // O^T tiles of NR dims
  constexpr int NPV = R32 ? 2 : 1;   // P.V k-steps per wave tile (16 / 32 keys each)
  constexpr int CPR = HD / 8;        // 8-dim pieces per V row
  constexpr int NVL = 32 * CPR / 64; // V pieces per lane per wave tile
  constexpr int TILEB = 32 * HD * 2; // bytes of a wave's V image
  static_assert(KV_PAGE % 256 == 0, "a chunk must not straddle a page");
  __shared__ __attribute__((aligned(16))) char vimg[4][TILEB];
  __shared__ float osum[HD][NR + 1];  // the workgroup's O^T (rows padded: both accesses conflict-free)
  __shared__ float sm[4][NR], sl[4][NR];
  __shared__ int last_sh;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & (NR - 1), hq = lane / NR;  // packed row; k-group of the fragment maps
  const int chunk = blockIdx.x, nsplit = gridDim.x;
  const int r = p.nq / p.nkv, hps = p.hps, nsl = (r + hps - 1) / hps;
  const int g = blockIdx.y / nsl, hs = blockIdx.y % nsl, b = blockIdx.z;
  const int h0 = hs * hps, nh = min(hps, r - h0);  // heads g*r + h0 .. + nh - 1
  const int sq = p.sq, nrow = nh * sq;             // packed rows in use (<= NR)
  const int CH = p.chunk, k0 = chunk * CH;
  const int n = p.kv_len ? min(p.kv_len[(int64_t)b * p.kv_len_sb], p.sk) : p.sk;
  const int win = p.window;
  // token 0 has the lowest bounds, token sq - 1 the highest: keys outside
  // [lo_min, n) count for no row
  const int lo_min = win > 0 ? max(n - (sq - 1) - win, 0) : 0;
  const bool live = k0 < n && k0 + CH > lo_min;
  // this lane's packed row: token tk of head h0 + hj sees keys [lo, e)
  const int hj = col / sq, tk = col - hj * sq;
  const bool rv = col < nrow;
  const int e = rv ? n - (sq - 1 - tk) : 0;
  const int lo = win > 0 ? max(e - win, 0) : 0;
  float sl2 = p.scale * 1.4426950408889634f, vsc = 1.f;
  if constexpr (KV8) {
    sl2 *= p.k_scale[g];
    vsc = p.v_scale[g];
  }
  auto ldk = [](const KT* a) -> kpiece {
    if constexpr (KV8) return *reinterpret_cast<const uint2*>(a);
    else return fa::ld8(a);
  };
  auto frag = [](kpiece v) -> x8 {
    if constexpr (KV8) return e4m3x8<T>(v);
    else return v;
  };
  // key (within the wave tile) of score register i of tile st; head dim (within
  // O^T tile dt) of accumulator register i
  auto koff = [&](int st, int i) { return R32 ? fa::acc_row(i, hq) : 16 * st + 4 * hq + i; };
  auto odim = [&](int dt, int i) { return NR * dt + (R32 ? fa::acc_row(i, hq) : 4 * hq + i); };

  if (live) {
    x8 qf[KS];  // B operand: packed row col, dims KW ks + 8 hq .. + 7 (absent rows: zero)
    {
      const T* qrow = (const T*)p.q + (int64_t)b * p.q_sb + (int64_t)g * p.q_sg +
                      (int64_t)(h0 + (rv ? hj : 0)) * p.q_sh + (int64_t)(rv ? tk : 0) * p.q_ss + 8 * hq;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = fa::ld8(qrow + KW * ks);
        if (!rv) qf[ks] = x8{};
      }
    }
    // r0: the cache row of the chunk's first key: k0 of column b, or (paged) its
    // place in the pool from one uniform table load, the entry clamped
    int r0 = k0;
    int64_t kb = (int64_t)b * p.k_sb, vb = (int64_t)b * p.v_sb;
    if constexpr (PAGED) {
      const int pg = p.page_table[(int64_t)b * p.pt_ld + k0 / KV_PAGE];
      r0 = min(max(pg, 0), p.n_pages - 1) * KV_PAGE + k0 % KV_PAGE;
      kb = vb = 0;
    }
    const KT* kbase = (const KT*)p.k + kb + (int64_t)g * p.k_sg + 8 * hq;
    const KT* vbase = (const KT*)p.v + vb + (int64_t)g * p.v_sg;
    char* img = vimg[wave];
    // transposed-read addresses: a 16-lane group reads 4 keys x 16 dims, lane gi
    // supplies 4 dims (4 tp ..) of key tq and receives dim gi of the 4 keys
    const int gi = lane & 15, tq = gi >> 2, tp = gi & 3;
    const int trow = 4 * hq + tq;                               // + 16 pv (32 rows); second half + 8 / + 16
    const int tdim = (R32 ? 16 * ((lane >> 4) & 1) : 0) + 4 * tp;  // + NR dt

    acc_t o[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int i = 0; i < AR; ++i) o[d][i] = 0.f;
    float m_i = -INFINITY, l_i = 0.f;

#pragma unroll 1
    for (int kt = wave * 32; kt < CH; kt += 128) {
      const int a0 = k0 + kt;  // the wave tile's keys a0 .. a0 + 31
      // keys that count for some row: [lo_k, hi_k); the others are loaded from a
      // key inside it (rows past the length may hold anything, NaN included)
      const int hi_k = min(n, a0 + 32), lo_k = max(lo_min, a0);
      if (hi_k <= lo_k) continue;  // (wave-uniform)
      auto crow = [&](int key) { return (int64_t)(r0 + min(max(key, lo_k), hi_k - 1) - k0); };
      kpiece kf[NST][KS], vv[NVL];
#pragma unroll
      for (int st = 0; st < NST; ++st) {
        const KT* kr = kbase + crow(a0 + NR * st + col) * p.k_ss;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[st][ks] = ldk(kr + KW * ks);
      }
#pragma unroll
      for (int i = 0; i < NVL; ++i) {
        const int idx = i * 64 + lane;
        vv[i] = ldk(vbase + crow(a0 + idx / CPR) * p.v_ss + 8 * (idx % CPR));
      }
      acc_t s[NST];
#pragma unroll
      for (int st = 0; st < NST; ++st) {
#pragma unroll
        for (int i = 0; i < AR; ++i) s[st][i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) s[st] = M::mfma(frag(kf[st][ks]), qf[ks], s[st]);
      }
      // V rows -> this wave's image (the previous tile's reads were consumed)
      asm volatile("" ::: "memory");
#pragma unroll
      for (int i = 0; i < NVL; ++i) {
        const int idx = i * 64 + lane;
        *reinterpret_cast<x8*>(img + fa::ia_off<HD>(idx / CPR, idx % CPR)) = frag(vv[i]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      // mask: only a tile that straddles some row's bound
      if (a0 + 32 > n - (sq - 1) || (win > 0 && a0 < n - win)) {
#pragma unroll
        for (int st = 0; st < NST; ++st)
#pragma unroll
          for (int i = 0; i < AR; ++i) {
            const int key = a0 + koff(st, i);
            if (key >= e || key < lo) s[st][i] = -INFINITY;
          }
      }
      float mt = -INFINITY;
#pragma unroll
      for (int st = 0; st < NST; ++st)
#pragma unroll
        for (int i = 0; i < AR; ++i) mt = fmaxf(mt, s[st][i]);
#pragma unroll
      for (int x = NR; x < 64; x <<= 1) mt = fmaxf(mt, __shfl_xor(mt, x, 64));
      mt *= sl2;
      const float m_new = fmaxf(m_i, mt);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f(m_i - m_use);
      float rsum = 0.f;
#pragma unroll
      for (int st = 0; st < NST; ++st)
#pragma unroll
        for (int i = 0; i < AR; ++i) {
          s[st][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[st][i], sl2, -m_use));
          rsum += s[st][i];
        }
#pragma unroll
      for (int x = NR; x < 64; x <<= 1) rsum += __shfl_xor(rsum, x, 64);
      l_i = l_i * alpha + rsum;
      m_i = m_new;
      if (__builtin_amdgcn_ballot_w64(alpha != 1.f)) {
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
          for (int i = 0; i < AR; ++i) o[d][i] *= alpha;
      }
      // P.V: the accumulator registers of a lane are its B fragment: k-step pv
      // holds keys 16 pv + 8 (j >> 2) + 4 hq + (j & 3) (32 rows), 16 (j >> 2) +
      // 4 hq + (j & 3) (16 rows); the two transposed reads match that order
#pragma unroll
      for (int pv = 0; pv < NPV; ++pv) {
        x8 pf;
        if constexpr (R32) {
          pf = fa::acc_frag<T>(s[0], pv);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            pf[j] = (T)s[0][j];
            pf[4 + j] = (T)s[1][j];
          }
        }
        const int row0 = trow + 16 * pv, row1 = row0 + (R32 ? 8 : 16);
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          const int dim = NR * d + tdim;
          const x4 v0 = fa::MT<T>::tr_read((const T*)(img + fa::ia_off<HD>(row0, dim >> 3) + 2 * (dim & 7)));
          const x4 v1 = fa::MT<T>::tr_read((const T*)(img + fa::ia_off<HD>(row1, dim >> 3) + 2 * (dim & 7)));
          o[d] = M::mfma(fa::join<T>(v0, v1), pf, o[d]);
        }
      }
      asm volatile("" ::: "memory");
    }

    // the four waves meet: M = max m_w, every wave scales its O by 2^(m_w - M),
    // then the waves add into osum in wave order
    if (hq == 0) {
      sm[wave][col] = m_i;
      sl[wave][col] = l_i;
    }
    __syncthreads();
    const float Mx = fmaxf(fmaxf(sm[0][col], sm[1][col]), fmaxf(sm[2][col], sm[3][col]));
    const float a = m_i == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m_i - Mx);
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int i = 0; i < AR; ++i) o[d][i] *= a;
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
      if (wave == w) {
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
          for (int i = 0; i < AR; ++i) {
            float* dst = &osum[odim(d, i)][col];
            *dst = w == 0 ? o[d][i] : *dst + o[d][i];
          }
      }
      __syncthreads();
    }
  }

  // chunk partials [b][nq][sq][split][HD] and (max, sum) per (row, split): write-
  // through (agent-scope) stores, drained before the arrival is counted; the
  // last workgroup of this (sequence, group, slice) acquires and combines them
  // (the protocol of decode_attn_k).  An idle chunk leaves only (-inf, 0).
  auto put = [](float* a, float v) { __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
  // workspace row of packed row pr
  auto wrow = [&](int pr) { return ((int64_t)b * p.nq + g * r + h0 + pr / sq) * sq + pr % sq; };
  if (live) {
    for (int i = tid; i < nrow * HD; i += 256) {
      const int pr = i / HD, d = i % HD;
      put(p.ws_o + (wrow(pr) * nsplit + chunk) * HD + d, osum[d][pr]);
    }
  }
  if (tid < nrow) {
    float Mx = -INFINITY, L = 0.f;
    if (live) {
      Mx = fmaxf(fmaxf(sm[0][tid], sm[1][tid]), fmaxf(sm[2][tid], sm[3][tid]));
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if (sm[w][tid] != -INFINITY) L += sl[w][tid] * __builtin_amdgcn_exp2f(sm[w][tid] - Mx);
    }
    const int64_t idx = wrow(tid) * nsplit + chunk;
    put(p.ws_ml + 2 * idx, Mx);
    put(p.ws_ml + 2 * idx + 1, L);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    unsigned* cnt = p.counters + (int64_t)b * gridDim.y + blockIdx.y;
    const unsigned prev = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = prev == (unsigned)nsplit - 1u;
    if (last) {
      // re-arm for the next launch (same stream: it starts after this one ends)
      __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    last_sh = last;
  }
  __syncthreads();
  if (!last_sh) return;
  // O = sum_s o_s 2^(m_s - M) / sum_s l_s 2^(m_s - M), splits in order
  // (deterministic); an idle split's O partial is never used
  for (int i = tid; i < nrow * HD; i += 256) {
    const int pr = i / HD, d = i % HD;
    const int64_t wr = wrow(pr);
    const float2* ml = reinterpret_cast<const float2*>(p.ws_ml) + wr * nsplit;
    const float* os = p.ws_o + wr * nsplit * HD + d;
    float Mx = -INFINITY;
    for (int s0 = 0; s0 < nsplit; s0 += 8) {
      float2 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = ml[min(s0 + u, nsplit - 1)];
#pragma unroll
      for (int u = 0; u < 8; ++u) Mx = fmaxf(Mx, v[u].x);
    }
    float L = 0.f, ov = 0.f;
    for (int s0 = 0; s0 < nsplit; s0 += 8) {
      float2 v[8];
      float pv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int sp = min(s0 + u, nsplit - 1);
        v[u] = ml[sp];
        pv[u] = os[(int64_t)sp * HD];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (s0 + u >= nsplit || v[u].x == -INFINITY) continue;
        const float w = __builtin_amdgcn_exp2f(v[u].x - Mx);
        L = __builtin_fmaf(v[u].y, w, L);
        ov = __builtin_fmaf(pv[u], w, ov);
      }
    }
    const int head = g * r + h0 + pr / sq, t = pr % sq;
    ((T*)p.o)[(int64_t)b * p.o_sb + (int64_t)t * p.o_ss + (int64_t)head * p.o_sh + d] =
        (T)(L > 0.f ? (KV8 ? ov / L * vsc : ov / L) : 0.f);
  }
}

template <typename T, int HD, bool KV8, bool PAGED>
void launch_rows(const DecodeMqParams& p, hipStream_t s) {
  const int r = p.nq / p.nkv, nsl = (r + p.hps - 1) / p.hps;
  const dim3 grid(flash_decode_mq_splits(p.sk, p.chunk), p.nkv * nsl, p.b);
  if (p.hps * p.sq > 16) hipLaunchKernelGGL((decode_attn_mq_k<T, HD, KV8, PAGED, true>), grid, dim3(256), 0, s, p);
  else hipLaunchKernelGGL((decode_attn_mq_k<T, HD, KV8, PAGED, false>), grid, dim3(256), 0, s, p);
}

template <typename T, int HD>
void launch(const DecodeMqParams& p, hipStream_t s) {
  if (p.page_table) {
    if (p.kv_fp8) launch_rows<T, HD, true, true>(p, s);
    else launch_rows<T, HD, false, true>(p, s);
  } else {
    if (p.kv_fp8) launch_rows<T, HD, true, false>(p, s);
    else launch_rows<T, HD, false, false>(p, s);
  }
}

}  // namespace

int flash_decode_mq_heads(int sq, int nq, int nkv) {
  const int r = nq / nkv, fit = 32 / sq;
  return r < fit ? r : fit;
}
int flash_decode_mq_chunk(int b, int sq, int sk, int nq, int nkv) {
  const int r = nq / nkv, hps = flash_decode_mq_heads(sq, nq, nkv);
  const int64_t base = (int64_t)b * nkv * ((r + hps - 1) / hps);
  return base * ((sk + 255) / 256) >= 256 ? 256 : 128;
}
int flash_decode_mq_splits(int sk, int chunk) { return (sk + chunk - 1) / chunk; }
int flash_decode_mq_counters(int b, int sq, int nq, int nkv) {
  const int r = nq / nkv, hps = flash_decode_mq_heads(sq, nq, nkv);
  return b * nkv * ((r + hps - 1) / hps);
}
int64_t flash_decode_mq_workspace(int b, int sq, int nq, int splits, int hd) {
  return (int64_t)b * nq * sq * splits * (hd + 2);
}

void flash_decode_mq(const DecodeMqParams& p, int dt, hipStream_t s) {
  if (dt == DT_BF16) {
    if (p.hd == 128) launch<bf16, 128>(p, s);
    else launch<bf16, 64>(p, s);
  } else {
    if (p.hd == 128) launch<fp16, 128>(p, s);
    else launch<fp16, 64>(p, s);
  }
}

}  // namespace ema
