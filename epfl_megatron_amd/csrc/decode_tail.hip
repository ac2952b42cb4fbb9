// Tail of one graphed decode step (inference/hip_graph.py), in ONE launch.
// greedy_tail_k (GraphedGreedyDecoder): per sequence the argmax over the
// vocabulary (first maximum, as torch.argmax), the next-token and history
// writes and the position increment; the last workgroup to finish advances
// the step index, the KV-cache slot and the valid-key count.  The eager form
// was seven launches (argmax, index_copy, copy, four adds: ~45 us per token at
// batch 1 with their graph seams, profiles/r4v_decode_b1_kernels.txt).
// sample_tail_k: the same with a temperature / top-k / top-p draw.  Both move
// the batch in lockstep: one step index, cache slot and key count for all rows.
// ragged_tail_k (inference/continuous.py) is the tail of a batch of independent
// sequences: history index, cache slot, key count, position, limit and an
// active flag per row, so a finished row parks and can be refilled between
// replays of the same graph.  The selection code (argmax_row, draw_row) is
// shared; only thread 0's bookkeeping differs.  Its per-row form (template
// argument X) gives every row its own sampling settings, seed and Philox offset
// and reports the log-probability of the emitted token.
// spec_tail_k (inference/speculative.py) is the tail of a speculative greedy
// step: S logits rows per sequence, one workgroup each, and the last of a
// sequence's workgroups to arrive verifies the drafts, commits and drafts anew.
// spec_sample_tail_k is that tail with draw_row in place of the argmax.
//
// Reference: megatron/text_generation/generation.py:179-264 samples on the
// host-driven loop (greedy = argmax of the last position's logits).
#include "common.h"
#include "kernels.h"
#include "philox.h"

namespace ema {
namespace {

template <typename T>
struct Vec16;  // 16 bytes of T
template <>
struct Vec16<bf16> { typedef __attribute__((ext_vector_type(8))) unsigned short t; static constexpr int n = 8; };
template <>
struct Vec16<fp16> { typedef __attribute__((ext_vector_type(8))) unsigned short t; static constexpr int n = 8; };
template <>
struct Vec16<float> { typedef __attribute__((ext_vector_type(4))) float t; static constexpr int n = 4; };

template <typename T>
__device__ __forceinline__ float elem(const typename Vec16<T>::t& v, int e) {
  if constexpr (__is_same(T, float)) return v[e];
  else return (float)__builtin_bit_cast(T, (unsigned short)v[e]);
}

// (value, index) order of torch.argmax: larger value, then smaller index
__device__ __forceinline__ void take(float& bv, int& bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

// Online log-sum-exp of the raw logits (the ragged tail's log-probability
// output): sum_i exp(x_i) = s * exp(m), m the running maximum.  m starts at the
// lowest finite float so that a -inf logit adds exp(-inf) = 0 instead of
// exp(-inf - -inf); one hardware exp per element, the branch is a select.
struct Lse {
  float m, s;
};
constexpr float LSE_LOW = -3.4028234664e38f;

__device__ __forceinline__ void lse_add(Lse& a, float x) {
  const float d = x - a.m, e = __expf(-fabsf(d));
  a.s = d > 0.f ? a.s * e + 1.f : a.s + e;
  a.m = fmaxf(a.m, x);
}

// the rescaling combine of two partial sums
__device__ __forceinline__ void lse_merge(Lse& a, float om, float os) {
  const float m = fmaxf(a.m, om);
  a.s = a.s * __expf(a.m - m) + os * __expf(om - m);
  a.m = m;
}

// Merge of the 1024 per-thread pairs in a fixed order (lane butterfly 32, 16,
// .. 1, then waves 0..15 in sequence on thread 0): same row, same bits.  Ends
// on a barrier-free read of thread 0's own result; red_m / red_s are 16 floats
// of LDS each, not in use by anyone else between the two barriers.
__device__ __forceinline__ void lse_block(Lse& a, float* red_m, float* red_s, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(a.m, o, 64), os = __shfl_xor(a.s, o, 64);
    lse_merge(a, om, os);
  }
  __syncthreads();
  if (lane == 0) {
    red_m[wave] = a.m;
    red_s[wave] = a.s;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < 1024 / 64; ++w) lse_merge(a, red_m[w], red_s[w]);
  }
}

// argmax of one row over the 1024 threads of a workgroup: the result is valid
// in thread 0 (shared by greedy_tail_k and the ragged tail).  LP: the same
// sweep carries the log-sum-exp of the row into *lse (thread 0).
template <typename T, bool LP = false>
__device__ __forceinline__ int argmax_row(const T* __restrict__ lr, int V, int tid, Lse* lse = nullptr) {
  typedef typename Vec16<T>::t vec;
  constexpr int NV = Vec16<T>::n;
  const int lane = tid & 63, wave = tid >> 6;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  Lse acc{LSE_LOW, 0.f};
  // 16-B loads, 8 in flight per thread per round over 1024 threads (one
  // round covers a 32k fp32 vocabulary: the row is latency-, not
  // bandwidth-bound; ld and the row base are 16-B aligned: checked by the
  // host); the < NV tail element-wise
  constexpr int NT = 1024, UR = 8;
  const int nvec = V / NV;
  for (int v0 = tid; v0 < nvec; v0 += UR * NT) {
    vec x[UR];
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const int vi = v0 + u * NT;
      x[u] = vi < nvec ? reinterpret_cast<const vec*>(lr)[vi] : vec{};
    }
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const int vi = v0 + u * NT;
      if (vi < nvec) {
#pragma unroll
        for (int e = 0; e < NV; ++e) {
          const float xe = elem<T>(x[u], e);
          take(bv, bi, xe, vi * NV + e);
          if constexpr (LP) lse_add(acc, xe);
        }
      }
    }
  }
  for (int i = nvec * NV + tid; i < V; i += NT) {
    const float xe = (float)lr[i];
    take(bv, bi, xe, i);
    if constexpr (LP) lse_add(acc, xe);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    take(bv, bi, ov, oi);
  }
  __shared__ float sv[NT / 64];
  __shared__ int si[NT / 64];
  if (lane == 0) {
    sv[wave] = bv;
    si[wave] = bi;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) take(bv, bi, sv[w], si[w]);
  }
  if constexpr (LP) {
    __shared__ float lm[NT / 64], ls[NT / 64];
    lse_block(acc, lm, ls, tid);
    *lse = acc;
  }
  return bi;
}

template <typename T>
__global__ __launch_bounds__(1024) void greedy_tail_k(const T* __restrict__ logits, int64_t ld, int V,
                                                     int64_t* tokens, int64_t* history,
                                                     int64_t hist_ld, int64_t* step_idx,
                                                     int64_t* pos, int64_t* slot, int* kv_len,
                                                     unsigned* counter) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const int bi = argmax_row<T>(logits + (int64_t)row * ld, V, tid);
  if (tid != 0) return;
  const int64_t s = *step_idx;
  tokens[row] = bi;
  history[(int64_t)row * hist_ld + s] = bi;
  pos[row] += 1;
  // every workgroup has read the step index (its history store used it)
  // before it arrives; the last one advances the shared counters and re-arms
  const unsigned prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (prev == gridDim.x - 1) {
    *step_idx = s + 1;
    *slot += 1;
    *kv_len += 1;
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------- sampling tail
// sample_tail_k: the same tail with a temperature / top-k / top-p draw in
// place of the argmax.  Per row, y_i = x_i / temperature (fp32, IEEE divide);
//   top-k (k >= 2): keep i iff fewer than k elements are strictly greater
//                   than y_i (ties with the k-th value are all kept);
//   top-p:          keep i iff M(y_i) <= p, M(y) = softmax mass of the elements
//                   strictly greater than y (the crossing token stays, and so
//                   does every element tied with it: torch.sort would keep an
//                   arbitrary one of them);
//   draw:           argmax over the kept i of y_i + g_i (Gumbel-max), g_i =
//                   -log(-log(u_i)), u_i = ((w >> 8) + 0.5) * 2^-24 with w word
//                   i & 3 of philox((row << 32) | (i >> 2), offset0 + step,
//                   seed); larger key, then smaller index (take());
//   top_k == 1:     the plain argmax, no noise;  then min(token, vocab_limit-1).
// A row whose input token is stop_id emits stop_id again; the last workgroup
// writes the number of rows that emitted stop_id into ctl[5].
//
// Both filters are "keep key(y_i) >= K*" for one 32-bit threshold K* over the
// order-preserving integer key of y: K* is the smallest key K whose weight
// strictly above (count for top-k, fixed-point softmax mass for top-p) is
// <= the budget (k - 1, or p * total mass).  It is found by a three-digit
// (12 + 10 + 10 bit) radix descent over integer LDS histograms, so the result
// does not depend on the order the atomics arrive in: same input, same
// token, bitwise.  The row (64-256 KiB) is read from L2 per pass: [the max,
// for top-p,] the first digit's histogram, then one pass that draws the
// elements of the bins above the threshold bin and collects that bin's (key,
// index) pairs in LDS; the two lower digits and the remaining draws run on
// that list (on the row again if more than ST_CAP elements share the bin).
// The noise is only computed for kept elements.
constexpr int ST_NT = 1024, ST_NB = 4096, ST_CAP = 2048;
typedef unsigned long long u64;

// monotone float -> uint32 map (-0 has been folded into +0 by the caller)
__device__ __forceinline__ uint32_t okey(float y) {
  const uint32_t b = __float_as_uint(y);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ float tempered(float x, float temp) {
  float y = x;
  if (temp != 1.f) y = x / temp;  // (uniform branch: the IEEE divide is ~10 instructions)
  return y == 0.f ? 0.f : y;
}

// natural log of a normal positive float on the hardware log2 (v_log_f32,
// 1 ulp): ~2 ulp relative, which is all the Gumbel key needs
__device__ __forceinline__ float fast_ln(float x) {
  return 0.693147180559945f * __builtin_amdgcn_logf(x);
}

// g = -log(-log(u)), u = (n + 0.5) * 2^-24, n = w >> 8.  n + 0.5 has 25
// significant bits from n = 2^23 on, so there t = -log(u) goes through the
// exact v = 1 - u = (2^24 - 1 - n + 0.5) * 2^-24: the series of -log(1 - v)
// below 2^-4 (next term v^6 / 6: < 2e-7 relative), else log(1 - v), where the
// rounding of 1 - v (2^-25) is < 1e-6 of t.  g is within ~2e-6 of its fp64 value.
__device__ __forceinline__ float gumbel(uint32_t w) {
  const uint32_t n = w >> 8;
  float t;
  if (n < (1u << 23)) {
    t = -fast_ln(((float)n + 0.5f) * 0x1p-24f);
  } else {
    const float v = ((float)(0xffffffu - n) + 0.5f) * 0x1p-24f;
    t = v < 0x1p-4f ? v * (1.f + v * (0.5f + v * (1.f / 3.f + v * (0.25f + v * 0.2f))))
                    : -fast_ln(1.f - v);
  }
  return -fast_ln(t);
}

template <typename T, typename F>
__device__ __forceinline__ void row_for_each(const T* __restrict__ lr, int V, int tid, F f) {
  typedef typename Vec16<T>::t vec;
  constexpr int NV = Vec16<T>::n, UR = 4;
  const int nvec = V / NV;
  for (int v0 = tid; v0 < nvec; v0 += UR * ST_NT) {
    vec x[UR];
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const int vi = v0 + u * ST_NT;
      x[u] = vi < nvec ? reinterpret_cast<const vec*>(lr)[vi] : vec{};
    }
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const int vi = v0 + u * ST_NT;
      if (vi < nvec) {
#pragma unroll
        for (int e = 0; e < NV; ++e) f(elem<T>(x[u], e), vi * NV + e);
      }
    }
  }
  for (int i = nvec * NV + tid; i < V; i += ST_NT) f((float)lr[i], i);
}

// The draw of one row (the filters and the Gumbel-max of the comment above, or
// the plain argmax at top_k == 1) over the 1024 threads of a workgroup, noise
// at Philox counter-high word chi_hi (the row, or 0 for noise that belongs to a
// request) and offset a.offset0 + step: the token is valid in thread 0, before
// the vocab_limit clamp (shared by sample_tail_k and the ragged tail).
// LP: the log-sum-exp of the raw row (before tempering and filtering, all V
// columns) into *lse, carried through the first sweep each path makes anyway:
// the argmax sweep (top_k == 1), the draw sweep (no filter), the max sweep
// (top-p) and the first digit's histogram pass (top-k).  No path reads the row
// one more time for it.
template <typename T, bool LP = false>
__device__ __forceinline__ int draw_row(const T* __restrict__ lr, int V, int chi_hi, int tid,
                                        const SampleArgs& a, int64_t step, Lse* lse = nullptr) {
  const int lane = tid & 63, wave = tid >> 6;
  __shared__ u64 hist[ST_NB];
  __shared__ u64 swt[ST_NT / 64];
  __shared__ u64 ssel[2];
  __shared__ uint32_t ckey[ST_CAP];
  __shared__ int cidx[ST_CAP];
  __shared__ unsigned ncand;
  __shared__ float sv[ST_NT / 64];
  __shared__ int si[ST_NT / 64];
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  Lse acc{LSE_LOW, 0.f};
  if (a.top_k == 1) {
    row_for_each<T>(lr, V, tid, [&](float x, int i) {
      take(bv, bi, x, i);
      if constexpr (LP) lse_add(acc, x);
    });
  } else {
    const float temp = a.temperature;
    const bool topk = a.top_k > 1, topp = !topk && a.top_p > 0.f;
    uint32_t kstar = 0;
    const uint64_t off = (uint64_t)(a.offset0 + step), seed = (uint64_t)a.seed;
    const uint64_t chi = (uint64_t)chi_hi << 32;
    auto draw = [&](float y, int i) {
      const U4 r = philox(chi | (uint32_t)(i >> 2), off, seed);
      const int q = i & 3;
      const uint32_t w = q == 0 ? r.x : q == 1 ? r.y : q == 2 ? r.z : r.w;
      take(bv, bi, y + gumbel(w), i);
    };
    if (!(topk || topp)) {
      row_for_each<T>(lr, V, tid, [&](float x, int i) {
        draw(tempered(x, temp), i);
        if constexpr (LP) lse_add(acc, x);
      });
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) hist[4 * tid + j] = 0;
      if (tid == 0) ncand = 0;
      float m = 0.f;
      if (topp) {
        float lm = -INFINITY;
        row_for_each<T>(lr, V, tid, [&](float x, int) {
          lm = fmaxf(lm, tempered(x, temp));
          if constexpr (LP) lse_add(acc, x);
        });
        m = block_max(lm, sv);
      }
      __syncthreads();
      u64 carry = 0, budget = topk ? (u64)(a.top_k - 1) : 0;
      unsigned nlist = 0;
      bool in_list = false;  // the threshold bin's elements are in ckey / cidx
      for (int p = 0; p < 3; ++p) {
        const int shift = p == 0 ? 20 : p == 1 ? 10 : 0;
        const int bits = p == 0 ? 12 : 10;
        const uint32_t prefix = kstar;
        auto add = [&](float y, uint32_t k) {
          if (p == 0 || (k >> (shift + bits)) == prefix) {
            u64 w = 1;
            // fixed-point softmax numerator, exp(y - max) * 2^40 <= 2^40:
            // V <= 2^22 of them sum below 2^63 (hardware exp2: the argument's
            // rounding is < 3e-6 relative at y - max = -30, where the mass is nil)
            if (topp) w = y == -INFINITY ? 0 : (u64)(__expf(y - m) * 0x1p40f);
            atomicAdd(&hist[(k >> shift) & ((1u << bits) - 1u)], w);
          }
        };
        if (in_list) {
          for (unsigned c = tid; c < nlist; c += ST_NT) add(unkey(ckey[c]), ckey[c]);
        } else {
          row_for_each<T>(lr, V, tid, [&](float x, int) {
            const float y = tempered(x, temp);
            add(y, okey(y));
            if constexpr (LP) {
              if (p == 0 && topk) lse_add(acc, x);  // (top-p carried it through the max sweep)
            }
          });
        }
        __syncthreads();
        u64 h[4], loc = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          h[j] = hist[4 * tid + j];
          hist[4 * tid + j] = 0;
          loc += h[j];
        }
        // inclusive suffix sum over the 1024 threads (integers: exact)
        u64 incl = loc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const u64 t = __shfl_down(incl, o, 64);
          if (lane + o < 64) incl += t;
        }
        if (lane == 0) swt[wave] = incl;
        __syncthreads();
        u64 after = 0, total = 0;
#pragma unroll
        for (int w = 0; w < ST_NT / 64; ++w) {
          const u64 v = swt[w];
          total += v;
          if (w > wave) after += v;
        }
        if (p == 0 && topp)
          budget = a.top_p >= 1.f ? total : (u64)((double)a.top_p * (double)total);
        // above[j]: weight strictly above bin 4 tid + j; the digit is the
        // smallest bin with above <= budget (exactly one bin qualifies)
        u64 above = carry + after + (incl - loc);
#pragma unroll
        for (int j = 3; j >= 0; --j) {
          const u64 below = above + h[j];  // weight above bin 4 tid + j - 1
          if (above <= budget && (below > budget || 4 * tid + j == 0)) {
            ssel[0] = (u64)(4 * tid + j);
            ssel[1] = above;
          }
          above = below;
        }
        __syncthreads();
        kstar = (kstar << bits) | (uint32_t)ssel[0];
        carry = ssel[1];
        if (p == 0) {
          // the first digit d of K* is known: every element of a bin above d
          // is kept and drawn now; bin d's (key, index) go to an LDS list,
          // from which the two lower digits and the last draws are taken
          // (the row is read again for them only if the list overflows)
          const uint32_t d = kstar;
          row_for_each<T>(lr, V, tid, [&](float x, int i) {
            const float y = tempered(x, temp);
            const uint32_t k = okey(y);
            if ((k >> 20) > d) {
              draw(y, i);
            } else if ((k >> 20) == d) {
              const unsigned c = atomicAdd(&ncand, 1u);
              if (c < ST_CAP) {
                ckey[c] = k;
                cidx[c] = i;
              }
            }
          });
          __syncthreads();
          nlist = ncand;
          in_list = nlist <= ST_CAP;
        }
      }
      if (in_list) {
        for (unsigned c = tid; c < nlist; c += ST_NT)
          if (ckey[c] >= kstar) draw(unkey(ckey[c]), cidx[c]);
      } else {
        row_for_each<T>(lr, V, tid, [&](float x, int i) {
          const float y = tempered(x, temp);
          const uint32_t k = okey(y);
          if ((k >> 20) == (kstar >> 20) && k >= kstar) draw(y, i);
        });
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    take(bv, bi, ov, oi);
  }
  __syncthreads();
  if (lane == 0) {
    sv[wave] = bv;
    si[wave] = bi;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < ST_NT / 64; ++w) take(bv, bi, sv[w], si[w]);
  }
  if constexpr (LP) {
    __shared__ float lm[ST_NT / 64], ls[ST_NT / 64];
    lse_block(acc, lm, ls, tid);
    *lse = acc;
  }
  return bi;
}

template <typename T>
__global__ __launch_bounds__(1024) void sample_tail_k(const T* __restrict__ logits, int64_t ld, int V,
                                                     int64_t* tokens, int64_t* history,
                                                     int64_t hist_ld, int64_t hist_cols,
                                                     int64_t* step_idx, int64_t* pos,
                                                     int64_t* slot, int* kv_len, unsigned* counter,
                                                     int64_t* ctl, const float* fctl,
                                                     SampleArgs a) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const T* lr = logits + (int64_t)row * ld;
  if (ctl) {
    a.seed = ctl[0];
    a.offset0 = ctl[1];
    a.top_k = ctl[2];
    a.vocab_limit = ctl[3];
    a.stop_id = ctl[4];
    a.temperature = fctl[0];
    a.top_p = fctl[1];
  }
  const bool tail = history != nullptr;
  const int64_t step = tail ? *step_idx : 0;
  const bool stopped = tail && a.stop_id >= 0 && tokens[row] == a.stop_id;
  int bi = 0;
  if (!stopped) bi = draw_row<T>(lr, V, row, tid, a, step);
  if (tid != 0) return;
  int64_t tok = a.stop_id;
  if (!stopped) {
    tok = bi;
    if (a.vocab_limit > 0 && tok >= a.vocab_limit) tok = a.vocab_limit - 1;
  }
  tokens[row] = tok;
  if (!tail) return;
  if (step >= 0 && step < hist_cols) history[(int64_t)row * hist_ld + step] = tok;
  pos[row] += 1;
  // arrival counter: low 16 bits count workgroups, the high bits the rows that
  // emitted stop_id (one atomic, nothing to order); the last one to arrive
  // advances the shared state and re-arms, as greedy_tail_k does
  const unsigned emitted = a.stop_id >= 0 && tok == a.stop_id ? 1u : 0u;
  const unsigned prev = __hip_atomic_fetch_add(counter, 1u + (emitted << 16), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
  if ((prev & 0xffffu) == gridDim.x - 1) {
    *step_idx = step + 1;
    *slot += 1;
    *kv_len += 1;
    ctl[5] = (int64_t)((prev >> 16) + emitted);
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------- ragged tails
// ragged_tail_k (inference/continuous.py): the tail of a decode step whose rows
// are independent sequences.  Every row has its own history index, cache slot,
// key count, position, limit and an `active` flag (RaggedTail); shared are the
// replay count *tick and ctl / fctl of the sampling tail.  SAMPLE: draw_row
// with the noise at Philox offset offset0 + *tick (a refilled row starts at
// history index 0 again and must not replay its predecessor's noise), else
// argmax_row.  A row with active == 0 reads no logits and writes nothing.  An
// active row stores its token (tokens, history[row, hist_idx]) and advances
// hist_idx; if the token is stop_id (stop_id >= 0) or hist_idx reached its
// limit the row parks itself: active = 0, and pos / slot / kv_len stay, so a
// parked row keeps rewriting a cache slot it owns (never the one at the
// capacity); otherwise the three advance by one (paged cache, RaggedTail::
// page_table: the slot becomes the pool row of the new position, table[row][pos
// / KV_PAGE] * KV_PAGE + pos % KV_PAGE, the entry clamped to the pool).  The
// arrival counter's high bits count the rows still active; the last workgroup
// advances *tick, writes that count to ctl[5] and re-arms the counter.
//
// Per-row form, X != 0 (RaggedRows; X = 0 compiles to the tail above, its
// branches are `if constexpr`):
//   RAGGED_ROWS  (SAMPLE only) every row takes seed, offset0, top_k and stop_id
//     from row_ctl[row] and temperature, top_p from row_fctl[row]; vocab_limit
//     stays ctl[3].  draw_row's branches are uniform over a workgroup, so a
//     greedy (top_k == 1: no noise, argmax_row's order), a top-k, a top-p and a
//     temperature-only row sit side by side in one launch.  The noise belongs
//     to the request, not to its place: Philox counter-high 0, offset offset0 +
//     hist_idx[row], key seed: the n-th token of a request is the draw of a
//     one-row lockstep call at (seed, offset0 + n) in whichever row and replay
//     it is made.  The row parks on its own stop_id.
//   RAGGED_LOGP  the log-probability of the emitted (clamped) token under the
//     raw logits row, x[tok] - max - log(sum exp(x - max)) in fp32 over all V
//     columns, to logprob[row] and hist_logprob[row, hist_idx] (either may be
//     nullptr).  The (max, sum) pair rides the first sweep of the selection
//     (argmax_row / draw_row, LP): no path needed an extra sweep of the row;
//     thread 0 reads x[tok] again, one element.  An inactive row writes nothing.
constexpr int RAGGED_ROWS = 1, RAGGED_LOGP = 2;

template <typename T, bool SAMPLE, int X>
__global__ __launch_bounds__(1024) void ragged_tail_k(const T* __restrict__ logits, int64_t ld, int V,
                                                     int64_t* tokens, int64_t* history,
                                                     int64_t hist_ld, int64_t hist_cols,
                                                     RaggedTail st, unsigned* counter, int64_t* ctl,
                                                     const float* fctl, RaggedRows rr) {
  constexpr bool ROWS = (X & RAGGED_ROWS) != 0, LP = (X & RAGGED_LOGP) != 0;
  static_assert(SAMPLE || !ROWS, "per-row settings belong to the sampling tail");
  const int row = blockIdx.x, tid = threadIdx.x;
  const bool act = st.active[row] != 0;
  int64_t stop_id;
  if constexpr (ROWS) stop_id = rr.row_ctl[4 * row + 3];
  else stop_id = ctl[4];
  int bi = 0;
  Lse lse{0.f, 1.f};
  if (act) {
    const T* lr = logits + (int64_t)row * ld;
    if constexpr (ROWS) {
      // hist_idx[row]: thread 0 alone stores it, behind draw_row's barriers
      const int64_t* rc = rr.row_ctl + 4 * row;
      const SampleArgs a{rc[0], rc[1], rc[2], ctl[3], stop_id, rr.row_fctl[2 * row], rr.row_fctl[2 * row + 1]};
      bi = draw_row<T, LP>(lr, V, 0, tid, a, st.hist_idx[row], &lse);
    } else if constexpr (SAMPLE) {
      const SampleArgs a{ctl[0], ctl[1], ctl[2], ctl[3], stop_id, fctl[0], fctl[1]};
      if constexpr (LP) bi = draw_row<T, true>(lr, V, row, tid, a, *st.tick, &lse);
      else bi = draw_row<T>(lr, V, row, tid, a, *st.tick);
    } else {
      if constexpr (LP) bi = argmax_row<T, true>(lr, V, tid, &lse);
      else bi = argmax_row<T>(lr, V, tid);
    }
  }
  if (tid != 0) return;
  unsigned still = 0u;
  if (act) {
    int64_t tok = bi;
    if (SAMPLE && ctl[3] > 0 && tok >= ctl[3]) tok = ctl[3] - 1;
    const int64_t hi = st.hist_idx[row];
    tokens[row] = tok;
    if (hi >= 0 && hi < hist_cols) history[(int64_t)row * hist_ld + hi] = tok;
    if constexpr (LP) {
      // (a row of NaNs selects no index: nothing of the row is read then)
      const float xt = tok >= 0 && tok < V ? (float)logits[(int64_t)row * ld + tok] : NAN;
      const float lp = (xt - lse.m) - logf(lse.s);
      if (rr.logprob) rr.logprob[row] = lp;
      if (rr.hist_logprob && hi >= 0 && hi < hist_cols) rr.hist_logprob[(int64_t)row * rr.lp_ld + hi] = lp;
    }
    st.hist_idx[row] = hi + 1;
    if ((stop_id >= 0 && tok == stop_id) || hi + 1 >= st.limit[row]) {
      st.active[row] = 0;
    } else {
      const int64_t np = st.pos[row] + 1;
      st.pos[row] = np;
      if (st.page_table) {
        const int64_t pi = min(max(np / KV_PAGE, (int64_t)0), (int64_t)st.pt_ld - 1);
        const int pg = st.page_table[(int64_t)row * st.pt_ld + pi];
        st.slot[row] = (int64_t)min(max(pg, 0), st.n_pages - 1) * KV_PAGE + (np & (KV_PAGE - 1));
      } else {
        st.slot[row] += 1;
      }
      st.kv_len[row] += 1;
      still = 1u;
    }
  }
  // every workgroup has read *tick (its draw used it) before it arrives
  const unsigned prev = __hip_atomic_fetch_add(counter, 1u + (still << 16), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
  if ((prev & 0xffffu) == gridDim.x - 1) {
    *st.tick += 1;
    ctl[5] = (int64_t)((prev >> 16) + still);
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------- speculative tail
// spec_tail_k (inference/speculative.py): the tail of one speculative greedy
// step of b sequences with S rows each (S in 2..16, D = S - 1 drafts).  Row 0
// of a sequence carries its last committed token, rows 1..D the drafts; the
// forward ran all S through the multi-row device step, so logits row r * S + t
// is the model's answer after draft t.  State per sequence r (SpecTail), with p
// = hist_len[r] - 1: tokens[r, :], pos[r, t] = p + t, slot[r] = p, kv_len[r] =
// p + S, history[r, :hist_len[r]] = the whole context by position.
//
// Grid: b * S workgroups of 1024 threads, those of a sequence adjacent.
// Workgroup (r, t) takes argmax_row of its logits row, stores it in am[r, t]
// (write-through, agent scope, drained before the arrival is counted: the
// protocol of decode_attn_k's combine) and arrives at counters[r].  Nobody
// waits: the last of the S to arrive acquires am[r, :] and does the
// sequence's bookkeeping with all its threads (the flag goes through LDS):
//   accept n   = leading t in 0..D-1 with tokens[r, t + 1] == a[t];
//   commit     a[0..n], cut to max(limit - hist_len, 1) tokens and after the
//              first stop_id: c >= 1 tokens appended to history, hist_len += c,
//              accepted += c - 1;
//   park       if it ended on stop_id or hist_len reached limit: active = 0,
//              tokens / pos / slot / kv_len stay (the row rewrites its S slots);
//   else       pos / slot / kv_len follow the new p, tokens[r, 0] = the last
//              committed token and tokens[r, 1..D] = the n-gram draft.
// Draft: for g = ngram (ctl[1], 0..4) down to 1, the largest start j <
// hist_len - g with history[j .. j + g) == the last g tokens; the first g with
// a match wins and draft k = history[j + g + k] where that is < hist_len, else
// the last committed token (as every draft without a match).  One pass serves
// every g: a candidate is its end e = j + g in [1, hist_len), m(e) = how many
// tokens before e agree with the tokens before hist_len (up to 4), and g's
// winner is the largest e with m(e) >= g: four max-reductions, side by side.
// An inactive sequence reads no logits and writes nothing.  Every workgroup
// then arrives at counters[b], the finisher of a sequence that goes on with
// 1 << 16 on top; the last one advances *tick, writes the number of sequences
// still active to ctl[2] and re-arms (each sequence's finisher re-armed its own).
//
// spec_sample_tail_k (SAMPLE, SpeculativeSamplingDecoder) is the same tail for
// sampled requests: a[t] is draw_row of row t (sample_tail_k's draw: tempered,
// the radix-descent top-k / top-p threshold, Gumbel-max; the plain argmax at
// top_k == 1), clamped to vocab_limit before it is compared or committed.  A
// draft is accepted iff it IS the token drawn from the row before it: with a
// deterministic draft that is exact speculative sampling (it is accepted with
// probability p(draft), and otherwise the committed token is distributed as p),
// so no softmax denominator and no second draw.  The noise of row t belongs to
// the token it would commit, generated token n = hist_len[r] + t - gen0[r] of
// sequence r: Philox counter row r, offset offset0 + n, the pair
// GraphedSamplingDecoder uses for that token.  Identical logits rows hence give
// the lockstep sampler's sequence token for token, whatever S or ngram is; the
// row behind a rejected draft draws at the same index again in the next step.
// Settings from the device: ctl int64 [7] = [stop_id, ngram, still active
// (written), seed, offset0, top_k, vocab_limit], fctl = [temperature, top_p].
constexpr int SPEC_MAX_G = 4;

template <typename T, bool SAMPLE>
__device__ __forceinline__ void spec_tail_body(const T* __restrict__ logits, int64_t ld, int V, int S,
                                               const SpecTail& st) {
  const int r = blockIdx.x / S, t = blockIdx.x % S, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  __shared__ int last_sh, hl_sh, a_sh[16], best_sh[1024 / 64][SPEC_MAX_G];
  __shared__ int64_t tok_sh[16], suf_sh[SPEC_MAX_G];
  unsigned still = 0u;
  bool finisher = false;
  if (st.active[r] != 0) {  // (the finisher alone writes it, after all S have read it)
    const T* lr = logits + ((int64_t)r * S + t) * ld;
    int bi;
    if constexpr (SAMPLE) {
      // hist_len[r], as active[r]: written by the finisher alone, after every
      // row's arrival, and the arrival follows the store of the token drawn here
      const SampleArgs a{st.ctl[3], st.ctl[4], st.ctl[5], st.ctl[6], st.ctl[0], st.fctl[0], st.fctl[1]};
      bi = draw_row<T>(lr, V, r, tid, a, st.hist_len[r] + t - st.gen0[r]);
      if (a.vocab_limit > 0 && bi >= a.vocab_limit) bi = (int)a.vocab_limit - 1;
    } else {
      bi = argmax_row<T>(lr, V, tid);
    }
    if (tid == 0) {
      __hip_atomic_store(st.am + r * S + t, bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned prev = __hip_atomic_fetch_add(st.counters + r, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = prev == (unsigned)S - 1u;
      if (last) {
        __hip_atomic_store(st.counters + r, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      last_sh = last;
    }
    __syncthreads();
    finisher = last_sh != 0;
  }
  if (finisher) {
    const int D = S - 1;
    int64_t* hist = st.history + (int64_t)r * st.hist_ld;
    if (tid < S) {
      a_sh[tid] = __hip_atomic_load(st.am + r * S + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      tok_sh[tid] = st.tokens[r * S + tid];
      // read before the barrier: thread 0 stores the new hist_len behind it
      if (tid == 0) hl_sh = (int)st.hist_len[r];
    }
    __syncthreads();
    const int64_t stop_id = st.ctl[0];
    const int G = (int)min(max(st.ctl[1], (int64_t)0), (int64_t)SPEC_MAX_G);
    const int hl = hl_sh;
    int n = 0;
    while (n < D && tok_sh[n + 1] == (int64_t)a_sh[n]) ++n;
    int c = min(n + 1, max((int)(st.limit[r] - hl), 1));
    bool stopped = false;
    if (stop_id >= 0) {
      for (int i = 0; i < c; ++i) {
        if ((int64_t)a_sh[i] == stop_id) {
          c = i + 1;
          stopped = true;
          break;
        }
      }
    }
    const int nl = hl + c;  // the new hist_len
    if (tid < c && hl + tid >= 0 && hl + tid < st.hist_cols) hist[hl + tid] = a_sh[tid];
    // the context by position, the tokens just committed included (from LDS:
    // no thread reads what another one has just stored)
    auto h = [&](int i) -> int64_t {
      return i >= hl ? (int64_t)a_sh[i - hl] : i < st.hist_cols ? hist[i] : (int64_t)-1;
    };
    const bool go = !stopped && nl < st.limit[r];
    if (tid == 0) {
      st.hist_len[r] = nl;
      st.accepted[r] += c - 1;
      if (!go) st.active[r] = 0;
    }
    if (go) {
      still = 1u;
      if (tid < SPEC_MAX_G) suf_sh[tid] = nl - 1 - tid >= 0 ? h(nl - 1 - tid) : (int64_t)-1;
      __syncthreads();
      int best[SPEC_MAX_G];
#pragma unroll
      for (int g = 0; g < SPEC_MAX_G; ++g) best[g] = -1;
      if (G > 0) {
        for (int e = 1 + tid; e < nl; e += 1024) {  // ascending: a later match replaces an earlier
          int m = 0;
          while (m < G && m < e && h(e - 1 - m) == suf_sh[m]) ++m;
#pragma unroll
          for (int g = 0; g < SPEC_MAX_G; ++g)
            if (m > g) best[g] = e;
        }
      }
#pragma unroll
      for (int g = 0; g < SPEC_MAX_G; ++g) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best[g] = max(best[g], __shfl_xor(best[g], o, 64));
        if (lane == 0) best_sh[wave][g] = best[g];
      }
      __syncthreads();
      if (tid < S) {
        int e = -1;  // one past the winning match
        for (int g = G - 1; g >= 0 && e < 0; --g)
          for (int w = 0; w < 1024 / 64; ++w) e = max(e, best_sh[w][g]);
        const int64_t last_tok = a_sh[c - 1];
        int64_t tok = last_tok;
        if (tid > 0 && e >= 0 && e + tid - 1 < nl) tok = h(e + tid - 1);
        st.tokens[r * S + tid] = tok;
        st.pos[r * S + tid] = nl - 1 + tid;
        if (tid == 0) {
          st.slot[r] = nl - 1;
          st.kv_len[r] = nl - 1 + S;
        }
      }
    }
  }
  if (tid != 0) return;
  const unsigned prev = __hip_atomic_fetch_add(st.counters + st.b, 1u + (still << 16), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
  if ((prev & 0xffffu) == gridDim.x - 1) {
    *st.tick += 1;
    st.ctl[2] = (int64_t)((prev >> 16) + still);
    __hip_atomic_store(st.counters + st.b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <typename T>
__global__ __launch_bounds__(1024) void spec_tail_k(const T* __restrict__ logits, int64_t ld, int V,
                                                   int S, SpecTail st) {
  spec_tail_body<T, false>(logits, ld, V, S, st);
}

template <typename T>
__global__ __launch_bounds__(1024) void spec_sample_tail_k(const T* __restrict__ logits, int64_t ld,
                                                          int V, int S, SpecTail st) {
  spec_tail_body<T, true>(logits, ld, V, S, st);
}

}  // namespace

void spec_tail(const void* logits, int64_t ld, int V, int S, int dt, const SpecTail& st, hipStream_t s) {
  EMA_DISPATCH_FLOAT(dt, T, {
    if (st.fctl)
      hipLaunchKernelGGL((spec_sample_tail_k<T>), dim3((unsigned)(st.b * S)), dim3(1024), 0, s,
                         (const T*)logits, ld, V, S, st);
    else
      hipLaunchKernelGGL((spec_tail_k<T>), dim3((unsigned)(st.b * S)), dim3(1024), 0, s, (const T*)logits,
                         ld, V, S, st);
  });
}

void ragged_tail(const void* logits, int64_t ld, int V, int b, int dt, bool sample, int64_t* tokens,
                 int64_t* history, int64_t hist_ld, int64_t hist_cols, const RaggedTail& st,
                 unsigned* counter, int64_t* ctl, const float* fctl, const RaggedRows& rr,
                 hipStream_t s) {
  // (row_ctl comes with row_fctl and sample == true: checked by the binding)
  const bool rows = rr.row_ctl != nullptr, lp = rr.logprob != nullptr || rr.hist_logprob != nullptr;
#define EMA_RAGGED_TAIL(SAMPLE, X)                                                                 \
  hipLaunchKernelGGL((ragged_tail_k<T, SAMPLE, X>), dim3((unsigned)b), dim3(1024), 0, s,           \
                     (const T*)logits, ld, V, tokens, history, hist_ld, hist_cols, st, counter, ctl, \
                     fctl, rr)
  EMA_DISPATCH_FLOAT(dt, T, {
    if (rows && lp) EMA_RAGGED_TAIL(true, RAGGED_ROWS | RAGGED_LOGP);
    else if (rows) EMA_RAGGED_TAIL(true, RAGGED_ROWS);
    else if (sample && lp) EMA_RAGGED_TAIL(true, RAGGED_LOGP);
    else if (sample) EMA_RAGGED_TAIL(true, 0);
    else if (lp) EMA_RAGGED_TAIL(false, RAGGED_LOGP);
    else EMA_RAGGED_TAIL(false, 0);
  });
#undef EMA_RAGGED_TAIL
}

void greedy_tail(const void* logits, int64_t ld, int V, int b, int dt, int64_t* tokens,
                 int64_t* history, int64_t hist_ld, int64_t* step_idx, int64_t* pos, int64_t* slot,
                 int* kv_len, unsigned* counter, hipStream_t s) {
  EMA_DISPATCH_FLOAT(dt, T, {
    hipLaunchKernelGGL((greedy_tail_k<T>), dim3((unsigned)b), dim3(1024), 0, s, (const T*)logits, ld,
                       V, tokens, history, hist_ld, step_idx, pos, slot, kv_len, counter);
  });
}

void sample_tail(const void* logits, int64_t ld, int V, int b, int dt, int64_t* tokens,
                 int64_t* history, int64_t hist_ld, int64_t hist_cols, int64_t* step_idx,
                 int64_t* pos, int64_t* slot, int* kv_len, unsigned* counter, int64_t* ctl,
                 const float* fctl, SampleArgs a, hipStream_t s) {
  EMA_DISPATCH_FLOAT(dt, T, {
    hipLaunchKernelGGL((sample_tail_k<T>), dim3((unsigned)b), dim3(1024), 0, s, (const T*)logits, ld,
                       V, tokens, history, hist_ld, hist_cols, step_idx, pos, slot, kv_len, counter,
                       ctl, fctl, a);
  });
}

}  // namespace ema
