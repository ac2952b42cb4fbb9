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
// shared; only thread 0's bookkeeping differs.
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

// argmax of one row over the 1024 threads of a workgroup: the result is valid
// in thread 0 (shared by greedy_tail_k and the ragged tail)
template <typename T>
__device__ __forceinline__ int argmax_row(const T* __restrict__ lr, int V, int tid) {
  typedef typename Vec16<T>::t vec;
  constexpr int NV = Vec16<T>::n;
  const int lane = tid & 63, wave = tid >> 6;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
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
        for (int e = 0; e < NV; ++e) take(bv, bi, elem<T>(x[u], e), vi * NV + e);
      }
    }
  }
  for (int i = nvec * NV + tid; i < V; i += NT) take(bv, bi, (float)lr[i], i);
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
// at Philox offset a.offset0 + step: the token is valid in thread 0, before the
// vocab_limit clamp (shared by sample_tail_k and the ragged tail)
template <typename T>
__device__ __forceinline__ int draw_row(const T* __restrict__ lr, int V, int row, int tid,
                                        const SampleArgs& a, int64_t step) {
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
  if (a.top_k == 1) {
    row_for_each<T>(lr, V, tid, [&](float x, int i) { take(bv, bi, x, i); });
  } else {
    const float temp = a.temperature;
    const bool topk = a.top_k > 1, topp = !topk && a.top_p > 0.f;
    uint32_t kstar = 0;
    const uint64_t off = (uint64_t)(a.offset0 + step), seed = (uint64_t)a.seed;
    const uint64_t chi = (uint64_t)row << 32;
    auto draw = [&](float y, int i) {
      const U4 r = philox(chi | (uint32_t)(i >> 2), off, seed);
      const int q = i & 3;
      const uint32_t w = q == 0 ? r.x : q == 1 ? r.y : q == 2 ? r.z : r.w;
      take(bv, bi, y + gumbel(w), i);
    };
    if (!(topk || topp)) {
      row_for_each<T>(lr, V, tid, [&](float x, int i) { draw(tempered(x, temp), i); });
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) hist[4 * tid + j] = 0;
      if (tid == 0) ncand = 0;
      float m = 0.f;
      if (topp) {
        float lm = -INFINITY;
        row_for_each<T>(lr, V, tid, [&](float x, int) { lm = fmaxf(lm, tempered(x, temp)); });
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
template <typename T, bool SAMPLE>
__global__ __launch_bounds__(1024) void ragged_tail_k(const T* __restrict__ logits, int64_t ld, int V,
                                                     int64_t* tokens, int64_t* history,
                                                     int64_t hist_ld, int64_t hist_cols,
                                                     RaggedTail st, unsigned* counter, int64_t* ctl,
                                                     const float* fctl) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const bool act = st.active[row] != 0;
  const int64_t stop_id = ctl[4];
  int bi = 0;
  if (act) {
    const T* lr = logits + (int64_t)row * ld;
    if constexpr (SAMPLE) {
      const SampleArgs a{ctl[0], ctl[1], ctl[2], ctl[3], stop_id, fctl[0], fctl[1]};
      bi = draw_row<T>(lr, V, row, tid, a, *st.tick);
    } else {
      bi = argmax_row<T>(lr, V, tid);
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

}  // namespace

void ragged_tail(const void* logits, int64_t ld, int V, int b, int dt, bool sample, int64_t* tokens,
                 int64_t* history, int64_t hist_ld, int64_t hist_cols, const RaggedTail& st,
                 unsigned* counter, int64_t* ctl, const float* fctl, hipStream_t s) {
  EMA_DISPATCH_FLOAT(dt, T, {
    if (sample)
      hipLaunchKernelGGL((ragged_tail_k<T, true>), dim3((unsigned)b), dim3(1024), 0, s, (const T*)logits,
                         ld, V, tokens, history, hist_ld, hist_cols, st, counter, ctl, fctl);
    else
      hipLaunchKernelGGL((ragged_tail_k<T, false>), dim3((unsigned)b), dim3(1024), 0, s, (const T*)logits,
                         ld, V, tokens, history, hist_ld, hist_cols, st, counter, ctl, fctl);
  });
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
