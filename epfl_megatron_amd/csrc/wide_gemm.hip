// Weight-streaming GEMM for decode batches of 33-64 rows on gfx950:
//
//     Y[M, N] = epi(X[M, K] · W[N, K]^T)        33 <= M <= 64, bf16/fp16, fp32 accumulate
//
// A decode step at 64 rows is still far below the machine's flop / byte
// balance: its time is the weight stream, the problem skinny_gemm.hip solves
// for <= 32 rows.  That kernel keeps every X fragment of its K slice in
// registers beside the weight ring, which three or four row blocks cannot
// afford (~256 VGPRs for X alone).  Here the two operands take different
// paths: W through the register ring, X through LDS.
//
// W comes from the decode-packed copies the skinny kernel reads (16-bit
// ops/decode_pack.py, e4m3 ops/fp8_weights.py, MXFP4 ops/mxfp4_weights.py, all
// with half_tail = 0; K % 256 == 0, N % 16 == 0).  For one 16-feature block the
// eight per-wave sub-streams of that layout lie back to back in ascending k,
// so a wave can walk any 8 / KS consecutive ones as a single run of bytes.
//
// Work split.  A workgroup is 8 waves = FB feature blocks x KS K-slices
// (FB KS = 8).  Wave (f, s) = (wave / KS, wave % KS) owns block FB wg + f and
// the packed sub-streams [s FB, (s + 1) FB): k in [s K / KS, (s + 1) K / KS),
// FB S k-steps of 32 (S = K / 256).  The host picks FB so that the grid covers
// the chip (wide_gemm_split).  A ragged last workgroup's surplus waves stream
// the last block again, take part in the X staging and every barrier, and
// write nothing.
//
// W path.  A ring of U k-steps of 16-B non-temporal loads per wave, filled at
// kernel entry and refilled slot by slot behind the MFMAs that consume it.
// A slot is one piece: one k-step (16-bit), two (e4m3) or four with their
// scale dword (MXFP4); a sub-stream's odd / leftover steps are the 8-B / 4-B
// pieces of those layouts.  A piece is expanded to an A fragment right before
// its MFMAs (fp8x8 / fp4x8 of skinny_epi.h).  The ring's main loop refills
// unconditionally, so that hipcc counts vmcnt down to the slot it needs and
// not to zero; the last < 2 U steps run a guarded copy.
//
// X path.  All waves advance one chunk of FB k-steps together; the chunk's X
// is KS slabs x FB k-steps of [64 rows x 32 k] = 32 KiB whatever the split.
// The whole workgroup stages it: four 16-B loads per thread (rows >= M read
// row 0 and are zeroed), held in registers for one chunk, written to a
// three-stage LDS ring one chunk before its use; one barrier per chunk.  In a
// slab, row m's 16-B piece q sits at 64 m + 16 (q ^ ((m >> 2) & 3)): the
// B-fragment ds_read_b128 (lane L: row L & 15, 8 k at 8 (L >> 4)) touches every
// bank once per 16 lanes.
//
// Inner step.  One A fragment, MB = ceil(M / 16) B fragments from LDS, MB
// v_mfma_f32_16x16x32 into MB accumulators.  MB is a template argument: the
// accumulators and B fragments need static register names, and a uniform loop
// bound puts a scalar branch between the MFMAs of every k-step.
//
// Reduction and epilogue.  With KS > 1 the slices' partial tiles meet in LDS
// (the dead X ring) and the slice-0 wave adds them in slice order:
// deterministic.  That wave runs skinny_epi.h's epilogue per row block:
// plain, residual, erf GeLU, the four GLU kinds, QKV with RoPE and the KV-cache write
// (16-bit or e4m3 cache, host / device / per-row slot); e4m3 row scales are
// applied before the first rounding; its operands are fetched before the
// k-loop.  No RMSNorm prologue: at these row counts the norm is its own kernel.
//
// A wave accumulates its k-steps in ascending order in every weight format, so
// for one (FB, KS) the e4m3 and MXFP4 forms equal the 16-bit form on the
// dequantised weights bit for bit.
#include <cstdlib>
#include <type_traits>

#include "skinny_epi.h"

namespace ema {
namespace {

constexpr int WIDE_STAGES = 3;
constexpr int WIDE_SLAB_B = 64 * 32 * 2;       // [64 rows x 32 k] of 16-bit X
constexpr int WIDE_STAGE_B = 8 * WIDE_SLAB_B;  // one chunk: KS slices x FB k-steps

// FMT: 0 16-bit, 1 e4m3 (p.w_scale), 2 MXFP4 (p.w_mx); fbl = log2 FB
template <typename T, int EPI, int ACT, int MB, int FMT>
__global__ __launch_bounds__(512) void wide_gemm_k(const SkinnyArgs p, const int fbl) {
  typedef typename fa::MT<T>::x8 x8;
  constexpr bool W8 = FMT == 1, W4 = FMT == 2;
  typedef std::conditional_t<W4, W4Slot, std::conditional_t<W8, i4, x8>> wslot;
  constexpr int SPU = W4 ? 4 : W8 ? 2 : 1;        // k-steps per ring slot
  constexpr int SB = W4 ? 256 : W8 ? 512 : 1024;  // stream bytes per k-step
  // 16 KiB of weight loads in flight per wave (MXFP4: 8 KiB), 128 / 64 KiB per CU
  constexpr int U = FMT == 0 ? 16 : 32, US = U / SPU;
  __shared__ __attribute__((aligned(16))) unsigned char xsh[WIDE_STAGES * WIDE_STAGE_B];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int FB = 1 << fbl, KS = 8 >> fbl;
  const int f = wave >> (3 - fbl), s = wave & (KS - 1);
  const int M = p.M, K = p.K, S = K >> 8;
  const int nblocks = EPI == EPI_GLU ? p.N / 8 : p.N / 16;
  const bool live = FB * (int)blockIdx.x + f < nblocks;
  const int blk = live ? FB * (int)blockIdx.x + f : nblocks - 1;
  const int r = lane & 15, q = lane >> 4;
  const int NT = FB * S;  // k-steps of this wave; chunks of the workgroup: S
  const T* __restrict__ x = (const T*)p.x;

  // ---- W ring: the wave's FB sub-streams are one run; k-step t at wb + SB t
  const unsigned char* wb = (const unsigned char*)p.w + ((int64_t)blk * 8 + s * FB) * S * SB;
  const unsigned char* sb = W4 ? p.w_mx + ((int64_t)blk * 8 + s * FB) * S * 16 : nullptr;
  // the piece that starts at k-step t, `left` steps before its sub-stream's end
  auto fetch = [&](int t, int left) -> wslot {
    if constexpr (W4) {
      if (left >= 4)
        return W4Slot{__builtin_nontemporal_load(reinterpret_cast<const i4*>(wb + 256 * t + 16 * lane)),
                      __builtin_nontemporal_load(reinterpret_cast<const int*>(sb + 16 * t + 4 * r))};
      W4Slot v{i4{0, 0, 0, 0}, 0};  // 1-3 leftover steps: 4-B pieces, one scale byte each
#pragma unroll
      for (int h = 0; h < 3; ++h) {
        if (h < left) {
          v.v[h] = __builtin_nontemporal_load(reinterpret_cast<const int*>(wb + 256 * (t + h) + 4 * lane));
          v.sc |= (int)__builtin_nontemporal_load(sb + 16 * (t + h) + r) << (8 * h);
        }
      }
      return v;
    } else if constexpr (W8) {
      if (left >= 2)
        return __builtin_nontemporal_load(reinterpret_cast<const i4*>(wb + 512 * t + 16 * lane));
      const i2 v = __builtin_nontemporal_load(reinterpret_cast<const i2*>(wb + 512 * t + 8 * lane));
      return i4{v[0], v[1], 0, 0};  // the odd last step: an 8-B piece
    } else {
      return __builtin_nontemporal_load(reinterpret_cast<const x8*>(wb + 1024 * t + 16 * lane));
    }
  };
  auto afrag = [&](const wslot& v, int h) -> x8 {  // A fragment of the slot's k-step h
    if constexpr (W4) return fp4x8<T>(v.v[h], v.sc, h);
    else if constexpr (W8) return fp8x8<T>(v[2 * h], v[2 * h + 1]);
    else return v;
  };
  int ft = 0, fs = 0;  // next piece to fetch: its k-step in the run / in its sub-stream
  auto fetch_next = [&](wslot& dst) {
    const int left = S - fs, adv = left < SPU ? left : SPU;
    dst = fetch(ft, left);
    ft += adv;
    fs = fs + adv == S ? 0 : fs + adv;
  };
  wslot a[US];
#pragma unroll
  for (int u = 0; u < US; ++u) {
    a[u] = wslot{};
    if (ft < NT) fetch_next(a[u]);
  }

  // ---- epilogue operands of the slice-0 wave, in flight behind the ring
  EpiPre<T, EPI> pre[MB];
  const bool owner = live && s == 0;
  if (owner) {
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      epi_init<T, EPI>(p, lane, pre[mb], 16 * mb);
      epi_prefetch<T, EPI>(p, blk, lane, pre[mb], 16 * mb);
    }
    if constexpr (W8) pre[0].sc = epi_scale<EPI>(p, blk, -1, lane);
  }

  // ---- X staging: piece j of thread tid is 16-B piece tid + 512 j of the
  // chunk: slab (tid + 512 j) / 256 = (slice, k-step in chunk), then row, q
  int xoff[4], xw[4];
  bool xok[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int pid = (int)threadIdx.x + 512 * j, slab = pid >> 8, row = (pid & 255) >> 2, xq = pid & 3;
    xok[j] = row < M;
    xoff[j] = (xok[j] ? row : 0) * K + (slab >> fbl) * (K >> (3 - fbl)) + (slab & (FB - 1)) * 32 + 8 * xq;
    xw[j] = slab * WIDE_SLAB_B + row * 64 + ((xq ^ ((row >> 2) & 3)) << 4);
  }
  x8 xs[4];
  auto xload = [&](int c) {  // chunk c: k-steps c FB .. of every slice
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const x8 v = *reinterpret_cast<const x8*>(x + xoff[j] + c * FB * 32);
      xs[j] = xok[j] ? v : x8{};
    }
  };
  auto xstore = [&](int stage) {
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<x8*>(xsh + stage * WIDE_STAGE_B + xw[j]) = xs[j];
  };
  xload(0);
  xstore(0);
  if (S > 1) xload(1);
  // chunk c is read from stage c % 3.  At its head the registers hold chunk
  // c + 1 (loaded one chunk ago): it goes to stage (c + 1) % 3, last read in
  // chunk c - 2, which every wave left before the previous barrier; the loads
  // of chunk c + 2 follow, and the barrier publishes chunk c + 1 a chunk early.
  int st = 0;
  auto boundary = [&](int c) {
    if (c > 0) st = st == 2 ? 0 : st + 1;
    if (c + 1 < S) xstore(st == 2 ? 0 : st + 1);
    if (c + 2 < S) xload(c + 2);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };

  f4 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = f4{0.f, 0.f, 0.f, 0.f};
  const int rd = r * 64 + ((q ^ ((r >> 2) & 3)) << 4);  // B fragment inside a slab
  int t = 0, cs = 0;  // k-step of the wave / inside its sub-stream
  auto step = [&](const x8& af) {
    const int i = t & (FB - 1);
    if (i == 0) boundary(t >> fbl);
    const unsigned char* xb = xsh + st * WIDE_STAGE_B + ((s << fbl) + i) * WIDE_SLAB_B + rd;
    x8 b[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) b[mb] = *reinterpret_cast<const x8*>(xb + 1024 * mb);
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[mb] = mfma16x16x32<T>(af, b[mb], acc[mb]);
    ++t;
  };
  auto consume = [&](const wslot& v) {
    const int left = S - cs, adv = left < SPU ? left : SPU;
#pragma unroll
    for (int h = 0; h < SPU; ++h) {
      if (SPU == 1 || h < left) step(afrag(v, h));
    }
    cs = cs + adv == S ? 0 : cs + adv;
  };
  const int NP = FB * ((S + SPU - 1) / SPU);  // pieces of this wave
  int i0 = 0;
  for (; i0 + 2 * US <= NP; i0 += US) {
#pragma unroll
    for (int u = 0; u < US; ++u) {
      consume(a[u]);
      fetch_next(a[u]);
      // {MFMAs of slot u, refill u} in program order (as in skinny_gemm_k)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  for (; i0 < NP; i0 += US) {
#pragma unroll
    for (int u = 0; u < US; ++u) {
      if (i0 + u < NP) {
        consume(a[u]);
        if (ft < NT) fetch_next(a[u]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- reduction over the K slices (slice order) and epilogue
  if (KS > 1) {
    f4* part = reinterpret_cast<f4*>(xsh);  // [wave][MB][64]; the X ring is dead
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) part[(wave * MB + mb) * 64 + lane] = acc[mb];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (!owner) return;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      for (int i = 1; i < KS; ++i) acc[mb] += part[((wave + i) * MB + mb) * 64 + lane];
    }
  }
  if (!owner) return;
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    f4 tile = acc[mb];
    if constexpr (W8) tile = scale_tile(tile, pre[0].sc);
    epilogue<T, EPI, ACT>(p, blk, tile, lane, -1, pre[mb], true, 16 * mb);
  }
}

int wide_cus() {
  static const int n = [] {
    int dev = 0, c = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      c = 256;
    return c;
  }();
  return n;
}

template <typename T, int EPI, int ACT>
void launch(const SkinnyArgs& p, int fbl, hipStream_t s) {
  const int nblocks = EPI == EPI_GLU ? p.N / 8 : p.N / 16, FB = 1 << fbl;
  const dim3 grid((unsigned)((nblocks + FB - 1) / FB)), wg(512);
#define EMA_WIDE(MB_, FMT_) \
  hipLaunchKernelGGL((wide_gemm_k<T, EPI, ACT, MB_, FMT_>), grid, wg, 0, s, p, fbl)
  // 33-48 rows do not pay for a fourth row block
  if (p.M > 48) {
    if (p.w_mx) EMA_WIDE(4, 2);
    else if (p.w_scale) EMA_WIDE(4, 1);
    else EMA_WIDE(4, 0);
  } else {
    if (p.w_mx) EMA_WIDE(3, 2);
    else if (p.w_scale) EMA_WIDE(3, 1);
    else EMA_WIDE(3, 0);
  }
#undef EMA_WIDE
}

template <typename T>
void dispatch(const SkinnyArgs& p, int epi, int fbl, hipStream_t s) {
  switch (epi) {
    case EPI_RES: launch<T, EPI_RES, 0>(p, fbl, s); break;
    case EPI_QKV: launch<T, EPI_QKV, 0>(p, fbl, s); break;
    case EPI_ACT: launch<T, EPI_ACT, 0>(p, fbl, s); break;
    case EPI_GLU:
      switch (p.act) {
        case 0: launch<T, EPI_GLU, 0>(p, fbl, s); break;
        case 1: launch<T, EPI_GLU, 1>(p, fbl, s); break;
        case 2: launch<T, EPI_GLU, 2>(p, fbl, s); break;
        default: launch<T, EPI_GLU, 3>(p, fbl, s); break;
      }
      break;
    default: launch<T, EPI_PLAIN, 0>(p, fbl, s);
  }
}

}  // namespace

bool wide_gemm_supported(int64_t M, int64_t N, int64_t K) {
  return M >= 33 && M <= 64 && N > 0 && K > 0 && N % 16 == 0 && K % 256 == 0 &&
         N * K < ((int64_t)1 << 40) && M * K < ((int64_t)1 << 31);
}

// Feature blocks per workgroup for `nblocks` 16-row blocks of W: the largest
// FB of 8, 4, 2 that still leaves workgroups for 0.6 of the CUs, else 1 (KS =
// 8: the N = 4096 projections, one block per workgroup like the skinny
// kernel).  Measured on the Llama-2-7B products (profiles/r19a_wide_decode.txt):
// 256 blocks FB = 1, qkv's 768 FB = 4, fc1's 1376 and the LM head's 2000 FB = 8.
int wide_gemm_split(int64_t nblocks) {
  for (int fb = 8; fb > 1; fb /= 2)
    if ((nblocks + fb - 1) / fb * 5 >= 3 * (int64_t)wide_cus()) return fb;
  return 1;
}

// fb: 1, 2, 4 or 8 feature blocks per workgroup (KS = 8 / fb); 0: wide_gemm_split
void wide_gemm_ex(const SkinnyArgs& p, int epi, int dt, int fb, hipStream_t s) {
  if (fb == 0) fb = wide_gemm_split(epi == EPI_GLU ? p.N / 8 : p.N / 16);
  const int fbl = fb == 8 ? 3 : fb == 4 ? 2 : fb == 2 ? 1 : 0;
  if (dt == DT_BF16) dispatch<bf16>(p, epi, fbl, s);
  else dispatch<fp16>(p, epi, fbl, s);
}

}  // namespace ema
