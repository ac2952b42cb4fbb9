// The K-step of the persistent 4-wave 256x256 GEMMs (gemm_nt.hip gemm_nt6_k,
// gemm_wgrad.hip wgrad4_k): one K-step = 128 MFMAs per wave over two register
// fragment sets (k-half 0 / 1), two LDS slots.  The slot plan is plain
// constexpr (host code may include this header); the executor that both
// kernels run is device code.
#pragma once

namespace ema {

// K-step slot plan of the persistent kernel: the event lists say after which
// MFMA (0..127) of a K-step each fragment read / DMA piece / barrier issues.
//   rd1: the 16 k-half-1 fragments (0..7 A, 8..15 B) from the current slot:
//        A before barrier b1, B between b1 and b2;
//   dma: the 16 pieces of step t+2 into the current slot: A after b1 (every
//        wave has read A's k-half 1), B after b2; 13 of them before w;
//   w:   vmcnt(13) + barrier: step t+1 landed (own DMA, then everyone's);
//   rd0: the next step's k-half-0 fragments from the other slot, after w.
// (the vendor 256x256 kernel's placement, measured in scripts/gemm_lab.py:
// one load burst right after each refill barrier, B's last three pieces
// after the wait; +1-5 % over the round-4 plan, profiles/r5e_gemm_lab.txt)
struct NtPlan {
  int rd1[16], dma[16], rd0[16];
  int b1, b2, w;
};
inline constexpr NtPlan kNtPlan = {
    {0, 2, 4, 6, 8, 10, 12, 14, 24, 27, 30, 33, 36, 38, 40, 42},
    {22, 25, 28, 31, 34, 52, 55, 58, 61, 64, 85, 87, 89, 96, 100, 124},
    {93, 94, 95, 97, 98, 102, 103, 104, 105, 106, 109, 112, 114, 117, 120, 123},
    20, 50, 91};
inline constexpr int nt_plan_vmw() {
  int n = 0;
  for (int q = 0; q < 16; ++q) n += kNtPlan.dma[q] <= kNtPlan.w;
  return n;
}
static_assert(nt_plan_vmw() == 13, "pieces issued before the step-t+1 wait");

}  // namespace ema

#ifdef __HIPCC__
#include "fa_common.h"

namespace ema {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __amdgpu_buffer_rsrc_t Rsrc;

// 16x16x32 MFMAs as asm with the accumulator tied to an AGPR operand: a tile
// defined and updated only by these stays AGPR-resident.  mfma_acc: acc += a·b;
// mfma_acc0: acc = a·b (C = 0, the first k-half of a tile).
template <typename T>
__device__ __forceinline__ void mfma_acc(f32x4& acc, typename fa::MT<T>::x8 a,
                                         typename fa::MT<T>::x8 b) {
  if constexpr (__is_same(T, bf16))
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
  else
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
template <typename T>
__device__ __forceinline__ void mfma_acc0(f32x4& acc, typename fa::MT<T>::x8 a,
                                          typename fa::MT<T>::x8 b) {
  if constexpr (__is_same(T, bf16))
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=a"(acc) : "v"(a), "v"(b));
  else
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=a"(acc) : "v"(a), "v"(b));
}

// One K-step of kNtPlan.  set0 holds the step's k-half-0 fragments on entry
// and the next step's on exit ([0..7] A, [8..15] B; MFMA (I, J) takes B
// fragment J and A fragment I); ZERO: the first step of a tile.  The kernel
// supplies its addressing as three callables, each invoked with event index
// E as an integral_constant:
//   rd1(E)  read k-half-1 fragment E of this step from the current slot -> set1
//   dma(E)  issue DMA piece E of step t+2 into the current slot
//   rd0(E)  read k-half-0 fragment E of step t+1 from the other slot -> set0
template <typename T, bool ZERO, typename Rd1, typename Dma, typename Rd0>
__device__ __forceinline__ void nt_plan_kstep(f32x4 (&acc)[8][8], typename fa::MT<T>::x8 (&set0)[16],
                                              typename fa::MT<T>::x8 (&set1)[16], Rd1&& rd1,
                                              Dma&& dma, Rd0&& rd0) {
  constexpr int VMW = nt_plan_vmw();
  fa::static_for<128>([&](auto sc) {
    constexpr int S = decltype(sc)::value, IDX = S & 63, I = IDX / 8, J = IDX % 8;
    if constexpr (S < 64) {
      if constexpr (ZERO) mfma_acc0<T>(acc[I][J], set0[8 + J], set0[I]);
      else mfma_acc<T>(acc[I][J], set0[8 + J], set0[I]);
    } else {
      mfma_acc<T>(acc[I][J], set1[8 + J], set1[I]);
    }
    fa::static_for<16>([&](auto ec) {
      constexpr int E = decltype(ec)::value;
      if constexpr (kNtPlan.rd1[E] == S) rd1(ec);
      if constexpr (kNtPlan.dma[E] == S) dma(ec);
      if constexpr (kNtPlan.rd0[E] == S) rd0(ec);
    });
    if constexpr (S == kNtPlan.b1 || S == kNtPlan.b2) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
    }
    if constexpr (S == kNtPlan.w) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"(VMW) : "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
    }
    __builtin_amdgcn_sched_barrier(0);
  });
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

}  // namespace ema
#endif  // __HIPCC__
