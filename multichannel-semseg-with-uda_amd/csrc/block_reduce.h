// The block sums and finalizers of the loss and head kernels (device code only).
//
// Every reduced scalar of the library is deterministic by one recipe: per-thread partials -> wave sum (wave_sum / wave_sum_d of
// common.h) -> lane 0 of each wave writes an LDS slot -> one barrier -> the slots combined IN A FIXED ORDER into part[block * K + q]
// -> a one-block finalize kernel sums the partial rows in fp64 and writes the scalar.  The combination order decides the bits; the
// fused-vs-unfused bitwise tests, the determinism tests and tests/test_reduction_bits_gpu.py depend on it.  Two orders exist:
//
//   tree_total   pairwise, (r0 + r1) + (r2 + r3), one level deeper for 8 waves:
//                  label_wsum_kernel, softmax_ce_l1_kernel / softmax_ce_dist_kernel, predict_kernel          (loss.hip, loss_front.h)
//                  predict_up8_kernel (8 waves)                                                              (infer.hip)
//                  mse_kernel                                                                                (multitask.hip)
//                  sums_store: bce2d / boundary_head_bce / seg2bd forward (fp64)                             (boundary_blocks.h)
//                  seg2bd_dv_kernel (fp64)                                                                   (seg2bd.hip)
//                  prob_nll_partial_kernel (fp64)                                                            (fusion.hip)
//                  hha_gravity_partial_kernel (fp64, twelve sums)                                            (hha.hip)
//                  fill_system_kernel, fill_pv_kernel, fill_st_kernel, fill_xr_kernel, fill_residual_kernel
//                  (fp64, one or two dot products of the BiCGSTAB iteration each, through fill_block_sums)     (fill.hip)
//                  and every finalizer, through partials_total (loss_finalize_kernel: the same steps written out;
//                  hha_gravity_final_kernel: twelve columns, then the eigen-step in thread 0; fill_start_final_kernel,
//                  fill_alpha_final_kernel, fill_omega_final_kernel, fill_rho_final_kernel, fill_check_final_kernel: one or two
//                  columns, then the solver's scalars and the image's status in thread 0).
//   chain_total  left to right from zero, ((0 + r0) + r1) + ...; the zero stays: 0.f + -0.f is +0.f:
//                  up8_softmax_ce_l1_kernel, up8_softmax_ce_dist_kernel                                      (loss_front.h)
//                  up8_softmax_ce_l1_dma_kernel, up8_softmax_ce_dist_dma_kernel (the same steps written out) (loss_front.h)
//                  up8_uncertain_kernel                                                                      (uncertain.hip)
//
// A new kernel takes the order of the kernel it must agree with bit for bit, and is added to this list.
// Written out where a call would not do: the two kernels of the training step named above keep the instruction stream they had (the
// comments at their tails say what the call changed).  Outside: prob_nll_finalize_kernel (fusion.hip) adds its partial rows serially
// in one thread, and csrc/bn.hip keeps its own tails (a sum beside a running maximum).
#pragma once
#include <utility>

#include "common.h"

__device__ __forceinline__ float wave_total(float v) { return wave_sum(v); }
__device__ __forceinline__ double wave_total(double v) { return wave_sum_d(v); }

// v[k] <- its sum over the wave; lane 0 of each wave stores it to sh[k][wave]; one barrier.  sh is declared by the caller.
// Written over an index pack, not as loops over k: the K sums are straight-line code before any optimisation, as in the hand-written
// tails this replaces (out of a loop the compiler hoists the shuffles' lane arithmetic, and every calling kernel is scheduled anew).
template <int K, int WAVES, typename T, int... Q>
__device__ __forceinline__ void block_gather(T (&v)[K], T (&sh)[K][WAVES], std::integer_sequence<int, Q...>) {
  ((v[Q] = wave_total(v[Q])), ...);
  if ((threadIdx.x & 63) == 0) {
    ((sh[Q][threadIdx.x >> 6] = v[Q]), ...);
  }
  __syncthreads();
}
template <int K, int WAVES, typename T>
__device__ __forceinline__ void block_gather(T (&v)[K], T (&sh)[K][WAVES]) {
  block_gather(v, sh, std::make_integer_sequence<int, K>{});
}

template <int WAVES, typename T>
__device__ __forceinline__ T tree_total(const T* row) {
  static_assert(WAVES == 4 || WAVES == 8, "tree_total: 4 or 8 waves");
  if constexpr (WAVES == 4)
    return (row[0] + row[1]) + (row[2] + row[3]);
  else
    return tree_total<4>(row) + tree_total<4>(row + 4);
}

template <int WAVES, typename T>
__device__ __forceinline__ T chain_total(const T* row) {
  T t = 0;
  for (int k = 0; k < WAVES; ++k) t += row[k];
  return t;
}

// The finalize side, for a block of 256 threads: tot[k] = sum over i < count of part[i * row_stride + col + k], in fp64 -- a stride
// of 256 rows per thread, the wave sums, the pairwise tree.  Formed in thread 0 only.
template <int K, typename P, typename I>
__device__ __forceinline__ void partials_total(const P* __restrict__ part, I count, int row_stride, int col, double (&tot)[K]) {
  double s[K] = {};
  for (I i = threadIdx.x; i < count; i += 256)
    for (int k = 0; k < K; ++k) s[k] += (double)part[(size_t)i * row_stride + col + k];
  __shared__ double sh[K][4];
  for (int k = 0; k < K; ++k) {  // block_gather's steps one sum at a time, as loops: the form the finalizers always had
    const double v = wave_sum_d(s[k]);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 0; k < K; ++k) tot[k] = tree_total<4>(sh[k]);
}

// *out = scale * (the sum of n partials): the finalizer of every one-sum reduction (scale 1.0 is exact)
template <typename P>
__global__ __launch_bounds__(256) void sum_finalize_kernel(const P* __restrict__ part, int64_t n, double scale, float* __restrict__ out) {
  double tot[1];
  partials_total(part, n, 1, 0, tot);
  if (threadIdx.x == 0) *out = (float)(tot[0] * scale);
}
