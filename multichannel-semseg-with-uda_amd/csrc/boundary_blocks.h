// Building blocks the boundary-branch kernels share (csrc/boundary.hip, csrc/seg2bd.hip): the bilinear xS source index of torch's
// upsample_bilinear2d, the sigmoid, the class-balanced BCE term and its gradient, and the fp64 block partials of its three sums.
// fp contraction is off, so a kernel that calls these computes the very bits another kernel that calls them does.
#pragma once
#include "block_reduce.h"

namespace {

// source index / weights of torch's upsample_bilinear2d (align_corners=False) at scale S: src = (dst + 0.5)/S - 0.5, clamped
// at 0 (src_index of multitask.hip with 1/8 replaced by 1/S; S is a power of two, so 1/S is exact)
template <int S>
__device__ __forceinline__ void src_index_s(int dst, int in_size, int& i0, int& i1, float& l0, float& l1) {
  float s = (1.f / (float)S) * ((float)dst + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}

template <int S>
__device__ __forceinline__ float tap_weight_s(int dst, int in_size, int i) {
  int i0, i1;
  float l0, l1;
  src_index_s<S>(dst, in_size, i0, i1, l0, l1);
  return (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
}

// the bilinear xS value at output pixel (oy, ox) of one low-resolution plane [Hi, Wi]
template <int S>
__device__ __forceinline__ float up_at(const float* __restrict__ pl, int Hi, int Wi, int oy, int ox) {
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
  src_index_s<S>(oy, Hi, y0, y1, ly0, ly1);
  src_index_s<S>(ox, Wi, x0, x1, lx0, lx1);
  const float* r0 = pl + y0 * Wi;
  const float* r1 = pl + y1 * Wi;
  return ly0 * (lx0 * r0[x0] + lx1 * r0[x1]) + ly1 * (lx0 * r1[x0] + lx1 * r1[x1]);
}

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// F.binary_cross_entropy of the installed torch: both logarithms clamped at -100 before they are multiplied
__device__ __forceinline__ float bce_term(float p, float t) {
  const float lp = fmaxf(logf(p), -100.f);
  const float lq = fmaxf(log1pf(-p), -100.f);
  return (t - 1.f) * lq - t * lp;
}

// ... and its backward under the class-balancing weight w = 1 - beta + (2 beta - 1) t; gs = upstream / n
__device__ __forceinline__ float bce_grad(float p, float t, float beta, float gs) {
  const float w = (1.f - beta) + (2.f * beta - 1.f) * t;
  return gs * (p - t) / fmaxf((1.f - p) * p, 1e-12f) * w;
}

struct Sums {
  float t, b, tb;
};

__device__ __forceinline__ void sums_add(Sums& s, float p, float t) {
  const float b = bce_term(p, t);
  s.t += t;
  s.b += b;
  s.tb += t * b;
}

// block partials: [block][3] doubles (sum t, sum bce, sum t*bce)
__device__ __forceinline__ void sums_store(const Sums& s, double* __restrict__ part) {
  __shared__ double sh[3][4];
  double v[3] = {(double)s.t, (double)s.b, (double)s.tb};
  block_gather(v, sh);
  if (threadIdx.x < 3) part[(size_t)blockIdx.x * 3 + threadIdx.x] = tree_total<4>(sh[threadIdx.x]);
}

// the totals of those partials over n elements -> beta = 1 - sum t / n,  loss = ((1 - beta) sum bce + (2 beta - 1) sum t bce) / n
__device__ __forceinline__ void balanced_bce(const double (&tot)[3], double n, double& loss, double& beta) {
  beta = 1.0 - tot[0] / n;
  loss = ((1.0 - beta) * tot[1] + (2.0 * beta - 1.0) * tot[2]) / n;
}

int sum_blocks(int64_t n) { return ceil_div64(n, 256 * 16, 2048); }

}  // namespace
