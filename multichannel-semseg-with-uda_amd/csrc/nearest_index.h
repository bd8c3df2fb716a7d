// The source indices of Pillow's NEAREST resize over a whole axis: the one statement of that rule, shared by the kernels that gather
// through it (csrc/io.hip resize_nearest_u8, csrc/ensemble.hip label_resize_colorize).
#pragma once
#include "common.h"

namespace {

// ImagingScaleAffine (Geometry.c) source indices for NEAREST over a whole axis: xo = a0/2, then xo += a0 per step (sequential,
// as Pillow accumulates it), index = xo < 0 ? -1 : (int)xo
__global__ void nearest_index_kernel(int in_size, int out_size, int* __restrict__ idx) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double a0 = (double)in_size / (double)out_size;
  double xo = a0 * 0.5;
  for (int x = 0; x < out_size; ++x) {
    int xin = xo < 0.0 ? -1 : (int)xo;
    xin = xin < 0 ? 0 : (xin > in_size - 1 ? in_size - 1 : xin);
    idx[x] = xin;
    xo += a0;
  }
}

}  // namespace
