// The joint transform of the reference's trainers (joint_transforms.py:248-255): RandomHorizontallyFlip, RandomRotate(angle),
// RandomCrop(size), applied to an image and its label map together, in front of ToTensor/Normalize and ToLabel/ReLabel.
//
// One gather pass per tensor: crop, rotation and flip are composed into ONE index map from the output pixel back to the bytes the
// loader delivered -- no flipped or rotated intermediate image exists.  The per-sample parameters come from two small device tables
// (drawn on the host, mcdseg/augment.py), so one launch serves a batch whose samples are all transformed differently:
//     affine [N][6]  double   the matrix PIL.Image.rotate hands to Image.transform (destination -> source)
//     geom   [N][10] int32    {mode, flip, x1, y1, fa0, fa1, fa2, fa3, fa4, fa5}
// mode: 0 copy (angle == 0), 1 affine, 2 / 3 / 4 = Pillow's exact ROTATE_180 / ROTATE_90 / ROTATE_270 (Image.rotate takes them for
// 180 degrees, and for 90 / 270 on a square image); (x1, y1) the crop's corner in the rotated image; fa* the 16.16 fixed-point matrix of
// Pillow's nearest-neighbour path.  The arithmetic is Pillow's (Geometry.c), so the bytes are Pillow's:
//   * images:  ImagingGenericTransform with affine_transform + bilinear_filter8, all in double (the library is compiled with
//              -ffp-contract=off, which keeps `a + (b - a) * d` two roundings); a source position outside the image is fill 0.
//   * labels:  affine_fixed -- source = (fa2 + y*fa1 + x*fa0) >> 16 (Pillow's running sums, here as one 64-bit product sum);
//              outside the image is label 0, a real class: mask.rotate(angle, NEAREST) of the reference fills 0, not the background id.
// The flip comes first in the reference, so every source column i is read at W-1-i.  The output is uint8, or the next transform fused:
// ToTensor+Normalize (fp32 NCHW, the arithmetic of normalize_u8) / ToLabel+ReLabel (int64, as relabel_u8).
// One thread per output pixel does all Cs channels of it (the HWC bytes of a tap are contiguous, the NCHW stores coalesced along x);
// sample and mode are uniform per block.  Every source index is range-checked in the kernel: no table content reads out of bounds.
#include <cmath>
#include "common.h"

namespace {

constexpr int JA_COPY = 0, JA_AFFINE = 1, JA_ROT180 = 2, JA_ROT90 = 3, JA_ROT270 = 4;
constexpr int JA_GEOM = 10;

// (row, column) in the flipped-then-rotated image's SOURCE, i.e. in the flipped image, for the exact modes; false = outside
__device__ __forceinline__ bool ja_exact_source(int mode, int X, int Y, int H, int W, int* row, int* col) {
  int r, c;
  if (mode == JA_ROT180) {
    r = H - 1 - Y, c = W - 1 - X;
  } else if (mode == JA_ROT90) {  // ImagingRotate90: out[W-1-x][y] = in[y][x]
    r = X, c = W - 1 - Y;
  } else if (mode == JA_ROT270) {  // ImagingRotate270: out[x][H-1-y] = in[y][x]
    r = H - 1 - X, c = Y;
  } else {
    r = Y, c = X;
  }
  *row = r, *col = c;
  return r >= 0 && r < H && c >= 0 && c < W;
}

template <int CS, bool FUSED>
__global__ __launch_bounds__(256) void joint_augment_image_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst_u8,
                                                                  float* __restrict__ dst_f, const float* __restrict__ mean,
                                                                  const float* __restrict__ stdv, const double* __restrict__ affine,
                                                                  const int32_t* __restrict__ geom, int H, int W, int OH, int OW, int C,
                                                                  int c_off, int cs_rt) {
  const int cs = CS > 0 ? CS : cs_rt;
  const int n = blockIdx.y;
  const int32_t* g = geom + (size_t)n * JA_GEOM;
  const int mode = g[0], x1 = g[2], y1 = g[3];
  const bool flip = g[1] != 0;
  const double* a = affine + (size_t)n * 6;
  const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5];
  const uint8_t* s = src + (size_t)n * H * W * cs;
  const int OHW = OH * OW;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < OHW; p += gridDim.x * blockDim.x) {
    const int y = p / OW, x = p - y * OW;
    const int X = x + x1, Y = y + y1;
    // taps: t00/t01 on the upper row, t10/t11 on the lower; fill = no source; lerp = bilinear (else the byte at t00)
    const uint8_t *t00 = s, *t01 = s, *t10 = s, *t11 = s;
    double dx = 0.0, dy = 0.0;
    bool fill = true, lerp = false, two_rows = false;
    if (mode == JA_AFFINE) {
      double xin = a0 * ((double)X + 0.5) + a1 * ((double)Y + 0.5) + a2;
      double yin = a3 * ((double)X + 0.5) + a4 * ((double)Y + 0.5) + a5;
      if (!(xin < 0.0 || xin >= (double)W || yin < 0.0 || yin >= (double)H)) {
        xin -= 0.5;
        yin -= 0.5;
        const int ix = (int)floor(xin), iy = (int)floor(yin);
        dx = xin - (double)ix;
        dy = yin - (double)iy;
        int c0 = ix < 0 ? 0 : (ix < W ? ix : W - 1);
        int c1 = ix + 1 < 0 ? 0 : (ix + 1 < W ? ix + 1 : W - 1);
        if (flip) c0 = W - 1 - c0, c1 = W - 1 - c1;
        const int r0 = iy < 0 ? 0 : (iy < H ? iy : H - 1);
        two_rows = iy + 1 >= 0 && iy + 1 < H;
        const int r1 = two_rows ? iy + 1 : r0;
        t00 = s + ((size_t)r0 * W + c0) * cs;
        t01 = s + ((size_t)r0 * W + c1) * cs;
        t10 = s + ((size_t)r1 * W + c0) * cs;
        t11 = s + ((size_t)r1 * W + c1) * cs;
        fill = false, lerp = true;
      }
    } else {
      int r, c;
      if (ja_exact_source(mode, X, Y, H, W, &r, &c)) {
        if (flip) c = W - 1 - c;
        t00 = s + ((size_t)r * W + c) * cs;
        fill = false;
      }
    }
#pragma unroll
    for (int c = 0; c < (CS > 0 ? CS : 8); ++c) {
      if (c >= cs) break;
      int u = 0;
      if (!fill) {
        if (lerp) {
          const int p00 = t00[c], p01 = t01[c];
          const double v1 = (double)p00 + (double)(p01 - p00) * dx;
          double v2 = v1;
          if (two_rows) {
            const int p10 = t10[c], p11 = t11[c];
            v2 = (double)p10 + (double)(p11 - p10) * dx;
          }
          const double v = v1 + (v2 - v1) * dy;
          u = (int)v;  // (UINT8)v: truncation
        } else {
          u = t00[c];
        }
      }
      if (FUSED) {
        const float v = (float)u / 255.0f;
        dst_f[((size_t)n * C + c_off + c) * OHW + p] = (v - mean[c]) / stdv[c];
      } else {
        dst_u8[((size_t)n * OHW + p) * cs + c] = (uint8_t)u;
      }
    }
  }
}

template <bool FUSED>
__global__ __launch_bounds__(256) void joint_augment_label_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst_u8,
                                                                  int64_t* __restrict__ dst_l, const int32_t* __restrict__ geom, int H,
                                                                  int W, int OH, int OW, int olabel, int nlabel) {
  const int n = blockIdx.y;
  const int32_t* g = geom + (size_t)n * JA_GEOM;
  const int mode = g[0], x1 = g[2], y1 = g[3];
  const bool flip = g[1] != 0;
  const int64_t fa0 = g[4], fa1 = g[5], fa2 = g[6], fa3 = g[7], fa4 = g[8], fa5 = g[9];
  const uint8_t* s = src + (size_t)n * H * W;
  const int OHW = OH * OW;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < OHW; p += gridDim.x * blockDim.x) {
    const int y = p / OW, x = p - y * OW;
    const int X = x + x1, Y = y + y1;
    int v = 0;
    int r, c;
    bool inside;
    if (mode == JA_AFFINE) {
      const int64_t xi = (fa2 + (int64_t)Y * fa1 + (int64_t)X * fa0) >> 16;
      const int64_t yi = (fa5 + (int64_t)Y * fa4 + (int64_t)X * fa3) >> 16;
      inside = xi >= 0 && xi < W && yi >= 0 && yi < H;
      r = (int)yi, c = (int)xi;
    } else {
      inside = ja_exact_source(mode, X, Y, H, W, &r, &c);
    }
    if (inside) {
      if (flip) c = W - 1 - c;
      v = s[(size_t)r * W + c];
    }
    if (FUSED)
      dst_l[(size_t)n * OHW + p] = v == olabel ? nlabel : v;
    else
      dst_u8[(size_t)n * OHW + p] = (uint8_t)v;
  }
}

int ja_check(const char* what, const void* src, const void* dst, const void* affine, const void* geom, int N, int H, int W, int OH, int OW) {
  MCD_REQUIRE(src && dst && geom, "%s: null pointer", what);
  MCD_REQUIRE(N > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "%s: bad dims", what);
  MCD_REQUIRE(N <= 65535 && (int64_t)H * W < (1ll << 31) && (int64_t)OH * OW < (1ll << 31), "%s: image too large", what);
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(geom) & 3) == 0 && (reinterpret_cast<uintptr_t>(affine) & 7) == 0,
              "%s: the parameter tables must be aligned to their element size", what);
  return 0;
}

dim3 ja_grid(int N, int OH, int OW) {
  int blocks = ceil_div(OH * OW, 256);
  if (blocks > 1024) blocks = 1024;
  return dim3(blocks, N);
}

template <bool FUSED>
void ja_launch_image(const uint8_t* src, uint8_t* dst_u8, float* dst_f, const float* mean, const float* stdv, const double* affine,
                     const int32_t* geom, int N, int H, int W, int Cs, int OH, int OW, int C, int c_off, hipStream_t st) {
  const dim3 grid = ja_grid(N, OH, OW);
  if (Cs == 3)
    hipLaunchKernelGGL((joint_augment_image_kernel<3, FUSED>), grid, dim3(256), 0, st, src, dst_u8, dst_f, mean, stdv, affine, geom, H, W, OH,
                       OW, C, c_off, Cs);
  else if (Cs == 1)
    hipLaunchKernelGGL((joint_augment_image_kernel<1, FUSED>), grid, dim3(256), 0, st, src, dst_u8, dst_f, mean, stdv, affine, geom, H, W, OH,
                       OW, C, c_off, Cs);
  else
    hipLaunchKernelGGL((joint_augment_image_kernel<0, FUSED>), grid, dim3(256), 0, st, src, dst_u8, dst_f, mean, stdv, affine, geom, H, W, OH,
                       OW, C, c_off, Cs);
}

}  // namespace

extern "C" int mcdseg_joint_augment_u8(const uint8_t* src, uint8_t* dst, const double* affine, const int32_t* geom, int32_t N, int32_t H,
                                       int32_t W, int32_t Cs, int32_t OH, int32_t OW, void* stream) {
  if (int rc = ja_check("joint_augment_u8", src, dst, affine, geom, N, H, W, OH, OW)) return rc;
  MCD_REQUIRE(affine, "joint_augment_u8: null pointer");
  MCD_REQUIRE(Cs > 0 && Cs <= 8, "joint_augment_u8: bad dims");
  ja_launch_image<false>(src, dst, nullptr, nullptr, nullptr, affine, geom, N, H, W, Cs, OH, OW, 0, 0, (hipStream_t)stream);
  MCD_LAUNCH_CHECK("joint_augment_u8");
  return 0;
}

extern "C" int mcdseg_joint_augment_normalize_u8(const uint8_t* src, float* dst, const float* mean, const float* stdv, const double* affine,
                                                 const int32_t* geom, int32_t N, int32_t H, int32_t W, int32_t Cs, int32_t OH, int32_t OW,
                                                 int32_t C, int32_t c_off, void* stream) {
  if (int rc = ja_check("joint_augment_normalize_u8", src, dst, affine, geom, N, H, W, OH, OW)) return rc;
  MCD_REQUIRE(affine && mean && stdv, "joint_augment_normalize_u8: null pointer");
  MCD_REQUIRE(Cs > 0 && Cs <= 8 && c_off >= 0 && c_off + Cs <= C, "joint_augment_normalize_u8: bad dims");
  ja_launch_image<true>(src, nullptr, dst, mean, stdv, affine, geom, N, H, W, Cs, OH, OW, C, c_off, (hipStream_t)stream);
  MCD_LAUNCH_CHECK("joint_augment_normalize_u8");
  return 0;
}

extern "C" int mcdseg_joint_augment_label_u8(const uint8_t* src, uint8_t* dst, const int32_t* geom, int32_t N, int32_t H, int32_t W,
                                             int32_t OH, int32_t OW, void* stream) {
  if (int rc = ja_check("joint_augment_label_u8", src, dst, nullptr, geom, N, H, W, OH, OW)) return rc;
  MCD_REQUIRE(H < 32768 && W < 32768, "joint_augment_label_u8: the 16.16 fixed-point path needs H, W < 32768");
  hipLaunchKernelGGL(joint_augment_label_kernel<false>, ja_grid(N, OH, OW), dim3(256), 0, (hipStream_t)stream, src, dst, (int64_t*)nullptr,
                     geom, H, W, OH, OW, 0, 0);
  MCD_LAUNCH_CHECK("joint_augment_label_u8");
  return 0;
}

extern "C" int mcdseg_joint_augment_relabel_u8(const uint8_t* src, int64_t* dst, const int32_t* geom, int32_t N, int32_t H, int32_t W,
                                               int32_t OH, int32_t OW, int32_t olabel, int32_t nlabel, void* stream) {
  if (int rc = ja_check("joint_augment_relabel_u8", src, dst, nullptr, geom, N, H, W, OH, OW)) return rc;
  MCD_REQUIRE(H < 32768 && W < 32768, "joint_augment_relabel_u8: the 16.16 fixed-point path needs H, W < 32768");
  hipLaunchKernelGGL(joint_augment_label_kernel<true>, ja_grid(N, OH, OW), dim3(256), 0, (hipStream_t)stream, src, (uint8_t*)nullptr, dst,
                     geom, H, W, OH, OW, olabel, nlabel);
  MCD_LAUNCH_CHECK("joint_augment_relabel_u8");
  return 0;
}
