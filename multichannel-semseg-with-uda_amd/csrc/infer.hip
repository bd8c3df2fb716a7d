// Inference tails of the multitask and source-only testers, fused so that the full-resolution logits are never stored:
//   predict_up8:  z = up(s), with up = the learned x8 up-sampler (ConvTranspose2d(C,C,16,stride 8,pad 4,groups=C), DRNSeg.up,
//                 models/dilated_fcn.py:357-366) or the bilinear x8 up-sampler with align_corners=False (MCDMultiTaskDecoder.upsample,
//                 :676); then label = argmax over the first C_used classes and the entropy term of util.py:44-48
//                 (adapt_multitask_tester.py:118-141, source_tester.py:119-143).
//   depth_image:  bilinear x8 of the depth head, then transform.unnormalize to an HWC uint8 image (adapt_multitask_tester.py:148-155,
//                 transform.py:285-294), numpy's float64 arithmetic and float64 -> uint8 cast included.
// The interpolation expressions are restated from bilinear8_fwd_kernel (multitask.hip) and up8_fwd_kernel (up8.hip): the build
// compiles with -ffp-contract=off, so the same expression in the same order gives the same bits, and the labels equal those of the
// unfused composition bit for bit.
#include "block_reduce.h"
#include "predict_pixel.h"

namespace {

constexpr int INF_NT = 512;  // 8 waves: two workgroups per CU are what the LDS of the learned form (67 KB at C = 41) allows

// upsample_bilinear2d's source index / weights (align_corners=False): src = (dst + 0.5)/8 - 0.5, clamped at 0
__device__ __forceinline__ void bl_index(int dst, int in_size, int& i0, int& i1, float& l0, float& l1) {
  float s = 0.125f * ((float)dst + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}

// One workgroup = one image n and one band b of output rows, [8b-4, 8b+4) clipped to [0, 8Hi), b = 0..Hi.  Every pixel of the band
// reads input rows r0 = max(b-1, 0) and r0+1 (clamped) only, under either up-sampler: bilinear y0 = b-1 (0 in band 0), y1 = y0+1
// clamped; learned iy = b and b-1 where they exist.  Those two rows of all C channels (and the C 16x16 kernels) are staged in LDS,
// then each thread forms a pixel's C logits in registers and runs predict_kernel's softmax / argmax / entropy (predict_pixel.h) on them.
template <int NCMAX, bool LEARNED>
__global__ __launch_bounds__(INF_NT) void predict_up8_kernel(const float* __restrict__ s, const float* __restrict__ w,
                                                             uint8_t* __restrict__ labels, float* __restrict__ part, int C, int C_used,
                                                             int Hi, int Wi) {
  extern __shared__ float ism[];
  const int n = blockIdx.x / (Hi + 1);
  const int band = blockIdx.x - n * (Hi + 1);
  const int Wo = 8 * Wi, Ho = 8 * Hi;
  const int r0 = band > 0 ? band - 1 : 0;
  const int r1 = r0 + 1 < Hi ? r0 + 1 : Hi - 1;
  const int cw = C * Wi;
  float* xs = ism;           // [2][C][Wi]: slot 0 = row r0, slot 1 = row r1
  float* ws = ism + 2 * cw;  // [C][16][16]
  const float* sn = s + (size_t)n * C * Hi * Wi;
  for (int i = threadIdx.x; i < 2 * cw; i += INF_NT) {
    const int slot = i >= cw ? 1 : 0;
    const int rem = i - slot * cw;
    const int c = rem / Wi;
    const int ix = rem - c * Wi;
    xs[i] = sn[((size_t)c * Hi + (slot ? r1 : r0)) * Wi + ix];
  }
  if (LEARNED)
    for (int i = threadIdx.x; i < C * 256; i += INF_NT) ws[i] = w[i];
  __syncthreads();

  const int oy_begin = band > 0 ? 8 * band - 4 : 0;
  const int oy_end = 8 * band + 4 < Ho ? 8 * band + 4 : Ho;
  const int npix = (oy_end - oy_begin) * Wo;
  uint8_t* lab = labels + ((size_t)n * Ho + oy_begin) * Wo;
  float ent = 0.f;
  for (int p = threadIdx.x; p < npix; p += INF_NT) {
    const int ry = p / Wo;
    const int oy = oy_begin + ry;
    const int ox = p - ry * Wo;
    float a[NCMAX];
    if (LEARNED) {
      // up8_fwd_kernel's taps in its order: (iy_hi, ix_hi), (iy_hi, ix_hi-1), (iy_hi-1, ix_hi), (iy_hi-1, ix_hi-1), each skipped
      // when outside the input, accumulated by fmaf from 0
      const int iy_hi = (oy + 4) >> 3, ky0 = (oy + 4) & 7;
      const int ix_hi = (ox + 4) >> 3, kx0 = (ox + 4) & 7;
      const bool ya = iy_hi < Hi, yb = iy_hi >= 1, xa = ix_hi < Wi, xb = ix_hi >= 1;
      const float* rowa = xs + (iy_hi - r0) * cw;             // slot 0 in band 0, else slot 1 (unread in band Hi)
      const float* rowb = xs + (yb ? iy_hi - 1 - r0 : 0) * cw;  // slot 0 (unread in band 0)
#pragma unroll
      for (int c = 0; c < NCMAX; ++c) {
        float v = -INFINITY;
        if (c < C) {
          const float* wk = ws + c * 256;
          float o = 0.f;
          if (ya) {
            if (xa) o = fmaf(rowa[c * Wi + ix_hi], wk[ky0 * 16 + kx0], o);
            if (xb) o = fmaf(rowa[c * Wi + ix_hi - 1], wk[ky0 * 16 + kx0 + 8], o);
          }
          if (yb) {
            if (xa) o = fmaf(rowb[c * Wi + ix_hi], wk[(ky0 + 8) * 16 + kx0], o);
            if (xb) o = fmaf(rowb[c * Wi + ix_hi - 1], wk[(ky0 + 8) * 16 + kx0 + 8], o);
          }
          v = o;
        }
        a[c] = v;
      }
    } else {
      int y0, y1, x0, x1;
      float ly0, ly1, lx0, lx1;
      bl_index(oy, Hi, y0, y1, ly0, ly1);
      bl_index(ox, Wi, x0, x1, lx0, lx1);
      const float* q0 = xs + (y0 - r0) * cw;
      const float* q1 = xs + (y1 - r0) * cw;
#pragma unroll
      for (int c = 0; c < NCMAX; ++c) {
        float v = -INFINITY;
        if (c < C) {
          const float* t0 = q0 + c * Wi;
          const float* t1 = q1 + c * Wi;
          v = ly0 * (lx0 * t0[x0] + lx1 * t0[x1]) + ly1 * (lx0 * t1[x0] + lx1 * t1[x1]);
        }
        a[c] = v;
      }
    }
    int best;
    MCD_PREDICT_PIXEL(a, best, ent)
    lab[p] = (uint8_t)best;
  }
  __shared__ float sh[1][INF_NT / 64];
  float v[1] = {ent};
  block_gather(v, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tree_total<INF_NT / 64>(sh[0]);
}

// np.uint8(t) for a float64 t as numpy does it on x86-64: the C cast (npy_ubyte)t, compiled as a truncating conversion to int32
// (cvttsd2si) whose low byte is kept; NaN, +-inf and everything outside the int32 range give the "integer indefinite" 0x80000000,
// i.e. 0.  (Measured with numpy 2.2.6: -1.0 -> 255, -200.2 -> 56, 256.0 -> 0, 300.7 -> 44, 2^31 - 0.5 -> 255, 3e9 + 7 -> 0, nan -> 0.)
__device__ __forceinline__ uint8_t numpy_u8(double t) {
  return (t > -2147483649.0 && t < 2147483648.0) ? (uint8_t)(unsigned)(int)t : (uint8_t)0;
}

// one thread per output byte img[n, oy, ox, k]: v = bilinear8(d)[n, Cd == 1 ? 0 : k, oy, ox] (fp32, bilinear8_fwd_kernel's expression),
// then unnormalize's (v * std[k] + mean[k]) * 255 with every operation rounded in double, as numpy promotes the float32 array against
// the float64 constants; a single depth channel is broadcast into three differently scaled ones, as numpy's (H,W,1) * (3,) does
__global__ __launch_bounds__(256) void depth_image_kernel(const float* __restrict__ d, uint8_t* __restrict__ img, int Cd, int Hi,
                                                          int Wi, int64_t total) {
  const int Wo = 8 * Wi, Ho = 8 * Hi;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % 3);
    const int64_t pix = i / 3;
    const int ox = (int)(pix % Wo);
    const int64_t t = pix / Wo;
    const int oy = (int)(t % Ho);
    const int64_t n = t / Ho;
    const float* x = d + ((size_t)n * Cd + (Cd == 1 ? 0 : k)) * Hi * Wi;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    bl_index(oy, Hi, y0, y1, ly0, ly1);
    bl_index(ox, Wi, x0, x1, lx0, lx1);
    const float* q0 = x + y0 * Wi;
    const float* q1 = x + y1 * Wi;
    const float v = ly0 * (lx0 * q0[x0] + lx1 * q0[x1]) + ly1 * (lx0 * q1[x0] + lx1 * q1[x1]);
    const double sd = k == 0 ? 0.229 : (k == 1 ? 0.224 : 0.225);  // transform.py:287-288, not the training transform's constants
    const double mn = k == 0 ? 0.485 : (k == 1 ? 0.456 : 0.406);
    img[i] = numpy_u8((((double)v * sd) + mn) * 255.0);
  }
}

size_t predict_up8_lds(int C, int Wi, bool learned) { return ((size_t)2 * C * Wi + (learned ? (size_t)C * 256 : 0)) * sizeof(float); }

template <int NCMAX>
int launch_predict_up8(bool learned, int blocks, size_t lds, hipStream_t st, const float* s, const float* w, uint8_t* labels,
                       float* part, int C, int C_used, int Hi, int Wi) {
  auto go = [&](auto kern) {
    if (lds > 64 * 1024) {
      const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) {
        mcdseg_set_error("predict_labels_up8: cannot reserve %zu bytes of LDS: %s", lds, hipGetErrorString(e));
        return -5;
      }
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(INF_NT), lds, st, s, w, labels, part, C, C_used, Hi, Wi);
    return 0;
  };
  return learned ? go(predict_up8_kernel<NCMAX, true>) : go(predict_up8_kernel<NCMAX, false>);
}

}  // namespace

extern "C" size_t mcdseg_predict_up8_workspace_bytes(int32_t N, int32_t Hi) {
  return (N > 0 && Hi > 0) ? (size_t)N * (Hi + 1) * sizeof(float) : 0;
}

extern "C" int mcdseg_predict_labels_up8(const float* s, const float* w, uint8_t* labels, float* entropy, int32_t N, int32_t C,
                                         int32_t C_used, int32_t Hi, int32_t Wi, void* workspace, size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(s && labels && entropy && workspace, "predict_labels_up8: null pointer");
  MCD_REQUIRE(N > 0 && Hi > 0 && Wi > 0 && C > 0 && C <= 48 && C_used > 0 && C_used <= C, "predict_labels_up8: bad dims");
  MCD_REQUIRE((int64_t)N * (Hi + 1) < (1ll << 31) && (int64_t)Hi * Wi * 64 < (1ll << 31), "predict_labels_up8: too large");
  MCD_REQUIRE(workspace_bytes >= mcdseg_predict_up8_workspace_bytes(N, Hi), "predict_labels_up8: workspace too small");
  const bool learned = w != nullptr;
  const size_t lds = predict_up8_lds(C, Wi, learned);
  MCD_REQUIRE(lds <= 160 * 1024, "predict_labels_up8: two input rows of %d channels x %d columns%s need %zu bytes of LDS (at most 160 KB)", C, Wi,
              learned ? " and the up-sampling kernels" : "", lds);
  const int blocks = N * (Hi + 1);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  int rc;
  if (C <= 16)
    rc = launch_predict_up8<16>(learned, blocks, lds, st, s, w, labels, part, C, C_used, Hi, Wi);
  else if (C <= 24)
    rc = launch_predict_up8<24>(learned, blocks, lds, st, s, w, labels, part, C, C_used, Hi, Wi);
  else if (C == 41)  // the datasets' 41 classes get their own instantiation: no padding classes, 128 VGPRs or fewer, 4 waves per SIMD
    rc = launch_predict_up8<41>(learned, blocks, lds, st, s, w, labels, part, C, C_used, Hi, Wi);
  else
    rc = launch_predict_up8<48>(learned, blocks, lds, st, s, w, labels, part, C, C_used, Hi, Wi);
  if (rc != 0) return rc;
  MCD_LAUNCH_CHECK("predict_labels_up8");
  const double P = (double)N * Hi * Wi * 64;
  hipLaunchKernelGGL(sum_finalize_kernel<float>, dim3(1), dim3(256), 0, st, (const float*)part, (int64_t)blocks, -1.0 / (P * (double)C),
                     entropy);
  MCD_LAUNCH_CHECK("predict_labels_up8 (finalize)");
  return 0;
}

extern "C" int mcdseg_depth_image_u8(const float* d, uint8_t* img, int32_t N, int32_t Cd, int32_t Hi, int32_t Wi, void* stream) {
  MCD_REQUIRE(d && img && N > 0 && Hi > 0 && Wi > 0 && (Cd == 1 || Cd == 3), "depth_image_u8: bad arguments");
  const int64_t total = (int64_t)N * Hi * Wi * 64 * 3;
  int64_t blocks = ceil_div64(total, 256 * 4);
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(depth_image_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d, img, Cd, Hi, Wi, total);
  MCD_LAUNCH_CHECK("depth_image_u8");
  return 0;
}
