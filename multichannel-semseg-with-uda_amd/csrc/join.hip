// The stage join of the FuseNet-style generator (FuseDRNSegBase.forward, models/dilated_fcn.py:308-328): y = a + b behind every
// stage of the RGB pass, with the pre-split companion of y for the next stage's convolutions written in the same pass.
//
//   y        = a + b                          the fp32 add and nothing else
//   y_bound  = a_bound + b_bound              |a + b| <= bound_a + bound_b: no reduction, both bounds travel with the tensors
//   y_cb     = split(y, scale(y_bound))       bitwise what mcdseg_split_cb(y, y_bound) writes: operand_scale / split_store of split.h
//
// HBM-bound: 8 B read and 4 B + the pieces (4 B f16x3, 6 B bf16x6) written per element.  One thread = 8 channels of one pixel
// (join_cb_kernel<P, 1>: any HW) or of FOUR adjacent pixels (join_cb_kernel<P, 4>: HW % 4 == 0 and 16-byte aligned fp32 pointers --
// every fp32 access is then 16 bytes per lane, and the lane's four companion units are 64 consecutive bytes per piece, the wave's 4 KB).
// Every element is computed by one expression, so the two forms give the same bits.  No LDS, no scratch, no atomics.
#include "split.h"

namespace {

template <class P, int PIX>
__global__ __launch_bounds__(256) void join_cb_kernel(const float* __restrict__ a, const float* __restrict__ a_bound,
                                                      const float* __restrict__ b, const float* __restrict__ b_bound,
                                                      float* __restrict__ y, typename P::elem* __restrict__ cb,
                                                      float* __restrict__ y_bound, int N, int C, int HW) {
  const int C8 = C >> 3;
  const int ng = blockIdx.y;  // n * C8 + g
  const int g = ng % C8;
  const int n = ng / C8;
  float bound = 0.f;
  if (y_bound != nullptr) {           // (always there for a scaled policy: cb_check)
    bound = a_bound[0] + b_bound[0];  // every thread forms the same sum: nobody reads y_bound here
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) y_bound[0] = bound;
  }
  const float inv_scale = 1.f / operand_scale<P>(&bound);
  const int pix = (blockIdx.x * 256 + threadIdx.x) * PIX;
  if (pix >= HW) return;  // (PIX == 4: HW % 4 == 0, a quad is inside or outside as a whole)
  const size_t base = ((size_t)n * C + 8 * g) * HW + pix;
  if constexpr (PIX == 1) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[e] = a[base + (size_t)e * HW] + b[base + (size_t)e * HW];
      y[base + (size_t)e * HW] = v[e];
    }
    split_store<P>(v, inv_scale, cb, (size_t)N * C * HW, (size_t)ng * HW + pix);
  } else {
    float4 va[8], vb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      va[e] = *reinterpret_cast<const float4*>(a + base + (size_t)e * HW);
      vb[e] = *reinterpret_cast<const float4*>(b + base + (size_t)e * HW);
    }
    float v[4][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float4 s;
      s.x = va[e].x + vb[e].x;
      s.y = va[e].y + vb[e].y;
      s.z = va[e].z + vb[e].z;
      s.w = va[e].w + vb[e].w;
      *reinterpret_cast<float4*>(y + base + (size_t)e * HW) = s;
      v[0][e] = s.x;
      v[1][e] = s.y;
      v[2][e] = s.z;
      v[3][e] = s.w;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) split_store<P>(v[q], inv_scale, cb, (size_t)N * C * HW, (size_t)ng * HW + pix + q);
  }
}

// y = a + b alone (y_cb == NULL: any channel count): float4 body + scalar tail when the pointers allow, all scalar otherwise
__global__ __launch_bounds__(256) void join_plain_kernel(const float* __restrict__ a, const float* __restrict__ a_bound,
                                                         const float* __restrict__ b, const float* __restrict__ b_bound,
                                                         float* __restrict__ y, float* __restrict__ y_bound, int64_t n4, int64_t n) {
  if (y_bound != nullptr && blockIdx.x == 0 && threadIdx.x == 0) y_bound[0] = a_bound[0] + b_bound[0];
  const float4* a4 = reinterpret_cast<const float4*>(a);
  const float4* b4 = reinterpret_cast<const float4*>(b);
  float4* y4 = reinterpret_cast<float4*>(y);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 p = a4[i], q = b4[i];
    float4 s;
    s.x = p.x + q.x;
    s.y = p.y + q.y;
    s.z = p.z + q.z;
    s.w = p.w + q.w;
    y4[i] = s;
  }
  for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) y[i] = a[i] + b[i];
}

bool join_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <class P>
void join_cb_launch(const float* a, const float* a_bound, const float* b, const float* b_bound, float* y, void* y_cb, float* y_bound,
                    int N, int C, int HW, hipStream_t st) {
  typedef typename P::elem E;
  const bool vec = (HW % 4 == 0) && join_aligned16(a) && join_aligned16(b) && join_aligned16(y);
  const dim3 grid(ceil_div(HW, vec ? 1024 : 256), N * (C / 8));
  if (vec)
    hipLaunchKernelGGL((join_cb_kernel<P, 4>), grid, dim3(256), 0, st, a, a_bound, b, b_bound, y, (E*)y_cb, y_bound, N, C, HW);
  else
    hipLaunchKernelGGL((join_cb_kernel<P, 1>), grid, dim3(256), 0, st, a, a_bound, b, b_bound, y, (E*)y_cb, y_bound, N, C, HW);
}

}  // namespace

extern "C" int mcdseg_stage_join(const float* a, const float* a_bound, const float* b, const float* b_bound, float* y, void* y_cb,
                                 float* y_bound, int32_t math, int32_t N, int32_t C, int32_t HW, void* stream) {
  MCD_REQUIRE(a && b && y, "stage_join: null pointer");
  MCD_REQUIRE(N > 0 && C > 0 && HW > 0, "stage_join: bad dims");
  const bool bounds = a_bound && b_bound && y_bound;
  MCD_REQUIRE(bounds || !(a_bound || b_bound || y_bound), "stage_join: the bounds come as all three pointers or none");
  hipStream_t st = (hipStream_t)stream;
  if (y_cb == nullptr) {
    const int64_t n = (int64_t)N * C * HW;
    const int64_t n4 = (join_aligned16(a) && join_aligned16(b) && join_aligned16(y)) ? n / 4 : 0;
    int64_t blocks = ceil_div64(n4 > 0 ? n4 : n, 256 * 4);
    if (blocks < 1) blocks = 1;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(join_plain_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, a_bound, b, b_bound, y, y_bound, n4, n);
    MCD_LAUNCH_CHECK("stage_join");
    return 0;
  }
  MCD_REQUIRE(mcd_math_known(math), "stage_join: unknown math %d", math);
  math = mcd_storage_math(math);  // F16X1 shares F16X3's storage
  if (int rc = cb_check("stage_join", math, bounds ? a_bound : nullptr, N, C, HW)) return rc;
  if (math == MCDSEG_MATH_F16X3)
    join_cb_launch<SplitF16x3>(a, a_bound, b, b_bound, y, y_cb, y_bound, N, C, HW, st);
  else
    join_cb_launch<SplitBf16x6>(a, a_bound, b, b_bound, y, y_cb, y_bound, N, C, HW, st);
  MCD_LAUNCH_CHECK("stage_join");
  return 0;
}
