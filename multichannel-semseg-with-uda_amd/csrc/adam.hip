// Adam on flat fp32 buffers (torch.optim.Adam as configured by models/model_util.py:293-294: L2 weight decay added to the
// gradient, no amsgrad, no maximize, no decoupled decay).  One streaming pass: reads p, g, m, v and writes p, m, v (28 B per
// parameter).  The bias corrections arrive folded into two scalars (lr / (1 - b1^t) and 1 / sqrt(1 - b2^t), formed by the host in
// double precision), so the kernel reads no step counter; grad_scale folds the 1/world_size of the data-parallel all-reduce
// into the same pass.
#include <cmath>

#include "common.h"

namespace {

struct AdamArgs {
  float step;  // lr / (1 - b1^t)
  float omb1;  // 1 - b1
  float b2;
  float omb2;  // 1 - b2
  float isb2;  // 1 / sqrt(1 - b2^t)
  float eps;
  float wd;
  float gs;
};

__device__ __forceinline__ void adam_one(float& p, const float g, float& m, float& v, const AdamArgs& a) {
  const float d = fmaf(a.wd, p, g * a.gs);
  // torch's lerp(m, d, 1 - b1), in its own two forms: each is exact at its end of the weight's range
  m = a.omb1 < 0.5f ? fmaf(a.omb1, d - m, m) : fmaf(-(1.f - a.omb1), d - m, d);
  v = fmaf(a.omb2 * d, d, a.b2 * v);
  p = fmaf(-a.step, m / fmaf(sqrtf(v), a.isb2, a.eps), p);
}

// The float4 body is software-pipelined one iteration deep: the four loads of the NEXT iteration are issued in front of the three
// stores of this one, so that the wait in front of the arithmetic is a counted one (the stores may still be in flight) and not
// a drain of the whole queue between one iteration's stores and the next one's loads.
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n4, int64_t n, AdamArgs a) {
  float4* p4 = reinterpret_cast<float4*>(p);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* m4 = reinterpret_cast<float4*>(m);
  float4* v4 = reinterpret_cast<float4*>(v);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n4) {
    float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];
    for (;;) {
      const int64_t j = i + stride;
      const bool more = j < n4;
      float4 pn = pp, gn = gg, mn = mm, vn = vv;
      if (more) {
        pn = p4[j];
        gn = g4[j];
        mn = m4[j];
        vn = v4[j];
      }
      adam_one(pp.x, gg.x, mm.x, vv.x, a);
      adam_one(pp.y, gg.y, mm.y, vv.y, a);
      adam_one(pp.z, gg.z, mm.z, vv.z, a);
      adam_one(pp.w, gg.w, mm.w, vv.w, a);
      m4[i] = mm;
      v4[i] = vv;
      p4[i] = pp;
      if (!more) break;
      pp = pn, gg = gn, mm = mn, vv = vn;
      i = j;
    }
  }
  for (i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    float pp = p[i], mm = m[i], vv = v[i];
    adam_one(pp, g[i], mm, vv, a);
    m[i] = mm;
    v[i] = vv;
    p[i] = pp;
  }
}

// 1 - beta in double precision.  A float beta near 1 carries 1 - beta to a relative 6e-8 / (1 - beta) only (5e-5 for 0.999), which
// would go straight into exp_avg_sq; a beta written with up to six decimals (0.9, 0.5, 0.999, ...) is the only such decimal its
// float stands for, so it is taken as written.  Any other value is taken as the float it is.
double one_minus(float beta) {
  const double b = (double)beta, r = std::nearbyint(b * 1e6) / 1e6;
  return 1.0 - ((float)r == beta ? r : b);
}

}  // namespace

extern "C" int mcdseg_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr_over_bc1, float beta1, float beta2,
                                float inv_sqrt_bc2, float eps, float weight_decay, float grad_scale, void* stream) {
  MCD_REQUIRE(p && g && m && v && n >= 0, "adam_flat: bad arguments");
  MCD_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, "adam_flat: betas outside [0, 1) or negative eps");
  if (n == 0) return 0;
  const bool al = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                    reinterpret_cast<uintptr_t>(v)) & 15) == 0;
  const int64_t n4 = al ? n / 4 : 0;
  int64_t blocks = ceil_div64(n4 > 0 ? n4 : n, 256);
  if (blocks > 2048) blocks = 2048;
  const AdamArgs a = {lr_over_bc1, (float)one_minus(beta1), beta2, (float)one_minus(beta2), inv_sqrt_bc2, eps, weight_decay, grad_scale};
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n4, n, a);
  MCD_LAUNCH_CHECK("adam_flat");
  return 0;
}
