// Late-fusion operators of the MFNet classifiers other than the plain sum (models/fusion.py:6-50) and the loss that
// goes with the gated ones (ProbCrossEntropyLoss2d, loss.py:16-30).  All HBM-bound single passes.
//
//  gate_mix      out = x1*s + x2*(1-s),  s = sigmoid(g)                         (GateFusion.forward, fusion.py:19-22)
//                dx1 = dy*s ; dx2 = dy*(1-s) ; dg = dy*(x1-x2)*s*(1-s)
//                any element count > 0 and any 4-byte-aligned pointers: float4 body + scalar tail when every pointer of the
//                call is 16-byte aligned, all scalar otherwise; the same bits either way
//  softmax_ch    y = softmax over the channel axis of NCHW                      (F.softmax, fusion.py:13-15)
//                dx = y*(dy - sum_c dy*y)
//  prob_nll      loss = sum_i w[y_i]*(-log p[y_i]) / sum_i w[y_i]                (NLLLoss2d(log(p)), loss.py:30)
//                dp[n,c,i] = (c == y_i) ? -w[y_i] / (p[y_i] * sum w) : 0
#include "block_reduce.h"

namespace {


// float4 body over [0, 4*n4), scalar tail over [4*n4, n); n4 = 0 (all scalar) when a pointer is off the 16-byte grid.  Body and
// tail evaluate one expression per element, so a value does not depend on which of the two computed it.
__device__ __forceinline__ float gate_sigmoid(float g) { return 1.0f / (1.0f + expf(-g)); }
__device__ __forceinline__ float gate_mix_one(float a, float b, float g) {
  const float s = gate_sigmoid(g);
  return a * s + b * (1.0f - s);
}

__global__ __launch_bounds__(256) void gate_mix_fwd_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                           const float* __restrict__ g, float* __restrict__ out, int64_t n4,
                                                           int64_t n) {
  const float4* a4 = reinterpret_cast<const float4*>(x1);
  const float4* b4 = reinterpret_cast<const float4*>(x2);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* o4 = reinterpret_cast<float4*>(out);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 a = a4[i], b = b4[i], gg = g4[i];
    float4 o;
    o.x = gate_mix_one(a.x, b.x, gg.x);
    o.y = gate_mix_one(a.y, b.y, gg.y);
    o.z = gate_mix_one(a.z, b.z, gg.z);
    o.w = gate_mix_one(a.w, b.w, gg.w);
    o4[i] = o;
  }
  for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = gate_mix_one(x1[i], x2[i], g[i]);
}

__device__ __forceinline__ void gate_mix_bwd_one(float d, float a, float b, float g, float& o1, float& o2, float& og) {
  const float s = gate_sigmoid(g);
  o1 = d * s;
  o2 = d * (1.0f - s);
  og = d * (a - b) * (s * (1.0f - s));
}

__global__ __launch_bounds__(256) void gate_mix_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x1,
                                                           const float* __restrict__ x2, const float* __restrict__ g,
                                                           float* __restrict__ dx1, float* __restrict__ dx2,
                                                           float* __restrict__ dg, int64_t n4, int64_t n) {
  const float4* d4 = reinterpret_cast<const float4*>(dy);
  const float4* a4 = reinterpret_cast<const float4*>(x1);
  const float4* b4 = reinterpret_cast<const float4*>(x2);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* o14 = reinterpret_cast<float4*>(dx1);
  float4* o24 = reinterpret_cast<float4*>(dx2);
  float4* og4 = reinterpret_cast<float4*>(dg);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 d = d4[i], a = a4[i], b = b4[i], gg = g4[i];
    float4 o1, o2, og;
    gate_mix_bwd_one(d.x, a.x, b.x, gg.x, o1.x, o2.x, og.x);
    gate_mix_bwd_one(d.y, a.y, b.y, gg.y, o1.y, o2.y, og.y);
    gate_mix_bwd_one(d.z, a.z, b.z, gg.z, o1.z, o2.z, og.z);
    gate_mix_bwd_one(d.w, a.w, b.w, gg.w, o1.w, o2.w, og.w);
    o14[i] = o1;
    o24[i] = o2;
    og4[i] = og;
  }
  for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    gate_mix_bwd_one(dy[i], x1[i], x2[i], g[i], dx1[i], dx2[i], dg[i]);
}

// one lane = one pixel, channels walked with stride HW (every per-channel access of a wave is a contiguous 256-B run)
template <int NCMAX>
__global__ __launch_bounds__(256) void softmax_ch_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int HW) {
  const int n = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= HW) return;
  const float* xi = x + (size_t)n * C * HW + p;
  float* yi = y + (size_t)n * C * HW + p;
  float v[NCMAX];
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < NCMAX; ++c)
    if (c < C) {
      v[c] = xi[(size_t)c * HW];
      m = fmaxf(m, v[c]);
    }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NCMAX; ++c)
    if (c < C) {
      v[c] = expf(v[c] - m);
      s += v[c];
    }
  const float inv = 1.0f / s;
#pragma unroll
  for (int c = 0; c < NCMAX; ++c)
    if (c < C) yi[(size_t)c * HW] = v[c] * inv;
}

template <int NCMAX>
__global__ __launch_bounds__(256) void softmax_ch_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                             float* __restrict__ dx, int C, int HW) {
  const int n = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= HW) return;
  const size_t base = (size_t)n * C * HW + p;
  float yy[NCMAX], dd[NCMAX];
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < NCMAX; ++c)
    if (c < C) {
      yy[c] = y[base + (size_t)c * HW];
      dd[c] = dy[base + (size_t)c * HW];
      dot += yy[c] * dd[c];
    }
#pragma unroll
  for (int c = 0; c < NCMAX; ++c)
    if (c < C) dx[base + (size_t)c * HW] = yy[c] * (dd[c] - dot);
}

// pass 1: per-block partial (sum w*(-log p), sum w) in fp64
__global__ __launch_bounds__(256) void prob_nll_partial_kernel(const float* __restrict__ p, const int64_t* __restrict__ labels,
                                                               const float* __restrict__ weight, int64_t ignore_index, int C,
                                                               int HW, int64_t npix, double* __restrict__ part) {
  double ls = 0.0, ws = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t y = labels[i];
    if (y == ignore_index || y < 0 || y >= C) continue;
    const int64_t n = i / HW;
    const float w = weight ? weight[y] : 1.0f;
    const float pv = p[((size_t)n * C + y) * HW + (i - n * HW)];
    ls += (double)(w * -logf(pv));
    ws += (double)w;
  }
  __shared__ double sh[2][4];
  double v[2] = {ls, ws};
  block_gather(v, sh);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = tree_total<4>(sh[0]);
    part[2 * blockIdx.x + 1] = tree_total<4>(sh[1]);
  }
}

// Adds the partial rows serially, in one thread: an order of its own, not partials_total's (block_reduce.h) -- routing it through the
// helper would change the bits of the loss.
__global__ void prob_nll_finalize_kernel(const double* __restrict__ part, int blocks, float* __restrict__ loss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double ls = 0.0, ws = 0.0;
  for (int b = 0; b < blocks; ++b) {
    ls += part[2 * b];
    ws += part[2 * b + 1];
  }
  loss[0] = (float)(ls / ws);  // size_average=True
  loss[1] = (float)ls;         // size_average=False
  loss[2] = (float)ws;
}

// pass 2: dense gradient (zeros off the label channel), scaled by 1/sum w read from the device
__global__ __launch_bounds__(256) void prob_nll_grad_kernel(const float* __restrict__ p, const int64_t* __restrict__ labels,
                                                            const float* __restrict__ weight, int64_t ignore_index,
                                                            const float* __restrict__ loss, int size_average, int C, int HW,
                                                            float* __restrict__ grad) {
  const int n = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= HW) return;
  const int64_t y = labels[(size_t)n * HW + i];
  const bool live = !(y == ignore_index || y < 0 || y >= C);
  const float scale = size_average ? 1.0f / loss[2] : 1.0f;
  const size_t base = (size_t)n * C * HW + i;
  for (int c = 0; c < C; ++c) {
    float gv = 0.f;
    if (live && c == (int)y) gv = -(weight ? weight[y] : 1.0f) * scale / p[base + (size_t)c * HW];
    grad[base + (size_t)c * HW] = gv;
  }
}

int stream_blocks(int64_t n) { return ceil_div64(n, 256 * 4, 4096); }

}  // namespace

extern "C" int mcdseg_gate_mix_fwd(const float* x1, const float* x2, const float* g, float* out, int64_t n, void* stream) {
  MCD_REQUIRE(x1 && x2 && g && out, "gate_mix_fwd: null pointer");
  MCD_REQUIRE(n > 0, "gate_mix_fwd: element count must be positive (got %lld)", (long long)n);
  const bool al = ((reinterpret_cast<uintptr_t>(x1) | reinterpret_cast<uintptr_t>(x2) | reinterpret_cast<uintptr_t>(g) |
                    reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int64_t n4 = al ? n / 4 : 0;
  hipLaunchKernelGGL(gate_mix_fwd_kernel, dim3(stream_blocks(n4 > 0 ? n4 : n)), dim3(256), 0, (hipStream_t)stream, x1, x2, g, out,
                     n4, n);
  MCD_LAUNCH_CHECK("gate_mix_fwd");
  return 0;
}

extern "C" int mcdseg_gate_mix_bwd(const float* dy, const float* x1, const float* x2, const float* g, float* dx1, float* dx2,
                                   float* dg, int64_t n, void* stream) {
  MCD_REQUIRE(dy && x1 && x2 && g && dx1 && dx2 && dg, "gate_mix_bwd: null pointer");
  MCD_REQUIRE(n > 0, "gate_mix_bwd: element count must be positive (got %lld)", (long long)n);
  const bool al = ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(x1) | reinterpret_cast<uintptr_t>(x2) |
                    reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(dx1) | reinterpret_cast<uintptr_t>(dx2) |
                    reinterpret_cast<uintptr_t>(dg)) & 15) == 0;
  const int64_t n4 = al ? n / 4 : 0;
  hipLaunchKernelGGL(gate_mix_bwd_kernel, dim3(stream_blocks(n4 > 0 ? n4 : n)), dim3(256), 0, (hipStream_t)stream, dy, x1, x2, g,
                     dx1, dx2, dg, n4, n);
  MCD_LAUNCH_CHECK("gate_mix_bwd");
  return 0;
}

extern "C" int mcdseg_softmax_ch_fwd(const float* x, float* y, int32_t N, int32_t C, int32_t HW, void* stream) {
  MCD_REQUIRE(x && y, "softmax_ch_fwd: null pointer");
  MCD_REQUIRE(N > 0 && N <= 65535 && C > 0 && C <= 64 && HW > 0, "softmax_ch_fwd: bad dims (C <= 64)");
  dim3 grid(ceil_div(HW, 256), N);
  if (C <= 24)
    hipLaunchKernelGGL(softmax_ch_fwd_kernel<24>, grid, dim3(256), 0, (hipStream_t)stream, x, y, C, HW);
  else if (C <= 48)
    hipLaunchKernelGGL(softmax_ch_fwd_kernel<48>, grid, dim3(256), 0, (hipStream_t)stream, x, y, C, HW);
  else
    hipLaunchKernelGGL(softmax_ch_fwd_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, x, y, C, HW);
  MCD_LAUNCH_CHECK("softmax_ch_fwd");
  return 0;
}

extern "C" int mcdseg_softmax_ch_bwd(const float* dy, const float* y, float* dx, int32_t N, int32_t C, int32_t HW, void* stream) {
  MCD_REQUIRE(dy && y && dx, "softmax_ch_bwd: null pointer");
  MCD_REQUIRE(N > 0 && N <= 65535 && C > 0 && C <= 64 && HW > 0, "softmax_ch_bwd: bad dims (C <= 64)");
  dim3 grid(ceil_div(HW, 256), N);
  if (C <= 24)
    hipLaunchKernelGGL(softmax_ch_bwd_kernel<24>, grid, dim3(256), 0, (hipStream_t)stream, dy, y, dx, C, HW);
  else if (C <= 48)
    hipLaunchKernelGGL(softmax_ch_bwd_kernel<48>, grid, dim3(256), 0, (hipStream_t)stream, dy, y, dx, C, HW);
  else
    hipLaunchKernelGGL(softmax_ch_bwd_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, dy, y, dx, C, HW);
  MCD_LAUNCH_CHECK("softmax_ch_bwd");
  return 0;
}

extern "C" size_t mcdseg_prob_nll_workspace_bytes(int32_t N, int32_t HW) {
  if (N <= 0 || HW <= 0) return 0;
  return (size_t)stream_blocks((int64_t)N * HW) * 2 * sizeof(double);
}

extern "C" int mcdseg_prob_nll(const float* p, const int64_t* labels, const float* weight, int64_t ignore_index,
                               int32_t size_average, float* grad, float* loss, int32_t N, int32_t C, int32_t HW, void* workspace,
                               size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(p && labels && loss && workspace, "prob_nll: null pointer");
  MCD_REQUIRE(N > 0 && N <= 65535 && C > 0 && HW > 0, "prob_nll: bad dims");
  const int64_t npix = (int64_t)N * HW;
  const int blocks = stream_blocks(npix);
  MCD_REQUIRE(workspace_bytes >= (size_t)blocks * 2 * sizeof(double), "prob_nll: workspace too small");
  MCD_REQUIRE(((uintptr_t)workspace & 7) == 0, "prob_nll: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(prob_nll_partial_kernel, dim3(blocks), dim3(256), 0, st, p, labels, weight, ignore_index, C, HW, npix,
                     (double*)workspace);
  MCD_LAUNCH_CHECK("prob_nll_partial");
  hipLaunchKernelGGL(prob_nll_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)workspace, blocks, loss);
  MCD_LAUNCH_CHECK("prob_nll_finalize");
  if (grad) {
    hipLaunchKernelGGL(prob_nll_grad_kernel, dim3(ceil_div(HW, 256), N), dim3(256), 0, st, p, labels, weight, ignore_index,
                       (const float*)loss, size_average, C, HW, grad);
    MCD_LAUNCH_CHECK("prob_nll_grad");
  }
  return 0;
}
