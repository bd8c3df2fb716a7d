// The three operators of the U-Net generator and classifiers (models/unet.py of the reference: UNetBase :122-171, UNetUp :29-43,
// UNetClassifier :174-199) that the library had no kernel for:
//
//   maxpool2     nn.MaxPool2d(kernel_size=2)                       y[n,c,i,j] = max of the 2x2 window; backward recomputes the arg-max from x
//   deconv2x2    nn.ConvTranspose2d(Cin, Cout, kernel_size=2, stride=2)
//                                                                 y[n,co,2i+a,2j+b] = bias[co] + sum_ci x[n,ci,i,j] * w[ci,co,a,b]
//   relu         the nn.ReLU behind the BatchNorm-less convolutions of UNetUp
//
// All fp32 NCHW.  The pool and the ReLU also write, on request, the pre-split companion of what they write -- the layout
// [piece][N][C/8][HW][8 x 16 bit], bitwise what mcdseg_split_cb(y, y_bound) writes (operand_scale / split_store of split.h) -- with
// y_bound = x_bound: |max of a window| and |max(x, 0)| cannot exceed the bound of x, so nothing is reduced.
//
// The pool's tie and NaN rule is torch's CPU max_pool2d: the window is walked (0,0), (0,1), (1,0), (1,1) from -inf, and a value takes
// over when it is GREATER than the best so far or is a NaN.  So the first of equal values wins (-0 against +0 included: neither is
// greater), a NaN wins over everything before it and loses to a later NaN only, and a window of four -inf keeps index 0.
//
// The up-convolution is plain fp32 FMA arithmetic in a fixed order (bias first, then ci ascending; the data gradient co ascending and
// within it the taps (0,0), (0,1), (1,0), (1,1)): a thread owns one INPUT pixel and a tile of channels, the weights of a tile are
// wave-uniform (scalar loads).  y and dy are addressed through a batch stride and a channel offset, so the operator writes and reads
// a channel slice of the concatenation buffer.  The weight and bias gradients are summed in two stages: fp32 per thread and wave,
// fp64 block partials in the workspace, one small finalize kernel -- no atomics, the same bits every run.
#include "split.h"

namespace {

bool unet_aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// ---------------------------------------------------------------------------------------------------------------- 2x2 max pooling
__device__ __forceinline__ void pool_take(float v, int k, float& best, int& at) {
  if (v > best || v != v) {
    best = v;
    at = k;
  }
}

// the window (a b / c d) by torch's rule; `at` = 0..3
__device__ __forceinline__ float pool_window(float a, float b, float c, float d, int& at) {
  float best = -INFINITY;
  at = 0;
  pool_take(a, 0, best, at);
  pool_take(b, 1, best, at);
  pool_take(c, 2, best, at);
  pool_take(d, 3, best, at);
  return best;
}

// PIX output pixels of one plane (base: the plane's first input element) at output row oi, column oj
template <int PIX>
__device__ __forceinline__ void pool_load(const float* __restrict__ plane, int W, int oi, int oj, float (&out)[PIX]) {
  const float* r0 = plane + (size_t)(2 * oi) * W + 2 * oj;
  const float* r1 = r0 + W;
  int at;
  if constexpr (PIX == 2) {  // (W % 4 == 0, oj even and a 16-byte aligned tensor: both reads are aligned)
    const float4 p = *reinterpret_cast<const float4*>(r0);
    const float4 q = *reinterpret_cast<const float4*>(r1);
    out[0] = pool_window(p.x, p.y, q.x, q.y, at);
    out[1] = pool_window(p.z, p.w, q.z, q.w, at);
  } else {
    out[0] = pool_window(r0[0], r0[1], r1[0], r1[1], at);
  }
}

// y alone: any channel count; one thread = PIX adjacent output pixels
template <int PIX>
__global__ __launch_bounds__(256) void maxpool2_plain_kernel(const float* __restrict__ x, const float* __restrict__ x_bound,
                                                             float* __restrict__ y, float* __restrict__ y_bound, int64_t units, int H,
                                                             int W) {
  if (y_bound != nullptr && blockIdx.x == 0 && threadIdx.x == 0) y_bound[0] = x_bound[0];
  const int Ho = H >> 1, Wo = W >> 1, Wq = Wo / PIX;
  for (int64_t u = blockIdx.x * (int64_t)256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
    const int64_t row = u / Wq;  // plane * Ho + oi
    const int oj = (int)(u - row * Wq) * PIX;
    const int64_t plane = row / Ho;
    const int oi = (int)(row - plane * Ho);
    float v[PIX];
    pool_load<PIX>(x + (size_t)plane * H * W, W, oi, oj, v);
    float* out = y + (size_t)row * Wo + oj;
    if constexpr (PIX == 2)
      *reinterpret_cast<float2*>(out) = make_float2(v[0], v[1]);
    else
      out[0] = v[0];
  }
}

// y and its companion: one thread = 8 channels of PIX adjacent output pixels; grid y = n * C/8 + g
template <class P, int PIX>
__global__ __launch_bounds__(256) void maxpool2_cb_kernel(const float* __restrict__ x, const float* __restrict__ x_bound,
                                                          float* __restrict__ y, typename P::elem* __restrict__ cb,
                                                          float* __restrict__ y_bound, int N, int C, int H, int W) {
  const int C8 = C >> 3;
  const int ng = blockIdx.y;
  const int g = ng % C8;
  const int n = ng / C8;
  float bound = 0.f;
  if (x_bound != nullptr) {  // (always there for a scaled policy: cb_check)
    bound = x_bound[0];
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) y_bound[0] = bound;
  }
  const float inv_scale = 1.f / operand_scale<P>(&bound);
  const int Ho = H >> 1, Wo = W >> 1, Wq = Wo / PIX;
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= Ho * Wq) return;
  const int oi = u / Wq;
  const int oj = (u - oi * Wq) * PIX;
  const size_t HWo = (size_t)Ho * Wo;
  const size_t first = (size_t)n * C + 8 * g;  // the first of the 8 planes
  float v[PIX][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float w[PIX];
    pool_load<PIX>(x + (first + e) * (size_t)H * W, W, oi, oj, w);
    float* out = y + (first + e) * HWo + (size_t)oi * Wo + oj;
    if constexpr (PIX == 2)
      *reinterpret_cast<float2*>(out) = make_float2(w[0], w[1]);
    else
      out[0] = w[0];
#pragma unroll
    for (int q = 0; q < PIX; ++q) v[q][e] = w[q];
  }
#pragma unroll
  for (int q = 0; q < PIX; ++q) split_store<P>(v[q], inv_scale, cb, (size_t)N * C * HWo, (size_t)ng * HWo + (size_t)oi * Wo + oj + q);
}

// dx: dy at the window's arg-max, 0 at the other three; every element of dx is written (H and W are even)
template <int PIX>
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           float* __restrict__ dx, int64_t units, int H, int W) {
  const int Ho = H >> 1, Wo = W >> 1, Wq = Wo / PIX;
  for (int64_t u = blockIdx.x * (int64_t)256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
    const int64_t row = u / Wq;
    const int oj = (int)(u - row * Wq) * PIX;
    const int64_t plane = row / Ho;
    const int oi = (int)(row - plane * Ho);
    const size_t in = (size_t)plane * H * W + (size_t)(2 * oi) * W + 2 * oj;
    const float* g = dy + (size_t)row * Wo + oj;
    int at;
    if constexpr (PIX == 2) {
      const float4 p = *reinterpret_cast<const float4*>(x + in);
      const float4 q = *reinterpret_cast<const float4*>(x + in + W);
      const float2 d = *reinterpret_cast<const float2*>(g);
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
      (void)pool_window(p.x, p.y, q.x, q.y, at);
      a.x = at == 0 ? d.x : 0.f;
      a.y = at == 1 ? d.x : 0.f;
      b.x = at == 2 ? d.x : 0.f;
      b.y = at == 3 ? d.x : 0.f;
      (void)pool_window(p.z, p.w, q.z, q.w, at);
      a.z = at == 0 ? d.y : 0.f;
      a.w = at == 1 ? d.y : 0.f;
      b.z = at == 2 ? d.y : 0.f;
      b.w = at == 3 ? d.y : 0.f;
      *reinterpret_cast<float4*>(dx + in) = a;
      *reinterpret_cast<float4*>(dx + in + W) = b;
    } else {
      const float d = g[0];
      (void)pool_window(x[in], x[in + 1], x[in + W], x[in + W + 1], at);
      dx[in] = at == 0 ? d : 0.f;
      dx[in + 1] = at == 1 ? d : 0.f;
      dx[in + W] = at == 2 ? d : 0.f;
      dx[in + W + 1] = at == 3 ? d : 0.f;
    }
  }
}

unsigned flat_blocks(int64_t units, int per_block) {
  int64_t blocks = ceil_div64(units, per_block);
  if (blocks < 1) blocks = 1;
  if (blocks > 65536) blocks = 65536;
  return (unsigned)blocks;
}

template <class P>
void maxpool2_cb_launch(const float* x, const float* x_bound, float* y, void* y_cb, float* y_bound, int N, int C, int H, int W, bool vec,
                        hipStream_t st) {
  typedef typename P::elem E;
  const int units = (H / 2) * ((W / 2) / (vec ? 2 : 1));
  const dim3 grid(ceil_div(units, 256), N * (C / 8));
  if (vec)
    hipLaunchKernelGGL((maxpool2_cb_kernel<P, 2>), grid, dim3(256), 0, st, x, x_bound, y, (E*)y_cb, y_bound, N, C, H, W);
  else
    hipLaunchKernelGGL((maxpool2_cb_kernel<P, 1>), grid, dim3(256), 0, st, x, x_bound, y, (E*)y_cb, y_bound, N, C, H, W);
}

// ---------------------------------------------------------------------------------------------------------------- ReLU
// torch's rule: a negative value becomes +0, everything else (-0 and NaN included) passes
__device__ __forceinline__ float relu_of(float v) { return v < 0.f ? 0.f : v; }

// (x and y may be the same tensor: every thread reads its own elements before it writes them)
template <class P, int PIX>
__global__ __launch_bounds__(256) void relu_cb_kernel(const float* x, const float* __restrict__ x_bound, float* y,
                                                      typename P::elem* __restrict__ cb, float* y_bound, int N, int C, int HW) {
  const int C8 = C >> 3;
  const int ng = blockIdx.y;
  const int g = ng % C8;
  const int n = ng / C8;
  float bound = 0.f;
  if (x_bound != nullptr) {
    bound = x_bound[0];
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) y_bound[0] = bound;
  }
  const float inv_scale = 1.f / operand_scale<P>(&bound);
  const int pix = (blockIdx.x * 256 + threadIdx.x) * PIX;
  if (pix >= HW) return;  // (PIX == 4: HW % 4 == 0, a quad is inside or outside as a whole)
  const size_t base = ((size_t)n * C + 8 * g) * HW + pix;
  if constexpr (PIX == 1) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = relu_of(x[base + (size_t)e * HW]);
#pragma unroll
    for (int e = 0; e < 8; ++e) y[base + (size_t)e * HW] = v[e];
    split_store<P>(v, inv_scale, cb, (size_t)N * C * HW, (size_t)ng * HW + pix);
  } else {
    float4 in[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) in[e] = *reinterpret_cast<const float4*>(x + base + (size_t)e * HW);
    float v[4][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float4 s = make_float4(relu_of(in[e].x), relu_of(in[e].y), relu_of(in[e].z), relu_of(in[e].w));
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

// y alone: float4 body + scalar tail when the pointers allow (n4 = n / 4), all scalar otherwise (n4 = 0)
__global__ __launch_bounds__(256) void relu_plain_kernel(const float* x, const float* __restrict__ x_bound, float* y, float* y_bound,
                                                         int64_t n4, int64_t n) {
  if (y_bound != nullptr && blockIdx.x == 0 && threadIdx.x == 0) y_bound[0] = x_bound[0];
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float4* y4 = reinterpret_cast<float4*>(y);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 p = x4[i];
    y4[i] = make_float4(relu_of(p.x), relu_of(p.y), relu_of(p.z), relu_of(p.w));
  }
  for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) y[i] = relu_of(x[i]);
}

// dx = y > 0 ? dy : 0 (dx may be dy)
__global__ __launch_bounds__(256) void relu_bwd_kernel(const float* __restrict__ y, const float* dy, float* dx, int64_t n4, int64_t n) {
  const float4* y4 = reinterpret_cast<const float4*>(y);
  const float4* g4 = reinterpret_cast<const float4*>(dy);
  float4* d4 = reinterpret_cast<float4*>(dx);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 p = y4[i], q = g4[i];
    d4[i] = make_float4(p.x > 0.f ? q.x : 0.f, p.y > 0.f ? q.y : 0.f, p.z > 0.f ? q.z : 0.f, p.w > 0.f ? q.w : 0.f);
  }
  for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dx[i] = y[i] > 0.f ? dy[i] : 0.f;
}

template <class P>
void relu_cb_launch(const float* x, const float* x_bound, float* y, void* y_cb, float* y_bound, int N, int C, int HW, hipStream_t st) {
  typedef typename P::elem E;
  const bool vec = (HW % 4 == 0) && unet_aligned(x, 16) && unet_aligned(y, 16);
  const dim3 grid(ceil_div(HW, vec ? 1024 : 256), N * (C / 8));
  if (vec)
    hipLaunchKernelGGL((relu_cb_kernel<P, 4>), grid, dim3(256), 0, st, x, x_bound, y, (E*)y_cb, y_bound, N, C, HW);
  else
    hipLaunchKernelGGL((relu_cb_kernel<P, 1>), grid, dim3(256), 0, st, x, x_bound, y, (E*)y_cb, y_bound, N, C, HW);
}

// ---------------------------------------------------------------------------------------------------------------- 2x2 stride-2 up-convolution
constexpr int UP_COT = 8;   // output channels per thread of the forward pass
constexpr int UP_CIT = 8;   // input channels per thread of the data gradient
constexpr int UW_CIT = 8;   // the weight gradient's tile: 8 input x 4 output channels x 4 taps = 128 sums per thread
constexpr int UW_COT = 4;
constexpr int UW_SUMS = UW_CIT * UW_COT * 4 + UW_COT;  // ... and the tile's bias sums

// where a slice tensor lives: element (n, c, r, s) of the [.., 2H, 2W] planes is base[n * batch_stride + (c_off + c) * 4HW + r * 2W + s]
struct UpSlice {
  int64_t batch_stride;
  int c_off;
};

template <bool VEC>
__device__ __forceinline__ void up_load4(const float* p, int W2, float (&d)[4]) {
  if constexpr (VEC) {
    const float2 a = *reinterpret_cast<const float2*>(p);
    const float2 b = *reinterpret_cast<const float2*>(p + W2);
    d[0] = a.x, d[1] = a.y, d[2] = b.x, d[3] = b.y;
  } else {
    d[0] = p[0], d[1] = p[1], d[2] = p[W2], d[3] = p[W2 + 1];
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void deconv2x2_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ y, UpSlice ys, int Cin,
                                                            int Cout, int H, int W) {
  const int HW = H * W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int co0 = blockIdx.y * UP_COT;
  const int n = blockIdx.z;
  if (p >= HW) return;
  int wo[UP_COT];  // the tile's channels, the ragged tail clamped (computed, not stored); wave-uniform
  float acc[UP_COT][4];
#pragma unroll
  for (int c = 0; c < UP_COT; ++c) {
    const int co = min(co0 + c, Cout - 1);
    wo[c] = co * 4;
    const float b = bias != nullptr ? bias[co] : 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[c][t] = b;
  }
  const float* xp = x + (size_t)n * Cin * HW + p;
  for (int ci = 0; ci < Cin; ++ci) {
    const float xv = xp[(size_t)ci * HW];
    const float* wp = w + (size_t)ci * Cout * 4;
#pragma unroll
    for (int c = 0; c < UP_COT; ++c)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[c][t] = __builtin_fmaf(xv, wp[wo[c] + t], acc[c][t]);
  }
  const int i = p / W, j = p - i * W, W2 = 2 * W;
  float* yp = y + (size_t)n * ys.batch_stride + ((size_t)(ys.c_off + co0) * 4) * HW + (size_t)(2 * i) * W2 + 2 * j;
#pragma unroll
  for (int c = 0; c < UP_COT; ++c) {
    if (co0 + c >= Cout) break;
    float* q = yp + (size_t)c * 4 * HW;
    if constexpr (VEC) {
      *reinterpret_cast<float2*>(q) = make_float2(acc[c][0], acc[c][1]);
      *reinterpret_cast<float2*>(q + W2) = make_float2(acc[c][2], acc[c][3]);
    } else {
      q[0] = acc[c][0], q[1] = acc[c][1], q[W2] = acc[c][2], q[W2 + 1] = acc[c][3];
    }
  }
}

// dx[n,ci,i,j] = sum_co sum_ab dy[n,co,2i+a,2j+b] * w[ci,co,a,b]
template <bool VEC>
__global__ __launch_bounds__(256) void deconv2x2_bwd_data_kernel(const float* __restrict__ dy, UpSlice ds, const float* __restrict__ w,
                                                                 float* __restrict__ dx, int Cin, int Cout, int H, int W) {
  const int HW = H * W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int ci0 = blockIdx.y * UP_CIT;
  const int n = blockIdx.z;
  if (p >= HW) return;
  size_t wo[UP_CIT];
  float acc[UP_CIT];
#pragma unroll
  for (int c = 0; c < UP_CIT; ++c) {
    wo[c] = (size_t)min(ci0 + c, Cin - 1) * Cout * 4;
    acc[c] = 0.f;
  }
  const int i = p / W, j = p - i * W, W2 = 2 * W;
  const float* gp = dy + (size_t)n * ds.batch_stride + ((size_t)ds.c_off * 4) * HW + (size_t)(2 * i) * W2 + 2 * j;
  for (int co = 0; co < Cout; ++co) {
    float d[4];
    up_load4<VEC>(gp + (size_t)co * 4 * HW, W2, d);
#pragma unroll
    for (int c = 0; c < UP_CIT; ++c) {
      const float* wp = w + wo[c] + co * 4;
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[c] = __builtin_fmaf(d[t], wp[t], acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < UP_CIT; ++c)
    if (ci0 + c < Cin) dx[((size_t)n * Cin + ci0 + c) * HW + p] = acc[c];
}

// how many pixel chunks the weight gradient cuts N * HW into: enough workgroups for the chip, at most 256 partials per sum
int up_wgrad_chunks(int N, int Cin, int Cout, int H, int W) {
  const int64_t pixels = (int64_t)N * H * W;
  const int64_t tiles = (int64_t)ceil_div(Cin, UW_CIT) * ceil_div(Cout, UW_COT);
  int64_t chunks = ceil_div64(2048, tiles);
  const int64_t most = ceil_div64(pixels, 256);
  if (chunks > most) chunks = most;
  if (chunks > 256) chunks = 256;
  if (chunks < 1) chunks = 1;
  return (int)chunks;
}

// stage 1: workgroup (chunk, tile) sums its tile's products over its pixels; part[chunk][Cin * Cout * 4 + Cout] in fp64
template <bool VEC>
__global__ __launch_bounds__(256) void deconv2x2_bwd_weight_kernel(const float* __restrict__ x, const float* __restrict__ dy, UpSlice ds,
                                                                   double* __restrict__ part, int64_t pixels, int64_t per_chunk, int Cin,
                                                                   int Cout, int H, int W) {
  __shared__ double red[4][UW_SUMS];
  const int HW = H * W, W2 = 2 * W;
  const int tiles_co = (Cout + UW_COT - 1) / UW_COT;
  const int ci0 = (blockIdx.y / tiles_co) * UW_CIT;
  const int co0 = (blockIdx.y % tiles_co) * UW_COT;
  size_t xo[UW_CIT], go[UW_COT];
#pragma unroll
  for (int c = 0; c < UW_CIT; ++c) xo[c] = (size_t)min(ci0 + c, Cin - 1) * HW;
#pragma unroll
  for (int o = 0; o < UW_COT; ++o) go[o] = (size_t)(ds.c_off + min(co0 + o, Cout - 1)) * 4 * HW;
  float acc[UW_CIT][UW_COT][4], sb[UW_COT];
#pragma unroll
  for (int o = 0; o < UW_COT; ++o) {
    sb[o] = 0.f;
#pragma unroll
    for (int c = 0; c < UW_CIT; ++c)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[c][o][t] = 0.f;
  }
  const int64_t q0 = blockIdx.x * per_chunk;
  const int64_t q1 = q0 + per_chunk < pixels ? q0 + per_chunk : pixels;
  for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
    const int n = (int)(q / HW);
    const int p = (int)(q - (int64_t)n * HW);
    const int i = p / W, j = p - i * W;
    const float* xp = x + (size_t)n * Cin * HW + p;
    const float* gp = dy + (size_t)n * ds.batch_stride + (size_t)(2 * i) * W2 + 2 * j;
    float xv[UW_CIT], d[UW_COT][4];
#pragma unroll
    for (int c = 0; c < UW_CIT; ++c) xv[c] = xp[xo[c]];
#pragma unroll
    for (int o = 0; o < UW_COT; ++o) {
      up_load4<VEC>(gp + go[o], W2, d[o]);
      sb[o] += (d[o][0] + d[o][1]) + (d[o][2] + d[o][3]);
    }
#pragma unroll
    for (int c = 0; c < UW_CIT; ++c)
#pragma unroll
      for (int o = 0; o < UW_COT; ++o)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[c][o][t] = __builtin_fmaf(xv[c], d[o][t], acc[c][o][t]);
  }
  // the wave's sums in fp32 (every lane is here: the loop above has no early exit), then the four waves' and the chunks' in fp64
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < UW_CIT; ++c)
#pragma unroll
    for (int o = 0; o < UW_COT; ++o)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float s = wave_sum(acc[c][o][t]);
        if (lane == 0) red[wave][(c * UW_COT + o) * 4 + t] = (double)s;
      }
#pragma unroll
  for (int o = 0; o < UW_COT; ++o) {
    const float s = wave_sum(sb[o]);
    if (lane == 0) red[wave][UW_CIT * UW_COT * 4 + o] = (double)s;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k >= UW_SUMS) return;
  const double total = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  double* out = part + (size_t)blockIdx.x * ((size_t)Cin * Cout * 4 + Cout);
  if (k < UW_CIT * UW_COT * 4) {
    const int c = k / (UW_COT * 4), o = (k / 4) % UW_COT, t = k & 3;
    if (ci0 + c < Cin && co0 + o < Cout) out[((size_t)(ci0 + c) * Cout + co0 + o) * 4 + t] = total;
  } else {
    const int o = k - UW_CIT * UW_COT * 4;
    if (ci0 == 0 && co0 + o < Cout) out[(size_t)Cin * Cout * 4 + co0 + o] = total;
  }
}

// stage 2: the chunks' partials in chunk order, rounded to fp32 once
__global__ __launch_bounds__(256) void deconv2x2_bwd_weight_finalize_kernel(const double* __restrict__ part, int chunks, int64_t n_dw,
                                                                            int64_t n_all, float* __restrict__ dw, float* __restrict__ db) {
  const int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (e >= n_all) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += part[(size_t)c * n_all + e];
  if (e < n_dw)
    dw[e] = (float)s;
  else if (db != nullptr)
    db[e - n_dw] = (float)s;
}

// what the three up-convolution entry points refuse alike
int up_check(const char* who, int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W, int64_t batch_stride, int32_t channels,
             int32_t c_off) {
  MCD_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, "%s: bad dims", who);
  MCD_REQUIRE(N <= 65535, "%s: N exceeds the grid limit", who);
  MCD_REQUIRE((int64_t)H * W <= (1 << 28), "%s: the plane is too large", who);
  MCD_REQUIRE(c_off >= 0 && channels > 0 && (int64_t)c_off + Cout <= channels && batch_stride >= (int64_t)channels * 4 * H * W,
              "%s: the channel slice [%d, %d) lies outside a buffer of %d channels and batch stride %lld", who, c_off, c_off + Cout, channels,
              (long long)batch_stride);
  return 0;
}

bool up_vec(const float* slice, int64_t batch_stride) { return unet_aligned(slice, 8) && (batch_stride % 2) == 0; }

}  // namespace

extern "C" int mcdseg_maxpool2_fwd(const float* x, const float* x_bound, float* y, void* y_cb, float* y_bound, int32_t math, int32_t N,
                                   int32_t C, int32_t H, int32_t W, void* stream) {
  MCD_REQUIRE(x && y, "maxpool2_fwd: null pointer");
  MCD_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "maxpool2_fwd: bad dims");
  MCD_REQUIRE((H % 2) == 0 && (W % 2) == 0, "maxpool2_fwd: H and W must be even, got %d x %d", H, W);
  MCD_REQUIRE((int64_t)H * W <= (1 << 30), "maxpool2_fwd: the plane is too large");
  MCD_REQUIRE((x_bound != nullptr) == (y_bound != nullptr), "maxpool2_fwd: the bounds come as both pointers or none");
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (W % 4 == 0) && unet_aligned(x, 16) && unet_aligned(y, 8);
  if (y_cb == nullptr) {
    const int64_t units = (int64_t)N * C * (H / 2) * ((W / 2) / (vec ? 2 : 1));
    if (vec)
      hipLaunchKernelGGL(maxpool2_plain_kernel<2>, dim3(flat_blocks(units, 256)), dim3(256), 0, st, x, x_bound, y, y_bound, units, H, W);
    else
      hipLaunchKernelGGL(maxpool2_plain_kernel<1>, dim3(flat_blocks(units, 256)), dim3(256), 0, st, x, x_bound, y, y_bound, units, H, W);
    MCD_LAUNCH_CHECK("maxpool2_fwd");
    return 0;
  }
  MCD_REQUIRE(mcd_math_known(math), "maxpool2_fwd: unknown math %d", math);
  math = mcd_storage_math(math);
  if (int rc = cb_check("maxpool2_fwd", math, x_bound, N, C, (H / 2) * (W / 2))) return rc;
  if (math == MCDSEG_MATH_F16X3)
    maxpool2_cb_launch<SplitF16x3>(x, x_bound, y, y_cb, y_bound, N, C, H, W, vec, st);
  else
    maxpool2_cb_launch<SplitBf16x6>(x, x_bound, y, y_cb, y_bound, N, C, H, W, vec, st);
  MCD_LAUNCH_CHECK("maxpool2_fwd");
  return 0;
}

extern "C" int mcdseg_maxpool2_bwd(const float* x, const float* dy, float* dx, int32_t N, int32_t C, int32_t H, int32_t W, void* stream) {
  MCD_REQUIRE(x && dy && dx, "maxpool2_bwd: null pointer");
  MCD_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "maxpool2_bwd: bad dims");
  MCD_REQUIRE((H % 2) == 0 && (W % 2) == 0, "maxpool2_bwd: H and W must be even, got %d x %d", H, W);
  MCD_REQUIRE((int64_t)H * W <= (1 << 30), "maxpool2_bwd: the plane is too large");
  const bool vec = (W % 4 == 0) && unet_aligned(x, 16) && unet_aligned(dx, 16) && unet_aligned(dy, 8);
  const int64_t units = (int64_t)N * C * (H / 2) * ((W / 2) / (vec ? 2 : 1));
  if (vec)
    hipLaunchKernelGGL(maxpool2_bwd_kernel<2>, dim3(flat_blocks(units, 256)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, units, H, W);
  else
    hipLaunchKernelGGL(maxpool2_bwd_kernel<1>, dim3(flat_blocks(units, 256)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, units, H, W);
  MCD_LAUNCH_CHECK("maxpool2_bwd");
  return 0;
}

extern "C" int mcdseg_relu_fwd(const float* x, const float* x_bound, float* y, void* y_cb, float* y_bound, int32_t math, int32_t N, int32_t C,
                               int32_t HW, void* stream) {
  MCD_REQUIRE(x && y, "relu_fwd: null pointer");
  MCD_REQUIRE(N > 0 && C > 0 && HW > 0, "relu_fwd: bad dims");
  MCD_REQUIRE((x_bound != nullptr) == (y_bound != nullptr), "relu_fwd: the bounds come as both pointers or none");
  hipStream_t st = (hipStream_t)stream;
  if (y_cb == nullptr) {
    const int64_t n = (int64_t)N * C * HW;
    const int64_t n4 = (unet_aligned(x, 16) && unet_aligned(y, 16)) ? n / 4 : 0;
    hipLaunchKernelGGL(relu_plain_kernel, dim3(flat_blocks(n4 > 0 ? n4 : n, 256 * 4)), dim3(256), 0, st, x, x_bound, y, y_bound, n4, n);
    MCD_LAUNCH_CHECK("relu_fwd");
    return 0;
  }
  MCD_REQUIRE(mcd_math_known(math), "relu_fwd: unknown math %d", math);
  math = mcd_storage_math(math);
  if (int rc = cb_check("relu_fwd", math, x_bound, N, C, HW)) return rc;
  if (math == MCDSEG_MATH_F16X3)
    relu_cb_launch<SplitF16x3>(x, x_bound, y, y_cb, y_bound, N, C, HW, st);
  else
    relu_cb_launch<SplitBf16x6>(x, x_bound, y, y_cb, y_bound, N, C, HW, st);
  MCD_LAUNCH_CHECK("relu_fwd");
  return 0;
}

extern "C" int mcdseg_relu_bwd(const float* y, const float* dy, float* dx, int64_t n, void* stream) {
  MCD_REQUIRE(y && dy && dx, "relu_bwd: null pointer");
  MCD_REQUIRE(n > 0, "relu_bwd: bad dims");
  const int64_t n4 = (unet_aligned(y, 16) && unet_aligned(dy, 16) && unet_aligned(dx, 16)) ? n / 4 : 0;
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(flat_blocks(n4 > 0 ? n4 : n, 256 * 4)), dim3(256), 0, (hipStream_t)stream, y, dy, dx, n4, n);
  MCD_LAUNCH_CHECK("relu_bwd");
  return 0;
}

extern "C" int mcdseg_deconv2x2_fwd(const float* x, const float* w, const float* bias, float* y, int64_t y_batch_stride, int32_t y_channels,
                                    int32_t y_channel_offset, int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W, void* stream) {
  MCD_REQUIRE(x && w && y, "deconv2x2_fwd: null pointer");
  if (int rc = up_check("deconv2x2_fwd", N, Cin, Cout, H, W, y_batch_stride, y_channels, y_channel_offset)) return rc;
  const UpSlice ys{y_batch_stride, y_channel_offset};
  const dim3 grid(ceil_div(H * W, 256), ceil_div(Cout, UP_COT), N);
  MCD_REQUIRE(grid.y <= 65535, "deconv2x2_fwd: Cout exceeds the grid limit");
  if (up_vec(y, y_batch_stride))
    hipLaunchKernelGGL(deconv2x2_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, w, bias, y, ys, Cin, Cout, H, W);
  else
    hipLaunchKernelGGL(deconv2x2_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, w, bias, y, ys, Cin, Cout, H, W);
  MCD_LAUNCH_CHECK("deconv2x2_fwd");
  return 0;
}

extern "C" int mcdseg_deconv2x2_bwd_data(const float* dy, int64_t dy_batch_stride, int32_t dy_channels, int32_t dy_channel_offset,
                                         const float* w, float* dx, int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W, void* stream) {
  MCD_REQUIRE(dy && w && dx, "deconv2x2_bwd_data: null pointer");
  if (int rc = up_check("deconv2x2_bwd_data", N, Cin, Cout, H, W, dy_batch_stride, dy_channels, dy_channel_offset)) return rc;
  const UpSlice ds{dy_batch_stride, dy_channel_offset};
  const dim3 grid(ceil_div(H * W, 256), ceil_div(Cin, UP_CIT), N);
  MCD_REQUIRE(grid.y <= 65535, "deconv2x2_bwd_data: Cin exceeds the grid limit");
  if (up_vec(dy, dy_batch_stride))
    hipLaunchKernelGGL(deconv2x2_bwd_data_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, dy, ds, w, dx, Cin, Cout, H, W);
  else
    hipLaunchKernelGGL(deconv2x2_bwd_data_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, dy, ds, w, dx, Cin, Cout, H, W);
  MCD_LAUNCH_CHECK("deconv2x2_bwd_data");
  return 0;
}

extern "C" size_t mcdseg_deconv2x2_bwd_weight_workspace_bytes(int32_t N, int32_t Cin, int32_t Cout, int32_t H, int32_t W) {
  if (N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)up_wgrad_chunks(N, Cin, Cout, H, W) * ((size_t)Cin * Cout * 4 + Cout) * sizeof(double);
}

extern "C" int mcdseg_deconv2x2_bwd_weight(const float* x, const float* dy, int64_t dy_batch_stride, int32_t dy_channels,
                                           int32_t dy_channel_offset, float* dw, float* db, int32_t N, int32_t Cin, int32_t Cout, int32_t H,
                                           int32_t W, void* workspace, size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(x && dy && dw && workspace, "deconv2x2_bwd_weight: null pointer");
  if (int rc = up_check("deconv2x2_bwd_weight", N, Cin, Cout, H, W, dy_batch_stride, dy_channels, dy_channel_offset)) return rc;
  MCD_REQUIRE(workspace_bytes >= mcdseg_deconv2x2_bwd_weight_workspace_bytes(N, Cin, Cout, H, W), "deconv2x2_bwd_weight: workspace too small");
  MCD_REQUIRE(unet_aligned(workspace, 8), "deconv2x2_bwd_weight: the workspace must be 8-byte aligned");
  const int64_t tiles = (int64_t)ceil_div(Cin, UW_CIT) * ceil_div(Cout, UW_COT);
  MCD_REQUIRE(tiles <= 65535, "deconv2x2_bwd_weight: Cin x Cout exceeds the grid limit");
  hipStream_t st = (hipStream_t)stream;
  const UpSlice ds{dy_batch_stride, dy_channel_offset};
  const int chunks = up_wgrad_chunks(N, Cin, Cout, H, W);
  const int64_t pixels = (int64_t)N * H * W;
  const int64_t per_chunk = ceil_div64(pixels, chunks);
  const dim3 grid(chunks, (unsigned)tiles);
  double* part = (double*)workspace;
  if (up_vec(dy, dy_batch_stride))
    hipLaunchKernelGGL(deconv2x2_bwd_weight_kernel<true>, grid, dim3(256), 0, st, x, dy, ds, part, pixels, per_chunk, Cin, Cout, H, W);
  else
    hipLaunchKernelGGL(deconv2x2_bwd_weight_kernel<false>, grid, dim3(256), 0, st, x, dy, ds, part, pixels, per_chunk, Cin, Cout, H, W);
  MCD_LAUNCH_CHECK("deconv2x2_bwd_weight");
  const int64_t n_dw = (int64_t)Cin * Cout * 4, n_all = n_dw + Cout;
  hipLaunchKernelGGL(deconv2x2_bwd_weight_finalize_kernel, dim3((unsigned)ceil_div64(n_all, 256)), dim3(256), 0, st, part, chunks, n_dw, n_all,
                     dw, db);
  MCD_LAUNCH_CHECK("deconv2x2_bwd_weight");
  return 0;
}
