// The boundary branch of the segmentation + boundary multitask decoder (MCDSegBDMultiTaskDecoder, models/dilated_fcn.py:1027-1222):
//   label_boundary     3x3 dilation != 3x3 erosion of a label map                         (get_boundary, :770-774)
//   boundary_head      p = (sigmoid(up2 s1) + sigmoid(up4 s2) + sigmoid(up8 s3)) / 3      (boundary_forward, :1118-1128)
//   bce2d              class-balanced binary cross-entropy                                (loss.py:131-138)
//   boundary_head_bce  the three of them in one forward and one backward pass             (get_boundary_loss, :1202-1204)
//   boundary_head_bce_target  the same pair against a given target plane (MCDTripleMultiTaskDecoder.get_boundary_loss, :1002-1004)
// HBM-bound streaming kernels on full-resolution maps.  Sums leave a block as fp64 partials and are finished by one small
// kernel in fp64; no float atomics anywhere, so every result is bitwise reproducible.  The fused pair calls the very device
// functions the unfused kernels are made of (fp contraction is off), which is what makes it equal to their composition.
#include "common.h"
#include "boundary_blocks.h"

namespace {

typedef long long ll2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------------------- building blocks

// the three planes of one image and the full-resolution size (H, W multiples of 8)
struct Head {
  const float* s1;
  const float* s2;
  const float* s3;
  int H, W;
};

__device__ __forceinline__ Head head_of(const float* s1, const float* s2, const float* s3, int img, int H, int W) {
  Head h;
  h.s1 = s1 + (size_t)img * (H / 2) * (W / 2);
  h.s2 = s2 + (size_t)img * (H / 4) * (W / 4);
  h.s3 = s3 + (size_t)img * (H / 8) * (W / 8);
  h.H = H;
  h.W = W;
  return h;
}

__device__ __forceinline__ void head_sigmoids(const Head& h, int oy, int ox, float& g1, float& g2, float& g3) {
  g1 = sigm(up_at<2>(h.s1, h.H / 2, h.W / 2, oy, ox));
  g2 = sigm(up_at<4>(h.s2, h.H / 4, h.W / 4, oy, ox));
  g3 = sigm(up_at<8>(h.s3, h.H / 8, h.W / 8, oy, ox));
}

__device__ __forceinline__ float head_mean(float g1, float g2, float g3) { return ((g1 + g2) + g3) / 3.f; }

__device__ __forceinline__ float head_p(const Head& h, int oy, int ox) {
  float g1, g2, g3;
  head_sigmoids(h, oy, ox, g1, g2, g3);
  return head_mean(g1, g2, g3);
}

// dilation != erosion at (y, x) of one label image: neighbours outside the image do not take part
template <typename T>
__device__ __forceinline__ float boundary_at(const T* __restrict__ lab, int H, int W, int y, int x) {
  const int ya = y > 0 ? y - 1 : 0, yb = y < H - 1 ? y + 1 : H - 1;
  const int xa = x > 0 ? x - 1 : 0, xb = x < W - 1 ? x + 1 : W - 1;
  long long mx = (long long)lab[(size_t)y * W + x], mn = mx;
  for (int yy = ya; yy <= yb; ++yy)
    for (int xx = xa; xx <= xb; ++xx) {
      const long long v = (long long)lab[(size_t)yy * W + xx];
      mx = v > mx ? v : mx;
      mn = v < mn ? v : mn;
    }
  return mx != mn ? 1.f : 0.f;
}


// out[0] = loss = ((1 - beta) sum bce + (2 beta - 1) sum t bce) / n,  out[1] = beta = 1 - sum t / n
__global__ __launch_bounds__(256) void bce_finalize_kernel(const double* __restrict__ part, int nblk, double n, float* __restrict__ out) {
  double tot[3];
  partials_total(part, nblk, 3, 0, tot);
  if (threadIdx.x == 0) {
    double loss, beta;
    balanced_bce(tot, n, loss, beta);
    out[0] = (float)loss;
    out[1] = (float)beta;
  }
}


// ---------------------------------------------------------------------------------------------------------- label_boundary
__device__ __forceinline__ void load8(const long long* p, long long v[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const ll2 a = *reinterpret_cast<const ll2*>(p + 2 * k);
    v[2 * k] = a.x;
    v[2 * k + 1] = a.y;
  }
}

__device__ __forceinline__ void load8(const uint8_t* p, long long v[8]) {
  const uint2 a = *reinterpret_cast<const uint2*>(p);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = (a.x >> (8 * k)) & 0xffu;
    v[4 + k] = (a.y >> (8 * k)) & 0xffu;
  }
}

// eight pixels of one row per thread (W % 8 == 0, 16-byte aligned base): rows y-1, y, y+1 with a one-pixel halo each side.  An
// out-of-image neighbour is replaced by an in-image member of the same window, which changes neither the max nor the min.
template <typename T>
__global__ __launch_bounds__(256) void label_boundary_vec_kernel(const T* __restrict__ lab, uint8_t* __restrict__ out, int H, int W, int64_t groups) {
  const int gpr = W >> 3;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
    const int gx = (int)(g % gpr);
    const int64_t r = g / gpr;
    const int y = (int)(r % H);
    const int64_t img = r / H;
    const int x0 = gx << 3;
    const T* base = lab + (size_t)img * H * W;
    long long mx[8], mn[8];
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= H) continue;
      const T* row = base + (size_t)yy * W + x0;
      long long v[10];
      load8(row, v + 1);
      v[0] = x0 > 0 ? (long long)row[-1] : v[1];
      v[9] = x0 + 8 < W ? (long long)row[8] : v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        long long a = v[k] > v[k + 1] ? v[k] : v[k + 1];
        a = a > v[k + 2] ? a : v[k + 2];
        long long b = v[k] < v[k + 1] ? v[k] : v[k + 1];
        b = b < v[k + 2] ? b : v[k + 2];
        if (dy == -1 || (dy == 0 && y == 0)) {
          mx[k] = a;
          mn[k] = b;
        } else {
          mx[k] = a > mx[k] ? a : mx[k];
          mn[k] = b < mn[k] ? b : mn[k];
        }
      }
    }
    uint2 o = make_uint2(0u, 0u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o.x |= (mx[k] != mn[k] ? 1u : 0u) << (8 * k);
      o.y |= (mx[4 + k] != mn[4 + k] ? 1u : 0u) << (8 * k);
    }
    *reinterpret_cast<uint2*>(out + ((size_t)img * H + y) * W + x0) = o;
  }
}

// any W / any alignment: one pixel per thread
template <typename T>
__global__ __launch_bounds__(256) void label_boundary_scalar_kernel(const T* __restrict__ lab, uint8_t* __restrict__ out, int H, int W, int64_t total) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const int64_t r = i / W;
    const int y = (int)(r % H);
    const int64_t img = r / H;
    out[i] = boundary_at(lab + (size_t)img * H * W, H, W, y, x) != 0.f ? 1 : 0;
  }
}

template <typename T>
int launch_label_boundary(const T* lab, uint8_t* out, int N, int H, int W, hipStream_t st) {
  const int64_t total = (int64_t)N * H * W;
  const bool vec = (W % 8 == 0) && ((reinterpret_cast<uintptr_t>(lab) & 15) == 0) && ((reinterpret_cast<uintptr_t>(out) & 7) == 0);
  if (vec) {
    const int64_t groups = total / 8;
    int64_t nb = ceil_div64(groups, 256);
    nb = nb > 8192 ? 8192 : nb;
    hipLaunchKernelGGL(label_boundary_vec_kernel<T>, dim3((unsigned)nb), dim3(256), 0, st, lab, out, H, W, groups);
  } else {
    int64_t nb = ceil_div64(total, 256);
    nb = nb > 8192 ? 8192 : nb;
    hipLaunchKernelGGL(label_boundary_scalar_kernel<T>, dim3((unsigned)nb), dim3(256), 0, st, lab, out, H, W, total);
  }
  MCD_LAUNCH_CHECK("label_boundary");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------- boundary head
// four output pixels (one float4) per thread
__global__ __launch_bounds__(256) void boundary_head_fwd_kernel(const float* __restrict__ s1, const float* __restrict__ s2, const float* __restrict__ s3,
                                                                float* __restrict__ p, int H, int W) {
  const int img = blockIdx.x;
  const Head h = head_of(s1, s2, s3, img, H, W);
  const int qpr = W >> 2;
  const int total = H * qpr;
  float4* out = reinterpret_cast<float4*>(p + (size_t)img * H * W);
  for (int idx = blockIdx.y * blockDim.x + threadIdx.x; idx < total; idx += gridDim.y * blockDim.x) {
    const int oy = idx / qpr;
    const int ox0 = (idx - oy * qpr) << 2;
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = head_p(h, oy, ox0 + j);
    out[idx] = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// Gather form of the backward, one thread per pixel of the scale-S map: pixel (iy, ix) collects from output rows / columns
// [S i - S/2, S i + 3S/2).  sigmoid' is recomputed from the s maps.  FUSED: the upstream dp is not read but recomputed -- p from the
// three maps, the target from the labels' 3x3 window -- as the bce backward forms it.
template <int S, bool FUSED>
__global__ __launch_bounds__(256) void boundary_head_bwd_kernel(const float* __restrict__ s1, const float* __restrict__ s2, const float* __restrict__ s3,
                                                                const float* __restrict__ dp, const long long* __restrict__ lab,
                                                                const float* __restrict__ beta_p, const float* __restrict__ g_p, float inv_n,
                                                                float* __restrict__ ds, int H, int W) {
  const int img = blockIdx.x;
  const Head h = head_of(s1, s2, s3, img, H, W);
  const int Hi = H / S, Wi = W / S;
  const float* up = dp ? dp + (size_t)img * H * W : nullptr;
  const long long* li = lab ? lab + (size_t)img * H * W : nullptr;
  float beta = 0.f, gs = 0.f;
  if (FUSED) {
    beta = *beta_p;
    gs = (g_p ? *g_p : 1.f) * inv_n;
  }
  const int total = Hi * Wi;
  for (int idx = blockIdx.y * blockDim.x + threadIdx.x; idx < total; idx += gridDim.y * blockDim.x) {
    const int iy = idx / Wi;
    const int ix = idx - iy * Wi;
    const int oy0 = S * iy - S / 2, ox0 = S * ix - S / 2;
    float acc = 0.f;
    for (int ky = 0; ky < 2 * S; ++ky) {
      const int oy = oy0 + ky;
      if (oy < 0 || oy >= H) continue;
      const float wy = tap_weight_s<S>(oy, Hi, iy);
      if (wy == 0.f) continue;  // (a clamped edge tap)
      float r = 0.f;
      for (int kx = 0; kx < 2 * S; ++kx) {
        const int ox = ox0 + kx;
        if (ox < 0 || ox >= W) continue;
        const float wx = tap_weight_s<S>(ox, Wi, ix);
        if (wx == 0.f) continue;
        float sg, d;
        if (FUSED) {
          float g1, g2, g3;
          head_sigmoids(h, oy, ox, g1, g2, g3);
          sg = S == 2 ? g1 : (S == 4 ? g2 : g3);
          d = bce_grad(head_mean(g1, g2, g3), boundary_at(li, H, W, oy, ox), beta, gs);
        } else {
          sg = sigm(up_at<S>(S == 2 ? h.s1 : (S == 4 ? h.s2 : h.s3), Hi, Wi, oy, ox));
          d = up[(size_t)oy * W + ox];
        }
        r = fmaf((d / 3.f) * ((1.f - sg) * sg), wx, r);
      }
      acc = fmaf(wy, r, acc);
    }
    ds[(size_t)img * total + idx] = acc;
  }
}

template <bool FUSED>
int launch_head_bwd(const float* s1, const float* s2, const float* s3, const float* dp, const long long* lab, const float* beta, const float* g,
                    float* ds1, float* ds2, float* ds3, int N, int H, int W, hipStream_t st) {
  const float inv_n = (float)(1.0 / ((double)N * H * W));
  auto chunks = [](int px) {
    const int c = ceil_div(px, 256);
    return c > 256 ? 256 : c;
  };
  hipLaunchKernelGGL((boundary_head_bwd_kernel<2, FUSED>), dim3(N, chunks((H / 2) * (W / 2))), dim3(256), 0, st, s1, s2, s3, dp, lab, beta, g, inv_n,
                     ds1, H, W);
  MCD_LAUNCH_CHECK("boundary_head_bwd<2>");
  hipLaunchKernelGGL((boundary_head_bwd_kernel<4, FUSED>), dim3(N, chunks((H / 4) * (W / 4))), dim3(256), 0, st, s1, s2, s3, dp, lab, beta, g, inv_n,
                     ds2, H, W);
  MCD_LAUNCH_CHECK("boundary_head_bwd<4>");
  hipLaunchKernelGGL((boundary_head_bwd_kernel<8, FUSED>), dim3(N, chunks((H / 8) * (W / 8))), dim3(256), 0, st, s1, s2, s3, dp, lab, beta, g, inv_n,
                     ds3, H, W);
  MCD_LAUNCH_CHECK("boundary_head_bwd<8>");
  return 0;
}

// The fused backward against a GIVEN target (one plane per image, fp32 or uint8, image n's plane tstride elements behind image
// n - 1's): boundary_head_bwd_kernel<S, true> with the target read instead of derived from the labels' 3x3 window.
template <int S, typename T>
__global__ __launch_bounds__(256) void boundary_head_bwd_target_kernel(const float* __restrict__ s1, const float* __restrict__ s2,
                                                                       const float* __restrict__ s3, const T* __restrict__ tgt, int64_t tstride,
                                                                       const float* __restrict__ beta_p, const float* __restrict__ g_p, float inv_n,
                                                                       float* __restrict__ ds, int H, int W) {
  const int img = blockIdx.x;
  const Head h = head_of(s1, s2, s3, img, H, W);
  const int Hi = H / S, Wi = W / S;
  const T* ti = tgt + (size_t)img * tstride;
  const float beta = *beta_p;
  const float gs = (g_p ? *g_p : 1.f) * inv_n;
  const int total = Hi * Wi;
  for (int idx = blockIdx.y * blockDim.x + threadIdx.x; idx < total; idx += gridDim.y * blockDim.x) {
    const int iy = idx / Wi;
    const int ix = idx - iy * Wi;
    const int oy0 = S * iy - S / 2, ox0 = S * ix - S / 2;
    float acc = 0.f;
    for (int ky = 0; ky < 2 * S; ++ky) {
      const int oy = oy0 + ky;
      if (oy < 0 || oy >= H) continue;
      const float wy = tap_weight_s<S>(oy, Hi, iy);
      if (wy == 0.f) continue;  // (a clamped edge tap)
      float r = 0.f;
      for (int kx = 0; kx < 2 * S; ++kx) {
        const int ox = ox0 + kx;
        if (ox < 0 || ox >= W) continue;
        const float wx = tap_weight_s<S>(ox, Wi, ix);
        if (wx == 0.f) continue;
        float g1, g2, g3;
        head_sigmoids(h, oy, ox, g1, g2, g3);
        const float sg = S == 2 ? g1 : (S == 4 ? g2 : g3);
        const float d = bce_grad(head_mean(g1, g2, g3), (float)ti[(size_t)oy * W + ox], beta, gs);
        r = fmaf((d / 3.f) * ((1.f - sg) * sg), wx, r);
      }
      acc = fmaf(wy, r, acc);
    }
    ds[(size_t)img * total + idx] = acc;
  }
}

template <typename T>
int launch_head_bwd_target(const float* s1, const float* s2, const float* s3, const T* tgt, int64_t tstride, const float* beta, const float* g,
                           float* ds1, float* ds2, float* ds3, int N, int H, int W, hipStream_t st) {
  const float inv_n = (float)(1.0 / ((double)N * H * W));
  auto chunks = [](int px) {
    const int c = ceil_div(px, 256);
    return c > 256 ? 256 : c;
  };
  hipLaunchKernelGGL((boundary_head_bwd_target_kernel<2, T>), dim3(N, chunks((H / 2) * (W / 2))), dim3(256), 0, st, s1, s2, s3, tgt, tstride, beta, g,
                     inv_n, ds1, H, W);
  MCD_LAUNCH_CHECK("boundary_head_bwd_target<2>");
  hipLaunchKernelGGL((boundary_head_bwd_target_kernel<4, T>), dim3(N, chunks((H / 4) * (W / 4))), dim3(256), 0, st, s1, s2, s3, tgt, tstride, beta, g,
                     inv_n, ds2, H, W);
  MCD_LAUNCH_CHECK("boundary_head_bwd_target<4>");
  hipLaunchKernelGGL((boundary_head_bwd_target_kernel<8, T>), dim3(N, chunks((H / 8) * (W / 8))), dim3(256), 0, st, s1, s2, s3, tgt, tstride, beta, g,
                     inv_n, ds3, H, W);
  MCD_LAUNCH_CHECK("boundary_head_bwd_target<8>");
  return 0;
}

// ---------------------------------------------------------------------------------------------------------- bce2d
__device__ __forceinline__ void load_t16(const uint8_t* t, int64_t i16, float v[16]) {
  const uint4 a = reinterpret_cast<const uint4*>(t)[i16];
  const unsigned w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = (float)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
}

__device__ __forceinline__ void load_t16(const float* t, int64_t i16, float v[16]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float4 a = reinterpret_cast<const float4*>(t)[i16 * 4 + k];
    v[4 * k] = a.x, v[4 * k + 1] = a.y, v[4 * k + 2] = a.z, v[4 * k + 3] = a.w;
  }
}

__device__ __forceinline__ void load_p16(const float* p, int64_t i16, float v[16]) { load_t16(p, i16, v); }

// sixteen elements per thread and iteration (n16 of them in 16-byte accesses, the rest -- everything when a pointer is not
// 16-byte aligned -- one by one)
template <typename T>
__global__ __launch_bounds__(256) void bce2d_fwd_kernel(const float* __restrict__ p, const T* __restrict__ t, double* __restrict__ part, int64_t n16,
                                                        int64_t n) {
  Sums s = {0.f, 0.f, 0.f};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
    float pv[16], tv[16];
    load_p16(p, i, pv);
    load_t16(t, i, tv);
#pragma unroll
    for (int k = 0; k < 16; ++k) sums_add(s, pv[k], tv[k]);
  }
  for (int64_t i = n16 * 16 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    sums_add(s, p[i], (float)t[i]);
  sums_store(s, part);
}

template <typename T>
__global__ __launch_bounds__(256) void bce2d_bwd_kernel(const float* __restrict__ p, const T* __restrict__ t, const float* __restrict__ beta_p,
                                                        const float* __restrict__ g_p, float inv_n, float* __restrict__ dp, int64_t n16, int64_t n) {
  const float beta = *beta_p;
  const float gs = (g_p ? *g_p : 1.f) * inv_n;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
    float pv[16], tv[16];
    load_p16(p, i, pv);
    load_t16(t, i, tv);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      reinterpret_cast<float4*>(dp)[i * 4 + k] =
          make_float4(bce_grad(pv[4 * k], tv[4 * k], beta, gs), bce_grad(pv[4 * k + 1], tv[4 * k + 1], beta, gs),
                      bce_grad(pv[4 * k + 2], tv[4 * k + 2], beta, gs), bce_grad(pv[4 * k + 3], tv[4 * k + 3], beta, gs));
  }
  for (int64_t i = n16 * 16 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dp[i] = bce_grad(p[i], (float)t[i], beta, gs);
}

// ---------------------------------------------------------------------------------------------------------- fused forward
// four pixels of one row per thread: p from the three maps, the target from the labels' rows y-1..y+1 (16-byte loads of the four
// centre columns, the two halo columns one by one), the three sums; neither p nor the target is stored
__global__ __launch_bounds__(256) void boundary_head_bce_fwd_kernel(const float* __restrict__ s1, const float* __restrict__ s2, const float* __restrict__ s3,
                                                                    const long long* __restrict__ lab, double* __restrict__ part, int H, int W,
                                                                    int64_t quads) {
  const int qpr = W >> 2;
  Sums s = {0.f, 0.f, 0.f};
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    const int qx = (int)(q % qpr);
    const int64_t r = q / qpr;
    const int y = (int)(r % H);
    const int img = (int)(r / H);
    const int x0 = qx << 2;
    const Head h = head_of(s1, s2, s3, img, H, W);
    const long long* li = lab + (size_t)img * H * W;
    long long mx[4], mn[4];
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= H) continue;
      const long long* row = li + (size_t)yy * W + x0;
      long long v[6];
      const ll2 a = *reinterpret_cast<const ll2*>(row), b = *reinterpret_cast<const ll2*>(row + 2);
      v[1] = a.x, v[2] = a.y, v[3] = b.x, v[4] = b.y;
      v[0] = x0 > 0 ? row[-1] : v[1];
      v[5] = x0 + 4 < W ? row[4] : v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        long long hi = v[k] > v[k + 1] ? v[k] : v[k + 1];
        hi = hi > v[k + 2] ? hi : v[k + 2];
        long long lo = v[k] < v[k + 1] ? v[k] : v[k + 1];
        lo = lo < v[k + 2] ? lo : v[k + 2];
        if (dy == -1 || (dy == 0 && y == 0)) {
          mx[k] = hi;
          mn[k] = lo;
        } else {
          mx[k] = hi > mx[k] ? hi : mx[k];
          mn[k] = lo < mn[k] ? lo : mn[k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) sums_add(s, head_p(h, y, x0 + k), mx[k] != mn[k] ? 1.f : 0.f);
  }
  sums_store(s, part);
}

// the fused forward against a given target: one pixel per thread (any alignment of the planes), p from the three maps, the three sums
template <typename T>
__global__ __launch_bounds__(256) void boundary_head_bce_target_fwd_kernel(const float* __restrict__ s1, const float* __restrict__ s2,
                                                                           const float* __restrict__ s3, const T* __restrict__ tgt, int64_t tstride,
                                                                           double* __restrict__ part, int H, int W, int64_t total) {
  const int64_t HW = (int64_t)H * W;
  Sums s = {0.f, 0.f, 0.f};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int img = (int)(i / HW);
    const int r = (int)(i - img * HW);
    const int y = r / W;
    const Head h = head_of(s1, s2, s3, img, H, W);
    sums_add(s, head_p(h, y, r - y * W), (float)tgt[(size_t)img * tstride + r]);
  }
  sums_store(s, part);
}

bool head_args_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0 && (int64_t)H * W < (1ll << 31); }

}  // namespace

extern "C" int mcdseg_label_boundary(const void* labels, int32_t labels_u8, uint8_t* boundary, int32_t N, int32_t H, int32_t W, void* stream) {
  MCD_REQUIRE(labels && boundary && N > 0 && H > 0 && W > 0, "label_boundary: bad arguments");
  if (labels_u8) return launch_label_boundary((const uint8_t*)labels, boundary, N, H, W, (hipStream_t)stream);
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(labels) & 7) == 0, "label_boundary: int64 labels must be 8-byte aligned");
  return launch_label_boundary((const long long*)labels, boundary, N, H, W, (hipStream_t)stream);
}

extern "C" int mcdseg_boundary_head_fwd(const float* s1, const float* s2, const float* s3, float* p, int32_t N, int32_t H, int32_t W, void* stream) {
  MCD_REQUIRE(s1 && s2 && s3 && p && head_args_ok(N, H, W), "boundary_head_fwd: bad arguments (H and W must be multiples of 8)");
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15) == 0, "boundary_head_fwd: p must be 16-byte aligned");
  int chunks = ceil_div(H * (W / 4), 256 * 2);
  if (chunks > 512) chunks = 512;
  hipLaunchKernelGGL(boundary_head_fwd_kernel, dim3(N, chunks), dim3(256), 0, (hipStream_t)stream, s1, s2, s3, p, H, W);
  MCD_LAUNCH_CHECK("boundary_head_fwd");
  return 0;
}

extern "C" int mcdseg_boundary_head_bwd(const float* s1, const float* s2, const float* s3, const float* dp, float* ds1, float* ds2, float* ds3,
                                        int32_t N, int32_t H, int32_t W, void* stream) {
  MCD_REQUIRE(s1 && s2 && s3 && dp && ds1 && ds2 && ds3 && head_args_ok(N, H, W), "boundary_head_bwd: bad arguments (H and W must be multiples of 8)");
  return launch_head_bwd<false>(s1, s2, s3, dp, nullptr, nullptr, nullptr, ds1, ds2, ds3, N, H, W, (hipStream_t)stream);
}

extern "C" size_t mcdseg_bce2d_workspace_bytes(int64_t n) { return n > 0 ? (size_t)sum_blocks(n) * 3 * sizeof(double) : 0; }

extern "C" int mcdseg_bce2d(const float* p, const void* target, int32_t target_u8, float* out, int64_t n, void* workspace, size_t workspace_bytes,
                            void* stream) {
  MCD_REQUIRE(p && target && out && workspace && n > 0, "bce2d: bad arguments");
  const int nb = sum_blocks(n);
  MCD_REQUIRE(workspace_bytes >= (size_t)nb * 3 * sizeof(double) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
              "bce2d: workspace too small or not 8-byte aligned");
  const bool al = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(target)) & 15) == 0;
  const int64_t n16 = al ? n / 16 : 0;
  hipStream_t st = (hipStream_t)stream;
  if (target_u8)
    hipLaunchKernelGGL(bce2d_fwd_kernel<uint8_t>, dim3(nb), dim3(256), 0, st, p, (const uint8_t*)target, (double*)workspace, n16, n);
  else
    hipLaunchKernelGGL(bce2d_fwd_kernel<float>, dim3(nb), dim3(256), 0, st, p, (const float*)target, (double*)workspace, n16, n);
  MCD_LAUNCH_CHECK("bce2d");
  hipLaunchKernelGGL(bce_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, nb, (double)n, out);
  MCD_LAUNCH_CHECK("bce2d_finalize");
  return 0;
}

extern "C" int mcdseg_bce2d_bwd(const float* p, const void* target, int32_t target_u8, const float* beta, const float* upstream, float* dp, int64_t n,
                                void* stream) {
  MCD_REQUIRE(p && target && beta && dp && n > 0, "bce2d_bwd: bad arguments");
  const bool al = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(dp)) & 15) == 0;
  const int64_t n16 = al ? n / 16 : 0;
  const int nb = sum_blocks(n);
  const float inv_n = (float)(1.0 / (double)n);
  hipStream_t st = (hipStream_t)stream;
  if (target_u8)
    hipLaunchKernelGGL(bce2d_bwd_kernel<uint8_t>, dim3(nb), dim3(256), 0, st, p, (const uint8_t*)target, beta, upstream, inv_n, dp, n16, n);
  else
    hipLaunchKernelGGL(bce2d_bwd_kernel<float>, dim3(nb), dim3(256), 0, st, p, (const float*)target, beta, upstream, inv_n, dp, n16, n);
  MCD_LAUNCH_CHECK("bce2d_bwd");
  return 0;
}

extern "C" int mcdseg_boundary_head_bce_fwd(const float* s1, const float* s2, const float* s3, const int64_t* labels, float* out, int32_t N, int32_t H,
                                            int32_t W, void* workspace, size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(s1 && s2 && s3 && labels && out && workspace && head_args_ok(N, H, W),
              "boundary_head_bce_fwd: bad arguments (H and W must be multiples of 8)");
  const int64_t n = (int64_t)N * H * W;
  const int nb = sum_blocks(n);
  MCD_REQUIRE(workspace_bytes >= (size_t)nb * 3 * sizeof(double) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
              "boundary_head_bce_fwd: workspace too small or not 8-byte aligned");
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(labels) & 15) == 0, "boundary_head_bce_fwd: labels must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(boundary_head_bce_fwd_kernel, dim3(nb), dim3(256), 0, st, s1, s2, s3, (const long long*)labels, (double*)workspace, H, W, n / 4);
  MCD_LAUNCH_CHECK("boundary_head_bce_fwd");
  hipLaunchKernelGGL(bce_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, nb, (double)n, out);
  MCD_LAUNCH_CHECK("boundary_head_bce_finalize");
  return 0;
}

extern "C" int mcdseg_boundary_head_bce_bwd(const float* s1, const float* s2, const float* s3, const int64_t* labels, const float* beta,
                                            const float* upstream, float* ds1, float* ds2, float* ds3, int32_t N, int32_t H, int32_t W, void* stream) {
  MCD_REQUIRE(s1 && s2 && s3 && labels && beta && ds1 && ds2 && ds3 && head_args_ok(N, H, W),
              "boundary_head_bce_bwd: bad arguments (H and W must be multiples of 8)");
  return launch_head_bwd<true>(s1, s2, s3, nullptr, (const long long*)labels, beta, upstream, ds1, ds2, ds3, N, H, W, (hipStream_t)stream);
}

extern "C" int mcdseg_boundary_head_bce_target_fwd(const float* s1, const float* s2, const float* s3, const void* target, int32_t target_u8,
                                                   int64_t target_batch_stride, float* out, int32_t N, int32_t H, int32_t W, void* workspace,
                                                   size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(s1 && s2 && s3 && target && out && workspace && head_args_ok(N, H, W),
              "boundary_head_bce_target_fwd: bad arguments (H and W must be multiples of 8)");
  MCD_REQUIRE(target_batch_stride >= (int64_t)H * W, "boundary_head_bce_target_fwd: the target's batch stride is smaller than a plane");
  MCD_REQUIRE(target_u8 || (reinterpret_cast<uintptr_t>(target) & 3) == 0, "boundary_head_bce_target_fwd: an fp32 target must be 4-byte aligned");
  const int64_t n = (int64_t)N * H * W;
  const int nb = sum_blocks(n);
  MCD_REQUIRE(workspace_bytes >= (size_t)nb * 3 * sizeof(double) && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
              "boundary_head_bce_target_fwd: workspace too small or not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (target_u8)
    hipLaunchKernelGGL(boundary_head_bce_target_fwd_kernel<uint8_t>, dim3(nb), dim3(256), 0, st, s1, s2, s3, (const uint8_t*)target,
                       target_batch_stride, (double*)workspace, H, W, n);
  else
    hipLaunchKernelGGL(boundary_head_bce_target_fwd_kernel<float>, dim3(nb), dim3(256), 0, st, s1, s2, s3, (const float*)target, target_batch_stride,
                       (double*)workspace, H, W, n);
  MCD_LAUNCH_CHECK("boundary_head_bce_target_fwd");
  hipLaunchKernelGGL(bce_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, nb, (double)n, out);
  MCD_LAUNCH_CHECK("boundary_head_bce_target_finalize");
  return 0;
}

extern "C" int mcdseg_boundary_head_bce_target_bwd(const float* s1, const float* s2, const float* s3, const void* target, int32_t target_u8,
                                                   int64_t target_batch_stride, const float* beta, const float* upstream, float* ds1, float* ds2,
                                                   float* ds3, int32_t N, int32_t H, int32_t W, void* stream) {
  MCD_REQUIRE(s1 && s2 && s3 && target && beta && ds1 && ds2 && ds3 && head_args_ok(N, H, W),
              "boundary_head_bce_target_bwd: bad arguments (H and W must be multiples of 8)");
  MCD_REQUIRE(target_batch_stride >= (int64_t)H * W, "boundary_head_bce_target_bwd: the target's batch stride is smaller than a plane");
  MCD_REQUIRE(target_u8 || (reinterpret_cast<uintptr_t>(target) & 3) == 0, "boundary_head_bce_target_bwd: an fp32 target must be 4-byte aligned");
  if (target_u8)
    return launch_head_bwd_target(s1, s2, s3, (const uint8_t*)target, target_batch_stride, beta, upstream, ds1, ds2, ds3, N, H, W,
                                  (hipStream_t)stream);
  return launch_head_bwd_target(s1, s2, s3, (const float*)target, target_batch_stride, beta, upstream, ds1, ds2, ds3, N, H, W, (hipStream_t)stream);
}
