// The fully connected CRF of the reference's tools/crf.py (dense_crf, :14-60; its driver, :88-123) on the device: Kraehenbuehl-Koltun
// mean-field with a Gaussian and a bilateral Potts term, with the sums over all pairs taken EXACTLY where pydensecrf filters on the
// permutohedral lattice.  The definition, per image of N = H*W pixels and C classes:
//     U = -log_softmax(z)                               (stable; finite where the reference's -log(softmax) underflows to inf)
//     g_i = (x/sx, y/sy)   b_i = (x/sx', y/sy', r/sr, g/sg, b/sb)       k(i,j) = exp(-0.5 |f_i - f_j|^2), j = i included
//     n_i = 1 / sqrt(sum_j k(i,j) + 1e-20)              M_i = n_i sum_j k(i,j) n_j Q_j          (symmetric normalisation, per term)
//     Q^0 = softmax(-U)     Q^{t+1} = softmax(-U + w_g M_g(Q^t) + w_b M_b(Q^t))                (Potts: compatibility -w)
// All fp32, no float atomics: every sum has one fixed order, so a result is the same bits run to run and whatever the batch.
//
// The workspace is pixel-major, CP = 32 or 64 floats per pixel (C rounded up to the matrix tile), pad classes hold 0:
//     U[B N][CP]  Q[2][B N][CP] (Q^t and Q^{t+1})  pre[B N][CP]  n_g[B N]  n_b[B N]  feat[B N][8] (b_i; only with an image)
// The passes, each a kernel; they hand over through kernel boundaries only:
//     init    one thread per pixel: U, Q^0, b_i; with n_iters = 0 also the outputs
//     gnorm   n_g
//     dense<NORM>   n_b: the message pass below with ones in the place of n_j Q_j           (with an image; once per image)
//   per iteration
//     gauss   one thread per (pixel, class): pre = -U + w_g M_g(Q^t)
//     dense   (with an image) the hot path: M_b(Q^t), then the update in its epilogue: Q^{t+1} = softmax(pre + w_b M_b)
//     update  (without an image) Q^{t+1} = softmax(pre)
//   the last iteration's update also writes Q as [C][H][W] and the arg-max over the first C_used classes (first maximum on a tie).
//
// gauss: the Gaussian term is spatial only, so it runs over the window |dx| <= ceil(7.5 sx), |dy| <= ceil(7.5 sy), clipped to the image,
// for the sums of n_g and of the message alike.  A pair outside it has k < exp(-0.5 * 7.5^2) = 6.2e-13 < 2^-40; all pairs dropped for one
// pixel together are below 1e-12 sx sy, against a sum of at least 1 (the self term) -- far under half an ulp of the fp32 sum.
//
// dense: a workgroup of 4 waves owns 256 i-pixels, a wave 64 of them as two 32-row tiles of v_mfma_f32_32x32x2_f32: the product
// sum_j k(i,j) (n_j Q_j) is [i x j] x [j x class] with k evaluated on the vector units straight into the A operand -- lane l forms
// k(i = l % 32, j = l / 32), ONE kernel value per lane and matrix instruction, from the feature differences (not from an expanded
// dot product, which cancels at |x/sx| ~ 13) -- and the B operand n_j Q_j[class = l % 32] read from the j-tile staged in LDS (128 pixels:
// 8 feature floats + CP values each, n_j multiplied in while staging).  The f32-input matrix instruction is a k-ordered fmaf chain:
// exact fp32 products, one rounding per step.  Its rate is the vector units' own; what it buys is that the C multiply-adds per
// pair leave the vector units to the ~12 operations of k, and 16 accumulator registers per tile hold all classes of 32 pixels.
// The accumulators reach the update through LDS (the tile's buffer, 32 rows per wave at a time, row stride CP + 1): the matrix
// layout has a pixel's classes across 32 lanes, the softmax wants them in one.
#include "common.h"

namespace {

constexpr int CRF_TI = 256;    // i-pixels per workgroup of the dense pass
constexpr int CRF_TJ = 128;    // j-pixels per LDS tile
constexpr int CRF_F = 8;       // floats per staged feature row (5 used)
constexpr int CRF_MAX_C = 64;
constexpr float CRF_EPS = 1e-20f;
constexpr float CRF_NEG_HALF_LOG2E = -0.72134752044448170368f;  // exp(-0.5 d) = 2^(d * this)

struct CrfShape {
  int N, H, W, C, CP, C_used;
};

__device__ __forceinline__ float crf_kernel_value(float d2) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_exp2f(d2 * CRF_NEG_HALF_LOG2E);  // v_exp_f32: 1 ulp; below 2^-126 it gives 0, which such a pair is worth
#else
  return d2;
#endif
}

// s[0..C) holds the logits of one pixel (private to the calling thread: LDS, its own row of `pre`, or qrow itself); leaves exp(v - max)
// there unless it is qrow.
// Writes Q^{t+1} pixel-major (pads 0) and, for the last iteration, Q as [C][N] and the label.
__device__ __forceinline__ void crf_softmax_row(float* s, const CrfShape sh, float* qrow, float* __restrict__ qout,
                                                uint8_t* __restrict__ label) {
  float m = s[0];
  for (int c = 1; c < sh.C; ++c) m = fmaxf(m, s[c]);
  float sum = 0.f;
  for (int c = 0; c < sh.C; ++c) {
    const float e = expf(s[c] - m);
    s[c] = e;
    sum += e;
  }
  float best = -1.f;
  int arg = 0;
  for (int c = 0; c < sh.C; ++c) {
    const float q = s[c] / sum;
    qrow[c] = q;
    if (qout) qout[(size_t)c * sh.N] = q;
    if (c < sh.C_used && q > best) best = q, arg = c;  // strictly greater: the first maximum
  }
  for (int c = sh.C; c < sh.CP; ++c) qrow[c] = 0.f;
  if (label) *label = (uint8_t)arg;
}

// one thread per pixel; blockIdx.y = image
__global__ __launch_bounds__(256) void crf_init_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ rgb, float* __restrict__ U,
                                                       float* __restrict__ Q, float* __restrict__ feat, float* __restrict__ qout,
                                                       uint8_t* __restrict__ labels, CrfShape sh, float sx, float sy, float sr, float sg,
                                                       float sb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sh.N) return;
  const size_t img = blockIdx.y, p = img * sh.N + i;
  const float* z = logits + img * sh.C * sh.N + i;
  float m = z[0];
  for (int c = 1; c < sh.C; ++c) m = fmaxf(m, z[(size_t)c * sh.N]);
  float sum = 0.f;
  for (int c = 0; c < sh.C; ++c) sum += expf(z[(size_t)c * sh.N] - m);
  const float lse = logf(sum);
  float* u = U + p * sh.CP;
  float* q = Q + p * sh.CP;
  for (int c = 0; c < sh.C; ++c) {
    const float v = (z[(size_t)c * sh.N] - m) - lse;  // log_softmax
    u[c] = -v;
    q[c] = v;  // softmax(-U) is taken from -U itself, as the iteration takes it
  }
  crf_softmax_row(q, sh, q, qout ? qout + img * sh.C * sh.N + i : nullptr, labels ? labels + p : nullptr);
  if (feat) {
    const int y = i / sh.W, x = i - y * sh.W;
    const uint8_t* px = rgb + p * 3;
    float* f = feat + p * CRF_F;
    f[0] = (float)x / sx;
    f[1] = (float)y / sy;
    f[2] = (float)px[0] / sr;
    f[3] = (float)px[1] / sg;
    f[4] = (float)px[2] / sb;
    f[5] = f[6] = f[7] = 0.f;
  }
}

struct CrfWindow {
  int rx, ry;
  float sx, sy;
};

// k over the window of pixel (x, y) with every pixel (xx, yy) of it: the same expression in gnorm and gauss
__device__ __forceinline__ float crf_gauss_value(float fx, float fy, int xx, int yy, const CrfWindow w) {
  const float dx = fx - (float)xx / w.sx, dy = fy - (float)yy / w.sy;
  return crf_kernel_value(dx * dx + dy * dy);
}

__global__ __launch_bounds__(256) void crf_gnorm_kernel(float* __restrict__ ng, CrfShape sh, CrfWindow w) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sh.N) return;
  const int y = i / sh.W, x = i - y * sh.W;
  const float fx = (float)x / w.sx, fy = (float)y / w.sy;
  const int y0 = max(y - w.ry, 0), y1 = min(y + w.ry, sh.H - 1), x0 = max(x - w.rx, 0), x1 = min(x + w.rx, sh.W - 1);
  float sum = 0.f;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) sum += crf_gauss_value(fx, fy, xx, yy, w);
  ng[(size_t)blockIdx.y * sh.N + i] = 1.f / sqrtf(sum + CRF_EPS);
}

// one thread per (pixel, class), classes fastest: a wave reads whole pixel rows of Q
__global__ __launch_bounds__(256) void crf_gauss_kernel(const float* __restrict__ Q, const float* __restrict__ U, const float* __restrict__ ng,
                                                        float* __restrict__ pre, CrfShape sh, CrfWindow w, float wg) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = t / sh.CP, c = t - i * sh.CP;
  if (i >= sh.N || c >= sh.C) return;
  const size_t base = (size_t)blockIdx.y * sh.N;
  const float* q = Q + base * sh.CP + c;
  const float* n = ng + base;
  const int y = i / sh.W, x = i - y * sh.W;
  const float fx = (float)x / w.sx, fy = (float)y / w.sy;
  const int y0 = max(y - w.ry, 0), y1 = min(y + w.ry, sh.H - 1), x0 = max(x - w.rx, 0), x1 = min(x + w.rx, sh.W - 1);
  float acc = 0.f;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) {
      const int j = yy * sh.W + xx;
      acc = fmaf(crf_gauss_value(fx, fy, xx, yy, w), n[j] * q[(size_t)j * sh.CP], acc);
    }
  const size_t o = (base + i) * sh.CP + c;
  pre[o] = wg * (n[i] * acc) - U[o];
}

// without an image: Q^{t+1} = softmax(pre); one thread per pixel, `pre`'s own row is the scratch
__global__ __launch_bounds__(256) void crf_update_kernel(float* __restrict__ pre, float* __restrict__ Qnext, float* __restrict__ qout,
                                                         uint8_t* __restrict__ labels, CrfShape sh) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sh.N) return;
  const size_t img = blockIdx.y, p = img * sh.N + i;
  crf_softmax_row(pre + p * sh.CP, sh, Qnext + p * sh.CP, qout ? qout + img * sh.C * sh.N + i : nullptr, labels ? labels + p : nullptr);
}

// The all-pairs pass of the bilateral term.  NORM: n_b = 1 / sqrt(sum_j k + eps) (B = ones in class 0; NT = 1).  Otherwise the
// message and the update.  Grid: (ceil(N / 256), B).
template <int NT, bool NORM>
__global__ __launch_bounds__(256) void crf_dense_kernel(const float* __restrict__ feat, const float* __restrict__ Qcur, float* __restrict__ nb,
                                                        const float* __restrict__ pre, float* __restrict__ Qnext, float* __restrict__ qout,
                                                        uint8_t* __restrict__ labels, CrfShape sh, float wb) {
  constexpr int CP = NT * 32;
  constexpr int SB = NORM ? 0 : CRF_TJ * CP;                 // the staged n_j Q_j; its floats also hold the epilogue's 4 x 32 x (CP + 1)
  __shared__ __attribute__((aligned(16))) float s_f[CRF_TJ * CRF_F];
  __shared__ __attribute__((aligned(16))) float s_b[NORM ? 4 : SB + CRF_TJ * 2];
  static_assert(NORM || SB + CRF_TJ * 2 >= 4 * 32 * (CP + 1), "the epilogue's rows fit the tile buffer");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
  const int N = sh.N;
  const size_t base = (size_t)blockIdx.y * N;
  const float* f = feat + base * CRF_F;
  const int i0 = blockIdx.x * CRF_TI + wave * 64;

  float fi[2][5];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int i = min(i0 + it * 32 + col, N - 1);  // rows past the image repeat its last pixel and are not written
    const float4 a = *reinterpret_cast<const float4*>(f + (size_t)i * CRF_F);
    fi[it][0] = a.x, fi[it][1] = a.y, fi[it][2] = a.z, fi[it][3] = a.w, fi[it][4] = f[(size_t)i * CRF_F + 4];
  }
  f32x16 acc[2][NT];
#pragma unroll
  for (int it = 0; it < 2; ++it)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[it][nt][r] = 0.f;

  for (int j0 = 0; j0 < N; j0 += CRF_TJ) {
    __syncthreads();  // the previous tile has been read
    {                 // 128 rows x 8 floats: one float4 per thread; rows past the image are zeros (k finite, B zero)
      const int j = j0 + (threadIdx.x >> 1);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < N) v = *reinterpret_cast<const float4*>(f + (size_t)j * CRF_F + (threadIdx.x & 1) * 4);
      reinterpret_cast<float4*>(s_f)[threadIdx.x] = v;
    }
    if (!NORM) {
      const float* q = Qcur + base * CP;
      for (int t = threadIdx.x; t < CRF_TJ * CP / 4; t += 256) {
        const int r = t / (CP / 4), j = j0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < N) {
          v = *reinterpret_cast<const float4*>(q + (size_t)j * CP + (t - r * (CP / 4)) * 4);
          const float n = nb[base + j];
          v.x *= n, v.y *= n, v.z *= n, v.w *= n;
        }
        reinterpret_cast<float4*>(s_b)[t] = v;
      }
    }
    __syncthreads();
#pragma unroll 4
    for (int jj = 0; jj < CRF_TJ; jj += 2) {
      const int jr = jj + half;  // this lane's j: the K index of the matrix instruction
      const float4 a = *reinterpret_cast<const float4*>(s_f + jr * CRF_F);
      const float a4 = s_f[jr * CRF_F + 4];
      float bv[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bv[nt] = NORM ? ((col == 0 && j0 + jr < N) ? 1.f : 0.f) : s_b[jr * CP + nt * 32 + col];
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const float d0 = fi[it][0] - a.x, d1 = fi[it][1] - a.y, d2 = fi[it][2] - a.z, d3 = fi[it][3] - a.w, d4 = fi[it][4] - a4;
        const float k = crf_kernel_value(fmaf(d4, d4, fmaf(d3, d3, fmaf(d2, d2, fmaf(d1, d1, d0 * d0)))));
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[it][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(k, bv[nt], acc[it][nt], 0, 0, 0);
      }
    }
  }

  // register r of lane l holds row 8 (r / 4) + 4 (l / 32) + r % 4, column l % 32 of a 32 x 32 tile
  if (NORM) {
    if (col == 0) {
#pragma unroll
      for (int it = 0; it < 2; ++it)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = i0 + it * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
          if (i < N) nb[base + i] = 1.f / sqrtf(acc[it][0][r] + CRF_EPS);
        }
    }
    return;
  }
  float* stage = s_b + wave * (32 * (CP + 1));
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    __syncthreads();  // the tile (it = 0) or the rows of the first half (it = 1) have been read
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) stage[(8 * (r >> 2) + 4 * half + (r & 3)) * (CP + 1) + nt * 32 + col] = acc[it][nt][r];
    __syncthreads();
    const int i = i0 + it * 32 + lane;
    if (lane < 32 && i < N) {
      float* s = stage + lane * (CP + 1);
      const size_t p = base + i;
      const float w = wb * nb[p];
      const float* g = pre + p * CP;
      for (int c = 0; c < sh.C; ++c) s[c] = g[c] + w * s[c];
      crf_softmax_row(s, sh, Qnext + p * CP, qout ? qout + (size_t)blockIdx.y * sh.C * N + i : nullptr, labels ? labels + p : nullptr);
    }
  }
}

size_t crf_pad(size_t b) { return (b + 255) & ~(size_t)255; }

int crf_cp(int C) { return C <= 32 ? 32 : 64; }

struct CrfLayout {
  size_t u, q0, q1, pre, ng, nb, feat, total;
};

CrfLayout crf_layout(int64_t B, int64_t C, int64_t H, int64_t W, bool with_image) {
  const size_t pix = (size_t)(B * H * W), row = pix * crf_cp((int)C) * sizeof(float);
  CrfLayout l;
  size_t at = 0;
  l.u = at, at += crf_pad(row);
  l.q0 = at, at += crf_pad(row);
  l.q1 = at, at += crf_pad(row);
  l.pre = at, at += crf_pad(row);
  l.ng = at, at += crf_pad(pix * sizeof(float));
  l.nb = at, at += with_image ? crf_pad(pix * sizeof(float)) : 0;
  l.feat = at, at += with_image ? crf_pad(pix * CRF_F * sizeof(float)) : 0;
  l.total = at;
  return l;
}

// what the index arithmetic covers: pixel-major offsets of 64 floats per pixel stay below 2^31 (the kernels widen before they multiply,
// the launch grids do not), one image per blockIdx.y
bool crf_dims_ok(int64_t B, int64_t C, int64_t H, int64_t W) {
  return B >= 1 && H >= 1 && W >= 1 && C >= 1 && C <= CRF_MAX_C && B <= 65535 && H * W <= (1ll << 24) && B * H * W * CRF_MAX_C < (1ll << 31);
}

}  // namespace

extern "C" size_t mcdseg_dense_crf_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t with_image) {
  if (!crf_dims_ok(B, C, H, W)) return 0;
  return crf_layout(B, C, H, W, with_image != 0).total;
}

extern "C" int mcdseg_dense_crf(const float* logits, const uint8_t* rgb, const float* params, float* q, uint8_t* labels, int32_t C_used,
                                int32_t B, int32_t C, int32_t H, int32_t W, int32_t n_iters, void* ws, size_t ws_bytes, void* stream) {
  MCD_REQUIRE(logits && params && ws, "dense_crf: null pointer (logits, params and workspace are needed)");
  MCD_REQUIRE(q || labels, "dense_crf: neither q nor labels is asked for");
  MCD_REQUIRE(C >= 1 && C <= CRF_MAX_C, "dense_crf: C = %d, must be in [1, %d]", C, CRF_MAX_C);
  MCD_REQUIRE(C_used >= 1 && C_used <= C, "dense_crf: C_used = %d, must be in [1, C = %d]", C_used, C);
  MCD_REQUIRE(B >= 1 && H >= 1 && W >= 1, "dense_crf: bad dims B = %d, H = %d, W = %d", B, H, W);
  MCD_REQUIRE(crf_dims_ok(B, C, H, W), "dense_crf: too large: H*W must not exceed 2^24, B*H*W*64 must stay below 2^31 and B at most 65535");
  MCD_REQUIRE(n_iters >= 0, "dense_crf: n_iters = %d is negative", n_iters);
  const float sxg = params[0], syg = params[1], wg = params[2], sxb = params[3], syb = params[4], wb = params[5], sr = params[6],
              sg = params[7], sb = params[8];
  MCD_REQUIRE(sxg > 0.f && syg > 0.f && sxg <= 3.0e37f && syg <= 3.0e37f, "dense_crf: sxy_gaussian must be positive and finite");
  MCD_REQUIRE(wg == wg && wb == wb, "dense_crf: a compatibility is NaN");
  if (rgb)
    MCD_REQUIRE(sxb > 0.f && syb > 0.f && sr > 0.f && sg > 0.f && sb > 0.f && sxb <= 3.0e37f && syb <= 3.0e37f && sr <= 3.0e37f &&
                    sg <= 3.0e37f && sb <= 3.0e37f,
                "dense_crf: sxy_bilateral and srgb_bilateral must be positive and finite");
  const CrfLayout l = crf_layout(B, C, H, W, rgb != nullptr);
  MCD_REQUIRE(ws_bytes >= l.total, "dense_crf: workspace too small (%zu bytes, mcdseg_dense_crf_workspace_bytes asks for %zu)", ws_bytes,
              l.total);
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "dense_crf: workspace must be 16-byte aligned");
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(logits) & 3) == 0 && (reinterpret_cast<uintptr_t>(q) & 3) == 0,
              "dense_crf: logits and q must be 4-byte aligned");

  hipStream_t st = (hipStream_t)stream;
  CrfShape sh;
  sh.N = H * W, sh.H = H, sh.W = W, sh.C = C, sh.CP = crf_cp(C), sh.C_used = C_used;
  char* base = (char*)ws;
  float* U = (float*)(base + l.u);
  float* Q[2] = {(float*)(base + l.q0), (float*)(base + l.q1)};
  float* pre = (float*)(base + l.pre);
  float* ng = (float*)(base + l.ng);
  float* nb = rgb ? (float*)(base + l.nb) : nullptr;
  float* feat = rgb ? (float*)(base + l.feat) : nullptr;
  CrfWindow win;
  win.sx = sxg, win.sy = syg;
  // ceil(7.5 s), and never beyond the image (which also keeps the float -> int conversion in range)
  win.rx = (int)fminf(ceilf(7.5f * sxg), (float)W), win.ry = (int)fminf(ceilf(7.5f * syg), (float)H);
  const dim3 pix(ceil_div(sh.N, 256), B), cls((unsigned)ceil_div64((int64_t)sh.N * sh.CP, 256), B), tiles(ceil_div(sh.N, CRF_TI), B);
  const bool only_init = n_iters == 0;
  hipLaunchKernelGGL(crf_init_kernel, pix, dim3(256), 0, st, logits, rgb, U, Q[0], feat, only_init ? q : nullptr,
                     only_init ? labels : nullptr, sh, sxb, syb, sr, sg, sb);
  if (!only_init) {
    hipLaunchKernelGGL(crf_gnorm_kernel, pix, dim3(256), 0, st, ng, sh, win);
    if (rgb)
      hipLaunchKernelGGL((crf_dense_kernel<1, true>), tiles, dim3(256), 0, st, feat, (const float*)nullptr, nb, (const float*)nullptr,
                         (float*)nullptr, (float*)nullptr, (uint8_t*)nullptr, sh, 0.f);
  }
  for (int t = 0; t < n_iters; ++t) {
    const bool last = t == n_iters - 1;
    float* cur = Q[t & 1];
    float* next = Q[(t + 1) & 1];
    float* qo = last ? q : nullptr;
    uint8_t* lo = last ? labels : nullptr;
    hipLaunchKernelGGL(crf_gauss_kernel, cls, dim3(256), 0, st, cur, U, ng, pre, sh, win, wg);
    if (!rgb)
      hipLaunchKernelGGL(crf_update_kernel, pix, dim3(256), 0, st, pre, next, qo, lo, sh);
    else if (sh.CP == 32)
      hipLaunchKernelGGL((crf_dense_kernel<1, false>), tiles, dim3(256), 0, st, feat, cur, nb, pre, next, qo, lo, sh, wb);
    else
      hipLaunchKernelGGL((crf_dense_kernel<2, false>), tiles, dim3(256), 0, st, feat, cur, nb, pre, next, qo, lo, sh, wb);
  }
  MCD_LAUNCH_CHECK("dense_crf");
  return 0;
}
