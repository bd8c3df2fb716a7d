// The seg2bd branch of the triple multitask decoder (MCDTripleMultiTaskDecoder.get_boundary_loss_by_extra_conv,
// models/dilated_fcn.py:960-981, with seg2bd_conv of :863-864 and bce2d of loss.py:131-138):
//   loss_h = bce2d(sigmoid(conv5x5(up8(z_h)) + b), t)        for the two heads' low-resolution logits z_h [N,C,Hi,Wi]
// from the low-resolution logits in one pass each way.  The x8 bilinear map B and the 5x5 cross-correlation are both linear, and B
// has no parameters, so the channel sum commutes with B:
//   forward    S[k] = sum_c w[c,k] z[c]              25 low-resolution planes per image (k = 5 i + j: one per tap)
//              v[y,x] = b + sum_k (B S[k])[y+i-2, x+j-2]   with (B S[k]) read as 0 outside the image (the padding pads the up-sampled map)
//   backward   g = dL/dv = bce_grad(q, t) q (1 - q)  one full-resolution plane
//              T[k] = B^T (g shifted by tap k)       25 low-resolution planes per image, gather form
//              dz[c] = sum_k w[c,k] T[k],   dw[c,k] = sum_{n,pixels} z[c] T[k],   db = sum g
// No C-channel full-resolution tensor exists in either pass: the work per full-resolution pixel is 25 bilinear reads (forward) or 100
// gather taps (backward) instead of 25 C multiply-adds, and the C-dependent part runs on 1/64 of the pixels.  Full resolution holds v
// and g only, one plane per head each.  Every sum leaves its block as an fp64 partial that a small kernel finishes in a fixed order; no
// float atomics, so two launches are bitwise equal.  The BCE arithmetic is boundary_blocks.h's, i.e. mcdseg_bce2d's.
#include "common.h"
#include "boundary_blocks.h"

namespace {

constexpr int TAPS = 25;
constexpr int DW_ROWS = 64;     // low-resolution pixels per tile of the weight-gradient kernel
constexpr int DW_CH = 12;       // channels 256 consecutive (c, k) pairs can span: 256 / 25 + 2
constexpr int DW_CHUNKS = 128;  // blocks along the pixel axis of the weight-gradient kernel: rows of fp64 partials

struct Layout {  // of the workspace; doubles first
  int nb;        // blocks of the full-resolution passes, per head
  size_t loss_part, db_part, dw_part, v, g, st, bytes;
};

Layout layout_of(int N, int C, int Hi, int Wi) {
  Layout l;
  const size_t px = (size_t)N * Hi * Wi * 64;
  l.nb = sum_blocks((int64_t)px);
  l.loss_part = 0;
  l.db_part = l.loss_part + (size_t)2 * l.nb * 3 * sizeof(double);
  l.dw_part = l.db_part + (size_t)2 * l.nb * sizeof(double);
  l.v = l.dw_part + (size_t)DW_CHUNKS * C * TAPS * sizeof(double);
  l.g = l.v + 2 * px * sizeof(float);
  l.st = l.g + 2 * px * sizeof(float);
  l.bytes = l.st + (size_t)2 * N * TAPS * Hi * Wi * sizeof(float);
  return l;
}

// ---------------------------------------------------------------------------------------------------------- forward
// S[head][n][k][p] = sum_c w[c][k] z_head[n][c][p]: one thread per low-resolution pixel, channels in order
__global__ __launch_bounds__(256) void seg2bd_project_kernel(const float* __restrict__ z1, const float* __restrict__ z2, const float* __restrict__ w,
                                                             float* __restrict__ S, int N, int C, int P) {
  const int head = blockIdx.z, n = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float* zp = (head ? z2 : z1) + (size_t)n * C * P + p;
  float acc[TAPS];
#pragma unroll
  for (int k = 0; k < TAPS; ++k) acc[k] = 0.f;
  for (int c = 0; c < C; ++c) {
    const float zc = zp[(size_t)c * P];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) acc[k] = fmaf(w[c * TAPS + k], zc, acc[k]);
  }
  float* out = S + ((size_t)(head * N + n) * TAPS) * P + p;
#pragma unroll
  for (int k = 0; k < TAPS; ++k) out[(size_t)k * P] = acc[k];
}

// one full-resolution pixel per thread: v from the 25 planes of S, each read through the bilinear map at its tap's position; q, the
// three sums of the loss
template <typename T>
__global__ __launch_bounds__(256) void seg2bd_fwd_kernel(const float* __restrict__ S, const float* __restrict__ bias, const T* __restrict__ tgt,
                                                         int64_t tstride, float* __restrict__ v, double* __restrict__ part, int N, int Hi, int Wi,
                                                         int64_t total) {
  const int head = blockIdx.y;
  const int H = 8 * Hi, W = 8 * Wi, P = Hi * Wi;
  const int64_t HW = (int64_t)H * W;
  const float b = *bias;
  Sums s = {0.f, 0.f, 0.f};
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(idx / HW);
    const int r = (int)(idx - n * HW);
    const int y = r / W, x = r - y * W;
    const float* Sn = S + ((size_t)(head * N + n) * TAPS) * P;
    int x0[5], x1[5];
    float lx0[5], lx1[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) src_index_s<8>(x + j - 2, Wi, x0[j], x1[j], lx0[j], lx1[j]);  // (a position outside the image is skipped below)
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int yy = y + i - 2;
      if (yy < 0 || yy >= H) continue;
      int y0, y1;
      float ly0, ly1;
      src_index_s<8>(yy, Hi, y0, y1, ly0, ly1);
      float row = 0.f;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int xx = x + j - 2;
        if (xx < 0 || xx >= W) continue;
        const float* r0 = Sn + (size_t)(i * 5 + j) * P + y0 * Wi;
        const float* r1 = Sn + (size_t)(i * 5 + j) * P + y1 * Wi;
        row += ly0 * (lx0[j] * r0[x0[j]] + lx1[j] * r0[x1[j]]) + ly1 * (lx0[j] * r1[x0[j]] + lx1[j] * r1[x1[j]]);
      }
      acc += row;
    }
    const float vv = acc + b;
    v[(size_t)head * total + idx] = vv;
    sums_add(s, sigm(vv), (float)tgt[(size_t)n * tstride + r]);
  }
  sums_store(s, part + (size_t)head * gridDim.x * 3);
}

// out[0], out[1] = the two heads' losses (out[1] = 0 with one head), out[2] = beta = 1 - sum t / n; bce_finalize_kernel (boundary.hip) per head
__global__ __launch_bounds__(256) void seg2bd_finalize_kernel(const double* __restrict__ part, int nblk, int heads, double n, float* __restrict__ out) {
  for (int h = 0; h < 2; ++h) {
    if (h >= heads) {
      if (threadIdx.x == 0) out[h] = 0.f;
      continue;
    }
    double tot[3];
    partials_total(part + (size_t)h * nblk * 3, nblk, 3, 0, tot);
    if (threadIdx.x == 0) {
      double loss, beta;
      balanced_bce(tot, n, loss, beta);
      out[h] = (float)loss;
      if (h == 0) out[2] = (float)beta;
    }
    __syncthreads();  // the second head reuses the LDS slots
  }
}

// ---------------------------------------------------------------------------------------------------------- backward
// g = dL/dv = bce2d_bwd's dq times sigmoid' (torch's grad * (1 - q) * q), and the block's fp64 partial of sum g
template <typename T>
__global__ __launch_bounds__(256) void seg2bd_dv_kernel(const float* __restrict__ v, const T* __restrict__ tgt, int64_t tstride,
                                                        const float* __restrict__ beta_p, const float* __restrict__ up, float inv_n,
                                                        float* __restrict__ g, double* __restrict__ part, int64_t HW, int64_t total) {
  const int head = blockIdx.y;
  const float beta = *beta_p;
  const float gs = (up ? up[head] : 1.f) * inv_n;
  float sum = 0.f;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = idx / HW;
    const float q = sigm(v[(size_t)head * total + idx]);
    const float d = (bce_grad(q, (float)tgt[(size_t)n * tstride + (idx - n * HW)], beta, gs) * (1.f - q)) * q;
    g[(size_t)head * total + idx] = d;
    sum += d;
  }
  __shared__ double sh[1][4];
  double a[1] = {(double)sum};
  block_gather(a, sh);
  if (threadIdx.x == 0) part[(size_t)head * gridDim.x + blockIdx.x] = tree_total<4>(sh[0]);
}

// T[head][n][k][iy,ix] = sum over the up-sampled pixels (oy, ox) low-resolution pixel (iy, ix) feeds -- rows / columns [8 i - 4, 8 i + 12)
// of the image -- of B's weight times g at the pixel whose tap k reads (oy, ox): g[oy - i + 2, ox - j + 2].  Gather form, one thread per
// value, the order of bilinear8_bwd's sums.
__global__ __launch_bounds__(256) void seg2bd_gather_kernel(const float* __restrict__ g, float* __restrict__ T, int Hi, int Wi) {
  const int H = 8 * Hi, W = 8 * Wi, P = Hi * Wi;
  const int plane = blockIdx.y;  // (head * N + n) * 25 + k
  const int k = plane % TAPS;
  const int di = k / 5 - 2, dj = k % 5 - 2;
  const float* gi = g + (size_t)(plane / TAPS) * H * W;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < P; idx += gridDim.x * blockDim.x) {
    const int iy = idx / Wi;
    const int ix = idx - iy * Wi;
    const int oy0 = 8 * iy - 4, ox0 = 8 * ix - 4;
    float wx[16];
#pragma unroll
    for (int kx = 0; kx < 16; ++kx) {
      const int ox = ox0 + kx, gx = ox - dj;
      wx[kx] = (ox >= 0 && ox < W && gx >= 0 && gx < W) ? tap_weight_s<8>(ox, Wi, ix) : 0.f;
    }
    float acc = 0.f;
    for (int ky = 0; ky < 16; ++ky) {
      const int oy = oy0 + ky, gy = oy - di;
      if (oy < 0 || oy >= H || gy < 0 || gy >= H) continue;
      const float wy = tap_weight_s<8>(oy, Hi, iy);
      if (wy == 0.f) continue;  // (a clamped edge tap)
      const float* row = gi + (size_t)gy * W;
      float r = 0.f;
#pragma unroll
      for (int kx = 0; kx < 16; ++kx) {
        if (wx[kx] == 0.f) continue;
        r = fmaf(row[ox0 + kx - dj], wx[kx], r);
      }
      acc = fmaf(wy, r, acc);
    }
    T[(size_t)plane * P + idx] = acc;
  }
}

// dz_head[n][c][p] = sum_k w[c][k] T[head][n][k][p]
__global__ __launch_bounds__(256) void seg2bd_dz_kernel(const float* __restrict__ T, const float* __restrict__ w, float* __restrict__ dz1,
                                                        float* __restrict__ dz2, int N, int C, int P) {
  const int head = blockIdx.z, n = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float* tp = T + ((size_t)(head * N + n) * TAPS) * P + p;
  float t[TAPS];
#pragma unroll
  for (int k = 0; k < TAPS; ++k) t[k] = tp[(size_t)k * P];
  float* out = (head ? dz2 : dz1) + (size_t)n * C * P + p;
  for (int c = 0; c < C; ++c) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < TAPS; ++k) acc = fmaf(w[c * TAPS + k], t[k], acc);
    out[(size_t)c * P] = acc;
  }
}

// dw[c][k] = sum over heads, images and low-resolution pixels of z[c] T[k]: thread = one (c, k) pair, a block's 256 pairs span at most
// DW_CH channels; tiles of DW_ROWS pixels go through LDS (rows padded to 65 floats: the 25 k rows a wave reads lie in distinct banks),
// products and sums in fp64, one partial row per block along y
__global__ __launch_bounds__(256) void seg2bd_dw_kernel(const float* __restrict__ z1, const float* __restrict__ z2, const float* __restrict__ T,
                                                        double* __restrict__ part, int heads, int N, int C, int P) {
  __shared__ float zt[DW_CH][DW_ROWS + 1];
  __shared__ float tt[TAPS][DW_ROWS + 1];
  const int pairs = C * TAPS;
  const int pair = blockIdx.x * 256 + threadIdx.x;
  const int c_lo = (blockIdx.x * 256) / TAPS;
  const int c = pair / TAPS, k = pair - c * TAPS;
  const int64_t rows = (int64_t)heads * N * P;
  const int64_t tiles = (rows + DW_ROWS - 1) / DW_ROWS;
  double acc = 0.0;
  for (int64_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
    for (int e = threadIdx.x; e < (DW_CH + TAPS) * DW_ROWS; e += 256) {
      const int line = e / DW_ROWS, m = e - line * DW_ROWS;
      const int64_t row = tile * DW_ROWS + m;
      float val = 0.f;
      if (row < rows) {
        const int hn = (int)(row / P);  // head * N + n
        const int p = (int)(row - (int64_t)hn * P);
        if (line < DW_CH) {
          const int cc = c_lo + line;
          if (cc < C) val = (hn >= N ? z2 : z1)[((size_t)(hn >= N ? hn - N : hn) * C + cc) * P + p];
        } else {
          val = T[((size_t)hn * TAPS + (line - DW_CH)) * P + p];
        }
      }
      if (line < DW_CH)
        zt[line][m] = val;
      else
        tt[line - DW_CH][m] = val;
    }
    __syncthreads();
    if (pair < pairs) {
#pragma unroll 8
      for (int m = 0; m < DW_ROWS; ++m) acc += (double)zt[c - c_lo][m] * (double)tt[k][m];
    }
    __syncthreads();
  }
  if (pair < pairs) part[(size_t)blockIdx.y * pairs + pair] = acc;
}

// finishes dw (one thread per pair, the partial rows in order) and, in the block behind the last, db
__global__ __launch_bounds__(256) void seg2bd_dw_finalize_kernel(const double* __restrict__ dw_part, int chunks, int pairs, const double* __restrict__ db_part,
                                                                 int ndb, float* __restrict__ dw, float* __restrict__ db) {
  if (blockIdx.x + 1 < gridDim.x) {
    const int pair = blockIdx.x * 256 + threadIdx.x;
    if (pair >= pairs) return;
    double s = 0.0;
    for (int i = 0; i < chunks; ++i) s += dw_part[(size_t)i * pairs + pair];
    dw[pair] = (float)s;
    return;
  }
  double tot[1];
  partials_total(db_part, ndb, 1, 0, tot);
  if (threadIdx.x == 0) db[0] = (float)tot[0];
}

bool seg2bd_args_ok(int N, int C, int Hi, int Wi) {
  return N > 0 && C > 0 && Hi > 0 && Wi > 0 && (int64_t)Hi * Wi * 64 < (1ll << 31) && (int64_t)N * 2 * TAPS < 65536 && (int64_t)C * TAPS < (1ll << 24);
}

int dw_chunks(int heads, int N, int P) {
  const int64_t tiles = ceil_div64((int64_t)heads * N * P, DW_ROWS);
  return (int)(tiles < DW_CHUNKS ? tiles : DW_CHUNKS);
}

}  // namespace

extern "C" size_t mcdseg_seg2bd_bce_workspace_bytes(int32_t N, int32_t C, int32_t Hi, int32_t Wi) {
  return seg2bd_args_ok(N, C, Hi, Wi) ? layout_of(N, C, Hi, Wi).bytes : 0;
}

extern "C" int mcdseg_seg2bd_bce_fwd(const float* z1, const float* z2, const float* w, const float* b, const void* target, int32_t target_u8,
                                     int64_t target_batch_stride, float* out, int32_t N, int32_t C, int32_t Hi, int32_t Wi, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(z1 && w && b && target && out && workspace && seg2bd_args_ok(N, C, Hi, Wi), "seg2bd_bce_fwd: bad arguments");
  MCD_REQUIRE(target_batch_stride >= (int64_t)Hi * Wi * 64, "seg2bd_bce_fwd: the target's batch stride is smaller than a plane");
  MCD_REQUIRE(target_u8 || (reinterpret_cast<uintptr_t>(target) & 3) == 0, "seg2bd_bce_fwd: an fp32 target must be 4-byte aligned");
  const Layout l = layout_of(N, C, Hi, Wi);
  MCD_REQUIRE(workspace_bytes >= l.bytes && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "seg2bd_bce_fwd: workspace too small or not 8-byte aligned");
  char* ws = (char*)workspace;
  const int heads = z2 ? 2 : 1, P = Hi * Wi;
  const int64_t total = (int64_t)N * P * 64;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(seg2bd_project_kernel, dim3(ceil_div(P, 256), N, heads), dim3(256), 0, st, z1, z2, w, (float*)(ws + l.st), N, C, P);
  MCD_LAUNCH_CHECK("seg2bd_project");
  if (target_u8)
    hipLaunchKernelGGL(seg2bd_fwd_kernel<uint8_t>, dim3(l.nb, heads), dim3(256), 0, st, (const float*)(ws + l.st), b, (const uint8_t*)target,
                       target_batch_stride, (float*)(ws + l.v), (double*)(ws + l.loss_part), N, Hi, Wi, total);
  else
    hipLaunchKernelGGL(seg2bd_fwd_kernel<float>, dim3(l.nb, heads), dim3(256), 0, st, (const float*)(ws + l.st), b, (const float*)target,
                       target_batch_stride, (float*)(ws + l.v), (double*)(ws + l.loss_part), N, Hi, Wi, total);
  MCD_LAUNCH_CHECK("seg2bd_fwd");
  hipLaunchKernelGGL(seg2bd_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)(ws + l.loss_part), l.nb, heads, (double)total, out);
  MCD_LAUNCH_CHECK("seg2bd_finalize");
  return 0;
}

extern "C" int mcdseg_seg2bd_bce_bwd(const float* z1, const float* z2, const float* w, const float* b, const void* target, int32_t target_u8,
                                     int64_t target_batch_stride, const float* beta, const float* upstream, float* dz1, float* dz2, float* dw,
                                     float* db, int32_t N, int32_t C, int32_t Hi, int32_t Wi, void* workspace, size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(z1 && w && b && target && beta && dz1 && (!z2 == !dz2) && dw && db && workspace && seg2bd_args_ok(N, C, Hi, Wi),
              "seg2bd_bce_bwd: bad arguments");
  MCD_REQUIRE(target_batch_stride >= (int64_t)Hi * Wi * 64, "seg2bd_bce_bwd: the target's batch stride is smaller than a plane");
  MCD_REQUIRE(target_u8 || (reinterpret_cast<uintptr_t>(target) & 3) == 0, "seg2bd_bce_bwd: an fp32 target must be 4-byte aligned");
  const Layout l = layout_of(N, C, Hi, Wi);
  MCD_REQUIRE(workspace_bytes >= l.bytes && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "seg2bd_bce_bwd: workspace too small or not 8-byte aligned");
  char* ws = (char*)workspace;
  const int heads = z2 ? 2 : 1, P = Hi * Wi, pairs = C * TAPS;
  const int64_t HW = (int64_t)P * 64, total = (int64_t)N * HW;
  const float inv_n = (float)(1.0 / (double)total);
  float* g = (float*)(ws + l.g);
  float* T = (float*)(ws + l.st);
  hipStream_t st = (hipStream_t)stream;
  if (target_u8)
    hipLaunchKernelGGL(seg2bd_dv_kernel<uint8_t>, dim3(l.nb, heads), dim3(256), 0, st, (const float*)(ws + l.v), (const uint8_t*)target, target_batch_stride,
                       beta, upstream, inv_n, g, (double*)(ws + l.db_part), HW, total);
  else
    hipLaunchKernelGGL(seg2bd_dv_kernel<float>, dim3(l.nb, heads), dim3(256), 0, st, (const float*)(ws + l.v), (const float*)target, target_batch_stride,
                       beta, upstream, inv_n, g, (double*)(ws + l.db_part), HW, total);
  MCD_LAUNCH_CHECK("seg2bd_dv");
  int gchunks = ceil_div(P, 256);
  if (gchunks > 64) gchunks = 64;
  hipLaunchKernelGGL(seg2bd_gather_kernel, dim3(gchunks, heads * N * TAPS), dim3(256), 0, st, (const float*)g, T, Hi, Wi);
  MCD_LAUNCH_CHECK("seg2bd_gather");
  hipLaunchKernelGGL(seg2bd_dz_kernel, dim3(ceil_div(P, 256), N, heads), dim3(256), 0, st, (const float*)T, w, dz1, dz2, N, C, P);
  MCD_LAUNCH_CHECK("seg2bd_dz");
  const int chunks = dw_chunks(heads, N, P);
  hipLaunchKernelGGL(seg2bd_dw_kernel, dim3(ceil_div(pairs, 256), chunks), dim3(256), 0, st, z1, z2, (const float*)T, (double*)(ws + l.dw_part), heads, N,
                     C, P);
  MCD_LAUNCH_CHECK("seg2bd_dw");
  hipLaunchKernelGGL(seg2bd_dw_finalize_kernel, dim3(ceil_div(pairs, 256) + 1), dim3(256), 0, st, (const double*)(ws + l.dw_part), chunks, pairs,
                     (const double*)(ws + l.db_part), heads * l.nb, dw, db);
  MCD_LAUNCH_CHECK("seg2bd_dw_finalize");
  return 0;
}
