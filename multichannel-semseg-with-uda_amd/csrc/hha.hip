// Depth -> HHA (horizontal disparity, height above ground, angle with gravity: Gupta, Girshick, Arbelaez, Malik, ECCV 2014) on the
// device.  The definition is DESIGN.md section 4.13 (its fp64 numpy statement: tests/hha_ref.py), per image of P = H*W pixels:
//     Z fp32 centimetres, missing where <= 0 or not finite;  a = (u - cx)/fx, b = (v - cy)/fy, P = (aZ, bZ, Z), q = 100/Z
//     normals, for R = 3 and R = 10: the nine moments a^2 ab a b^2 b 1 | aq bq q (0 at a missing pixel) summed over the window
//         [v-R, v+R] x [u-R, u+R] clipped to the image -> M (3x3 symmetric), t;  n = adj(M) t, N = n/|n|, N_z >= 0;
//         (0,0,0) where the window holds fewer than 3 valid pixels or |n| is 0 (up to 1e-14 of its terms' scale: valid pixels on one
//         line, where fp64 leaves rounding noise) or not finite
//     gravity g from the R = 10 normals: g = (0,1,0); 5 iterations at 45 degrees, 5 at 15: s = g.N, F = {|s| > cos}, W = {|s| < sin},
//         A = sum_W N N^T - sum_F N N^T, g' = the unit eigenvector of A's smallest eigenvalue, g = +-g' with g.g' >= 0
//     h = -g.P; y_min = min over valid pixels, -130 if that is > -90; h -= y_min
//     bytes: 31000/max(Z,100) | h | acosd(clamp(N3.g)) + 38 (0 where N3 is invalid), rounded half away from zero, saturated
// All arithmetic is fp64 (the pass is bound by HBM and LDS, not by the vector units; the adjugate cancels ~10 digits on a 7 x 7 window),
// no atomics, every sum in one fixed order that depends on H and W alone: the same bits run to run and for an image alone or in a batch.
//
// The passes, each a kernel; they hand over through kernel boundaries only, and g never leaves the device:
//     camera     the cameras (<= 64 per launch, by value) as fp64 into the workspace; g = (0,1,0)
//     normals    a workgroup owns 16 x 16 pixels.  It stages q of the 36 x 36 tile-with-halo in LDS (0 outside the image and at missing
//                pixels: clipping and holes are the same case), then forms the window sums SEPARABLY: 5 row sums per staged row and
//                output column (v, va, va^2, q, aq over 21 taps; the 7 middle taps also feed the R = 3 sums) -- b is constant along a row,
//                so the nine moments are these five times 1, b, b^2 -- then 21 (7) rows per pixel.  84 + 189 LDS reads per pixel where
//                the plain window takes 9 x (441 + 49).  Both radii, all nine planes, one pass.
//     per iteration (10x):  gravity_partial  grid (nb, N): fp64 block partials of the twelve outer-product sums (block_reduce.h: wave sums,
//                                            one barrier, the pairwise tree)
//                           gravity_final    grid (N): the partial rows in block order (partials_total), then cyclic Jacobi on A, new g
//     ymin_partial / ymin_final   the same two-stage shape with min; the final also writes g as fp32 where asked for
//     encode     one thread per pixel: the three bytes, and the height where asked for
#include <float.h>

#include "block_reduce.h"
#include "common.h"

namespace {

constexpr int HHA_T = 16;                     // tile edge: 256 threads, one pixel each
constexpr int HHA_R = 10, HHA_R3 = 3;         // the two window radii
constexpr int HHA_S = HHA_T + 2 * HHA_R;      // 36: staged edge
constexpr int HHA_PER_BLOCK = 2048;           // pixels per reduction block (until HHA_MAX_BLOCKS are reached)
constexpr int HHA_MAX_BLOCKS = 128;
constexpr int HHA_CAM_PACK = 64;
constexpr double HHA_DEG = 57.295779513082320877;  // 180 / pi
// |n| <= this x max(sum a^2, sum b^2, count)^2 x max|t| counts as 0.  The constant is meant for fx, fy up to about 1000 pixels (VGA and HD depth cameras).  The smallest ratio of a window whose valid
// pixels do NOT lie on one line, measured on a room with 93 % of the pixels missing (three-pixel windows): 2e-12 at fx = 365, 6e-13 at 520,
// 3e-13 at 600, 3e-14 at 1050, 1e-14 at 1400 -- the collinear ones stay below 1e-15 at every fx.  Beyond fx ~ 1400 a window of three
// adjacent pixels counts as degenerate too; windows of six and more pixels were never dropped.
constexpr double HHA_DEGENERATE = 1e-14;

struct HhaCameraPack {
  float v[HHA_CAM_PACK][4];
};

struct HhaShape {
  int N, H, W, P, nb, tiles_x;
};

__device__ __forceinline__ bool hha_valid(float z) { return z > 0.f && z <= FLT_MAX; }  // (false for NaN)

__global__ __launch_bounds__(64) void hha_camera_kernel(HhaCameraPack pack, double* __restrict__ cam, double* __restrict__ g, int first,
                                                        int count) {
  const int i = threadIdx.x;
  if (i >= count) return;
  for (int k = 0; k < 4; ++k) cam[(size_t)(first + i) * 4 + k] = (double)pack.v[i][k];
  g[(size_t)(first + i) * 3 + 0] = 0.0, g[(size_t)(first + i) * 3 + 1] = 1.0, g[(size_t)(first + i) * 3 + 2] = 0.0;
}

// n = adj(M) t of the nine window sums; writes N (or zeros) to out[0..3)
__device__ __forceinline__ void hha_normal(const double (&m)[9], double* __restrict__ out, float* __restrict__ out32) {
  const double aa = m[0], ab = m[1], a1 = m[2], bb = m[3], b1 = m[4], n1 = m[5], ta = m[6], tb = m[7], tq = m[8];
  double nx = (bb * n1 - b1 * b1) * ta + (a1 * b1 - ab * n1) * tb + (ab * b1 - a1 * bb) * tq;
  double ny = (a1 * b1 - ab * n1) * ta + (aa * n1 - a1 * a1) * tb + (ab * a1 - aa * b1) * tq;
  double nz = (ab * b1 - bb * a1) * ta + (ab * a1 - aa * b1) * tb + (aa * bb - ab * ab) * tq;
  const double mag = sqrt(nx * nx + ny * ny + nz * nz);
  // "|n| is 0" in fp64: valid pixels on one line give adj(M) t = 0 exactly, evaluated to ~1e-16 of its terms -- rounding noise, no normal
  const double big = fmax(fmax(aa, bb), n1), scale = big * big * fmax(fmax(fabs(ta), fabs(tb)), fabs(tq));
  if (n1 >= 3.0 && mag > 0.0 && mag > HHA_DEGENERATE * scale && mag <= DBL_MAX) {
    nx /= mag, ny /= mag, nz /= mag;
    if (nz < 0.0) nx = -nx, ny = -ny, nz = -nz;
    nx += 0.0, ny += 0.0, nz += 0.0;  // no negative zeros
  } else {
    nx = ny = nz = 0.0;
  }
  out[0] = nx, out[1] = ny, out[2] = nz;
  if (out32) out32[0] = (float)nx, out32[1] = (float)ny, out32[2] = (float)nz;
}

// grid (tiles of 16 x 16, N)
__global__ __launch_bounds__(256) void hha_normals_kernel(const float* __restrict__ depth, const double* __restrict__ cam,
                                                          double* __restrict__ n3, double* __restrict__ n10, float* __restrict__ n3_out,
                                                          HhaShape sh) {
  __shared__ double s_q[HHA_S * HHA_S];
  __shared__ double s_a[HHA_S], s_b[HHA_S];
  __shared__ double s_h[10][HHA_S][HHA_T];  // [0..5) the R = 10 row sums v, va, va^2, q, aq; [5..10) the R = 3 ones
  const int img = blockIdx.y;
  const int tile_y = blockIdx.x / sh.tiles_x, tile_x = blockIdx.x - tile_y * sh.tiles_x;
  const int x0 = tile_x * HHA_T - HHA_R, y0 = tile_y * HHA_T - HHA_R;  // the staged tile's corner
  const float* z = depth + (size_t)img * sh.P;
  const double fx = cam[(size_t)img * 4 + 0], fy = cam[(size_t)img * 4 + 1], cx = cam[(size_t)img * 4 + 2], cy = cam[(size_t)img * 4 + 3];

  for (int i = threadIdx.x; i < HHA_S * HHA_S; i += 256) {
    const int r = i / HHA_S, c = i - r * HHA_S;
    const int v = y0 + r, u = x0 + c;
    double q = 0.0;
    if (v >= 0 && v < sh.H && u >= 0 && u < sh.W) {
      const float d = z[(size_t)v * sh.W + u];
      if (hha_valid(d)) q = 100.0 / (double)d;
    }
    s_q[i] = q;
  }
  if (threadIdx.x < HHA_S) {
    s_a[threadIdx.x] = ((double)(x0 + (int)threadIdx.x) - cx) / fx;
    s_b[threadIdx.x] = ((double)(y0 + (int)threadIdx.x) - cy) / fy;
  }
  __syncthreads();

  for (int i = threadIdx.x; i < HHA_S * HHA_T; i += 256) {
    const int r = i / HHA_T, c = i - r * HHA_T;
    double w[5] = {}, n[5] = {};
    for (int j = 0; j <= 2 * HHA_R; ++j) {
      const double q = s_q[r * HHA_S + c + j], a = s_a[c + j];
      const double v = q > 0.0 ? 1.0 : 0.0, va = v * a;
      const double t[5] = {v, va, va * a, q, a * q};
      const bool inner = j >= HHA_R - HHA_R3 && j <= HHA_R + HHA_R3;
      for (int k = 0; k < 5; ++k) {
        w[k] += t[k];
        if (inner) n[k] += t[k];
      }
    }
    for (int k = 0; k < 5; ++k) s_h[k][r][c] = w[k], s_h[5 + k][r][c] = n[k];
  }
  __syncthreads();

  const int ty = threadIdx.x / HHA_T, tx = threadIdx.x - ty * HHA_T;
  const int v = y0 + HHA_R + ty, u = x0 + HHA_R + tx;
  if (v >= sh.H || u >= sh.W) return;
  double m10[9] = {}, m3[9] = {};
  for (int j = 0; j <= 2 * HHA_R; ++j) {
    const int r = ty + j;
    const double b = s_b[r];
    {
      const double h1 = s_h[0][r][tx], ha = s_h[1][r][tx], haa = s_h[2][r][tx], hq = s_h[3][r][tx], haq = s_h[4][r][tx];
      const double bh1 = b * h1;
      m10[0] += haa, m10[1] += b * ha, m10[2] += ha, m10[3] += bh1 * b, m10[4] += bh1, m10[5] += h1;
      m10[6] += haq, m10[7] += b * hq, m10[8] += hq;
    }
    if (j >= HHA_R - HHA_R3 && j <= HHA_R + HHA_R3) {
      const double h1 = s_h[5][r][tx], ha = s_h[6][r][tx], haa = s_h[7][r][tx], hq = s_h[8][r][tx], haq = s_h[9][r][tx];
      const double bh1 = b * h1;
      m3[0] += haa, m3[1] += b * ha, m3[2] += ha, m3[3] += bh1 * b, m3[4] += bh1, m3[5] += h1;
      m3[6] += haq, m3[7] += b * hq, m3[8] += hq;
    }
  }
  const size_t p = ((size_t)img * sh.P + (size_t)v * sh.W + u) * 3;
  hha_normal(m10, n10 + p, nullptr);
  hha_normal(m3, n3 + p, n3_out ? n3_out + p : nullptr);
}

// the pixels [lo, hi) of block b out of nb over P pixels
__device__ __forceinline__ void hha_chunk(int P, int& lo, int& hi) {
  const int per = (P + (int)gridDim.x - 1) / (int)gridDim.x;
  lo = min((int)blockIdx.x * per, P);
  hi = min(lo + per, P);
}

// grid (nb, N): part[img][block][12] = the block's sums of xx xy xz yy yz zz over W, then over F
__global__ __launch_bounds__(256) void hha_gravity_partial_kernel(const double* __restrict__ n10, const double* __restrict__ g,
                                                                  double* __restrict__ part, HhaShape sh, double cos_t, double sin_t) {
  const int img = blockIdx.y;
  const double gx = g[(size_t)img * 3], gy = g[(size_t)img * 3 + 1], gz = g[(size_t)img * 3 + 2];
  const double* n = n10 + (size_t)img * sh.P * 3;
  int lo, hi;
  hha_chunk(sh.P, lo, hi);
  double v[12] = {};
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const double x = n[(size_t)i * 3], y = n[(size_t)i * 3 + 1], z = n[(size_t)i * 3 + 2];
    if (x == 0.0 && y == 0.0 && z == 0.0) continue;  // an invalid normal (a valid one has length 1)
    const double s = fabs(x * gx + y * gy + z * gz);
    const bool f = s > cos_t, w = s < sin_t;
    if (!f && !w) continue;
    const int o = f ? 6 : 0;  // (never both: cos >= sin at both thresholds, up to the last bit at 45 degrees, where f wins)
    v[o + 0] += x * x, v[o + 1] += x * y, v[o + 2] += x * z, v[o + 3] += y * y, v[o + 4] += y * z, v[o + 5] += z * z;
  }
  __shared__ double shm[12][4];
  block_gather(v, shm);
  if (threadIdx.x == 0) {
    double* out = part + ((size_t)img * sh.nb + blockIdx.x) * 12;
    for (int k = 0; k < 12; ++k) out[k] = tree_total<4>(shm[k]);
  }
}

// cyclic Jacobi on the symmetric 3 x 3 matrix a (upper part read); e = eigenvalues, vec[k] = the k-th eigenvector's components
__device__ void hha_jacobi3(double (&a)[3][3], double (&e)[3], double (&vec)[3][3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) vec[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    const double diag = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]);
    if (off <= 1e-300 || off <= 1e-22 * diag) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        const int r = 3 - p - q;  // the third index
        const double arp = a[min(r, p)][max(r, p)], arq = a[min(r, q)][max(r, q)];
        a[p][p] -= t * apq, a[q][q] += t * apq, a[p][q] = 0.0;
        a[min(r, p)][max(r, p)] = c * arp - s * arq;
        a[min(r, q)][max(r, q)] = s * arp + c * arq;
        for (int k = 0; k < 3; ++k) {
          const double vp = vec[k][p], vq = vec[k][q];
          vec[k][p] = c * vp - s * vq, vec[k][q] = s * vp + c * vq;
        }
      }
  }
  for (int k = 0; k < 3; ++k) e[k] = a[k][k];
}

// grid (N): sums the partial rows in block order, then the eigen-step; g is updated in place
__global__ __launch_bounds__(256) void hha_gravity_final_kernel(const double* __restrict__ part, double* __restrict__ g, HhaShape sh) {
  const int img = blockIdx.x;
  double tot[12];
  partials_total(part + (size_t)img * sh.nb * 12, sh.nb, 12, 0, tot);
  if (threadIdx.x != 0) return;
  if (tot[0] + tot[3] + tot[5] + tot[6] + tot[9] + tot[11] == 0.0) return;  // the traces count the two sets: both empty, g stays
  double a[3][3], e[3], vec[3][3];
  a[0][0] = tot[0] - tot[6], a[0][1] = tot[1] - tot[7], a[0][2] = tot[2] - tot[8];
  a[1][1] = tot[3] - tot[9], a[1][2] = tot[4] - tot[10], a[2][2] = tot[5] - tot[11];
  a[1][0] = a[2][0] = a[2][1] = 0.0;
  hha_jacobi3(a, e, vec);
  int k = 0;
  if (e[1] < e[k]) k = 1;
  if (e[2] < e[k]) k = 2;
  double x = vec[0][k], y = vec[1][k], z = vec[2][k];
  const double len = sqrt(x * x + y * y + z * z);
  x /= len, y /= len, z /= len;
  double* gi = g + (size_t)img * 3;
  if (gi[0] * x + gi[1] * y + gi[2] * z < 0.0) x = -x, y = -y, z = -z;
  gi[0] = x + 0.0, gi[1] = y + 0.0, gi[2] = z + 0.0;
}

__device__ __forceinline__ double hha_raw_height(double gx, double gy, double gz, double a, double b, double z) {
  return -(gx * (a * z) + gy * (b * z) + gz * z);
}

__device__ __forceinline__ double hha_wave_min(double v) {
  for (int m = 1; m < 64; m <<= 1) v = fmin(v, __shfl_xor(v, m));
  return v;
}

// grid (nb, N): pmin[img][block] = the smallest -g.P over the block's valid pixels (+inf without one)
__global__ __launch_bounds__(256) void hha_ymin_partial_kernel(const float* __restrict__ depth, const double* __restrict__ cam,
                                                               const double* __restrict__ g, double* __restrict__ pmin, HhaShape sh) {
  const int img = blockIdx.y;
  const double gx = g[(size_t)img * 3], gy = g[(size_t)img * 3 + 1], gz = g[(size_t)img * 3 + 2];
  const double fx = cam[(size_t)img * 4 + 0], fy = cam[(size_t)img * 4 + 1], cx = cam[(size_t)img * 4 + 2], cy = cam[(size_t)img * 4 + 3];
  const float* z = depth + (size_t)img * sh.P;
  int lo, hi;
  hha_chunk(sh.P, lo, hi);
  double m = INFINITY;
  for (int i = lo + threadIdx.x; i < hi; i += 256) {
    const float d = z[i];
    if (!hha_valid(d)) continue;
    const int v = i / sh.W, u = i - v * sh.W;
    m = fmin(m, hha_raw_height(gx, gy, gz, ((double)u - cx) / fx, ((double)v - cy) / fy, (double)d));
  }
  __shared__ double shm[4];
  m = hha_wave_min(m);
  if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) pmin[(size_t)img * sh.nb + blockIdx.x] = fmin(fmin(shm[0], shm[1]), fmin(shm[2], shm[3]));
}

// grid (N), one wave
__global__ __launch_bounds__(64) void hha_ymin_final_kernel(const double* __restrict__ pmin, const double* __restrict__ g,
                                                            double* __restrict__ ymin, float* __restrict__ g_out, HhaShape sh) {
  const int img = blockIdx.x;
  double m = INFINITY;
  for (int i = threadIdx.x; i < sh.nb; i += 64) m = fmin(m, pmin[(size_t)img * sh.nb + i]);
  m = hha_wave_min(m);
  if (threadIdx.x != 0) return;
  ymin[img] = m > -90.0 ? -130.0 : m;
  if (g_out)
    for (int k = 0; k < 3; ++k) g_out[(size_t)img * 3 + k] = (float)g[(size_t)img * 3 + k];
}

__device__ __forceinline__ uint8_t hha_byte(double x) {  // half away from zero, saturated (x is never NaN here)
  return (uint8_t)fmin(fmax(floor(x + 0.5), 0.0), 255.0);
}

// grid (ceil(P / 256), N)
__global__ __launch_bounds__(256) void hha_encode_kernel(const float* __restrict__ depth, const double* __restrict__ cam,
                                                         const double* __restrict__ g, const double* __restrict__ ymin,
                                                         const double* __restrict__ n3, uint8_t* __restrict__ hha,
                                                         float* __restrict__ height, HhaShape sh) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= sh.P) return;
  const int img = blockIdx.y;
  const size_t p = (size_t)img * sh.P + i;
  const float d = depth[p];
  uint8_t c0 = 0, c1 = 0, c2 = 0;
  float hout = 0.f;
  if (hha_valid(d)) {
    const double gx = g[(size_t)img * 3], gy = g[(size_t)img * 3 + 1], gz = g[(size_t)img * 3 + 2];
    const double fx = cam[(size_t)img * 4 + 0], fy = cam[(size_t)img * 4 + 1], cx = cam[(size_t)img * 4 + 2], cy = cam[(size_t)img * 4 + 3];
    const int v = i / sh.W, u = i - v * sh.W;
    const double z = (double)d;
    const double h = hha_raw_height(gx, gy, gz, ((double)u - cx) / fx, ((double)v - cy) / fy, z) - ymin[img];
    const double x = n3[p * 3], y = n3[p * 3 + 1], w = n3[p * 3 + 2];
    double ang = 0.0;
    if (x != 0.0 || y != 0.0 || w != 0.0) ang = acos(fmin(fmax(x * gx + y * gy + w * gz, -1.0), 1.0)) * HHA_DEG + 38.0;
    c0 = hha_byte(31000.0 / fmax(z, 100.0)), c1 = hha_byte(h), c2 = hha_byte(ang);
    hout = (float)h;
  }
  hha[p * 3] = c0, hha[p * 3 + 1] = c1, hha[p * 3 + 2] = c2;
  if (height) height[p] = hout;
}

size_t hha_pad(size_t b) { return (b + 255) & ~(size_t)255; }

int hha_blocks(int64_t P) { return ceil_div64(P, HHA_PER_BLOCK, HHA_MAX_BLOCKS); }

struct HhaLayout {
  size_t cam, g, ymin, part, pmin, n10, n3, total;
};

HhaLayout hha_layout(int64_t N, int64_t H, int64_t W) {
  const size_t n = (size_t)N, pix = (size_t)(N * H * W), nb = (size_t)hha_blocks(H * W);
  HhaLayout l;
  size_t at = 0;
  l.cam = at, at += hha_pad(n * 4 * sizeof(double));
  l.g = at, at += hha_pad(n * 3 * sizeof(double));
  l.ymin = at, at += hha_pad(n * sizeof(double));
  l.part = at, at += hha_pad(n * nb * 12 * sizeof(double));
  l.pmin = at, at += hha_pad(n * nb * sizeof(double));
  l.n10 = at, at += hha_pad(pix * 3 * sizeof(double));
  l.n3 = at, at += hha_pad(pix * 3 * sizeof(double));
  l.total = at;
  return l;
}

// what the index arithmetic covers: pixel indices of one image are ints, element offsets of [N][H*W][3] stay below 2^31 (the kernels
// widen before they multiply, the launch grids do not), one image per blockIdx.y
bool hha_dims_ok(int64_t N, int64_t H, int64_t W) {
  return N >= 1 && H >= 1 && W >= 1 && N <= 65535 && H <= (1 << 24) && W <= (1 << 24) && H * W <= (1ll << 24) && N * H * W * 3 < (1ll << 31);
}

}  // namespace

extern "C" size_t mcdseg_depth_to_hha_workspace_bytes(int32_t N, int32_t H, int32_t W) {
  if (!hha_dims_ok(N, H, W)) return 0;
  return hha_layout(N, H, W).total;
}

extern "C" int mcdseg_depth_to_hha(const float* depth_cm, const float* camera, uint8_t* hha, float* normals3, float* gravity, float* height,
                                   int32_t N, int32_t H, int32_t W, void* ws, size_t ws_bytes, void* stream) {
  MCD_REQUIRE(depth_cm && camera && hha && ws, "depth_to_hha: null pointer (depth, camera, hha and workspace are needed)");
  MCD_REQUIRE(N >= 1 && H >= 1 && W >= 1, "depth_to_hha: bad dims N = %d, H = %d, W = %d", N, H, W);
  MCD_REQUIRE(N <= 65535, "depth_to_hha: N = %d, at most 65535 images per call (one per grid row)", N);
  MCD_REQUIRE(hha_dims_ok(N, H, W), "depth_to_hha: too large: H*W must not exceed 2^24 and N*H*W*3 must stay below 2^31");
  for (int64_t i = 0; i < N; ++i) {
    const float fx = camera[i * 4], fy = camera[i * 4 + 1], cx = camera[i * 4 + 2], cy = camera[i * 4 + 3];
    MCD_REQUIRE(fx > 0.f && fy > 0.f && fx <= FLT_MAX && fy <= FLT_MAX,
                "depth_to_hha: fx and fy must be positive and finite (image %lld: fx = %g, fy = %g)", (long long)i, (double)fx, (double)fy);
    MCD_REQUIRE(fabsf(cx) <= FLT_MAX && fabsf(cy) <= FLT_MAX, "depth_to_hha: cx and cy must be finite (image %lld)", (long long)i);
  }
  const HhaLayout l = hha_layout(N, H, W);
  MCD_REQUIRE(ws_bytes >= l.total, "depth_to_hha: workspace too small (%zu bytes, mcdseg_depth_to_hha_workspace_bytes asks for %zu)",
              ws_bytes, l.total);
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "depth_to_hha: workspace must be 16-byte aligned");
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(depth_cm) & 3) == 0 && (reinterpret_cast<uintptr_t>(normals3) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(gravity) & 3) == 0 && (reinterpret_cast<uintptr_t>(height) & 3) == 0,
              "depth_to_hha: depth, normals3, gravity and height must be 4-byte aligned");

  hipStream_t st = (hipStream_t)stream;
  HhaShape sh;
  sh.N = N, sh.H = H, sh.W = W, sh.P = H * W, sh.nb = hha_blocks((int64_t)H * W), sh.tiles_x = ceil_div(W, HHA_T);
  char* base = (char*)ws;
  double* cam = (double*)(base + l.cam);
  double* g = (double*)(base + l.g);
  double* ymin = (double*)(base + l.ymin);
  double* part = (double*)(base + l.part);
  double* pmin = (double*)(base + l.pmin);
  double* n10 = (double*)(base + l.n10);
  double* n3 = (double*)(base + l.n3);

  for (int first = 0; first < N; first += HHA_CAM_PACK) {
    HhaCameraPack pack;
    const int count = N - first < HHA_CAM_PACK ? N - first : HHA_CAM_PACK;
    for (int i = 0; i < HHA_CAM_PACK; ++i)
      for (int k = 0; k < 4; ++k) pack.v[i][k] = i < count ? camera[(size_t)(first + i) * 4 + k] : 0.f;
    hipLaunchKernelGGL(hha_camera_kernel, dim3(1), dim3(64), 0, st, pack, cam, g, first, count);
  }
  const dim3 tiles(sh.tiles_x * ceil_div(H, HHA_T), N), red(sh.nb, N), pix(ceil_div(sh.P, 256), N);
  hipLaunchKernelGGL(hha_normals_kernel, tiles, dim3(256), 0, st, depth_cm, (const double*)cam, n3, n10, normals3, sh);
  const double pi = 3.14159265358979323846;
  for (int it = 0; it < 10; ++it) {
    const double t = (it < 5 ? 45.0 : 15.0) * pi / 180.0;
    hipLaunchKernelGGL(hha_gravity_partial_kernel, red, dim3(256), 0, st, (const double*)n10, (const double*)g, part, sh, cos(t), sin(t));
    hipLaunchKernelGGL(hha_gravity_final_kernel, dim3(N), dim3(256), 0, st, (const double*)part, g, sh);
  }
  hipLaunchKernelGGL(hha_ymin_partial_kernel, red, dim3(256), 0, st, depth_cm, (const double*)cam, (const double*)g, pmin, sh);
  hipLaunchKernelGGL(hha_ymin_final_kernel, dim3(N), dim3(64), 0, st, (const double*)pmin, (const double*)g, ymin, gravity, sh);
  hipLaunchKernelGGL(hha_encode_kernel, pix, dim3(256), 0, st, depth_cm, (const double*)cam, (const double*)g, (const double*)ymin,
                     (const double*)n3, hha, height, sh);
  MCD_LAUNCH_CHECK("depth_to_hha");
  return 0;
}
