// Colorization depth inpainting (Levin, Lischinski, Weiss 2004, as the NYU Depth toolbox's fill_depth_colorization applies it to depth)
// on the device.  The definition is DESIGN.md section 4.16 (its fp64 numpy/scipy statement: tests/fill_ref.py), per image of P = H*W:
//     known: Z finite, > 0 and (with max_valid_cm > 0) < max_valid_cm;  g = ((0.299 R + 0.587 G) + 0.114 B) / 255
//     zmax = the largest known Z; z = Z / zmax at known pixels (an image without a known pixel is `empty`: not solved, all zeros)
//     weights: over the 3 x 3 neighbours q of p inside the image, in row-major order: mu and the population variance of g over
//         N(p) + {p}; sigma = max(0.6 var, min_q (g_q - g_p)^2 / ln 100, 2e-6); w_pq = exp(-(g_q - g_p)^2 / sigma) / their sum
//     system M x = b: (1 + alpha k_p) x_p - sum_q w_pq x_q = alpha k_p z_p, D = diag(M) = 1 + alpha k
//     BiCGSTAB, right-preconditioned by D, from x0 = b/D; stopped on the TRUE residual b - M x (fill_residual_kernel)
//     filled = (float)(x zmax); with keep_known a known pixel gets its Z back
// All arithmetic is fp64, no atomics, every sum in one fixed order that depends on H and W alone: the same bits run to run and for an
// image alone or in a batch.  An image that is not `running` is frozen: every block of it returns at once, nothing of it is written.
//
// The launches, plain and in stream order (no grid barrier, no spinning, no cooperative launch); a workgroup owns 32 x 8 pixels and,
// where a stencil is applied, stages the 34 x 10 tile-with-halo in LDS; the scalars live in one FillRec per image ON THE DEVICE:
//     setup      prepare (known mask -> zk, luma, block maxima of Z) | zmax_final | system (the eight weight planes, b, x0, r = b - M x0,
//                rhat = r, u = 0, block sums of r.r and b.b) | start_final (|b|^2, rho' = r.r, rho = a = omega = 1, beta)
//     iteration  pv        p = r + beta u  (u = p - omega v of the iteration before, kept in t's plane), formed in LDS for the halo too,
//                          v = M (p/D), block sums of rhat.v                            | alpha_final   a = rho' / (rhat.v)
//                st        s = r - a v in LDS with halo, t = M (s/D), sums of t.s, t.t  | omega_final   omega = t.s / t.t
//                xr        x += a (p/D) + omega (s/D), r = s - omega t, u = p - omega v, sums of rhat.r
//                                                                                       | rho_final     rho' = rhat.r, beta, iterations + 1
//     check      residual  b - M x over the staged x, sums of its squares               | check_final   converged?, the status records
// A zero or non-finite rho' is noted (rho_bad) and becomes `breakdown` at the head of the NEXT iteration (alpha_final), so a true-residual
// check that falls between the two still sees the image running, as the statement's loop does.
#include <float.h>

#include "block_reduce.h"
#include "common.h"

namespace {

constexpr int FILL_TX = 32, FILL_TY = 8;                 // tile: 256 threads, one pixel each
constexpr int FILL_SX = FILL_TX + 2, FILL_SY = FILL_TY + 2;  // 34 x 10 staged
constexpr int FILL_STAGED = FILL_SX * FILL_SY;
constexpr double FILL_LN100 = 4.605170185988092;         // ln 100
constexpr double FILL_SIGMA_FLOOR = 2e-6;

struct FillRec {
  double zmax, alpha, bnorm2, rho, rho_new, a, omega, beta, res;
  int status, iters, rho_bad, pad;
};

struct FillStatus {  // what mcdseg_fill_depth_iterate writes per image
  int status, iters;
  double res;
};

struct FillShape {
  int N, H, W, P, nblk, tiles_x;
};

struct FillPlanes {  // the workspace, as pointers
  FillRec* rec;
  double* part;  // [N][nblk][2]
  float* zk;     // [N][P]: Z at known pixels, 0 at missing ones
  double* wts;   // [N][8][P]
  double *x, *r, *rhat, *p, *v, *s, *t, *b;  // [N][P] each; s holds the luma during setup, t holds u between iterations
};

__device__ __forceinline__ bool fill_known(float z, double max_valid) {
  return z > 0.f && z <= FLT_MAX && (!(max_valid > 0.0) || (double)z < max_valid);  // (false for NaN)
}

__device__ __forceinline__ double fill_wave_max(double v) {
  for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m));
  return v;
}

// the tile of this block and the thread's pixel in it
struct FillAt {
  int x0, y0, tx, ty, u, v;
  bool in;
  size_t px;  // the pixel's index in the image
};

__device__ __forceinline__ FillAt fill_at(const FillShape& sh) {
  FillAt a;
  const int tile_y = blockIdx.x / sh.tiles_x, tile_x = blockIdx.x - tile_y * sh.tiles_x;
  a.x0 = tile_x * FILL_TX, a.y0 = tile_y * FILL_TY;
  a.ty = threadIdx.x / FILL_TX, a.tx = threadIdx.x - a.ty * FILL_TX;
  a.u = a.x0 + a.tx, a.v = a.y0 + a.ty;
  a.in = a.u < sh.W && a.v < sh.H;
  a.px = (size_t)a.v * sh.W + a.u;
  return a;
}

// staged index i of the 34 x 10 tile -> the pixel's index in the image, or -1 outside it
__device__ __forceinline__ int fill_staged_pixel(int i, const FillAt& a, const FillShape& sh) {
  const int r = i / FILL_SX, c = i - r * FILL_SX;
  const int v = a.y0 - 1 + r, u = a.x0 - 1 + c;
  return (v >= 0 && v < sh.H && u >= 0 && u < sh.W) ? v * sh.W + u : -1;
}

// sum_k w_k * (the staged value of neighbour k), k in row-major order; a neighbour outside the image has weight 0 and staged value 0
__device__ __forceinline__ double fill_neighbours(const double* __restrict__ w, size_t P, size_t px, const double* st, const FillAt& a) {
  const double* c = st + (a.ty + 1) * FILL_SX + a.tx + 1;
  double acc = 0.0;
  acc += w[0 * P + px] * c[-FILL_SX - 1];
  acc += w[1 * P + px] * c[-FILL_SX];
  acc += w[2 * P + px] * c[-FILL_SX + 1];
  acc += w[3 * P + px] * c[-1];
  acc += w[4 * P + px] * c[1];
  acc += w[5 * P + px] * c[FILL_SX - 1];
  acc += w[6 * P + px] * c[FILL_SX];
  acc += w[7 * P + px] * c[FILL_SX + 1];
  return acc;
}

// one block sum into part[(img * nblk + block) * 2 + q]
template <int K>
__device__ __forceinline__ void fill_block_sums(double (&v)[K], double* __restrict__ part, const FillShape& sh, int img) {
  __shared__ double shm[K][4];
  block_gather(v, shm);
  if (threadIdx.x == 0)
    for (int k = 0; k < K; ++k) part[((size_t)img * sh.nblk + blockIdx.x) * 2 + k] = tree_total<4>(shm[k]);
}

// ---- setup ---------------------------------------------------------------------------------------------------------------------------
// grid (tiles, N): zk, the luma (into the s plane), part[..][0] = the block's largest known Z (0 without one)
__global__ __launch_bounds__(256) void fill_prepare_kernel(const uint8_t* __restrict__ rgb, const float* __restrict__ depth, FillPlanes pl,
                                                           FillShape sh, double max_valid) {
  const int img = blockIdx.y;
  const FillAt a = fill_at(sh);
  double m = 0.0;
  if (a.in) {
    const size_t q = (size_t)img * sh.P + a.px;
    const float z = depth[q];
    const bool known = fill_known(z, max_valid);
    pl.zk[q] = known ? z : 0.f;
    if (known) m = (double)z;
    const double R = (double)rgb[q * 3], G = (double)rgb[q * 3 + 1], B = (double)rgb[q * 3 + 2];
    pl.s[q] = ((0.299 * R + 0.587 * G) + 0.114 * B) / 255.0;
  }
  __shared__ double shm[4];
  m = fill_wave_max(m);
  if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) pl.part[((size_t)img * sh.nblk + blockIdx.x) * 2] = fmax(fmax(shm[0], shm[1]), fmax(shm[2], shm[3]));
}

// grid (N): zmax and the image's record
__global__ __launch_bounds__(256) void fill_zmax_final_kernel(FillPlanes pl, FillShape sh, double alpha) {
  const int img = blockIdx.x;
  double m = 0.0;
  for (int i = threadIdx.x; i < sh.nblk; i += 256) m = fmax(m, pl.part[((size_t)img * sh.nblk + i) * 2]);
  __shared__ double shm[4];
  m = fill_wave_max(m);
  if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x != 0) return;
  FillRec rec;
  rec.zmax = fmax(fmax(shm[0], shm[1]), fmax(shm[2], shm[3]));
  rec.alpha = alpha, rec.bnorm2 = 0.0, rec.rho = 1.0, rec.rho_new = 0.0, rec.a = 1.0, rec.omega = 1.0, rec.beta = 0.0, rec.res = 0.0;
  rec.status = rec.zmax > 0.0 ? MCDSEG_FILL_RUNNING : MCDSEG_FILL_EMPTY, rec.iters = 0, rec.rho_bad = 0, rec.pad = 0;
  pl.rec[img] = rec;
}

// grid (tiles, N): the weights, b, x0 = b/D, r = rhat = b - M x0, u = 0; block sums of r.r and b.b.  Runs for an empty image as well
// (its b, x0 and r are 0): the weights are defined by the RGB image alone, and x is what finish reads.
__global__ __launch_bounds__(256) void fill_system_kernel(FillPlanes pl, FillShape sh) {
  __shared__ double s_g[FILL_STAGED], s_x[FILL_STAGED];
  const int img = blockIdx.y;
  const FillAt a = fill_at(sh);
  const size_t base = (size_t)img * sh.P;
  const double zmax = pl.rec[img].zmax, alpha = pl.rec[img].alpha;
  for (int i = threadIdx.x; i < FILL_STAGED; i += 256) {
    const int q = fill_staged_pixel(i, a, sh);
    double g = 0.0, x = 0.0;
    if (q >= 0) {
      g = pl.s[base + q];
      const float z = pl.zk[base + q];
      if (z > 0.f) x = (alpha * ((double)z / zmax)) / (1.0 + alpha);
    }
    s_g[i] = g, s_x[i] = x;
  }
  __syncthreads();
  double sums[2] = {0.0, 0.0};
  if (a.in) {
    const int dy[8] = {-1, -1, -1, 0, 0, 1, 1, 1}, dx[8] = {-1, 0, 1, -1, 1, -1, 0, 1};
    const double* cg = s_g + (a.ty + 1) * FILL_SX + a.tx + 1;
    const double gp = cg[0];
    bool in[8];
    double gq[8], w[8];
    int count = 1;
    double total = gp;
    for (int k = 0; k < 8; ++k) {
      const int v = a.v + dy[k], u = a.u + dx[k];
      in[k] = v >= 0 && v < sh.H && u >= 0 && u < sh.W;
      gq[k] = cg[dy[k] * FILL_SX + dx[k]];
      if (in[k]) total += gq[k], ++count;
    }
    const double mu = total / (double)count;
    double var = (gp - mu) * (gp - mu), nearest = INFINITY;
    for (int k = 0; k < 8; ++k)
      if (in[k]) {
        var += (gq[k] - mu) * (gq[k] - mu);
        const double d = gq[k] - gp;
        w[k] = d * d;
        nearest = fmin(nearest, w[k]);
      }
    var /= (double)count;
    const double sigma = fmax(fmax(0.6 * var, nearest / FILL_LN100), FILL_SIGMA_FLOOR);
    double wsum = 0.0;
    for (int k = 0; k < 8; ++k)
      if (in[k]) {
        w[k] = exp(-w[k] / sigma);
        wsum += w[k];
      }
    const size_t q = base + a.px;
    double* wp = pl.wts + (size_t)img * 8 * sh.P;
    for (int k = 0; k < 8; ++k) wp[(size_t)k * sh.P + a.px] = in[k] ? w[k] / wsum : 0.0;

    const float z = pl.zk[q];
    const bool known = z > 0.f;
    const double D = known ? 1.0 + alpha : 1.0;
    const double b = known ? alpha * ((double)z / zmax) : 0.0;
    const double x0 = s_x[(a.ty + 1) * FILL_SX + a.tx + 1];
    const double* cx = s_x + (a.ty + 1) * FILL_SX + a.tx + 1;
    double acc = 0.0;
    for (int k = 0; k < 8; ++k)
      if (in[k]) acc += (w[k] / wsum) * cx[dy[k] * FILL_SX + dx[k]];
    const double r = b - (D * x0 - acc);
    pl.b[q] = b, pl.x[q] = x0, pl.r[q] = r, pl.rhat[q] = r, pl.t[q] = 0.0;
    sums[0] = r * r, sums[1] = b * b;
  }
  fill_block_sums(sums, pl.part, sh, img);
}

__device__ __forceinline__ bool fill_bad(double v) { return v == 0.0 || !(fabs(v) <= DBL_MAX); }

// grid (N)
__global__ __launch_bounds__(256) void fill_start_final_kernel(FillPlanes pl, FillShape sh) {
  const int img = blockIdx.x;
  if (pl.rec[img].status != MCDSEG_FILL_RUNNING) return;
  double tot[2];
  partials_total(pl.part + (size_t)img * sh.nblk * 2, sh.nblk, 2, 0, tot);
  if (threadIdx.x != 0) return;
  FillRec& rec = pl.rec[img];
  rec.bnorm2 = tot[1], rec.rho_new = tot[0], rec.rho_bad = fill_bad(tot[0]);
  rec.beta = (rec.rho_new / rec.rho) * (rec.a / rec.omega);
}

// ---- one iteration -------------------------------------------------------------------------------------------------------------------
// grid (tiles, N): p = r + beta u, v = M (p/D), block sums of rhat.v
__global__ __launch_bounds__(256) void fill_pv_kernel(FillPlanes pl, FillShape sh) {
  __shared__ double s_p[FILL_STAGED], s_pd[FILL_STAGED];
  const int img = blockIdx.y;
  if (pl.rec[img].status != MCDSEG_FILL_RUNNING || pl.rec[img].rho_bad) return;
  const double beta = pl.rec[img].beta, alpha = pl.rec[img].alpha;
  const FillAt a = fill_at(sh);
  const size_t base = (size_t)img * sh.P;
  for (int i = threadIdx.x; i < FILL_STAGED; i += 256) {
    const int q = fill_staged_pixel(i, a, sh);
    double p = 0.0, pd = 0.0;
    if (q >= 0) {
      p = pl.r[base + q] + beta * pl.t[base + q];
      pd = p / (pl.zk[base + q] > 0.f ? 1.0 + alpha : 1.0);
    }
    s_p[i] = p, s_pd[i] = pd;
  }
  __syncthreads();
  double sums[1] = {0.0};
  if (a.in) {
    const size_t q = base + a.px;
    const int c = (a.ty + 1) * FILL_SX + a.tx + 1;
    const double D = pl.zk[q] > 0.f ? 1.0 + alpha : 1.0;
    const double v = D * s_pd[c] - fill_neighbours(pl.wts + (size_t)img * 8 * sh.P, sh.P, a.px, s_pd, a);
    pl.p[q] = s_p[c], pl.v[q] = v;
    sums[0] = pl.rhat[q] * v;
  }
  fill_block_sums(sums, pl.part, sh, img);
}

// grid (N): a = rho' / (rhat.v); a noted rho' breakdown takes effect here
__global__ __launch_bounds__(256) void fill_alpha_final_kernel(FillPlanes pl, FillShape sh) {
  const int img = blockIdx.x;
  if (pl.rec[img].status != MCDSEG_FILL_RUNNING) return;
  if (pl.rec[img].rho_bad) {
    if (threadIdx.x == 0) pl.rec[img].status = MCDSEG_FILL_BREAKDOWN;
    return;
  }
  double tot[1];
  partials_total(pl.part + (size_t)img * sh.nblk * 2, sh.nblk, 2, 0, tot);
  if (threadIdx.x != 0) return;
  FillRec& rec = pl.rec[img];
  if (fill_bad(tot[0]))
    rec.status = MCDSEG_FILL_BREAKDOWN;
  else
    rec.a = rec.rho_new / tot[0];
}

// grid (tiles, N): s = r - a v, t = M (s/D), block sums of t.s and t.t
__global__ __launch_bounds__(256) void fill_st_kernel(FillPlanes pl, FillShape sh) {
  __shared__ double s_s[FILL_STAGED], s_sd[FILL_STAGED];
  const int img = blockIdx.y;
  if (pl.rec[img].status != MCDSEG_FILL_RUNNING) return;
  const double av = pl.rec[img].a, alpha = pl.rec[img].alpha;
  const FillAt a = fill_at(sh);
  const size_t base = (size_t)img * sh.P;
  for (int i = threadIdx.x; i < FILL_STAGED; i += 256) {
    const int q = fill_staged_pixel(i, a, sh);
    double s = 0.0, sd = 0.0;
    if (q >= 0) {
      s = pl.r[base + q] - av * pl.v[base + q];
      sd = s / (pl.zk[base + q] > 0.f ? 1.0 + alpha : 1.0);
    }
    s_s[i] = s, s_sd[i] = sd;
  }
  __syncthreads();
  double sums[2] = {0.0, 0.0};
  if (a.in) {
    const size_t q = base + a.px;
    const int c = (a.ty + 1) * FILL_SX + a.tx + 1;
    const double D = pl.zk[q] > 0.f ? 1.0 + alpha : 1.0;
    const double t = D * s_sd[c] - fill_neighbours(pl.wts + (size_t)img * 8 * sh.P, sh.P, a.px, s_sd, a);
    pl.s[q] = s_s[c], pl.t[q] = t;
    sums[0] = t * s_s[c], sums[1] = t * t;
  }
  fill_block_sums(sums, pl.part, sh, img);
}

// grid (N): omega = t.s / t.t
__global__ __launch_bounds__(256) void fill_omega_final_kernel(FillPlanes pl, FillShape sh) {
  const int img = blockIdx.x;
  if (pl.rec[img].status != MCDSEG_FILL_RUNNING) return;
  double tot[2];
  partials_total(pl.part + (size_t)img * sh.nblk * 2, sh.nblk, 2, 0, tot);
  if (threadIdx.x != 0) return;
  FillRec& rec = pl.rec[img];
  if (fill_bad(tot[1]))
    rec.status = MCDSEG_FILL_BREAKDOWN;
  else
    rec.omega = tot[0] / tot[1];
}

// grid (tiles, N), no stencil: x += a (p/D) + omega (s/D), r = s - omega t, u = p - omega v (into t's plane), block sums of rhat.r
__global__ __launch_bounds__(256) void fill_xr_kernel(FillPlanes pl, FillShape sh) {
  const int img = blockIdx.y;
  if (pl.rec[img].status != MCDSEG_FILL_RUNNING) return;
  const double av = pl.rec[img].a, omega = pl.rec[img].omega, alpha = pl.rec[img].alpha;
  const FillAt a = fill_at(sh);
  double sums[1] = {0.0};
  if (a.in) {
    const size_t q = (size_t)img * sh.P + a.px;
    const double D = pl.zk[q] > 0.f ? 1.0 + alpha : 1.0;
    const double p = pl.p[q], s = pl.s[q];
    pl.x[q] = pl.x[q] + (av * (p / D) + omega * (s / D));
    const double r = s - omega * pl.t[q];
    pl.r[q] = r;
    pl.t[q] = p - omega * pl.v[q];
    sums[0] = pl.rhat[q] * r;
  }
  fill_block_sums(sums, pl.part, sh, img);
}

// grid (N): the iteration is complete: rho' = rhat.r, beta of the next one
__global__ __launch_bounds__(256) void fill_rho_final_kernel(FillPlanes pl, FillShape sh) {
  const int img = blockIdx.x;
  if (pl.rec[img].status != MCDSEG_FILL_RUNNING) return;
  double tot[1];
  partials_total(pl.part + (size_t)img * sh.nblk * 2, sh.nblk, 2, 0, tot);
  if (threadIdx.x != 0) return;
  FillRec& rec = pl.rec[img];
  rec.rho = rec.rho_new, rec.rho_new = tot[0], rec.rho_bad = fill_bad(tot[0]);
  rec.beta = (rec.rho_new / rec.rho) * (rec.a / rec.omega);
  rec.iters += 1;
}

// ---- the true residual ---------------------------------------------------------------------------------------------------------------
// grid (tiles, N): block sums of (b - M x)^2
__global__ __launch_bounds__(256) void fill_residual_kernel(FillPlanes pl, FillShape sh) {
  __shared__ double s_x[FILL_STAGED];
  const int img = blockIdx.y;
  if (pl.rec[img].status != MCDSEG_FILL_RUNNING) return;
  const double alpha = pl.rec[img].alpha;
  const FillAt a = fill_at(sh);
  const size_t base = (size_t)img * sh.P;
  for (int i = threadIdx.x; i < FILL_STAGED; i += 256) {
    const int q = fill_staged_pixel(i, a, sh);
    s_x[i] = q >= 0 ? pl.x[base + q] : 0.0;
  }
  __syncthreads();
  double sums[1] = {0.0};
  if (a.in) {
    const size_t q = base + a.px;
    const double D = pl.zk[q] > 0.f ? 1.0 + alpha : 1.0;
    const double r = pl.b[q] - (D * s_x[(a.ty + 1) * FILL_SX + a.tx + 1] - fill_neighbours(pl.wts + (size_t)img * 8 * sh.P, sh.P, a.px, s_x, a));
    sums[0] = r * r;
  }
  fill_block_sums(sums, pl.part, sh, img);
}

// grid (N): converged?  and the image's status record, for every image
__global__ __launch_bounds__(256) void fill_check_final_kernel(FillPlanes pl, FillShape sh, double rtol, FillStatus* __restrict__ out) {
  const int img = blockIdx.x;
  if (pl.rec[img].status == MCDSEG_FILL_RUNNING) {
    double tot[1];
    partials_total(pl.part + (size_t)img * sh.nblk * 2, sh.nblk, 2, 0, tot);
    if (threadIdx.x == 0) {
      FillRec& rec = pl.rec[img];
      const double rn = sqrt(tot[0]), bn = sqrt(rec.bnorm2);
      rec.res = rn / bn;
      if (rn <= rtol * bn) rec.status = MCDSEG_FILL_CONVERGED;
    }
  }
  if (threadIdx.x == 0) {
    FillStatus s;
    s.status = pl.rec[img].status, s.iters = pl.rec[img].iters, s.res = pl.rec[img].res;
    out[img] = s;
  }
}

// ---- the output ----------------------------------------------------------------------------------------------------------------------
// grid (ceil(P / 256), N)
__global__ __launch_bounds__(256) void fill_finish_kernel(FillPlanes pl, FillShape sh, float* __restrict__ filled, double* __restrict__ x_out,
                                                          double* __restrict__ w_out, double* __restrict__ zmax_out, int keep_known) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int img = blockIdx.y;
  const double zmax = pl.rec[img].zmax;
  if (zmax_out && i == 0) zmax_out[img] = zmax;
  if (i >= sh.P) return;
  const size_t q = (size_t)img * sh.P + i;
  const double x = pl.x[q];
  const float z = pl.zk[q];
  filled[q] = keep_known && z > 0.f ? z : (float)(x * zmax);
  if (x_out) x_out[q] = x;
  if (w_out)
    for (int k = 0; k < 8; ++k) {
      const size_t at = ((size_t)img * 8 + k) * sh.P + i;
      w_out[at] = pl.wts[at];
    }
}

size_t fill_pad(size_t b) { return (b + 255) & ~(size_t)255; }

int fill_tiles(int64_t H, int64_t W) { return (int)(ceil_div64(W, FILL_TX) * ceil_div64(H, FILL_TY)); }

struct FillLayout {
  size_t rec, part, zk, wts, vec[8], total;
};

FillLayout fill_layout(int64_t N, int64_t H, int64_t W) {
  const size_t n = (size_t)N, pix = (size_t)(N * H * W), nblk = (size_t)fill_tiles(H, W);
  FillLayout l;
  size_t at = 0;
  l.rec = at, at += fill_pad(n * sizeof(FillRec));
  l.part = at, at += fill_pad(n * nblk * 2 * sizeof(double));
  l.zk = at, at += fill_pad(pix * sizeof(float));
  l.wts = at, at += fill_pad(pix * 8 * sizeof(double));
  for (int k = 0; k < 8; ++k) l.vec[k] = at, at += fill_pad(pix * sizeof(double));
  l.total = at;
  return l;
}

// what the index arithmetic covers: pixel indices of one image are ints (H*W <= 2^24, so 8*H*W too), offsets across the batch are
// size_t; one image per blockIdx.y; at most 2^21 tiles per image in blockIdx.x
bool fill_dims_ok(int64_t N, int64_t H, int64_t W) {
  return N >= 1 && H >= 1 && W >= 1 && N <= 65535 && H <= (1 << 24) && W <= (1 << 24) && H * W <= (1ll << 24) && H * W >= 2;
}

FillPlanes fill_planes(void* ws, const FillLayout& l) {
  char* base = (char*)ws;
  FillPlanes pl;
  pl.rec = (FillRec*)(base + l.rec), pl.part = (double*)(base + l.part), pl.zk = (float*)(base + l.zk), pl.wts = (double*)(base + l.wts);
  pl.x = (double*)(base + l.vec[0]), pl.r = (double*)(base + l.vec[1]), pl.rhat = (double*)(base + l.vec[2]), pl.p = (double*)(base + l.vec[3]);
  pl.v = (double*)(base + l.vec[4]), pl.s = (double*)(base + l.vec[5]), pl.t = (double*)(base + l.vec[6]), pl.b = (double*)(base + l.vec[7]);
  return pl;
}

FillShape fill_shape(int32_t N, int32_t H, int32_t W) {
  FillShape sh;
  sh.N = N, sh.H = H, sh.W = W, sh.P = H * W, sh.nblk = fill_tiles(H, W), sh.tiles_x = ceil_div(W, FILL_TX);
  return sh;
}

// the checks the three calls share; 0 or -EINVAL
int fill_common(const char* who, int32_t N, int32_t H, int32_t W, const void* ws, size_t ws_bytes) {
  MCD_REQUIRE(ws, "%s: null pointer (the workspace is needed)", who);
  MCD_REQUIRE(N >= 1 && H >= 1 && W >= 1, "%s: bad dims N = %d, H = %d, W = %d", who, N, H, W);
  MCD_REQUIRE(N <= 65535, "%s: N = %d, at most 65535 images per call (one per grid row)", who, N);
  MCD_REQUIRE((int64_t)H * W >= 2, "%s: too small: H*W must be at least 2 (a pixel needs a neighbour)", who);
  MCD_REQUIRE(fill_dims_ok(N, H, W), "%s: too large: H*W must not exceed 2^24", who);
  const size_t need = fill_layout(N, H, W).total;
  MCD_REQUIRE(ws_bytes >= need, "%s: workspace too small (%zu bytes, mcdseg_fill_depth_workspace_bytes asks for %zu)", who, ws_bytes, need);
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "%s: workspace must be 16-byte aligned", who);
  return 0;
}

}  // namespace

extern "C" size_t mcdseg_fill_depth_workspace_bytes(int32_t N, int32_t H, int32_t W) {
  if (!fill_dims_ok(N, H, W)) return 0;
  return fill_layout(N, H, W).total;
}

extern "C" int mcdseg_fill_depth_setup(const uint8_t* rgb, const float* depth_cm, double alpha, double max_valid_cm, int32_t N, int32_t H,
                                       int32_t W, void* ws, size_t ws_bytes, void* stream) {
  MCD_REQUIRE(rgb && depth_cm, "fill_depth_setup: null pointer (rgb, depth and workspace are needed)");
  if (int rc = fill_common("fill_depth_setup", N, H, W, ws, ws_bytes)) return rc;
  MCD_REQUIRE(alpha > 0.0 && alpha <= DBL_MAX, "fill_depth_setup: alpha must be positive and finite (got %g)", alpha);
  MCD_REQUIRE(max_valid_cm >= 0.0, "fill_depth_setup: max_valid_cm must be positive, or 0 for none (got %g)", max_valid_cm);
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(depth_cm) & 3) == 0, "fill_depth_setup: depth must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const FillShape sh = fill_shape(N, H, W);
  const FillPlanes pl = fill_planes(ws, fill_layout(N, H, W));
  const dim3 tiles(sh.nblk, N);
  hipLaunchKernelGGL(fill_prepare_kernel, tiles, dim3(256), 0, st, rgb, depth_cm, pl, sh, max_valid_cm);
  hipLaunchKernelGGL(fill_zmax_final_kernel, dim3(N), dim3(256), 0, st, pl, sh, alpha);
  hipLaunchKernelGGL(fill_system_kernel, tiles, dim3(256), 0, st, pl, sh);
  hipLaunchKernelGGL(fill_start_final_kernel, dim3(N), dim3(256), 0, st, pl, sh);
  MCD_LAUNCH_CHECK("fill_depth_setup");
  return 0;
}

extern "C" int mcdseg_fill_depth_iterate(int32_t n_iter, double rtol, int32_t N, int32_t H, int32_t W, void* ws, size_t ws_bytes,
                                         void* status_out, void* stream) {
  MCD_REQUIRE(status_out, "fill_depth_iterate: null pointer (the status records and the workspace are needed)");
  if (int rc = fill_common("fill_depth_iterate", N, H, W, ws, ws_bytes)) return rc;
  MCD_REQUIRE(n_iter >= 0 && n_iter <= 65536, "fill_depth_iterate: n_iter = %d outside [0, 65536]", n_iter);
  MCD_REQUIRE(rtol > 0.0 && rtol <= DBL_MAX, "fill_depth_iterate: rtol must be positive and finite (got %g)", rtol);
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(status_out) & 7) == 0, "fill_depth_iterate: the status records must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const FillShape sh = fill_shape(N, H, W);
  const FillPlanes pl = fill_planes(ws, fill_layout(N, H, W));
  const dim3 tiles(sh.nblk, N), one(N), block(256);
  for (int it = 0; it < n_iter; ++it) {
    hipLaunchKernelGGL(fill_pv_kernel, tiles, block, 0, st, pl, sh);
    hipLaunchKernelGGL(fill_alpha_final_kernel, one, block, 0, st, pl, sh);
    hipLaunchKernelGGL(fill_st_kernel, tiles, block, 0, st, pl, sh);
    hipLaunchKernelGGL(fill_omega_final_kernel, one, block, 0, st, pl, sh);
    hipLaunchKernelGGL(fill_xr_kernel, tiles, block, 0, st, pl, sh);
    hipLaunchKernelGGL(fill_rho_final_kernel, one, block, 0, st, pl, sh);
  }
  hipLaunchKernelGGL(fill_residual_kernel, tiles, block, 0, st, pl, sh);
  hipLaunchKernelGGL(fill_check_final_kernel, one, block, 0, st, pl, sh, rtol, (FillStatus*)status_out);
  MCD_LAUNCH_CHECK("fill_depth_iterate");
  return 0;
}

extern "C" int mcdseg_fill_depth_finish(int32_t N, int32_t H, int32_t W, void* ws, size_t ws_bytes, float* filled, double* x_f64,
                                        double* weights_f64, double* zmax_f64, int32_t keep_known, void* stream) {
  MCD_REQUIRE(filled, "fill_depth_finish: null pointer (filled and the workspace are needed)");
  if (int rc = fill_common("fill_depth_finish", N, H, W, ws, ws_bytes)) return rc;
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(filled) & 3) == 0, "fill_depth_finish: filled must be 4-byte aligned");
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(x_f64) & 7) == 0 && (reinterpret_cast<uintptr_t>(weights_f64) & 7) == 0 &&
                  (reinterpret_cast<uintptr_t>(zmax_f64) & 7) == 0,
              "fill_depth_finish: x, weights and zmax must be 8-byte aligned");
  const FillShape sh = fill_shape(N, H, W);
  const FillPlanes pl = fill_planes(ws, fill_layout(N, H, W));
  hipLaunchKernelGGL(fill_finish_kernel, dim3(ceil_div(sh.P, 256), N), dim3(256), 0, (hipStream_t)stream, pl, sh, filled, x_f64, weights_f64,
                     zmax_f64, keep_known);
  MCD_LAUNCH_CHECK("fill_depth_finish");
  return 0;
}
