// Fused per-pixel softmax -> weighted cross-entropy (one or two heads) -> L1 discrepancy, with the
// gradients w.r.t. both logit tensors written in the same pass.
//
// Reference ops this replaces (each a separate full-tensor ATen pass over [N,C,H,W]):
//   CrossEntropyLoss2d = log_softmax(dim 1) + weighted-mean NLL   (loss.py:7-13)
//   Diff2d             = mean |softmax(o1) - softmax(o2)|          (loss.py:93-100)
// Maths, per pixel i, p = softmax(z), W = sum_i w[y_i], M = N*C*H*W:
//   dCE/dz_c   = w[y_i] (p_c - [c == y_i]) / W
//   dDiff/dz1_c =  p1_c (s_c - sum_k s_k p1_k),  dDiff/dz2_c = -p2_c (s_c - sum_k s_k p2_k),  s = sign(p1-p2)/M
//
// One lane owns one pixel and keeps all C logits of both heads in registers; the class stride of NCHW is
// H*W so every per-class load/store of a wave is one contiguous 256-B run.  Algorithmic traffic:
// (2C reads + 2C writes) * 4 B + 8 B label per pixel; everything else stays in registers.
#include <stdlib.h>

#include "block_reduce.h"
#include "predict_pixel.h"

namespace {

constexpr int LOSS_BLOCK = 256;

__global__ __launch_bounds__(256) void label_wsum_kernel(const int64_t* __restrict__ labels, const float* __restrict__ cw,
                                                         int64_t ignore_index, int C, int64_t P, float* __restrict__ part) {
  float s = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < P; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t y = labels[i];
    if (y != ignore_index && y >= 0 && y < C) s += cw ? cw[y] : 1.f;
  }
  __shared__ float sh[1][4];
  float v[1] = {s};
  block_gather(v, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tree_total<4>(sh[0]);
}

// The per-pixel maths shared by the two front ends below: a[] / b[] hold the pixel's logits (-inf past C) and leave as its
// probabilities; the gradients go to g1 / g2 at base + c * HW.
// Precondition: a[c] = b[c] = -inf for c >= C, so the exponentials need no per-class select (exp(-inf) = 0).  The class loops
// are cut into groups by branches on an opaque, always-true scalar: basic-block boundaries are the only fence the instruction
// scheduler respects here, and without them it interleaves the exponential chains of all classes (about seven registers
// each) and spills hundreds of registers.
// (MCD_OPAQUE_TRUE, exp_nonpos and the patch constants UP_COLS / UP_JP / UP_NT live in up8_patch.h, with the staging fragments of the
// register-staged up-sampling front end, which csrc/uncertain.hip uses as well)
#include "up8_patch.h"

template <int NCMAX, bool TWO>
__device__ __forceinline__ void pixel_losses(float (&a)[NCMAX], float (&b)[NCMAX], int y, float wy, float ce_coef, float diff_coef,
                                             const float* __restrict__ losses_w, float* __restrict__ g1, float* __restrict__ g2,
                                             size_t base, size_t HW, int C, float inv_m, float& ce1, float& ce2, float& dsum) {
  float m1 = a[0], m2 = TWO ? b[0] : 0.f;
#pragma unroll
  for (int c = 1; c < NCMAX; ++c) {
    m1 = fmaxf(m1, a[c]);
    if (TWO) m2 = fmaxf(m2, b[c]);
  }
  float s1 = 0.f, s2 = 0.f, zy1 = 0.f, zy2 = 0.f;
#pragma unroll
  for (int c0 = 0; c0 < NCMAX; c0 += 4) {
    MCD_OPAQUE_TRUE(go);
    if (go) {
#pragma unroll
      for (int c = c0; c < c0 + 4; ++c) {
        if (c >= NCMAX) continue;
        if (c == y) {
          zy1 = a[c];
          if (TWO) zy2 = b[c];
        }
        a[c] = exp_nonpos(a[c] - m1);
        s1 += a[c];
        if (TWO) {
          b[c] = exp_nonpos(b[c] - m2);
          s2 += b[c];
        }
      }
    }
  }
  if (y >= 0) {
    ce1 = wy * ((m1 + logf(s1)) - zy1);
    if (TWO) ce2 = wy * ((m2 + logf(s2)) - zy2);
  }
  const float r1 = 1.f / s1, r2 = TWO ? 1.f / s2 : 0.f;
  float t1 = 0.f, t2 = 0.f;
#pragma unroll
  for (int c0 = 0; c0 < NCMAX; c0 += 8) {
    MCD_OPAQUE_TRUE(go);
    if (go) {
#pragma unroll
      for (int c = c0; c < c0 + 8; ++c) {
        if (c >= NCMAX) continue;
        a[c] *= r1;
        if (TWO) {
          b[c] *= r2;
          const float d = a[c] - b[c];
          const float sg = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);
          dsum += fabsf(d);
          t1 = fmaf(sg, a[c], t1);
          t2 = fmaf(sg, b[c], t2);
        }
      }
    }
  }
  if (g1 != nullptr || g2 != nullptr) {
    const float kce = (ce_coef != 0.f && y >= 0) ? ce_coef * wy / losses_w[3] : 0.f;
    const float kd = diff_coef * inv_m;
#pragma unroll
    for (int c = 0; c < NCMAX; ++c) {
      if (c < C) {
        const float oh = (c == y) ? 1.f : 0.f;
        float sg = 0.f;
        if (TWO) {
          const float d = a[c] - b[c];
          sg = (d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f);
        }
        if (g1 != nullptr) g1[base + (size_t)c * HW] = kce * (a[c] - oh) + (TWO ? kd * a[c] * (sg - t1) : 0.f);
        if (TWO && g2 != nullptr) g2[base + (size_t)c * HW] = kce * (b[c] - oh) - kd * b[c] * (sg - t2);
      }
    }
  }
}

// ---- the probability distances of --d_loss besides L1 (loss.py:66-189) -------------------------------------
// With p = softmax(z1), q = softmax(z2), lp = log p, lq = log q, all under the element mean 1/M that Diff2d uses:
//   SYMKL      0.5 (p - q)(lp - lq)                 Symkl2d / MySymkl2d       loss.py:103-118, 144-154
//   MIS_SYMKL  0.5 (p lp + q lq - 2 p q)            MisSymKLD / SpatialJSD2d  loss.py:66-75, 157-173
//   JSD        0.5 (p (lp - lm) + q (lq - lm)),  m = softmax((z1 + z2) / 2)   JSD  loss.py:78-89
// d/dz1_k = (1/M) (p_k u_k - p_k S + J_k),  S = sum_c p_c u_c,  u = d summand / dp:
//   SYMKL      p u = 0.5 (p (lp - lq) + (p - q))    (in this form nothing divides by a probability that flushed to zero)
//   MIS_SYMKL    u = 0.5 (lp + 1 - 2 q)
//   JSD          u = 0.5 (lp - lm)   (the "+ 1" of d(p lp)/dp is a constant, and p_k (const - sum_c p_c const) = 0: left out, identical
//                                     heads then give zeros exactly),   J_k = -0.25 (p_k + q_k - 2 m_k): the path through the mean logits
// and d/dz2 by symmetry (J is the same for both heads).
// a[] / b[] KEEP the logits: a probability and its logarithm are both needed per class and pass, and four arrays of NCMAX floats do not
// fit beside the up-sampler's state.  lp_c = z_c - (max + log sum) -- one logf per pixel and head, never log(p_c) -- and
// p_c = exp_nonpos(z_c - max) / sum is recomputed where it is used (two instructions and a multiply; the same expression as
// pixel_losses, so the cross-entropy terms are bitwise those of the L1 kernels).  Padding classes c >= C carry -inf, and 0 * -inf is
// NaN: unlike the L1 terms these multiply by log-probabilities, so the value loop carries the c < C guard too.
enum { DIST_L1 = MCDSEG_DIST_L1, DIST_SYMKL = MCDSEG_DIST_SYMKL, DIST_MIS_SYMKL = MCDSEG_DIST_MIS_SYMKL, DIST_JSD = MCDSEG_DIST_JSD };

template <int NCMAX, int KIND>
__device__ __forceinline__ void pixel_dist(float (&a)[NCMAX], float (&b)[NCMAX], int y, float wy, float ce_coef, float diff_coef,
                                           const float* __restrict__ losses_w, float* __restrict__ g1, float* __restrict__ g2,
                                           size_t base, size_t HW, int C, float inv_m, float& ce1, float& ce2, float& dsum) {
  constexpr bool JS = KIND == DIST_JSD;
  float m1 = a[0], m2 = b[0], m3 = JS ? 0.5f * (a[0] + b[0]) : 0.f;
#pragma unroll
  for (int c = 1; c < NCMAX; ++c) {
    m1 = fmaxf(m1, a[c]);
    m2 = fmaxf(m2, b[c]);
    if (JS) m3 = fmaxf(m3, 0.5f * (a[c] + b[c]));
  }
  float s1 = 0.f, s2 = 0.f, s3 = 0.f, zy1 = 0.f, zy2 = 0.f;
#pragma unroll
  for (int c0 = 0; c0 < NCMAX; c0 += 4) {
    MCD_OPAQUE_TRUE(go);
    if (go) {
#pragma unroll
      for (int c = c0; c < c0 + 4; ++c) {
        if (c >= NCMAX) continue;
        if (c == y) {
          zy1 = a[c];
          zy2 = b[c];
        }
        s1 += exp_nonpos(a[c] - m1);
        s2 += exp_nonpos(b[c] - m2);
        if (JS) s3 += exp_nonpos(0.5f * (a[c] + b[c]) - m3);
      }
    }
  }
  const float L1 = m1 + logf(s1), L2 = m2 + logf(s2), L3 = JS ? m3 + logf(s3) : 0.f;
  if (y >= 0) {
    ce1 = wy * (L1 - zy1);
    ce2 = wy * (L2 - zy2);
  }
  const float r1 = 1.f / s1, r2 = 1.f / s2, r3 = JS ? 1.f / s3 : 0.f;
  // p u of head 1 and q u of head 2 for class c (and, JSD, the third softmax)
  auto terms = [&](int c, float& p, float& q, float& pu, float& qu, float& pm) {
    p = exp_nonpos(a[c] - m1) * r1;
    q = exp_nonpos(b[c] - m2) * r2;
    const float lp = a[c] - L1, lq = b[c] - L2;
    pm = 0.f;
    if (KIND == DIST_SYMKL) {
      const float dl = lp - lq, dp = p - q;
      pu = 0.5f * (p * dl + dp);
      qu = 0.5f * (-dp - q * dl);
    } else if (KIND == DIST_MIS_SYMKL) {
      pu = p * (0.5f * ((lp + 1.f) - 2.f * q));
      qu = q * (0.5f * ((lq + 1.f) - 2.f * p));
    } else {
      const float zm = 0.5f * (a[c] + b[c]);
      const float lm = zm - L3;
      pm = exp_nonpos(zm - m3) * r3;
      pu = p * (0.5f * (lp - lm));
      qu = q * (0.5f * (lq - lm));
    }
  };
  float t1 = 0.f, t2 = 0.f;
#pragma unroll
  for (int c0 = 0; c0 < NCMAX; c0 += 4) {
    MCD_OPAQUE_TRUE(go);
    if (go) {
#pragma unroll
      for (int c = c0; c < c0 + 4; ++c) {
        if (c >= NCMAX) continue;
        if (c < C) {
          float p, q, pu, qu, pm;
          terms(c, p, q, pu, qu, pm);
          t1 += pu;
          t2 += qu;
          if (KIND == DIST_SYMKL)
            dsum += 0.5f * ((p - q) * ((a[c] - L1) - (b[c] - L2)));
          else if (KIND == DIST_MIS_SYMKL)
            dsum += 0.5f * ((p * (a[c] - L1) + q * (b[c] - L2)) - 2.f * (p * q));
          else
            dsum += pu + qu;
        }
      }
    }
  }
  if (g1 != nullptr || g2 != nullptr) {
    const float kce = (ce_coef != 0.f && y >= 0) ? ce_coef * wy / losses_w[3] : 0.f;
    const float kd = diff_coef * inv_m;
#pragma unroll
    for (int c0 = 0; c0 < NCMAX; c0 += 4) {
      MCD_OPAQUE_TRUE(go);
      if (go) {
#pragma unroll
        for (int c = c0; c < c0 + 4; ++c) {
          if (c >= NCMAX) continue;
          if (c < C) {
            const float oh = (c == y) ? 1.f : 0.f;
            float p, q, pu, qu, pm;
            terms(c, p, q, pu, qu, pm);
            const float j = JS ? -0.25f * ((p + q) - 2.f * pm) : 0.f;
            if (g1 != nullptr) g1[base + (size_t)c * HW] = kce * (p - oh) + kd * ((pu - p * t1) + j);
            if (g2 != nullptr) g2[base + (size_t)c * HW] = kce * (q - oh) + kd * ((qu - q * t2) + j);
          }
        }
      }
    }
  }
}

// The same losses with the x8 learned up-sampler (up8.hip) computed on the fly: the classifiers of the MCD configuration are
// nothing but that up-sampler (models/dilated_fcn.py:357-366 behind DRNSegPixelClassifier), so their full-resolution logits
// need never exist in memory -- each is four multiply-adds on the 64x smaller score map.
//
// Persistent workgroups of 8 waves, one per CU.  The 16x16 kernels of every class and head stay in LDS for the workgroup's
// life (re-ordered so that the four taps a pixel needs are one 16-byte read); the work items are patches of 8 rows x 64
// columns whose rows share their two input rows -- output rows 8i-4 .. 8i+3 -- so an item stages only 2 x 10 scores per class
// and head, fetched into registers while the previous item is being computed.  Wave k of the workgroup owns the patch row with
// kernel rows (k, k+8).  The multiply-adds run in the order of up8_fwd_kernel (absent inputs staged as zeros), so logits,
// the losses' summands and the gradients equal the two-pass result bit for bit; only the summation order of the loss
// values differs (per lane over its items, then the block, then fp64 over blocks).
// (UP_COLS = 64, UP_JP = 9 input-column pairs a 64-pixel row segment touches, UP_NT = 512: up8_patch.h)

// ---- the same kernel with nothing between an item's stores and the next item's inputs ----------------------------------------
// The kernel above fetches the next item's scores into registers (and reads labels and class weights from memory inside the item):
// loads the compiler tracks.  The counter that tracks them (vmcnt) also counts the item's 2 C gradient stores, in issue order, so
// the wait in front of the first use of any of those loads -- `s_waitcnt vmcnt(0)`, the stores sit behind data-dependent branches the
// compiler cannot count -- drains every store of the previous item: the workgroup, the only one on its CU, alternates between
// computing and writing (at the benchmark's shape 0.75 ms per launch with the gradients, 0.50 ms without them, for 0.34 ms of HBM writes at
// the rate a copy reaches; this kernel: 0.58 / 0.38 ms -- tools/probes/up8_loss_probe.py).
// Here every input of the loop arrives by LDS-DMA, which the compiler does not track, into two buffers: the next item's scores
// (one dword per lane, the staging layout as it is), its labels (16 B per lane: one row segment of 64 labels per wave) -- issued
// BEFORE the current item's stores, so that a counted `s_waitcnt vmcnt(63)` at the top of the next item proves them complete
// while up to 63 of the 2 C stores of each wave are still in flight (a wave that issued fewer than 63 stores waits for 0); class
// weights and the up-sampling kernels stay in LDS for the workgroup's life.  One barrier per item instead of two.  Classes past C
// (EXACT = false) get their -inf by a select instead of through staged constants (the DMA fills those slots with zeros).
// Arithmetic, item order and summation order are the register kernel's: gradients and loss values are bitwise the same.
constexpr unsigned UP_OOB = 0x80000000u;
template <int NCMAX, bool TWO>
struct UpDmaLayout {
  static constexpr int HEADS = TWO ? 2 : 1;
  static constexpr int SLOTS = NCMAX * UP_JP * 4;            // staged scores per head and item
  static constexpr int SPK = (SLOTS + UP_NT - 1) / UP_NT;    // DMA instructions per head, item and wave
  static constexpr int SP = SPK * UP_NT;                     // floats per head and buffer (the tail takes the DMA's zero fill)
  static constexpr int W_FLOATS = HEADS * NCMAX * 256;
  static constexpr int S_FLOATS = 2 * HEADS * SP;
  static constexpr int LAB_BYTES = 2 * (UP_NT / 64) * 1024;  // per buffer and wave: 64 labels (512 B) + 512 B of zero fill
  static constexpr int CW_FLOATS = (NCMAX + 63) / 64 * 64;
  static constexpr size_t BYTES = (size_t)(W_FLOATS + S_FLOATS + CW_FLOATS) * 4 + LAB_BYTES;
};

// The kernels themselves (loss_front.h), twice: the L1 family, then the two-head distances.  A wave of the LDS-DMA kernel issues the
// same 2 C gradient stores per item behind the next item's DMAs whatever the distance (pixel_dist stores where pixel_losses does), so
// its counted wait holds for the new kernels as well (_lib.loss_dma_store_counts for the L1 names, _lib.dist_dma_store_counts for the new ones).
#define MCD_FRONT_T2 template <int NCMAX, bool TWO>
#define MCD_FRONT_T3 template <int NCMAX, bool TWO, bool EXACT>
#define MCD_FRONT_PLAIN softmax_ce_l1_kernel
#define MCD_FRONT_UP8 up8_softmax_ce_l1_kernel
#define MCD_FRONT_DMA up8_softmax_ce_l1_dma_kernel
#define MCD_FRONT_HEADS
#define MCD_FRONT_PIXEL pixel_losses<NCMAX, TWO>
#include "loss_front.h"
#undef MCD_FRONT_T2
#undef MCD_FRONT_T3
#undef MCD_FRONT_PLAIN
#undef MCD_FRONT_UP8
#undef MCD_FRONT_DMA
#undef MCD_FRONT_HEADS
#undef MCD_FRONT_PIXEL

#define MCD_FRONT_T2 template <int NCMAX, int KIND>
#define MCD_FRONT_T3 template <int NCMAX, bool EXACT, int KIND>
#define MCD_FRONT_PLAIN softmax_ce_dist_kernel
#define MCD_FRONT_UP8 up8_softmax_ce_dist_kernel
#define MCD_FRONT_DMA up8_softmax_ce_dist_dma_kernel
#define MCD_FRONT_HEADS constexpr bool TWO = true
#define MCD_FRONT_PIXEL pixel_dist<NCMAX, KIND>
#include "loss_front.h"
#undef MCD_FRONT_T2
#undef MCD_FRONT_T3
#undef MCD_FRONT_PLAIN
#undef MCD_FRONT_UP8
#undef MCD_FRONT_DMA
#undef MCD_FRONT_HEADS
#undef MCD_FRONT_PIXEL

// has_ce: a cross-entropy term was requested.  With an all-background / all-ignored batch the normaliser W = sum w[y] is 0
// and the reference's weighted mean is 0/0: nn.NLLLoss2d returns NaN and NaN gradients (loss.py:7-13).  The kernel does the
// same -- value here, gradients through kce = ce_coef * w[y] / W in the main kernel -- so the failure is as visible as in
// the reference instead of a healthy-looking 0 in the log while NaN gradients reach the optimizer.
// The sums are partials_total<3> (block_reduce.h) written out: this kernel runs in every training step and is held to the instruction
// stream it always had, which the call does not reproduce (the LDS rows reach the helper as generic pointers and are scheduled anew).
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* __restrict__ part, int64_t nblk, float* __restrict__ losses,
                                                            double inv_m, int has_ce) {
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < nblk; i += 256) {
    s[0] += (double)part[i * 3 + 0];
    s[1] += (double)part[i * 3 + 1];
    s[2] += (double)part[i * 3 + 2];
  }
  __shared__ double sh[3][4];
  for (int q = 0; q < 3; ++q) {
    const double v = wave_sum_d(s[q]);
    if ((threadIdx.x & 63) == 0) sh[q][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double W = (double)losses[3];
    const double c1 = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
    const double c2 = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
    const double d = (sh[2][0] + sh[2][1]) + (sh[2][2] + sh[2][3]);
    losses[0] = has_ce ? (float)(c1 / W) : 0.f;
    losses[1] = has_ce ? (float)(c2 / W) : 0.f;
    losses[2] = (float)(d * inv_m);
  }
}

// Inference tail (adapt_tester.py:101-124, util.py:44-48): o = z1 or (z1 + z2)/2; label = argmax over the first C_used
// classes (the background channel is excluded unless it was trained); entropy term = sum_c p_c log(p_c + 1e-6) over ALL classes.
template <int NCMAX>
__global__ __launch_bounds__(256) void predict_kernel(const float* __restrict__ z1, const float* __restrict__ z2,
                                                      uint8_t* __restrict__ labels, float* __restrict__ part, int C, int C_used,
                                                      int HW, int64_t P) {
  const int64_t pix = blockIdx.x * (int64_t)LOSS_BLOCK + threadIdx.x;
  float ent = 0.f;
  if (pix < P) {
    const int64_t n = pix / HW;
    const int hw = (int)(pix - n * HW);
    const size_t base = (size_t)n * C * HW + hw;
    float a[NCMAX];
#pragma unroll
    for (int c = 0; c < NCMAX; ++c) {
      float v = -INFINITY;
      if (c < C) {
        v = z1[base + (size_t)c * HW];
        if (z2 != nullptr) v = (v + z2[base + (size_t)c * HW]) / 2.f;
      }
      a[c] = v;
    }
    int best;
    MCD_PREDICT_PIXEL(a, best, ent)
    labels[pix] = (uint8_t)best;
  }
  __shared__ float sh[1][4];
  float v[1] = {ent};
  block_gather(v, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tree_total<4>(sh[0]);
}

__global__ void scale_by_device_scalar_kernel(float* __restrict__ buf, const float* __restrict__ scale, int64_t n4, int64_t n) {
  const float s = *scale;
  float4* b4 = reinterpret_cast<float4*>(buf);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 v = b4[i];
    v.x *= s; v.y *= s; v.z *= s; v.w *= s;
    b4[i] = v;
  }
  for (int64_t i = n4 * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) buf[i] *= s;
}

int wsum_blocks(int64_t P) { return ceil_div64(P, 256 * 8, 1024); }

template <int NCMAX>
void launch_loss(int kind, bool two, dim3 grid, hipStream_t st, const float* z1, const float* z2, const int64_t* labels, const float* cw,
                 int64_t ignore_index, float ce_coef, float diff_coef, const float* losses, float* g1, float* g2, float* part,
                 int C, int HW, int64_t P, float inv_m) {
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(LOSS_BLOCK), 0, st, z1, z2, labels, cw, ignore_index, ce_coef, diff_coef, losses, g1, g2, part, C,
                       HW, P, inv_m);
  };
  switch (kind) {
    case DIST_SYMKL: go(softmax_ce_dist_kernel<NCMAX, DIST_SYMKL>); break;
    case DIST_MIS_SYMKL: go(softmax_ce_dist_kernel<NCMAX, DIST_MIS_SYMKL>); break;
    case DIST_JSD: go(softmax_ce_dist_kernel<NCMAX, DIST_JSD>); break;
    default:
      if (two)
        go(softmax_ce_l1_kernel<NCMAX, true>);
      else
        go(softmax_ce_l1_kernel<NCMAX, false>);
  }
}

template <int NCMAX>
int launch_up_loss(const char* entry, int kind, bool two, int blocks, size_t lds, hipStream_t st, const float* s1, const float* w1, const float* s2,
                   const float* w2, const int64_t* labels, const float* cw, int64_t ignore_index, float ce_coef, float diff_coef,
                   const float* losses, float* g1, float* g2, float* part, int N, int C, int Hi, int Wi, float inv_m) {
  auto go = [&](auto kern) {
    if (lds > 64 * 1024) {
      const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) {
        mcdseg_set_error("%s: cannot reserve %zu bytes of LDS: %s", entry, lds, hipGetErrorString(e));
        return -5;
      }
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(UP_NT), lds, st, s1, w1, s2, w2, labels, cw, ignore_index, ce_coef, diff_coef, losses,
                       g1, g2, part, N, C, Hi, Wi, inv_m);
    return 0;
  };
  switch (kind) {
    case DIST_SYMKL: return go(up8_softmax_ce_dist_kernel<NCMAX, DIST_SYMKL>);
    case DIST_MIS_SYMKL: return go(up8_softmax_ce_dist_kernel<NCMAX, DIST_MIS_SYMKL>);
    case DIST_JSD: return go(up8_softmax_ce_dist_kernel<NCMAX, DIST_JSD>);
    default: return two ? go(up8_softmax_ce_l1_kernel<NCMAX, true>) : go(up8_softmax_ce_l1_kernel<NCMAX, false>);
  }
}

template <int NCMAX, bool EXACT>
int launch_up_loss_dma(const char* entry, int kind, bool two, int blocks, hipStream_t st, const float* s1, const float* w1, const float* s2, const float* w2,
                       const int64_t* labels, const float* cw, int64_t ignore_index, float ce_coef, float diff_coef, const float* losses,
                       float* g1, float* g2, float* part, int N, int C, int Hi, int Wi, float inv_m) {
  auto go = [&](auto kern, size_t lds) {
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      mcdseg_set_error("%s: cannot reserve %zu bytes of LDS: %s", entry, lds, hipGetErrorString(e));
      return -5;
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(UP_NT), lds, st, s1, w1, s2, w2, labels, cw, ignore_index, ce_coef, diff_coef, losses,
                       g1, g2, part, N, C, Hi, Wi, inv_m);
    return 0;
  };
  switch (kind) {
    case DIST_SYMKL: return go(up8_softmax_ce_dist_dma_kernel<NCMAX, EXACT, DIST_SYMKL>, UpDmaLayout<NCMAX, true>::BYTES);
    case DIST_MIS_SYMKL: return go(up8_softmax_ce_dist_dma_kernel<NCMAX, EXACT, DIST_MIS_SYMKL>, UpDmaLayout<NCMAX, true>::BYTES);
    case DIST_JSD: return go(up8_softmax_ce_dist_dma_kernel<NCMAX, EXACT, DIST_JSD>, UpDmaLayout<NCMAX, true>::BYTES);
    default:
      return two ? go(up8_softmax_ce_l1_dma_kernel<NCMAX, true, EXACT>, UpDmaLayout<NCMAX, true>::BYTES)
                 : go(up8_softmax_ce_l1_dma_kernel<NCMAX, false, EXACT>, UpDmaLayout<NCMAX, false>::BYTES);
  }
}

// the instantiation of the DMA kernel for C classes: the benchmark's 41 has its own (no padding classes: 15 % less arithmetic)
int up_loss_dma_ncmax(int C) { return C <= 16 ? 16 : (C <= 24 ? 24 : (C == 41 ? 41 : 48)); }

// labels: 0 none, 1 at a 16-byte aligned base, 2 at a base that is only 8-byte aligned (a contiguous view that starts at an odd element
// of a larger int64 tensor).  The DMA kernel fetches labels as 16-byte units from base + a multiple of 16, and nothing establishes that
// a 16-byte LDS-DMA from an address that is not 16-byte aligned is legal: such labels go to the register-staged kernel, which reads
// them as single int64.
bool up_loss_dma_ok(int64_t N, int64_t C, int64_t Hi, int64_t Wi, int labels) {
  const bool on = mcd_opt(MCD_OPT_UP8_LOSS_DMA) != 0;  // 0: the register-staged kernel (A/B, and the parity test's other side)
  // buffer resources address 32 bits (the DMA's offsets are formed in int)
  return on && labels != 2 && N * C * Hi * Wi * 4 < (1ll << 31) && (!labels || N * Hi * Wi * 64 * 8 < (1ll << 31));
}
int up_loss_labels_kind(const int64_t* labels) { return labels == nullptr ? 0 : ((reinterpret_cast<uintptr_t>(labels) & 15) == 0 ? 1 : 2); }

}  // namespace

extern "C" size_t mcdseg_loss_workspace_bytes(int32_t N, int32_t HW) {
  if (N <= 0 || HW <= 0) return 0;
  const int64_t P = (int64_t)N * HW;
  return (size_t)(ceil_div64(P, LOSS_BLOCK) * 3 + wsum_blocks(P)) * sizeof(float);
}

extern "C" size_t mcdseg_label_weight_sum_workspace_bytes(int64_t P) { return P > 0 ? (size_t)wsum_blocks(P) * sizeof(float) : 0; }

extern "C" int mcdseg_label_weight_sum(const int64_t* labels, const float* class_weight, int64_t ignore_index, int32_t C, int64_t P,
                                       float* out, void* workspace, size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(labels && out && workspace && C > 0 && P > 0, "label_weight_sum: bad arguments");
  const int wb = wsum_blocks(P);
  MCD_REQUIRE(workspace_bytes >= (size_t)wb * sizeof(float), "label_weight_sum: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(label_wsum_kernel, dim3(wb), dim3(256), 0, st, labels, class_weight, ignore_index, C, P, (float*)workspace);
  MCD_LAUNCH_CHECK("label_wsum");
  hipLaunchKernelGGL(sum_finalize_kernel<float>, dim3(1), dim3(256), 0, st, (const float*)workspace, (int64_t)wb, 1.0, out);
  MCD_LAUNCH_CHECK("wsum_finalize");
  return 0;
}

// both entry points of the plain-logit kernels; ``kind`` has been checked
static int softmax_ce_any(const char* entry, int kind, const float* z1, const float* z2, const int64_t* labels, const float* class_weight,
                          int64_t ignore_index, float ce_coef, float diff_coef, const float* wsum_in, float* g1, float* g2, float* losses,
                          int32_t N, int32_t C, int32_t HW, void* workspace, size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(z1 && losses && workspace, "%s: null pointer", entry);
  MCD_REQUIRE(N > 0 && C > 0 && HW > 0, "%s: bad dims", entry);
  MCD_REQUIRE(C <= 48, "%s: at most 48 classes are kept in registers (got %d)", entry, C);
  MCD_REQUIRE(z2 != nullptr || (g2 == nullptr && diff_coef == 0.f), "%s: discrepancy needs z2", entry);
  MCD_REQUIRE(z2 != nullptr || kind == DIST_L1, "%s: dist_kind %d is a distance between two heads: z2 is NULL", entry, kind);
  MCD_REQUIRE(labels != nullptr || ce_coef == 0.f, "%s: cross-entropy needs labels", entry);
  MCD_REQUIRE(workspace_bytes >= mcdseg_loss_workspace_bytes(N, HW), "%s: workspace too small", entry);
  const int64_t P = (int64_t)N * HW;
  const int64_t nblk = ceil_div64(P, LOSS_BLOCK);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  float* wpart = part + nblk * 3;
  const int wb = wsum_blocks(P);
  if (wsum_in != nullptr) {
    // normaliser supplied by the caller (data parallel: the all-reduced sum of w[y] over every rank's shard)
    (void)hipMemcpyAsync(losses + 3, wsum_in, sizeof(float), hipMemcpyDeviceToDevice, st);
  } else if (labels != nullptr) {
    hipLaunchKernelGGL(label_wsum_kernel, dim3(wb), dim3(256), 0, st, labels, class_weight, ignore_index, C, P, wpart);
    MCD_LAUNCH_CHECK("label_wsum");
    hipLaunchKernelGGL(sum_finalize_kernel<float>, dim3(1), dim3(256), 0, st, (const float*)wpart, (int64_t)wb, 1.0, losses + 3);
    MCD_LAUNCH_CHECK("wsum_finalize");
  } else {
    (void)hipMemsetAsync(losses + 3, 0, sizeof(float), st);
  }
  const double inv_m = 1.0 / ((double)P * (double)C);
  dim3 grid((unsigned)nblk);
  const bool two = z2 != nullptr;
  if (C <= 16)
    launch_loss<16>(kind, two, grid, st, z1, z2, labels, class_weight, ignore_index, ce_coef, diff_coef, losses, g1, g2, part, C, HW, P,
                    (float)inv_m);
  else if (C <= 24)
    launch_loss<24>(kind, two, grid, st, z1, z2, labels, class_weight, ignore_index, ce_coef, diff_coef, losses, g1, g2, part, C, HW, P,
                    (float)inv_m);
  else
    launch_loss<48>(kind, two, grid, st, z1, z2, labels, class_weight, ignore_index, ce_coef, diff_coef, losses, g1, g2, part, C, HW, P,
                    (float)inv_m);
  MCD_LAUNCH_CHECK(entry);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)part, nblk, losses, inv_m,
                     labels != nullptr ? 1 : 0);
  MCD_LAUNCH_CHECK("loss_finalize");
  return 0;
}

extern "C" int mcdseg_softmax_ce_l1(const float* z1, const float* z2, const int64_t* labels, const float* class_weight,
                                    int64_t ignore_index, float ce_coef, float diff_coef, const float* wsum_in, float* g1, float* g2,
                                    float* losses, int32_t N, int32_t C, int32_t HW, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  return softmax_ce_any("softmax_ce_l1", DIST_L1, z1, z2, labels, class_weight, ignore_index, ce_coef, diff_coef, wsum_in, g1, g2, losses, N, C, HW,
                        workspace, workspace_bytes, stream);
}

extern "C" int mcdseg_softmax_ce_dist(const float* z1, const float* z2, const int64_t* labels, const float* class_weight,
                                      int64_t ignore_index, float ce_coef, float diff_coef, const float* wsum_in, float* g1, float* g2,
                                      float* losses, int32_t N, int32_t C, int32_t HW, int32_t dist_kind, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(dist_kind >= DIST_L1 && dist_kind <= DIST_JSD, "softmax_ce_dist: unknown dist_kind %d (MCDSEG_DIST_L1 .. MCDSEG_DIST_JSD)",
              dist_kind);
  return softmax_ce_any("softmax_ce_dist", dist_kind, z1, z2, labels, class_weight, ignore_index, ce_coef, diff_coef, wsum_in, g1, g2, losses, N, C, HW,
                        workspace, workspace_bytes, stream);
}

// persistent workgroups: one per CU (the kernels of all classes fill most of a CU's LDS), never more than there are items
static int up_loss_blocks(int32_t N, int32_t Hi, int32_t Wi) {
  const int64_t items = (int64_t)N * (Hi + 1) * ceil_div(8 * Wi, UP_COLS);
  return (int)(items < 256 ? items : 256);
}

extern "C" size_t mcdseg_up8_loss_workspace_bytes(int32_t N, int32_t Hi, int32_t Wi) {
  if (N <= 0 || Hi <= 0 || Wi <= 0) return 0;
  return (size_t)(up_loss_blocks(N, Hi, Wi) * 3 + wsum_blocks((int64_t)N * Hi * Wi * 64)) * sizeof(float);
}

static int up8_softmax_ce_any(const char* entry, int kind, const float* s1, const float* w1, const float* s2, const float* w2, const int64_t* labels,
                              const float* class_weight, int64_t ignore_index, float ce_coef, float diff_coef, const float* wsum_in,
                              float* g1, float* g2, float* losses, int32_t N, int32_t C, int32_t Hi, int32_t Wi, void* workspace,
                              size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(s1 && w1 && losses && workspace, "%s: null pointer", entry);
  MCD_REQUIRE(N > 0 && C > 0 && Hi > 0 && Wi > 0, "%s: bad dims", entry);
  MCD_REQUIRE(C <= 48, "%s: at most 48 classes are kept in registers (got %d)", entry, C);
  MCD_REQUIRE((s2 == nullptr) == (w2 == nullptr), "%s: s2 and w2 come together", entry);
  MCD_REQUIRE(s2 != nullptr || (g2 == nullptr && diff_coef == 0.f), "%s: discrepancy needs the second head", entry);
  MCD_REQUIRE(s2 != nullptr || kind == DIST_L1, "%s: dist_kind %d is a distance between two heads: s2 is NULL", entry, kind);
  MCD_REQUIRE(labels != nullptr || ce_coef == 0.f, "%s: cross-entropy needs labels", entry);
  MCD_REQUIRE((int64_t)N * (Hi + 1) * ceil_div(8 * Wi, UP_COLS) < (1ll << 31), "%s: too many patches", entry);
  MCD_REQUIRE(workspace_bytes >= mcdseg_up8_loss_workspace_bytes(N, Hi, Wi), "%s: workspace too small", entry);
  const int64_t P = (int64_t)N * Hi * Wi * 64;
  const int nblk = up_loss_blocks(N, Hi, Wi);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  float* wpart = part + (size_t)nblk * 3;
  const int wb = wsum_blocks(P);
  if (wsum_in != nullptr) {
    (void)hipMemcpyAsync(losses + 3, wsum_in, sizeof(float), hipMemcpyDeviceToDevice, st);
  } else if (labels != nullptr) {
    hipLaunchKernelGGL(label_wsum_kernel, dim3(wb), dim3(256), 0, st, labels, class_weight, ignore_index, C, P, wpart);
    MCD_LAUNCH_CHECK("label_wsum");
    hipLaunchKernelGGL(sum_finalize_kernel<float>, dim3(1), dim3(256), 0, st, (const float*)wpart, (int64_t)wb, 1.0, losses + 3);
    MCD_LAUNCH_CHECK("wsum_finalize");
  } else {
    (void)hipMemsetAsync(losses + 3, 0, sizeof(float), st);
  }
  const double inv_m = 1.0 / ((double)P * (double)C);
  const bool two = s2 != nullptr;
  if (up_loss_dma_ok(N, C, Hi, Wi, up_loss_labels_kind(labels))) {
    int rc;
#define MCD_UP_DMA(NC)                                                                                                              \
  rc = (C == NC) ? launch_up_loss_dma<NC, true>(entry, kind, two, nblk, st, s1, w1, s2, w2, labels, class_weight, ignore_index, ce_coef, diff_coef, \
                                                losses, g1, g2, part, N, C, Hi, Wi, (float)inv_m)                                    \
                 : launch_up_loss_dma<NC, false>(entry, kind, two, nblk, st, s1, w1, s2, w2, labels, class_weight, ignore_index, ce_coef,         \
                                                 diff_coef, losses, g1, g2, part, N, C, Hi, Wi, (float)inv_m)
    switch (up_loss_dma_ncmax(C)) {
      case 16: MCD_UP_DMA(16); break;
      case 24: MCD_UP_DMA(24); break;
      case 41: rc = launch_up_loss_dma<41, true>(entry, kind, two, nblk, st, s1, w1, s2, w2, labels, class_weight, ignore_index, ce_coef, diff_coef,
                                                 losses, g1, g2, part, N, C, Hi, Wi, (float)inv_m); break;
      default: MCD_UP_DMA(48); break;
    }
#undef MCD_UP_DMA
    if (rc != 0) return rc;
    MCD_LAUNCH_CHECK(entry);
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)part, (int64_t)nblk, losses, inv_m,
                       labels != nullptr ? 1 : 0);
    MCD_LAUNCH_CHECK("loss_finalize");
    return 0;
  }
  const int ncmax = C <= 16 ? 16 : (C <= 24 ? 24 : 48);  // the instantiation chosen below
  const size_t lds = (size_t)(two ? 2 : 1) * ncmax * (256 + 4 * UP_JP) * sizeof(float);
  int rc;
  if (C <= 16)
    rc = launch_up_loss<16>(entry, kind, two, nblk, lds, st, s1, w1, s2, w2, labels, class_weight, ignore_index, ce_coef, diff_coef, losses, g1, g2,
                            part, N, C, Hi, Wi, (float)inv_m);
  else if (C <= 24)
    rc = launch_up_loss<24>(entry, kind, two, nblk, lds, st, s1, w1, s2, w2, labels, class_weight, ignore_index, ce_coef, diff_coef, losses, g1, g2,
                            part, N, C, Hi, Wi, (float)inv_m);
  else
    rc = launch_up_loss<48>(entry, kind, two, nblk, lds, st, s1, w1, s2, w2, labels, class_weight, ignore_index, ce_coef, diff_coef, losses, g1, g2,
                            part, N, C, Hi, Wi, (float)inv_m);
  if (rc != 0) return rc;
  MCD_LAUNCH_CHECK(entry);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)part, (int64_t)nblk, losses, inv_m,
                     labels != nullptr ? 1 : 0);
  MCD_LAUNCH_CHECK("loss_finalize");
  return 0;
}

extern "C" int mcdseg_up8_softmax_ce_l1(const float* s1, const float* w1, const float* s2, const float* w2, const int64_t* labels,
                                        const float* class_weight, int64_t ignore_index, float ce_coef, float diff_coef,
                                        const float* wsum_in, float* g1, float* g2, float* losses, int32_t N, int32_t C, int32_t Hi,
                                        int32_t Wi, void* workspace, size_t workspace_bytes, void* stream) {
  return up8_softmax_ce_any("up8_softmax_ce_l1", DIST_L1, s1, w1, s2, w2, labels, class_weight, ignore_index, ce_coef, diff_coef, wsum_in, g1, g2, losses, N,
                            C, Hi, Wi, workspace, workspace_bytes, stream);
}

extern "C" int mcdseg_up8_softmax_ce_dist(const float* s1, const float* w1, const float* s2, const float* w2, const int64_t* labels,
                                          const float* class_weight, int64_t ignore_index, float ce_coef, float diff_coef,
                                          const float* wsum_in, float* g1, float* g2, float* losses, int32_t N, int32_t C, int32_t Hi,
                                          int32_t Wi, int32_t dist_kind, void* workspace, size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(dist_kind >= DIST_L1 && dist_kind <= DIST_JSD,
              "up8_softmax_ce_dist: unknown dist_kind %d (MCDSEG_DIST_L1 .. MCDSEG_DIST_JSD)", dist_kind);
  return up8_softmax_ce_any("up8_softmax_ce_dist", dist_kind, s1, w1, s2, w2, labels, class_weight, ignore_index, ce_coef, diff_coef, wsum_in, g1, g2, losses, N,
                            C, Hi, Wi, workspace, workspace_bytes, stream);
}

extern "C" size_t mcdseg_predict_workspace_bytes(int32_t N, int32_t HW) {
  return (N > 0 && HW > 0) ? (size_t)ceil_div64((int64_t)N * HW, LOSS_BLOCK) * sizeof(float) : 0;
}

extern "C" int mcdseg_predict_labels(const float* z1, const float* z2, uint8_t* labels, float* entropy, int32_t N, int32_t C,
                                     int32_t C_used, int32_t HW, void* workspace, size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(z1 && labels && entropy && workspace, "predict_labels: null pointer");
  MCD_REQUIRE(N > 0 && HW > 0 && C > 0 && C <= 48 && C_used > 0 && C_used <= C && C_used <= 256, "predict_labels: bad dims");
  MCD_REQUIRE(workspace_bytes >= mcdseg_predict_workspace_bytes(N, HW), "predict_labels: workspace too small");
  const int64_t P = (int64_t)N * HW;
  const int64_t nblk = ceil_div64(P, LOSS_BLOCK);
  hipStream_t st = (hipStream_t)stream;
  if (C <= 16)
    hipLaunchKernelGGL(predict_kernel<16>, dim3((unsigned)nblk), dim3(LOSS_BLOCK), 0, st, z1, z2, labels, (float*)workspace, C, C_used, HW, P);
  else if (C <= 24)
    hipLaunchKernelGGL(predict_kernel<24>, dim3((unsigned)nblk), dim3(LOSS_BLOCK), 0, st, z1, z2, labels, (float*)workspace, C, C_used, HW, P);
  else
    hipLaunchKernelGGL(predict_kernel<48>, dim3((unsigned)nblk), dim3(LOSS_BLOCK), 0, st, z1, z2, labels, (float*)workspace, C, C_used, HW, P);
  MCD_LAUNCH_CHECK("predict_labels");
  hipLaunchKernelGGL(sum_finalize_kernel<float>, dim3(1), dim3(256), 0, st, (const float*)workspace, nblk, -1.0 / ((double)P * (double)C), entropy);
  MCD_LAUNCH_CHECK("predict_finalize");
  return 0;
}

extern "C" int mcdseg_scale_by_device_scalar(float* buf, const float* scale, int64_t n, void* stream) {
  MCD_REQUIRE(buf && scale && n >= 0, "scale_by_device_scalar: bad arguments");
  if (n == 0) return 0;
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(buf) & 15) == 0, "scale_by_device_scalar: buffer must be 16-byte aligned");
  const int64_t n4 = n / 4;
  int64_t blocks = ceil_div64(n4 > 0 ? n4 : n, 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(scale_by_device_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, buf, scale, n4, n);
  MCD_LAUNCH_CHECK("scale_by_device_scalar");
  return 0;
}

// Which kernel mcdseg_up8_softmax_ce_l1 launches for a problem (profilers, bench.py's per-kernel tables): the class count of the LDS-DMA
// kernel's instantiation (16, 24, 41, 48), or MINUS that of the register-staged kernel (16, 24, 48) when the option UP8_LOSS_DMA is 0
// or a tensor outgrows a 32-bit buffer resource, or the labels start at an address that is not 16-byte aligned (labelled = 2; 1: labels at
// an aligned base, 0: none).
extern "C" int32_t mcdseg_up8_loss_variant(int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t labelled) {
  if (N <= 0 || C <= 0 || Hi <= 0 || Wi <= 0) return 0;
  if (up_loss_dma_ok(N, C, Hi, Wi, labelled == 2 ? 2 : (labelled != 0 ? 1 : 0))) return up_loss_dma_ncmax(C);
  return -(C <= 16 ? 16 : (C <= 24 ? 24 : 48));
}
