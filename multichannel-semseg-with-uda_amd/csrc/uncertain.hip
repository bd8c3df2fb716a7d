// The aleatoric-uncertainty loss of UncertainDRNSeg.get_loss (models/dilated_fcn.py:169-214) over all T Monte-Carlo dropout draws in
// ONE pass over the pixels, with the gradients w.r.t. the two (never stored) full-resolution maps, and the tester's uncertainty map.
//
// The reference runs the whole network T = n_dropout_exp times per step.  Its only randomness is Dropout2d(0.2) on the 1/8-resolution
// scores s (a factor m_t[n,c] in {0, 1/(1-p)} per channel and draw) and one scalar r_t = np.random.rand() per draw; both up-samplers
// are depthwise and linear, so with U = up(s), V = up_std(s) formed once (dilated_fcn.py:153-161)
//   pred_mean_t = m_t U,   pred_std_t = relu(m_t V) = m_t relu(V),   y_hat_t = m_t U + (m_t relu(V)) r_t          (:177-181)
// and per pixel i of sample n with label g, class weights cw, W = sum_i cw[g_i], HW = 64 Hi Wi, lambda = uncertain_weight:
//   B   = (1/T) sum_t CrossEntropyLoss2d(pred_mean_t, g) = (1/(T W)) sum_t sum_i cw[g_i] (logsumexp(m_t U) - m_t[g] U[g])   (:178, :202)
//   p_t = softmax(y_hat_t)[g],  S = sum_t p_t                                                                      (:183-200)
//   U_n = (lambda/HW) sum_i log(S_i / T)                                                                           (:203-204, :212)
// (the sign of U_n is the reference's: + log, where Kendall & Gal minimise - log; DESIGN.md says what that means).
// Gradients for upstream gb (of B) and gu[n] (of U_n), draws summed in registers:
//   a_t[c] = gb cw[g] / (T W) (softmax(m_t U)[c] - [c = g])
//   b_t[c] = gu[n] (lambda/HW) (p_t / S) ([c = g] - softmax(y_hat_t)[c])
//   GU[c]  = sum_t m_t[c] (a_t[c] + b_t[c])            = dL/dU
//   GV[c]  = sum_t m_t[c] [V[c] > 0] r_t b_t[c]        = dL/dV
// which mcdseg_up8_bwd turns into d/ds and the two weight gradients.  Softmax and log-sum-exp subtract the maximum; the reference's
// bare log(sum(exp)) is the same value wherever it is finite.
//
// Kernel: the register-staged up-sampling front end of the two-head loss kernel (up8_patch.h) with s1 == s2 = s, w1 = up.weight,
// w2 = up_std.weight: workgroups of 8 waves walk patches of 8 rows x 64 columns, one lane per pixel with U[] and relu(V)[] in
// registers.  A workgroup stays within ONE sample (grid.y), so that sample's T x C dropout factors and the T scalars r_t are
// staged in LDS once.  Loop 1 over the draws accumulates the cross-entropy and S; loop 2 (backward only) recomputes the two softmaxes
// of each draw -- 2 C exponentials beside 2 C four-byte stores per pixel -- and accumulates GU and GV.  No tensor with a T
// dimension exists.  Loss values: per-lane sums over the lane's pixels, one partial per workgroup, fp64 in the finalize launch; no
// atomics, so results are bit-reproducible.
#include "block_reduce.h"

namespace {

#include "up8_patch.h"

constexpr int UNC_TMAX = 32;

// one draw of one pixel: maxima, sums of exponentials and the label's entries of y_t = m_t U and y_hat_t = y_t + (m_t relu(V)) r_t.
// mt: the draw's NCMAX factors in LDS (1 for the padding classes, whose U is -inf and relu(V) is 0: both logits stay -inf).
template <int NCMAX>
__device__ __forceinline__ void draw_stats(const float (&u)[NCMAX], const float (&v)[NCMAX], const float* mt, float rt, int y, float& m1,
                                           float& m2, float& s1, float& s2, float& y1g, float& y2g) {
  m1 = -INFINITY;
  m2 = -INFINITY;
#pragma unroll
  for (int c0 = 0; c0 < NCMAX; c0 += 8) {
    MCD_OPAQUE_TRUE(go);
    if (go) {
#pragma unroll
      for (int c = c0; c < c0 + 8; ++c) {
        if (c >= NCMAX) continue;
        const float y1 = mt[c] * u[c];
        const float y2 = y1 + (mt[c] * v[c]) * rt;
        m1 = fmaxf(m1, y1);
        m2 = fmaxf(m2, y2);
      }
    }
  }
  s1 = 0.f;
  s2 = 0.f;
  y1g = 0.f;
  y2g = 0.f;
#pragma unroll
  for (int c0 = 0; c0 < NCMAX; c0 += 4) {
    MCD_OPAQUE_TRUE(go);
    if (go) {
#pragma unroll
      for (int c = c0; c < c0 + 4; ++c) {
        if (c >= NCMAX) continue;
        const float y1 = mt[c] * u[c];
        const float y2 = y1 + (mt[c] * v[c]) * rt;
        if (c == y) {
          y1g = y1;
          y2g = y2;
        }
        s1 += exp_nonpos(y1 - m1);
        s2 += exp_nonpos(y2 - m2);
      }
    }
  }
}

template <int NCMAX, bool BWD>
__global__ __launch_bounds__(UP_NT) void up8_uncertain_kernel(const float* __restrict__ s, const float* __restrict__ w_up,
                                                              const float* __restrict__ w_std, const int64_t* __restrict__ labels,
                                                              const float* __restrict__ cw, int64_t ignore_index,
                                                              const uint8_t* __restrict__ keep, const float* __restrict__ rnd,
                                                              float keep_scale, const float* __restrict__ wsum, float lam_hw,
                                                              const float* __restrict__ gb, const float* __restrict__ gu,
                                                              float* __restrict__ GU, float* __restrict__ GV, float* __restrict__ part,
                                                              int N, int C, int Hi, int Wi, int T) {
  extern __shared__ __attribute__((aligned(16))) float up_sm[];
  constexpr int HEADS = 2;
  constexpr int SREG = (HEADS * NCMAX * UP_JP * 4 + UP_NT - 1) / UP_NT;
  constexpr int nstage = HEADS * NCMAX * UP_JP * 4;
  float* wl = up_sm;                         // [head][NCMAX][ky0 8][kx0 8][a 2][b 2]
  float* sin = up_sm + HEADS * NCMAX * 256;  // [head][NCMAX][pair UP_JP][a 2][b 2]
  float* mk = sin + nstage;                  // [T][NCMAX] dropout factors of this sample: 0 or keep_scale; 1 past C
  float* rl = mk + UNC_TMAX * NCMAX;         // [T]
  const float *s1 = s, *s2 = s, *w1 = w_up, *w2 = w_std;
  const int Wo = 8 * Wi, Ho = 8 * Hi;
  const int nseg = (Wo + UP_COLS - 1) / UP_COLS;
  const int per = (Hi + 1) * nseg;  // items of one sample
  const int ns = blockIdx.y;
  const int ky0 = threadIdx.x >> 6, lane = threadIdx.x & 63;
  MCD_UP8_STAGE_TAPS
  for (int i = threadIdx.x; i < T * NCMAX; i += UP_NT) {
    const int t = i / NCMAX, c = i - t * NCMAX;
    mk[i] = c < C ? (keep[((size_t)t * N + ns) * C + c] != 0 ? keep_scale : 0.f) : 1.f;
  }
  for (int i = threadIdx.x; i < T; i += UP_NT) rl[i] = rnd[i];
  float sreg[SREG];
  auto fetch = [&](int item) {
    MCD_UP8_FETCH(item)
  };
  // upstream gradients and the normaliser: device scalars (nothing synchronises with the host)
  float ka0 = 0.f, kb = 0.f;
  if (BWD) {
    ka0 = gb[0] / ((float)T * wsum[0]);
    kb = gu[ns] * lam_hw;
  }
  float bsum = 0.f, usum = 0.f;
  int it = blockIdx.x;
  if (it < per) fetch(ns * per + it);
  for (; it < per; it += gridDim.x) {
    __syncthreads();  // the previous item's readers are done (and, first time round, the kernels and factors are staged)
    MCD_UP8_COMMIT
    __syncthreads();
    if (it + (int)gridDim.x < per) fetch(ns * per + it + (int)gridDim.x);
    const int seg = it % nseg, iyg = it / nseg;
    const int oy = 8 * iyg - 4 + ky0;
    const int ox = seg * UP_COLS + lane;
    if (oy >= 0 && oy < Ho && ox < Wo) {
      int Cv = C;
      asm volatile("" : "+s"(Cv));
      const int kx0 = (ox + 4) & 7;
      const int jp = ((ox + 4) >> 3) - seg * (UP_COLS / 8);
      int woff = (ky0 * 8 + kx0) * 4, soff = jp * 4;
      asm volatile("" : "+v"(woff), "+v"(soff));
      float u[NCMAX], v[NCMAX];
      MCD_UP8_LOGITS(u, v)
#pragma unroll
      for (int c = 0; c < NCMAX; ++c) v[c] = fmaxf(v[c], 0.f);  // relu(V); V > 0 <=> relu(V) > 0
      const size_t HW = (size_t)Ho * Wo;
      const size_t hw = (size_t)oy * Wo + ox;
      const size_t base = (size_t)ns * C * HW + hw;
      int y = -1;
      float wy = 0.f;
      const int64_t yl = labels[(size_t)ns * HW + hw];
      if (yl != ignore_index && yl >= 0 && yl < C) {
        y = (int)yl;
        wy = cw ? cw[y] : 1.f;
      }
      if (y >= 0) {
        float S = 0.f, ce = 0.f;
        for (int t = 0; t < T; ++t) {
          float m1, m2, e1, e2, y1g, y2g;
          draw_stats<NCMAX>(u, v, mk + t * NCMAX, rl[t], y, m1, m2, e1, e2, y1g, y2g);
          ce += wy * ((m1 + logf(e1)) - y1g);
          S += exp_nonpos(y2g - m2) / e2;
        }
        bsum += ce;
        usum += logf(S / (float)T);
        if (BWD) {
          // GU / GV of GCH classes at a time: with all of them the 41- and 48-class kernels hold 4 NCMAX live floats and spill
          // inside the draw loop; a second walk over the draws (their statistics recomputed) costs arithmetic only
          constexpr int GCH = NCMAX <= 24 ? NCMAX : (NCMAX + 1) / 2;
          const float ka = ka0 * wy;
#pragma unroll
          for (int h0 = 0; h0 < NCMAX; h0 += GCH) {
            float gU[GCH], gV[GCH];
#pragma unroll
            for (int k = 0; k < GCH; ++k) {
              gU[k] = 0.f;
              gV[k] = 0.f;
            }
            for (int t = 0; t < T; ++t) {
              const float* mt = mk + t * NCMAX;
              const float rt = rl[t];
              float m1, m2, e1, e2, y1g, y2g;
              draw_stats<NCMAX>(u, v, mt, rt, y, m1, m2, e1, e2, y1g, y2g);
              const float r1 = 1.f / e1, r2 = 1.f / e2;
              const float kbt = kb * ((exp_nonpos(y2g - m2) / e2) / S);  // p_t as loop 1 formed it
#pragma unroll
              for (int k0 = 0; k0 < GCH; k0 += 4) {
                MCD_OPAQUE_TRUE(go);
                if (go) {
#pragma unroll
                  for (int k = k0; k < k0 + 4; ++k) {
                    const int c = h0 + k;
                    if (k >= GCH || c >= NCMAX) continue;
                    const float m = mt[c];
                    const float y1 = m * u[c];
                    const float y2 = y1 + (m * v[c]) * rt;
                    const float oh = (c == y) ? 1.f : 0.f;
                    const float at = ka * (exp_nonpos(y1 - m1) * r1 - oh);
                    const float bt = kbt * (oh - exp_nonpos(y2 - m2) * r2);
                    gU[k] += m * (at + bt);
                    gV[k] += (v[c] > 0.f) ? m * (rt * bt) : 0.f;
                  }
                }
              }
            }
#pragma unroll
            for (int k = 0; k < GCH; ++k) {
              const int c = h0 + k;
              if (c < NCMAX && c < Cv) {
                GU[base + (size_t)c * HW] = gU[k];
                GV[base + (size_t)c * HW] = gV[k];
              }
            }
          }
        }
      } else if (BWD) {
#pragma unroll
        for (int c = 0; c < NCMAX; ++c) {
          if (c < Cv) {
            GU[base + (size_t)c * HW] = 0.f;
            GV[base + (size_t)c * HW] = 0.f;
          }
        }
      }
    }
  }
  if (BWD) return;  // (uniform: the backward launch has no partial sums)
  __shared__ float sh[2][UP_NT / 64];
  float sums[2] = {bsum, usum};
  block_gather(sums, sh);
  if (threadIdx.x < 2) {
    const int q = threadIdx.x;
    part[((size_t)ns * gridDim.x + blockIdx.x) * 2 + q] = chain_total<UP_NT / 64>(sh[q]);
  }
}

// block n < N: U_n; block N: B.  part: [N][gx][2] (cross-entropy sum, sum of log(S / T)); losses[1] = W is in place.
__global__ __launch_bounds__(256) void uncertain_finalize_kernel(const float* __restrict__ part, int gx, int N, int T, double lam_hw,
                                                                 float* __restrict__ losses) {
  const int b = blockIdx.x;
  const int q = b < N ? 1 : 0;
  const int64_t first = b < N ? (int64_t)b * gx : 0, count = b < N ? gx : (int64_t)N * gx;
  double tot[1];
  partials_total(part + first * 2, count, 2, q, tot);
  if (threadIdx.x == 0) {
    const double v = tot[0];
    if (b < N)
      losses[2 + b] = (float)(v * lam_hw);
    else
      losses[0] = (float)(v / ((double)T * (double)losses[1]));  // 0/0 = NaN with no labelled pixel, as the reference's weighted mean
  }
}

// out[n,oy,ox] = sum_{c < C_used} relu(up8(s, w_std))[n,c,oy,ox]: the tester's map without the C-channel tensor.  The kernels of the
// summed classes in LDS (at most 48 KB); one lane per pixel, the four multiply-adds per class in the order of up8_fwd_kernel.
__global__ __launch_bounds__(256) void up8_std_sum_kernel(const float* __restrict__ s, const float* __restrict__ w, float* __restrict__ out,
                                                          int C, int C_used, int Hi, int Wi) {
  extern __shared__ __attribute__((aligned(16))) float std_w[];
  for (int i = threadIdx.x; i < C_used * 256; i += 256) std_w[i] = w[i];
  __syncthreads();
  const int n = blockIdx.y;
  const int Wo = 8 * Wi, Ho = 8 * Hi;
  const int64_t total = (int64_t)Ho * Wo;
  for (int64_t p = blockIdx.x * 256ll + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
    const int oy = (int)(p / Wo), ox = (int)(p - (int64_t)oy * Wo);
    const int iy_hi = (oy + 4) >> 3, ky0 = (oy + 4) & 7;
    const int ix_hi = (ox + 4) >> 3, kx0 = (ox + 4) & 7;
    float acc = 0.f;
    for (int c = 0; c < C_used; ++c) {
      const float* xin = s + ((size_t)n * C + c) * Hi * Wi;
      float o = 0.f;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int iy = iy_hi - a;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int ix = ix_hi - b;
          if (iy < 0 || iy >= Hi || ix < 0 || ix >= Wi) continue;
          o = fmaf(xin[iy * Wi + ix], std_w[c * 256 + (ky0 + 8 * a) * 16 + kx0 + 8 * b], o);
        }
      }
      acc += fmaxf(o, 0.f);
    }
    out[(size_t)n * total + p] = acc;
  }
}

int unc_ncmax(int C) { return C <= 16 ? 16 : (C <= 24 ? 24 : (C == 41 ? 41 : 48)); }

size_t unc_lds_bytes(int ncmax) { return (size_t)(2 * ncmax * (256 + 4 * UP_JP) + UNC_TMAX * ncmax + UNC_TMAX) * sizeof(float); }

// persistent workgroups, one per CU over the whole grid (the kernels of all classes fill most of a CU's LDS), each within one sample
int unc_blocks_x(int32_t N, int32_t Hi, int32_t Wi) {
  const int64_t per = (int64_t)(Hi + 1) * ceil_div(8 * Wi, UP_COLS);
  const int64_t share = N >= 256 ? 1 : 256 / N;
  return (int)(per < share ? per : share);
}

template <int NCMAX, bool BWD>
int launch_uncertain(const char* entry, int gx, hipStream_t st, const float* s, const float* w_up, const float* w_std, const int64_t* labels,
                     const float* cw, int64_t ignore_index, const uint8_t* keep, const float* r, float keep_scale, const float* wsum,
                     float lam_hw, const float* gb, const float* gu, float* GU, float* GV, float* part, int N, int C, int Hi, int Wi, int T) {
  const size_t lds = unc_lds_bytes(NCMAX);
  auto kern = up8_uncertain_kernel<NCMAX, BWD>;
  static bool reserved = false;  // per instantiation: the attribute belongs to the kernel, one call serves every later launch
  if (lds > 64 * 1024 && !reserved) {
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      mcdseg_set_error("%s: cannot reserve %zu bytes of LDS: %s", entry, lds, hipGetErrorString(e));
      return -5;
    }
    reserved = true;
  }
  hipLaunchKernelGGL(kern, dim3(gx, N), dim3(UP_NT), lds, st, s, w_up, w_std, labels, cw, ignore_index, keep, r, keep_scale, wsum, lam_hw, gb,
                     gu, GU, GV, part, N, C, Hi, Wi, T);
  return 0;
}

template <bool BWD>
int launch_uncertain_any(const char* entry, int gx, hipStream_t st, const float* s, const float* w_up, const float* w_std,
                         const int64_t* labels, const float* cw, int64_t ignore_index, const uint8_t* keep, const float* r, float keep_scale,
                         const float* wsum, float lam_hw, const float* gb, const float* gu, float* GU, float* GV, float* part, int N, int C,
                         int Hi, int Wi, int T) {
#define MCD_UNC(NC)                                                                                                                       \
  launch_uncertain<NC, BWD>(entry, gx, st, s, w_up, w_std, labels, cw, ignore_index, keep, r, keep_scale, wsum, lam_hw, gb, gu, GU, GV, part, \
                            N, C, Hi, Wi, T)
  switch (unc_ncmax(C)) {
    case 16: return MCD_UNC(16);
    case 24: return MCD_UNC(24);
    case 41: return MCD_UNC(41);
    default: return MCD_UNC(48);
  }
#undef MCD_UNC
}

// the checks both entries share; 0 or the argument error
int uncertain_check(const char* entry, const void* s, const void* w_up, const void* w_std, const void* labels, const void* keep, const void* r,
                    float keep_scale, int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t T) {
  MCD_REQUIRE(N > 0 && C > 0 && Hi > 0 && Wi > 0, "%s: bad dims", entry);
  MCD_REQUIRE(C <= 48, "%s: at most 48 classes are kept in registers (got %d)", entry, C);
  MCD_REQUIRE(N <= 65535, "%s: at most 65535 samples (one grid row each; got %d)", entry, N);
  MCD_REQUIRE(T >= 1 && T <= UNC_TMAX, "%s: between 1 and %d dropout draws (got %d)", entry, UNC_TMAX, T);
  MCD_REQUIRE(s && w_up && w_std && labels, "%s: null pointer", entry);
  MCD_REQUIRE(keep && r, "%s: the dropout draws (keep, r) are NULL", entry);
  MCD_REQUIRE(keep_scale > 0.f, "%s: keep_scale must be positive (1 / (1 - p))", entry);
  MCD_REQUIRE((int64_t)N * (Hi + 1) * ceil_div(8 * Wi, UP_COLS) < (1ll << 31), "%s: too many patches", entry);
  MCD_REQUIRE((int64_t)Hi * Wi * 64 < (1ll << 31) && (int64_t)T * N * C < (1ll << 31), "%s: too many pixels per sample", entry);
  return 0;
}

}  // namespace

extern "C" size_t mcdseg_up8_uncertain_loss_workspace_bytes(int32_t N, int32_t Hi, int32_t Wi) {
  if (N <= 0 || Hi <= 0 || Wi <= 0) return 0;
  return (size_t)unc_blocks_x(N, Hi, Wi) * N * 2 * sizeof(float) + mcdseg_label_weight_sum_workspace_bytes((int64_t)N * Hi * Wi * 64);
}

extern "C" int mcdseg_up8_uncertain_loss_fwd(const float* s, const float* w_up, const float* w_std, const int64_t* labels,
                                             const float* class_weight, int64_t ignore_index, const uint8_t* keep, const float* r,
                                             float keep_scale, const float* wsum_in, float lambda, float* losses, int32_t N, int32_t C,
                                             int32_t Hi, int32_t Wi, int32_t T, void* workspace, size_t workspace_bytes, void* stream) {
  const char* entry = "up8_uncertain_loss_fwd";
  const int bad = uncertain_check(entry, s, w_up, w_std, labels, keep, r, keep_scale, N, C, Hi, Wi, T);
  if (bad != 0) return bad;
  MCD_REQUIRE(losses && workspace, "%s: null pointer", entry);
  MCD_REQUIRE(workspace_bytes >= mcdseg_up8_uncertain_loss_workspace_bytes(N, Hi, Wi), "%s: workspace too small", entry);
  hipStream_t st = (hipStream_t)stream;
  const int gx = unc_blocks_x(N, Hi, Wi);
  const int64_t P = (int64_t)N * Hi * Wi * 64;
  float* part = (float*)workspace;
  float* wpart = part + (size_t)gx * N * 2;
  if (wsum_in != nullptr) {
    (void)hipMemcpyAsync(losses + 1, wsum_in, sizeof(float), hipMemcpyDeviceToDevice, st);
  } else {
    const int rc = mcdseg_label_weight_sum(labels, class_weight, ignore_index, C, P, losses + 1, wpart,
                                           mcdseg_label_weight_sum_workspace_bytes(P), stream);
    if (rc != 0) return rc;
  }
  const double lam_hw = (double)lambda / ((double)Hi * Wi * 64.0);
  const int rc = launch_uncertain_any<false>(entry, gx, st, s, w_up, w_std, labels, class_weight, ignore_index, keep, r, keep_scale, losses + 1,
                                             (float)lam_hw, nullptr, nullptr, nullptr, nullptr, part, N, C, Hi, Wi, T);
  if (rc != 0) return rc;
  MCD_LAUNCH_CHECK(entry);
  hipLaunchKernelGGL(uncertain_finalize_kernel, dim3(N + 1), dim3(256), 0, st, (const float*)part, gx, N, T, lam_hw, losses);
  MCD_LAUNCH_CHECK("uncertain_finalize");
  return 0;
}

extern "C" int mcdseg_up8_uncertain_loss_bwd(const float* s, const float* w_up, const float* w_std, const int64_t* labels,
                                             const float* class_weight, int64_t ignore_index, const uint8_t* keep, const float* r,
                                             float keep_scale, const float* wsum, float lambda, const float* gb, const float* gu, float* GU,
                                             float* GV, int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t T, void* stream) {
  const char* entry = "up8_uncertain_loss_bwd";
  const int bad = uncertain_check(entry, s, w_up, w_std, labels, keep, r, keep_scale, N, C, Hi, Wi, T);
  if (bad != 0) return bad;
  MCD_REQUIRE(wsum && gb && gu && GU && GV, "%s: null pointer", entry);
  const double lam_hw = (double)lambda / ((double)Hi * Wi * 64.0);
  const int rc = launch_uncertain_any<true>(entry, unc_blocks_x(N, Hi, Wi), (hipStream_t)stream, s, w_up, w_std, labels, class_weight,
                                            ignore_index, keep, r, keep_scale, wsum, (float)lam_hw, gb, gu, GU, GV, nullptr, N, C, Hi, Wi, T);
  if (rc != 0) return rc;
  MCD_LAUNCH_CHECK(entry);
  return 0;
}

extern "C" int mcdseg_up8_std_sum(const float* s, const float* w_std, float* out, int32_t N, int32_t C, int32_t C_used, int32_t Hi,
                                  int32_t Wi, void* stream) {
  MCD_REQUIRE(s && w_std && out, "up8_std_sum: null pointer");
  MCD_REQUIRE(N > 0 && C > 0 && Hi > 0 && Wi > 0, "up8_std_sum: bad dims");
  MCD_REQUIRE(C <= 48 && C_used > 0 && C_used <= C, "up8_std_sum: 1 <= C_used <= C <= 48 (got %d of %d)", C_used, C);
  MCD_REQUIRE(N <= 65535 && (int64_t)Hi * Wi * 64 < (1ll << 31), "up8_std_sum: too many pixels per sample");
  const int64_t total = (int64_t)Hi * Wi * 64;
  const int64_t want = ceil_div64(total, 256);
  const int gx = (int)(want < 64 ? want : 64);
  hipLaunchKernelGGL(up8_std_sum_kernel, dim3(gx, N), dim3(256), (size_t)C_used * 256 * sizeof(float), (hipStream_t)stream, s, w_std, out, C,
                     C_used, Hi, Wi);
  MCD_LAUNCH_CHECK("up8_std_sum");
  return 0;
}
