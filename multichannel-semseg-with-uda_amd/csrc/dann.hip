// The domain classifier of the DANN baseline (DRNSegDomainClassifier, models/dilated_fcn.py:494-551 of the reference), fused:
//   dann_down_*   one whole DownConv (conv3x3+bias, ReLU, conv3x3+bias, ReLU, MaxPool2d(2,2)) per launch;
//   dann_tail_*   flatten -> Linear(F,10) -> BatchNorm1d(10) -> ReLU -> Linear(10,2) -> two-class cross-entropy, every group
//                 (domain) of the batch in one launch.
// fp32 on the vector ALU throughout: 1 to 41 input channels and 10 or 1 output channels leave the matrix pipe nothing to do; what
// the head costs when it is composed from operators is their number (some 30 launches of microsecond kernels per call), so the
// full-resolution intermediates live in LDS only and the weight gradients are summed in a fixed order (no atomics).
#include "common.h"

namespace {

constexpr int DN_NT = 256;  // threads of a DownConv workgroup
constexpr int DN_T = 16;    // edge of the full-resolution tile a workgroup owns (8 x 8 pooled outputs); even, so no pooling window
                            // straddles two tiles
// Region edges around the tile, and the LDS stride of one channel of each (edge^2 + 1: odd, so the channels do not share a bank).
//   forward:  x with a 2-pixel halo (20), conv1 with a 1-pixel halo (18), conv2 on the tile (16)
//   backward: the gradient of the tile's x needs dz1 on 18, that needs dz2 on 20 -- whole pooling windows, rows -2..17 --, that
//             needs conv1 on 22 and x on 24; everything is recomputed from x, so no workgroup reads what another one wrote.
constexpr int FX = DN_T + 4, FA = DN_T + 2;
constexpr int FXS = FX * FX + 1, FAS = FA * FA + 1, FOS = DN_T * DN_T + 1;
constexpr int BX = DN_T + 8, BA = DN_T + 6, BG2 = DN_T + 4, BG1 = DN_T + 2;
constexpr int BXS = BX * BX + 1, BAS = BA * BA + 1, BG2S = BG2 * BG2 + 1, BG1S = BG1 * BG1 + 1;
// LDS budget (one workgroup may hold all 160 KiB = 163840 bytes of a CU):
//   forward   4 (max(401 Cin, 257 Cmid) + 325 Cmid) bytes:  Cin = 41, Cmid = 10:  78 764;  Cin = 10, Cmid = 1: 17 340
//   backward  4 (577 Cin + (485 + 401 + 325) Cmid) bytes:   Cin = 41, Cmid = 10: 143 068;  Cin = 10, Cmid = 1: 27 924
// The backward tile is the larger one, and a DownConv that can run forward but not backward trains nothing, so both entry points
// hold a shape to the backward's budget: Cin <= 50 at Cmid = 10, Cin <= 69 at Cmid = 1.
constexpr size_t DN_LDS_MAX = 160 * 1024;

size_t down_fwd_lds(int Cin, int CM) {
  const int xr = Cin * FXS > CM * FOS ? Cin * FXS : CM * FOS;  // (the conv2 tile reuses the x region before pooling)
  return (size_t)(xr + CM * FAS) * sizeof(float);
}
size_t down_bwd_lds(int Cin, int CM) { return (size_t)(Cin * BXS + CM * (BAS + BG2S + BG1S)) * sizeof(float); }
int down_items(int Cin, int CM) { return CM * Cin * 9 + CM + CM * CM * 9 + CM; }  // dw1 | db1 | dw2 | db2

// zero-padded copy of an E x E window of every channel of sample n, origin (y0, x0), into LDS
template <int E, int S>
__device__ __forceinline__ void stage_x(float* sx, const float* __restrict__ x, int n, int Cin, int H, int W, int y0, int x0) {
  for (int i = threadIdx.x; i < Cin * E * E; i += DN_NT) {
    const int ci = i / (E * E), p = i - ci * (E * E);
    const int gy = y0 + p / E, gx = x0 + p % E;
    float v = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = x[(((size_t)n * Cin + ci) * H + gy) * W + gx];
    sx[ci * S + p] = v;
  }
}

// relu(conv3x3(src) + bias) on an EO x EO region whose origin lies one pixel inside the ES x ES source region; positions outside
// the map are 0 (the next convolution's zero padding), whatever the convolution of the padded source would give there.
// One thread per position holds the CO sums; the weights are wave-uniform.  Sum order: bias, then channels, then taps row-major
// (the forward and the backward kernel must agree on every bit: the backward finds the pooling argmax on its own copy).
template <int CO, int ES, int SS, int EO, int SO>
__device__ __forceinline__ void conv_relu_region(float* dst, const float* src, const float* __restrict__ w, const float* __restrict__ b,
                                                 int Cs, int H, int W, int y0, int x0) {
  for (int p = threadIdx.x; p < EO * EO; p += DN_NT) {
    const int py = p / EO, px = p - py * EO;
    float acc[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) acc[co] = b[co];
    for (int c = 0; c < Cs; ++c) {
      float v[9];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 0; d < 3; ++d) v[a * 3 + d] = src[c * SS + (py + a) * ES + px + d];
#pragma unroll
      for (int co = 0; co < CO; ++co)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[co] = fmaf(v[t], w[(co * Cs + c) * 9 + t], acc[co]);
    }
    const int gy = y0 + py, gx = x0 + px;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
#pragma unroll
    for (int co = 0; co < CO; ++co) dst[co * SO + p] = in ? fmaxf(acc[co], 0.f) : 0.f;
  }
}

template <int CM>
__global__ __launch_bounds__(DN_NT) void dann_down_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w1,
                                                              const float* __restrict__ b1, const float* __restrict__ w2,
                                                              const float* __restrict__ b2, float* __restrict__ y, int Cin, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) float dn_sm[];
  const int xr = Cin * FXS > CM * FOS ? Cin * FXS : CM * FOS;
  float* sx = dn_sm;
  float* sa = dn_sm + xr;
  const int n = blockIdx.z, oy = blockIdx.y * DN_T, ox = blockIdx.x * DN_T;
  const int Hp = H / 2, Wp = W / 2;
  stage_x<FX, FXS>(sx, x, n, Cin, H, W, oy - 2, ox - 2);
  __syncthreads();
  conv_relu_region<CM, FX, FXS, FA, FAS>(sa, sx, w1, b1, Cin, H, W, oy - 1, ox - 1);
  __syncthreads();
  conv_relu_region<CM, FA, FAS, DN_T, FOS>(sx, sa, w2, b2, CM, H, W, oy, ox);  // (sx is free: conv1 has read it)
  __syncthreads();
  for (int i = threadIdx.x; i < CM * (DN_T / 2) * (DN_T / 2); i += DN_NT) {
    const int co = i / 64, q = i - co * 64, qy = q / 8, qx = q - qy * 8;
    const int Py = blockIdx.y * (DN_T / 2) + qy, Px = blockIdx.x * (DN_T / 2) + qx;
    if (Py < Hp && Px < Wp) {
      const float* o = sx + co * FOS + 2 * qy * DN_T + 2 * qx;
      y[(((size_t)n * CM + co) * Hp + Py) * Wp + Px] = fmaxf(fmaxf(o[0], o[1]), fmaxf(o[DN_T], o[DN_T + 1]));
    }
  }
}

template <int CM>
__global__ __launch_bounds__(DN_NT) void dann_down_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w1,
                                                              const float* __restrict__ b1, const float* __restrict__ w2,
                                                              const float* __restrict__ b2, const float* __restrict__ dy,
                                                              float* __restrict__ dx, float* __restrict__ part, int Cin, int H, int W) {
  extern __shared__ __attribute__((aligned(16))) float dn_sm[];
  float* sx = dn_sm;             // x        origin (oy-4, ox-4), 24 x 24
  float* sa = sx + Cin * BXS;    // a1       origin (oy-3, ox-3), 22 x 22
  float* sg2 = sa + CM * BAS;    // a2, then dz2   origin (oy-2, ox-2), 20 x 20
  float* sg1 = sg2 + CM * BG2S;  // dz1      origin (oy-1, ox-1), 18 x 18
  const int n = blockIdx.z, oy = blockIdx.y * DN_T, ox = blockIdx.x * DN_T;
  const int Hp = H / 2, Wp = W / 2;
  stage_x<BX, BXS>(sx, x, n, Cin, H, W, oy - 4, ox - 4);
  __syncthreads();
  conv_relu_region<CM, BX, BXS, BA, BAS>(sa, sx, w1, b1, Cin, H, W, oy - 3, ox - 3);
  __syncthreads();
  conv_relu_region<CM, BA, BAS, BG2, BG2S>(sg2, sa, w2, b2, CM, H, W, oy - 2, ox - 2);
  __syncthreads();
  // max-pooling backward on whole windows: the gradient goes to the first maximum in row-major order (torch's max_pool2d keeps an
  // index only for a strictly larger value), and through the ReLU only where that maximum is positive
  for (int i = threadIdx.x; i < CM * (BG2 / 2) * (BG2 / 2); i += DN_NT) {
    constexpr int WE = BG2 / 2;
    const int co = i / (WE * WE), q = i - co * (WE * WE), wy = q / WE, wx = q - wy * WE;
    const int Py = blockIdx.y * (DN_T / 2) - 1 + wy, Px = blockIdx.x * (DN_T / 2) - 1 + wx;
    float* o = sg2 + co * BG2S + 2 * wy * BG2 + 2 * wx;
    const int off[4] = {0, 1, BG2, BG2 + 1};
    float best = o[0];
    int at = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const float v = o[off[k]];
      if (v > best) best = v, at = k;
    }
    float g = 0.f;
    if (Py >= 0 && Py < Hp && Px >= 0 && Px < Wp && best > 0.f) g = dy[(((size_t)n * CM + co) * Hp + Py) * Wp + Px];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[off[k]] = (k == at) ? g : 0.f;
  }
  __syncthreads();
  // dz1 = [a1 > 0] * (dz2 correlated with w2 transposed); a1 is 0 outside the map, so dz1 is
  for (int p = threadIdx.x; p < BG1 * BG1; p += DN_NT) {
    const int py = p / BG1, px = p - py * BG1;
    float acc[CM];
#pragma unroll
    for (int cm = 0; cm < CM; ++cm) acc[cm] = 0.f;
    for (int co = 0; co < CM; ++co) {
      float v[9];  // v[t] = dz2 at (position - (tap - 1)): region coordinates (py + 2 - a, px + 2 - d)
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 0; d < 3; ++d) v[a * 3 + d] = sg2[co * BG2S + (py + 2 - a) * BG2 + px + 2 - d];
#pragma unroll
      for (int cm = 0; cm < CM; ++cm)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[cm] = fmaf(v[t], w2[(co * CM + cm) * 9 + t], acc[cm]);
    }
#pragma unroll
    for (int cm = 0; cm < CM; ++cm) sg1[cm * BG1S + p] = sa[cm * BAS + (py + 2) * BA + px + 2] > 0.f ? acc[cm] : 0.f;
  }
  __syncthreads();
  // dx on the tile: the 3 x 3 x CM neighbourhood of dz1 in registers, the weights wave-uniform
  if (dx != nullptr) {
    const int py = threadIdx.x / DN_T, px = threadIdx.x % DN_T;
    const int gy = oy + py, gx = ox + px;
    float v[CM * 9];
#pragma unroll
    for (int cm = 0; cm < CM; ++cm)
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 0; d < 3; ++d) v[cm * 9 + a * 3 + d] = sg1[cm * BG1S + (py + 2 - a) * BG1 + px + 2 - d];
    if (gy < H && gx < W) {
      for (int ci = 0; ci < Cin; ++ci) {
        float acc = 0.f;
#pragma unroll
        for (int cm = 0; cm < CM; ++cm)
#pragma unroll
          for (int t = 0; t < 9; ++t) acc = fmaf(v[cm * 9 + t], w1[(cm * Cin + ci) * 9 + t], acc);
        dx[(((size_t)n * Cin + ci) * H + gy) * W + gx] = acc;
      }
    }
  }
  // this workgroup's share of the parameter gradients: sums over the 16 x 16 positions it owns, rows then columns
  float* mine = part + (size_t)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (CM * Cin * 9 + CM + CM * CM * 9 + CM);
  for (int it = threadIdx.x; it < Cin * 9; it += DN_NT) {  // dw1[:, ci, tap]
    const int ci = it / 9, t = it - ci * 9, a = t / 3, d = t - a * 3;
    float acc[CM];
#pragma unroll
    for (int cm = 0; cm < CM; ++cm) acc[cm] = 0.f;
    for (int py = 0; py < DN_T; ++py)
      for (int px = 0; px < DN_T; ++px) {
        const float xv = sx[ci * BXS + (py + 3 + a) * BX + px + 3 + d];
#pragma unroll
        for (int cm = 0; cm < CM; ++cm) acc[cm] = fmaf(sg1[cm * BG1S + (py + 1) * BG1 + px + 1], xv, acc[cm]);
      }
#pragma unroll
    for (int cm = 0; cm < CM; ++cm) mine[(cm * Cin + ci) * 9 + t] = acc[cm];
  }
  float* m_b1 = mine + CM * Cin * 9;
  float* m_w2 = m_b1 + CM;
  float* m_b2 = m_w2 + CM * CM * 9;
  for (int it = threadIdx.x; it < CM * CM * 9; it += DN_NT) {  // dw2[co, cm, tap]
    const int co = it / (CM * 9), r = it - co * (CM * 9), cm = r / 9, t = r - cm * 9, a = t / 3, d = t - a * 3;
    float acc = 0.f;
    for (int py = 0; py < DN_T; ++py)
      for (int px = 0; px < DN_T; ++px)
        acc = fmaf(sg2[co * BG2S + (py + 2) * BG2 + px + 2], sa[cm * BAS + (py + 2 + a) * BA + px + 2 + d], acc);
    m_w2[it] = acc;
  }
  for (int it = threadIdx.x; it < 2 * CM; it += DN_NT) {  // db1 | db2
    const bool second = it >= CM;
    const int c = second ? it - CM : it;
    float acc = 0.f;
    for (int py = 0; py < DN_T; ++py)
      for (int px = 0; px < DN_T; ++px)
        acc += second ? sg2[c * BG2S + (py + 2) * BG2 + px + 2] : sg1[c * BG1S + (py + 1) * BG1 + px + 1];
    (second ? m_b2 : m_b1)[c] = acc;
  }
}

// second stage: out[item] = sum over the workgroups' partials in a fixed order.  Per group of samples (a domain; its workgroups are
// contiguous): 16 interleaved running sums (workgroups r, r + 16, ... of the group), then those 16 in order; then the groups in order.
// So the gradient of a batch of G groups is, bit for bit, the sum of the gradients of G calls with one group each.
// 16 items x 16 rows per block.
__global__ __launch_bounds__(256) void dann_down_reduce_kernel(const float* __restrict__ part, int nwg_group, int groups, int items, int n_w1,
                                                               int CM, float* __restrict__ dw1, float* __restrict__ db1,
                                                               float* __restrict__ dw2, float* __restrict__ db2) {
  __shared__ float rows[16][17];
  const int lane = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int item = blockIdx.x * 16 + lane;
  float total = 0.f;
  for (int g = 0; g < groups; ++g) {
    float acc = 0.f;
    if (item < items) {
      const float* mine = part + (size_t)g * nwg_group * items + item;
#pragma unroll 8
      for (int w = r; w < nwg_group; w += 16) acc += mine[(size_t)w * items];
    }
    rows[r][lane] = acc;
    __syncthreads();
    if (r == 0) {
      float s = rows[0][lane];
#pragma unroll
      for (int k = 1; k < 16; ++k) s += rows[k][lane];
      total = g == 0 ? s : total + s;
    }
    __syncthreads();
  }
  if (r == 0 && item < items) {
    const float s = total;
    int i = item;
    if (i < n_w1) { dw1[i] = s; return; }
    i -= n_w1;
    if (i < CM) { db1[i] = s; return; }
    i -= CM;
    if (i < CM * CM * 9) { dw2[i] = s; return; }
    db2[i - CM * CM * 9] = s;
  }
}

// ------------------------------------------------------------------------------------------------ the tail
constexpr int TL_NT = 1024;  // one workgroup: the batch couples the rows, and the whole problem is a few kilobytes
constexpr int TL_HID = 10;   // Linear(F, 10), BatchNorm1d(10), Linear(10, 2)
constexpr int TL_GMAX = 64;  // groups (domains) per launch

// the saved buffer of the forward pass: z [R][10] fp32 (fc1's output) | mean [G][10] | rstd [G][10], both fp64   (R = G n rows).
// The BatchNorm1d arithmetic -- statistics, xhat, and the backward's combination -- is carried in fp64: with a handful of rows per
// group the backward is a difference of nearly equal terms (at n = 2 it is (1 - xhat^2) times the upstream gradient, and xhat^2 is
// 1 - eps / (var + eps)), so every ulp of an fp32 xhat would come back some 10^4 times larger.  A few hundred values: no cost.
__device__ __forceinline__ const double* tail_mean(const float* save, int R) { return (const double*)(save + (size_t)R * TL_HID); }
__device__ __forceinline__ double tail_xhat(const float* save, int R, int G, int r, int g, int j) {
  const double* mean = tail_mean(save, R);
  const double* rstd = mean + G * TL_HID;
  return ((double)save[(size_t)r * TL_HID + j] - mean[g * TL_HID + j]) * rstd[g * TL_HID + j];
}
__device__ __forceinline__ float tail_act(double xhat, float gamma, float beta) { return fmaxf((float)(xhat * (double)gamma + (double)beta), 0.f); }

__global__ __launch_bounds__(TL_NT) void dann_tail_fwd_kernel(const float* __restrict__ h, const int32_t* __restrict__ labels,
                                                              const float* __restrict__ w1, const float* __restrict__ b1,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              float* running_mean, float* running_var, const float* __restrict__ w2,
                                                              const float* __restrict__ b2, float momentum, float eps, int training,
                                                              float* loss, float* logits, float* save, int G, int n, int F) {
  __shared__ double var_unbiased[TL_GMAX * TL_HID];
  const int R = G * n, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  double* mean = (double*)(save + (size_t)R * TL_HID);
  double* rstd = mean + G * TL_HID;
  // fc1: one wave per row, the ten dot products side by side; lanes stride the features, then the wave's butterfly sum
  for (int r = wave; r < R; r += TL_NT / 64) {
    float acc[TL_HID];
#pragma unroll
    for (int j = 0; j < TL_HID; ++j) acc[j] = 0.f;
    for (int f = lane; f < F; f += 64) {
      const float hv = h[(size_t)r * F + f];
#pragma unroll
      for (int j = 0; j < TL_HID; ++j) acc[j] = fmaf(hv, w1[(size_t)j * F + f], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < TL_HID; ++j) acc[j] = wave_sum(acc[j]);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < TL_HID; ++j) save[(size_t)r * TL_HID + j] = acc[j] + b1[j];
    }
  }
  __syncthreads();
  // BatchNorm1d statistics, per group: the batch's (biased variance normalises) or the running ones
  for (int i = tid; i < G * TL_HID; i += TL_NT) {
    const int g = i / TL_HID, j = i - g * TL_HID;
    double m, v;
    if (training) {
      double s = 0.0;
      for (int r = g * n; r < (g + 1) * n; ++r) s += (double)save[(size_t)r * TL_HID + j];
      m = s / (double)n;
      double q = 0.0;
      for (int r = g * n; r < (g + 1) * n; ++r) {
        const double d = (double)save[(size_t)r * TL_HID + j] - m;
        q += d * d;
      }
      v = q / (double)n;
      var_unbiased[i] = q / (double)(n - 1);
    } else {
      m = (double)running_mean[j];
      v = (double)running_var[j];
    }
    mean[i] = m;
    rstd[i] = 1.0 / sqrt(v + (double)eps);
  }
  __syncthreads();
  if (training && tid < TL_HID) {  // the running update, group after group, as one module call per domain would apply it
    float m = running_mean[tid], v = running_var[tid];
    for (int g = 0; g < G; ++g) {  // (each call's result is an fp32 buffer, as torch's is)
      m = (float)((1.0 - (double)momentum) * (double)m + (double)momentum * mean[g * TL_HID + tid]);
      v = (float)((1.0 - (double)momentum) * (double)v + (double)momentum * var_unbiased[g * TL_HID + tid]);
    }
    running_mean[tid] = m;
    running_var[tid] = v;
  }
  for (int r = tid; r < R; r += TL_NT) {
    const int g = r / n;
    float l0 = b2[0], l1 = b2[1];
#pragma unroll
    for (int j = 0; j < TL_HID; ++j) {
      const float a = tail_act(tail_xhat(save, R, G, r, g, j), gamma[j], beta[j]);
      l0 = fmaf(a, w2[j], l0);
      l1 = fmaf(a, w2[TL_HID + j], l1);
    }
    logits[2 * r] = l0;
    logits[2 * r + 1] = l1;
  }
  __syncthreads();
  for (int g = tid; g < G; g += TL_NT) {  // mean cross-entropy of the group against its one label
    const bool one = labels[g] != 0;
    float s = 0.f;
    for (int r = g * n; r < (g + 1) * n; ++r) {
      const float l0 = logits[2 * r], l1 = logits[2 * r + 1], m = fmaxf(l0, l1);
      s += m + logf(expf(l0 - m) + expf(l1 - m)) - (one ? l1 : l0);
    }
    loss[g] = s / (float)n;
  }
}

// ws: dz [R][10] (first the gradient behind the ReLU, then fc1's output gradient, in place) | dl [R][2] (the logits' gradient)
__global__ __launch_bounds__(TL_NT) void dann_tail_bwd_kernel(const float* __restrict__ h, const int32_t* __restrict__ labels,
                                                              const float* __restrict__ w1, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float* __restrict__ w2,
                                                              const float* __restrict__ logits, const float* __restrict__ save,
                                                              const float* __restrict__ up, float* __restrict__ dh, float* __restrict__ dw1,
                                                              float* __restrict__ db1, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              float* __restrict__ dw2, float* __restrict__ db2, float* ws, int training, int G,
                                                              int n, int F) {
  __shared__ double s1[TL_GMAX * TL_HID], s2[TL_GMAX * TL_HID];  // per group and feature: sum of dz, sum of dz * xhat
  const int R = G * n, tid = threadIdx.x;
  const double* rstd = tail_mean(save, R) + G * TL_HID;
  float* dz = ws;
  float* dl = ws + (size_t)R * TL_HID;
  for (int r = tid; r < R; r += TL_NT) {
    const int g = r / n;
    const bool one = labels[g] != 0;
    const float l0 = logits[2 * r], l1 = logits[2 * r + 1], m = fmaxf(l0, l1);
    const float e0 = expf(l0 - m), e1 = expf(l1 - m), inv = 1.f / (e0 + e1);
    const float c = up[g] / (float)n;
    const float d0 = c * (e0 * inv - (one ? 0.f : 1.f)), d1 = c * (e1 * inv - (one ? 1.f : 0.f));
    dl[2 * r] = d0;
    dl[2 * r + 1] = d1;
#pragma unroll
    for (int j = 0; j < TL_HID; ++j) {
      const float a = tail_act(tail_xhat(save, R, G, r, g, j), gamma[j], beta[j]);
      dz[(size_t)r * TL_HID + j] = a > 0.f ? fmaf(d1, w2[TL_HID + j], d0 * w2[j]) : 0.f;
    }
  }
  __syncthreads();
  if (tid < 2 * TL_HID) {  // dw2[k][j], rows in order
    const int k = tid / TL_HID, j = tid - k * TL_HID;
    float total = 0.f;
    for (int g = 0; g < G; ++g) {  // (per group, then the groups in order: what G calls with one group each would accumulate)
      float acc = 0.f;
      for (int r = g * n; r < (g + 1) * n; ++r) acc = fmaf(dl[2 * r + k], tail_act(tail_xhat(save, R, G, r, g, j), gamma[j], beta[j]), acc);
      total = g == 0 ? acc : total + acc;
    }
    dw2[tid] = total;
  } else if (tid < 2 * TL_HID + 2) {
    const int k = tid - 2 * TL_HID;
    float total = 0.f;
    for (int g = 0; g < G; ++g) {
      float acc = 0.f;
      for (int r = g * n; r < (g + 1) * n; ++r) acc += dl[2 * r + k];
      total = g == 0 ? acc : total + acc;
    }
    db2[k] = total;
  } else if (tid >= 64) {
    for (int i = tid - 64; i < G * TL_HID; i += TL_NT - 64) {
      const int g = i / TL_HID, j = i - g * TL_HID;
      double a1 = 0.0, a2 = 0.0;
      for (int r = g * n; r < (g + 1) * n; ++r) {
        const double d = (double)dz[(size_t)r * TL_HID + j];
        a1 += d;
        a2 += d * tail_xhat(save, R, G, r, g, j);
      }
      s1[i] = a1;
      s2[i] = a2;
    }
  }
  __syncthreads();
  if (tid < TL_HID) {
    float a1 = 0.f, a2 = 0.f;  // (each group's sum rounded to fp32 first: the gradient one call per group would leave)
    for (int g = 0; g < G; ++g) {
      const float b1g = (float)s1[g * TL_HID + tid], b2g = (float)s2[g * TL_HID + tid];
      a1 = g == 0 ? b1g : a1 + b1g;
      a2 = g == 0 ? b2g : a2 + b2g;
    }
    dbeta[tid] = a1;
    dgamma[tid] = a2;
  }
  for (int i = tid; i < R * TL_HID; i += TL_NT) {  // BatchNorm1d backward: batch statistics couple the group's rows, running ones do not
    const int r = i / TL_HID, j = i - r * TL_HID, g = r / n, gi = g * TL_HID + j;
    double d = (double)dz[i];
    if (training) d = d - s1[gi] / (double)n - tail_xhat(save, R, G, r, g, j) * (s2[gi] / (double)n);
    dz[i] = (float)((double)gamma[j] * rstd[gi] * d);
  }
  __syncthreads();
  if (tid < TL_HID) {
    float total = 0.f;
    for (int g = 0; g < G; ++g) {
      float acc = 0.f;
      for (int r = g * n; r < (g + 1) * n; ++r) acc += dz[(size_t)r * TL_HID + tid];
      total = g == 0 ? acc : total + acc;
    }
    db1[tid] = total;
  }
  for (int f = tid; f < F; f += TL_NT) {  // dw1[:, f], rows in order
    float total[TL_HID];
    for (int g = 0; g < G; ++g) {
      float acc[TL_HID];
#pragma unroll
      for (int j = 0; j < TL_HID; ++j) acc[j] = 0.f;
      for (int r = g * n; r < (g + 1) * n; ++r) {
        const float hv = h[(size_t)r * F + f];
#pragma unroll
        for (int j = 0; j < TL_HID; ++j) acc[j] = fmaf(dz[(size_t)r * TL_HID + j], hv, acc[j]);
      }
#pragma unroll
      for (int j = 0; j < TL_HID; ++j) total[j] = g == 0 ? acc[j] : total[j] + acc[j];
    }
#pragma unroll
    for (int j = 0; j < TL_HID; ++j) dw1[(size_t)j * F + f] = total[j];
  }
  if (dh != nullptr) {
    for (int i = tid; i < R * F; i += TL_NT) {
      const int r = i / F, f = i - r * F;
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < TL_HID; ++j) acc = fmaf(dz[(size_t)r * TL_HID + j], w1[(size_t)j * F + f], acc);
      dh[i] = acc;
    }
  }
}

int down_check(const char* entry, int32_t N, int32_t Cin, int32_t Cmid, int32_t H, int32_t W) {
  MCD_REQUIRE(N > 0 && Cin > 0 && H >= 2 && W >= 2, "%s: bad dims (N %d, Cin %d, H %d, W %d; the pooling needs H, W >= 2)", entry, N, Cin, H, W);
  MCD_REQUIRE(Cmid == 1 || Cmid == 10, "%s: Cmid = Cout must be 1 or 10, the DownConv widths of the domain classifier (got %d)", entry, Cmid);
  MCD_REQUIRE(N <= 65535, "%s: at most 65535 samples (one grid plane each; got %d)", entry, N);
  MCD_REQUIRE(down_bwd_lds(Cin, Cmid) <= DN_LDS_MAX && down_fwd_lds(Cin, Cmid) <= DN_LDS_MAX,
              "%s: the tile of Cin = %d, Cmid = %d needs %zu bytes of LDS (backward), a CU has %zu", entry, Cin, Cmid,
              down_bwd_lds(Cin, Cmid), DN_LDS_MAX);
  MCD_REQUIRE((int64_t)N * Cin * H * W < (1ll << 40), "%s: tensor too large", entry);
  return 0;
}

// more than 64 KB of dynamic LDS has to be allowed per kernel AND per device (the attribute belongs to the current device's copy of
// the function), so it is asked for at every such launch: a host-side table look-up, no device work, and nothing to keep per process
template <typename K>
int reserve_lds(const char* entry, K kern, size_t lds) {
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      mcdseg_set_error("%s: cannot reserve %zu bytes of LDS: %s", entry, lds, hipGetErrorString(e));
      return -5;
    }
  }
  return 0;
}

template <int CM>
int launch_down_fwd(const char* entry, hipStream_t st, dim3 grid, const float* x, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* y, int Cin, int H, int W) {
  const size_t lds = down_fwd_lds(Cin, CM);
  const int rc = reserve_lds(entry, dann_down_fwd_kernel<CM>, lds);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(dann_down_fwd_kernel<CM>, grid, dim3(DN_NT), lds, st, x, w1, b1, w2, b2, y, Cin, H, W);
  return 0;
}

template <int CM>
int launch_down_bwd(const char* entry, hipStream_t st, dim3 grid, const float* x, const float* w1, const float* b1, const float* w2,
                    const float* b2, const float* dy, float* dx, float* part, int Cin, int H, int W) {
  const size_t lds = down_bwd_lds(Cin, CM);
  const int rc = reserve_lds(entry, dann_down_bwd_kernel<CM>, lds);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(dann_down_bwd_kernel<CM>, grid, dim3(DN_NT), lds, st, x, w1, b1, w2, b2, dy, dx, part, Cin, H, W);
  return 0;
}

dim3 down_grid(int N, int H, int W) { return dim3(ceil_div(W / 2, DN_T / 2), ceil_div(H / 2, DN_T / 2), N); }
// the backward's grid covers every position of the map (the dropped last row / column of an odd map still owns gradients)
dim3 down_grid_bwd(int N, int H, int W) { return dim3(ceil_div(W, DN_T), ceil_div(H, DN_T), N); }

int tail_check(const char* entry, int32_t G, int32_t n, int32_t F, int32_t training) {
  MCD_REQUIRE(G >= 1 && G <= TL_GMAX, "%s: between 1 and %d groups (got %d)", entry, TL_GMAX, G);
  MCD_REQUIRE(n >= 1 && F >= 1, "%s: bad dims (n %d, F %d)", entry, n, F);
  MCD_REQUIRE(!(training && n < 2), "%s: BatchNorm1d in training mode needs at least 2 rows per group (got %d), as torch does", entry, n);
  MCD_REQUIRE((int64_t)G * n * F < (1ll << 31), "%s: too many elements", entry);
  return 0;
}

}  // namespace

extern "C" size_t mcdseg_dann_down_workspace_bytes(int32_t N, int32_t Cin, int32_t Cmid, int32_t H, int32_t W) {
  if (N <= 0 || Cin <= 0 || Cmid <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * ceil_div(H, DN_T) * ceil_div(W, DN_T) * down_items(Cin, Cmid) * sizeof(float);
}

extern "C" int mcdseg_dann_down_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y, int32_t N,
                                    int32_t Cin, int32_t Cmid, int32_t H, int32_t W, void* stream) {
  const char* entry = "dann_down_fwd";
  const int bad = down_check(entry, N, Cin, Cmid, H, W);
  if (bad != 0) return bad;
  MCD_REQUIRE(x && w1 && b1 && w2 && b2 && y, "%s: null pointer", entry);
  const dim3 grid = down_grid(N, H, W);
  const int rc = Cmid == 1 ? launch_down_fwd<1>(entry, (hipStream_t)stream, grid, x, w1, b1, w2, b2, y, Cin, H, W)
                           : launch_down_fwd<10>(entry, (hipStream_t)stream, grid, x, w1, b1, w2, b2, y, Cin, H, W);
  if (rc != 0) return rc;
  MCD_LAUNCH_CHECK(entry);
  return 0;
}

extern "C" int mcdseg_dann_down_bwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* dy,
                                    float* dx, float* dw1, float* db1, float* dw2, float* db2, int32_t N, int32_t Cin, int32_t Cmid,
                                    int32_t H, int32_t W, int32_t groups, void* workspace, size_t workspace_bytes, void* stream) {
  const char* entry = "dann_down_bwd";
  const int bad = down_check(entry, N, Cin, Cmid, H, W);
  if (bad != 0) return bad;
  MCD_REQUIRE(groups >= 1 && N % groups == 0, "%s: %d samples do not split into %d equal groups", entry, N, groups);
  MCD_REQUIRE(x && w1 && b1 && w2 && b2 && dy && dw1 && db1 && dw2 && db2 && workspace, "%s: null pointer (only dx may be NULL)", entry);
  MCD_REQUIRE(workspace_bytes >= mcdseg_dann_down_workspace_bytes(N, Cin, Cmid, H, W), "%s: workspace too small", entry);
  const dim3 grid = down_grid_bwd(N, H, W);
  const int64_t nwg = (int64_t)grid.x * grid.y * grid.z;
  MCD_REQUIRE(nwg < (1ll << 31) / 16, "%s: too many tiles", entry);
  float* part = (float*)workspace;
  const int rc = Cmid == 1 ? launch_down_bwd<1>(entry, (hipStream_t)stream, grid, x, w1, b1, w2, b2, dy, dx, part, Cin, H, W)
                           : launch_down_bwd<10>(entry, (hipStream_t)stream, grid, x, w1, b1, w2, b2, dy, dx, part, Cin, H, W);
  if (rc != 0) return rc;
  MCD_LAUNCH_CHECK(entry);
  const int items = down_items(Cin, Cmid);
  hipLaunchKernelGGL(dann_down_reduce_kernel, dim3(ceil_div(items, 16)), dim3(256), 0, (hipStream_t)stream, (const float*)part, (int)(nwg / groups), groups,
                     items, Cmid * Cin * 9, Cmid, dw1, db1, dw2, db2);
  MCD_LAUNCH_CHECK("dann_down_reduce");
  return 0;
}

extern "C" size_t mcdseg_dann_tail_save_bytes(int32_t G, int32_t n) {
  if (G <= 0 || n <= 0) return 0;
  return (size_t)G * n * TL_HID * sizeof(float) + 2 * (size_t)G * TL_HID * sizeof(double);  // (40 G n bytes keep the doubles aligned)
}

extern "C" size_t mcdseg_dann_tail_workspace_bytes(int32_t G, int32_t n) {
  if (G <= 0 || n <= 0) return 0;
  return (size_t)G * n * (TL_HID + 2) * sizeof(float);
}

extern "C" int mcdseg_dann_tail_fwd(const float* h, const int32_t* labels, const float* w1, const float* b1, const float* gamma,
                                    const float* beta, float* running_mean, float* running_var, const float* w2, const float* b2,
                                    float momentum, float eps, int32_t training, float* loss, float* logits, float* save, int32_t G, int32_t n,
                                    int32_t F, void* stream) {
  const char* entry = "dann_tail_fwd";
  const int bad = tail_check(entry, G, n, F, training);
  if (bad != 0) return bad;
  MCD_REQUIRE(h && labels && w1 && b1 && gamma && beta && running_mean && running_var && w2 && b2 && loss && logits && save,
              "%s: null pointer", entry);
  hipLaunchKernelGGL(dann_tail_fwd_kernel, dim3(1), dim3(TL_NT), 0, (hipStream_t)stream, h, labels, w1, b1, gamma, beta, running_mean,
                     running_var, w2, b2, momentum, eps, (int)training, loss, logits, save, G, n, F);
  MCD_LAUNCH_CHECK(entry);
  return 0;
}

extern "C" int mcdseg_dann_tail_bwd(const float* h, const int32_t* labels, const float* w1, const float* gamma, const float* beta,
                                    const float* w2, const float* logits, const float* save, const float* upstream, float* dh, float* dw1,
                                    float* db1, float* dgamma, float* dbeta, float* dw2, float* db2, int32_t training, int32_t G, int32_t n,
                                    int32_t F, void* workspace, size_t workspace_bytes, void* stream) {
  const char* entry = "dann_tail_bwd";
  const int bad = tail_check(entry, G, n, F, training);
  if (bad != 0) return bad;
  MCD_REQUIRE(h && labels && w1 && gamma && beta && w2 && logits && save && upstream && dw1 && db1 && dgamma && dbeta && dw2 && db2 && workspace,
              "%s: null pointer (only dh may be NULL)", entry);
  MCD_REQUIRE(workspace_bytes >= mcdseg_dann_tail_workspace_bytes(G, n), "%s: workspace too small", entry);
  hipLaunchKernelGGL(dann_tail_bwd_kernel, dim3(1), dim3(TL_NT), 0, (hipStream_t)stream, h, labels, w1, gamma, beta, w2, logits, save, upstream,
                     dh, dw1, db1, dgamma, dbeta, dw2, db2, (float*)workspace, (int)training, G, n, F);
  MCD_LAUNCH_CHECK(entry);
  return 0;
}
