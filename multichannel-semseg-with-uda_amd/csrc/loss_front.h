// The three front ends of the fused loss kernels, as text: csrc/loss.hip includes this file once per family of kernels -- the L1 kernels
// under the names profiles, tests and bench.py know, and the other probability distances as kernels of their own -- with
//   MCD_FRONT_T2 / MCD_FRONT_T3   the template heads (<NCMAX, TWO> / <NCMAX, TWO, EXACT> for L1; <NCMAX, KIND> / <NCMAX, EXACT, KIND>)
//   MCD_FRONT_PLAIN / _UP8 / _DMA the kernel names
//   MCD_FRONT_HEADS               first statement of every body: empty for L1, `constexpr bool TWO = true` for the two-head distances
//   MCD_FRONT_PIXEL               the per-pixel core
// (a shared __device__ body behind two __global__ wrappers was tried first: it changed the code of the L1 kernels -- different
// alias scopes after inlining; included as text, the L1 kernels compile from the token stream they always had.)
// What each kernel does is described above its include in loss.hip.
MCD_FRONT_T2
__global__ __launch_bounds__(256) void MCD_FRONT_PLAIN(const float* __restrict__ z1, const float* __restrict__ z2,
                                                            const int64_t* __restrict__ labels, const float* __restrict__ cw,
                                                            int64_t ignore_index, float ce_coef, float diff_coef,
                                                            const float* __restrict__ losses_w, float* __restrict__ g1,
                                                            float* __restrict__ g2, float* __restrict__ part, int C, int HW,
                                                            int64_t P, float inv_m) {
  MCD_FRONT_HEADS;
  const int64_t pix = blockIdx.x * (int64_t)LOSS_BLOCK + threadIdx.x;
  const bool valid = pix < P;
  float ce1 = 0.f, ce2 = 0.f, dsum = 0.f;
  if (valid) {
    const int64_t n = pix / HW;
    const int hw = (int)(pix - n * HW);
    const size_t base = (size_t)n * C * HW + hw;
    float a[NCMAX], b[NCMAX];
#pragma unroll
    for (int c = 0; c < NCMAX; ++c) {
      a[c] = (c < C) ? z1[base + (size_t)c * HW] : -INFINITY;
      b[c] = (TWO && c < C) ? z2[base + (size_t)c * HW] : -INFINITY;
    }
    int y = -1;
    float wy = 0.f;
    if (labels != nullptr) {
      const int64_t yl = labels[pix];
      if (yl != ignore_index && yl >= 0 && yl < C) {
        y = (int)yl;
        wy = cw ? cw[y] : 1.f;
      }
    }
    MCD_FRONT_PIXEL(a, b, y, wy, ce_coef, diff_coef, losses_w, g1, g2, base, (size_t)HW, C, inv_m, ce1, ce2, dsum);
  }
  __shared__ float sh[3][4];
  float v[3] = {ce1, ce2, dsum};
  block_gather(v, sh);
  if (threadIdx.x < 3) {
    const int q = threadIdx.x;
    part[(size_t)blockIdx.x * 3 + q] = tree_total<4>(sh[q]);
  }
}

MCD_FRONT_T2
__global__ __launch_bounds__(UP_NT) void MCD_FRONT_UP8(const float* __restrict__ s1, const float* __restrict__ w1,
                                                                  const float* __restrict__ s2, const float* __restrict__ w2,
                                                                  const int64_t* __restrict__ labels, const float* __restrict__ cw,
                                                                  int64_t ignore_index, float ce_coef, float diff_coef,
                                                                  const float* __restrict__ losses_w, float* __restrict__ g1,
                                                                  float* __restrict__ g2, float* __restrict__ part, int N, int C,
                                                                  int Hi, int Wi, float inv_m) {
  MCD_FRONT_HEADS;
  extern __shared__ __attribute__((aligned(16))) float up_sm[];
  constexpr int HEADS = TWO ? 2 : 1;
  constexpr int SREG = (HEADS * NCMAX * UP_JP * 4 + UP_NT - 1) / UP_NT;  // staged scores per thread and item
  // Class stride NCMAX, not C, and the four taps / four scores of a pixel as one 16-byte unit: every LDS read below is then
  // the lane's base address plus an immediate offset.  (With C in the stride, or with the scores as plain rows read by
  // ds_read2_b32 -- whose offset field reaches 1 KB -- the 2 x NCMAX addresses become registers of their own and the
  // kernel spills hundreds of them.)
  float* wl = up_sm;                         // [head][NCMAX][ky0 8][kx0 8][a 2][b 2]
  float* sin = up_sm + HEADS * NCMAX * 256;  // [head][NCMAX][pair UP_JP][a 2][b 2]: score (row iyg - a, column ixb + pair + 1 - b)
  const int Wo = 8 * Wi, Ho = 8 * Hi;
  const int nseg = (Wo + UP_COLS - 1) / UP_COLS;
  const int items = N * (Hi + 1) * nseg;
  const int ky0 = threadIdx.x >> 6, lane = threadIdx.x & 63;
  MCD_UP8_STAGE_TAPS  // (csrc/up8_patch.h, as the other MCD_UP8_ fragments of this kernel)
  constexpr int nstage = HEADS * NCMAX * UP_JP * 4;
  float sreg[SREG];
  auto fetch = [&](int item) {  // scores of one item -> registers (zeros outside the map)
    MCD_UP8_FETCH(item)
  };
  float ce1 = 0.f, ce2 = 0.f, dsum = 0.f;
  int item = blockIdx.x;
  if (item < items) fetch(item);
  for (; item < items; item += gridDim.x) {
    __syncthreads();  // the previous item's readers are done (and, first time round, the kernels are staged)
    MCD_UP8_COMMIT
    __syncthreads();
    if (item + (int)gridDim.x < items) fetch(item + gridDim.x);
    const int seg = item % nseg, r = item / nseg;
    const int iyg = r % (Hi + 1), n = r / (Hi + 1);
    const int oy = 8 * iyg - 4 + ky0;
    const int ox = seg * UP_COLS + lane;
    if (oy >= 0 && oy < Ho && ox < Wo) {
      // the class count re-read as an opaque scalar: otherwise the NCMAX "c < C" store guards are hoisted out of the item loop
      // and their results spill
      int Cv = C;
      asm volatile("" : "+s"(Cv));
      const int kx0 = (ox + 4) & 7;
      const int jp = ((ox + 4) >> 3) - seg * (UP_COLS / 8);  // pair whose b = 0 member is this pixel's right-hand input column
      // the lane's LDS offsets, opaque too: the kernel taps do not depend on the item ((ox + 4) & 7 is the lane's), and left
      // alone the compiler hoists all 2 x NCMAX 16-byte reads out of the item loop
      int woff = (ky0 * 8 + kx0) * 4, soff = jp * 4;
      asm volatile("" : "+v"(woff), "+v"(soff));
      float a[NCMAX], b[NCMAX];
      MCD_UP8_LOGITS(a, b)
      const size_t HW = (size_t)Ho * Wo;
      const size_t hw = (size_t)oy * Wo + ox;
      int y = -1;
      float wy = 0.f;
      if (labels != nullptr) {
        const int64_t yl = labels[(size_t)n * HW + hw];
        if (yl != ignore_index && yl >= 0 && yl < C) {
          y = (int)yl;
          wy = cw ? cw[y] : 1.f;
        }
      }
      float e1 = 0.f, e2 = 0.f, ds = 0.f;
      MCD_FRONT_PIXEL(a, b, y, wy, ce_coef, diff_coef, losses_w, g1, g2, (size_t)n * C * HW + hw, HW, Cv, inv_m, e1, e2, ds);
      ce1 += e1;
      ce2 += e2;
      dsum += ds;
    }
  }
  __shared__ float sh[3][UP_NT / 64];
  float v[3] = {ce1, ce2, dsum};
  block_gather(v, sh);
  if (threadIdx.x < 3) {
    const int q = threadIdx.x;
    part[(size_t)blockIdx.x * 3 + q] = chain_total<UP_NT / 64>(sh[q]);
  }
}

MCD_FRONT_T3
__global__ __launch_bounds__(UP_NT) void MCD_FRONT_DMA(const float* __restrict__ s1, const float* __restrict__ w1,
                                                                      const float* __restrict__ s2, const float* __restrict__ w2,
                                                                      const int64_t* __restrict__ labels, const float* __restrict__ cw,
                                                                      int64_t ignore_index, float ce_coef, float diff_coef,
                                                                      const float* __restrict__ losses_w, float* __restrict__ g1,
                                                                      float* __restrict__ g2, float* __restrict__ part, int N, int C,
                                                                      int Hi, int Wi, float inv_m) {
  MCD_FRONT_HEADS;
  extern __shared__ __attribute__((aligned(16))) float up_sm[];
  using L = UpDmaLayout<NCMAX, TWO>;
  constexpr int HEADS = L::HEADS, SPK = L::SPK, SP = L::SP;
  float* wl = up_sm;                                                   // [head][NCMAX][ky0 8][kx0 8][a 2][b 2]
  float* sin0 = up_sm + L::W_FLOATS;                                   // [buffer 2][head][SP]: [NCMAX][pair UP_JP][a 2][b 2] + tail
  float* cwl = sin0 + L::S_FLOATS;                                     // [NCMAX] class weights (1 without)
  unsigned char* lab0 = reinterpret_cast<unsigned char*>(cwl + L::CW_FLOATS);  // [buffer 2][wave 8][1 KB]
  const int Wo = 8 * Wi, Ho = 8 * Hi;
  const int nseg = (Wo + UP_COLS - 1) / UP_COLS;
  const int items = N * (Hi + 1) * nseg;
  const int lane = threadIdx.x & 63;
  const int ky0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int i = threadIdx.x; i < HEADS * NCMAX * 256; i += UP_NT) {
    const int b = i & 1, a = (i >> 1) & 1, kx = (i >> 2) & 7, ky = (i >> 5) & 7, hc = i >> 8;
    const int c = hc % NCMAX;
    wl[i] = c < C ? (hc >= NCMAX ? w2 : w1)[c * 256 + (ky + 8 * a) * 16 + kx + 8 * b] : 0.f;
  }
  for (int i = threadIdx.x; i < NCMAX; i += UP_NT) cwl[i] = (cw != nullptr && i < C) ? cw[i] : 1.f;
  const mcd_i32x4 rs1 = mcd_raw_rsrc(s1, N * C * Hi * Wi * 4);
  const mcd_i32x4 rs2 = mcd_raw_rsrc(TWO ? s2 : s1, N * C * Hi * Wi * 4);
  const mcd_i32x4 rsl = mcd_raw_rsrc(labels != nullptr ? (const void*)labels : (const void*)s1, labels != nullptr ? N * Ho * Wo * 8 : 0);
  const unsigned lds_s = (unsigned)(size_t)(__attribute__((address_space(3))) float*)sin0;
  const unsigned lds_l = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lab0;
  auto issue = [&](int item, int buf) {  // the inputs of one item -> LDS buffer `buf` (zeros outside the map)
    const int seg = item % nseg, r = item / nseg;
    const int iyg = r % (Hi + 1), n = r / (Hi + 1);
    const int ixb = seg * (UP_COLS / 8) - 1;
#pragma unroll
    for (int k = 0; k < SPK; ++k) {
      const int i = threadIdx.x + k * UP_NT;
      const int b = i & 1, a = (i >> 1) & 1, q = i >> 2;
      const int j = q % UP_JP, c = q / UP_JP;
      const int iy = iyg - a, ix = ixb + j + 1 - b;
      const bool ok = c < C && (unsigned)iy < (unsigned)Hi && (unsigned)ix < (unsigned)Wi;
      const unsigned voff = ok ? (unsigned)((((n * C + c) * Hi + iy) * Wi + ix) * 4) : UP_OOB;
      mcd_hidden_dma<4>(rs1, __builtin_amdgcn_readfirstlane(lds_s + 4u * ((buf * HEADS) * SP + k * UP_NT + ky0 * 64)), voff);
      if (TWO) mcd_hidden_dma<4>(rs2, __builtin_amdgcn_readfirstlane(lds_s + 4u * ((buf * HEADS + 1) * SP + k * UP_NT + ky0 * 64)), voff);
    }
    if (labels != nullptr) {
      const int oy = 8 * iyg - 4 + ky0;
      const unsigned voff = (lane < 32 && (unsigned)oy < (unsigned)Ho) ? (unsigned)(((n * Ho + oy) * Wo + seg * UP_COLS + 2 * lane) * 8) : UP_OOB;
      mcd_hidden_dma<16>(rsl, __builtin_amdgcn_readfirstlane(lds_l + 1024u * (buf * (UP_NT / 64) + ky0)), voff);
    }
  };
  const int nst = (g1 != nullptr ? C : 0) + ((TWO && g2 != nullptr) ? C : 0);  // stores per wave and item
  float ce1 = 0.f, ce2 = 0.f, dsum = 0.f;
  int item = blockIdx.x, buf = 0;
  int behind = 0;  // wave-uniform: the stores this wave issued after its last DMA
  __syncthreads();  // (the kernels and class weights are staged before anybody's DMA could be mistaken for them -- and for the first barrier below)
  if (item < items) issue(item, 0);
  for (; item < items; item += gridDim.x, buf ^= 1) {
    // this item's inputs have landed (issued before `behind` stores: in-order counter), every wave is done with the other buffer
    if (__builtin_amdgcn_readfirstlane(behind) >= 63)
      asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // (outside the branch: one barrier whatever the compiler makes of it)
    if (item + (int)gridDim.x < items) issue(item + gridDim.x, buf ^ 1);
    behind = 0;
    const int seg = item % nseg, r = item / nseg;
    const int iyg = r % (Hi + 1), n = r / (Hi + 1);
    const int oy = 8 * iyg - 4 + ky0;
    const int ox = seg * UP_COLS + lane;
    if (oy >= 0 && oy < Ho) {  // wave-uniform
      behind = nst;
      if (ox < Wo) {
        int Cv = C;
        asm volatile("" : "+s"(Cv));
        const int kx0 = (ox + 4) & 7;
        const int jp = ((ox + 4) >> 3) - seg * (UP_COLS / 8);
        int woff = (ky0 * 8 + kx0) * 4, soff = jp * 4 + buf * HEADS * SP;
        asm volatile("" : "+v"(woff), "+v"(soff));
        float a[NCMAX], b[NCMAX];
#pragma unroll
        for (int c0 = 0; c0 < NCMAX; c0 += 4) {
          MCD_OPAQUE_TRUE(go);
          if (go) {
#pragma unroll
            for (int c = c0; c < c0 + 4; ++c) {
              if (c >= NCMAX) continue;
              b[c] = -INFINITY;
#pragma unroll
              for (int h = 0; h < HEADS; ++h) {
                const float4 wv = *reinterpret_cast<const float4*>(wl + woff + (h * NCMAX + c) * 256);
                const float4 sv = *reinterpret_cast<const float4*>(sin0 + soff + h * SP + c * (UP_JP * 4));
                float o = 0.f;
                o = fmaf(sv.x, wv.x, o);
                o = fmaf(sv.y, wv.y, o);
                o = fmaf(sv.z, wv.z, o);
                o = fmaf(sv.w, wv.w, o);
                if (!EXACT && c >= Cv) o = -INFINITY;
                if (h == 0)
                  a[c] = o;
                else
                  b[c] = o;
              }
            }
          }
        }
        const size_t HW = (size_t)Ho * Wo;
        const size_t hw = (size_t)oy * Wo + ox;
        int y = -1;
        float wy = 0.f;
        if (labels != nullptr) {
          const int64_t yl = *reinterpret_cast<const int64_t*>(lab0 + (buf * (UP_NT / 64) + ky0) * 1024 + lane * 8);
          if (yl != ignore_index && yl >= 0 && yl < C) {
            y = (int)yl;
            wy = cwl[y];
          }
        }
        float e1 = 0.f, e2 = 0.f, ds = 0.f;
        MCD_FRONT_PIXEL(a, b, y, wy, ce_coef, diff_coef, losses_w, g1, g2, (size_t)n * C * HW + hw, HW, Cv, inv_m, e1, e2, ds);
        ce1 += e1;
        ce2 += e2;
        dsum += ds;
      }
    }
  }
  // block_gather + chain_total (block_reduce.h) written out: through the call, the two-head 24-class instantiations of this kernel come
  // out with two instructions in another order, and the kernels of the training step keep the instruction stream they had
  __shared__ float sh[3][UP_NT / 64];
  ce1 = wave_sum(ce1);
  ce2 = wave_sum(ce2);
  dsum = wave_sum(dsum);
  if (lane == 0) {
    sh[0][ky0] = ce1;
    sh[1][ky0] = ce2;
    sh[2][ky0] = dsum;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int q = threadIdx.x;
    float t = 0.f;
    for (int k = 0; k < UP_NT / 64; ++k) t += sh[q][k];
    part[(size_t)blockIdx.x * 3 + q] = t;
  }
}
