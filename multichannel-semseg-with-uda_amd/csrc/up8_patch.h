// The register-staged x8 up-sampling patch of the fused loss kernels, as text: what a kernel needs to form the logits of one or two
// heads, up8(s1, w1) and up8(s2, w2), for the pixels of a patch of 8 rows x 64 columns from ONE staged copy of the scores.  Users:
// csrc/loss_front.h (`up8_softmax_ce_l1_kernel`, `up8_softmax_ce_dist_kernel`) and csrc/uncertain.hip (`up8_uncertain_kernel`, the same
// structure with s1 == s2, w1 = up.weight, w2 = up_std.weight and a per-pixel body of its own).  Included INSIDE the includer's
// anonymous namespace.
//
// Macros, not functions, for the reason given at the head of loss_front.h: a shared __device__ body changed the code of the L1
// kernels; as text they compile from the token stream they always had.  The fragments name the kernel's variables directly:
//   template / constants   NCMAX, HEADS (1 or 2), SREG = ceil(HEADS * NCMAX * UP_JP * 4 / UP_NT), nstage = HEADS * NCMAX * UP_JP * 4
//   arguments              s1, w1, s2, w2, C, Hi, Wi
//   LDS                    wl  [head][NCMAX][ky0 8][kx0 8][a 2][b 2]   the 16 x 16 kernels, four taps of a pixel = one 16-byte read
//                          sin [head][NCMAX][pair UP_JP][a 2][b 2]     score (row iyg - a, column ixb + pair + 1 - b) of the item
//   registers              float sreg[SREG]; int nseg = ceil(8 Wi / UP_COLS)
// Names the fragments DECLARE in the scope they are expanded in (keep them free there):
//   MCD_UP8_STAGE_TAPS   none outside its own loop body (i, a, b, kx, ky, hc, c inside it)
//   MCD_UP8_FETCH(item)  seg, r, iyg, n, ixb -- at the top level of the expansion, which is why it is expanded inside a lambda of its
//                        own and why a kernel argument must not be called r or n; i, v, a, b, q, j, hc, c, iy, ix, k inside its loop
//   MCD_UP8_COMMIT       k, i inside its loop
//   MCD_UP8_LOGITS(a, b) c0, go, c, h, wv, sv, o inside its loops (MCD_OPAQUE_TRUE declares the name it is given)
// The layout (class stride NCMAX, the -inf logit of the classes past C from taps (1, 0, 0, 0) against scores (-inf, 0, 0, 0)) is
// described where the fragments are used in loss_front.h.
#pragma once

#define MCD_OPAQUE_TRUE(name) \
  int name = 1;               \
  asm volatile("" : "+s"(name))

// exp of a NON-POSITIVE argument (a logit minus the pixel's maximum): v_exp_f32(x log2 e), two instructions where expf spends fifteen on
// a range reduction and a scaling that such an argument never needs (round 6: the fused loss kernel evaluates 82 of these per pixel and
// was bound by them after round 5's wait fix).  Relative error: the instruction's 1 ulp plus |x| 2^-24 from rounding x log2 e -- below
// 2e-7 for every class that carries probability (x > -3); exp(-inf) = 0 for the padding classes; results below 2^-126 flush to zero.
__device__ __forceinline__ float exp_nonpos(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

constexpr int UP_COLS = 64, UP_JP = 9, UP_NT = 512;  // UP_JP: input-column pairs (ix-1, ix) a 64-pixel row segment touches

// the kernels of every class and head -> LDS, once per workgroup
#define MCD_UP8_STAGE_TAPS                                                                                                         \
  for (int i = threadIdx.x; i < HEADS * NCMAX * 256; i += UP_NT) {                                                                 \
    const int b = i & 1, a = (i >> 1) & 1, kx = (i >> 2) & 7, ky = (i >> 5) & 7, hc = i >> 8;                                      \
    const int c = hc % NCMAX;                                                                                                      \
    /* classes past C: taps (1, 0, 0, 0) against scores (-inf, 0, 0, 0) below give the logit -inf with no test in the pixel loop */ \
    wl[i] = c < C ? (hc >= NCMAX ? w2 : w1)[c * 256 + (ky + 8 * a) * 16 + kx + 8 * b] : ((a | b) == 0 ? 1.f : 0.f);                \
  }

// scores of one item -> registers (zeros outside the map)
#define MCD_UP8_FETCH(item)                                                            \
  const int seg = item % nseg, r = item / nseg;                                        \
  const int iyg = r % (Hi + 1), n = r / (Hi + 1);                                      \
  const int ixb = seg * (UP_COLS / 8) - 1;                                             \
  _Pragma("unroll") for (int k = 0; k < SREG; ++k) {                                   \
    const int i = threadIdx.x + k * UP_NT;                                             \
    float v = 0.f;                                                                     \
    if (i < nstage) {                                                                  \
      const int b = i & 1, a = (i >> 1) & 1, q = i >> 2;                               \
      const int j = q % UP_JP, hc = q / UP_JP;                                         \
      const int c = hc % NCMAX;                                                        \
      const int iy = iyg - a, ix = ixb + j + 1 - b;                                    \
      if (c >= C)                                                                      \
        v = (a | b) == 0 ? -INFINITY : 0.f;                                            \
      else if (iy >= 0 && iy < Hi && ix >= 0 && ix < Wi)                               \
        v = (hc >= NCMAX ? s2 : s1)[(((size_t)n * C + c) * Hi + iy) * Wi + ix];        \
    }                                                                                  \
    sreg[k] = v;                                                                       \
  }

// the fetched scores -> LDS (between two barriers of the caller's)
#define MCD_UP8_COMMIT                               \
  _Pragma("unroll") for (int k = 0; k < SREG; ++k) { \
    const int i = threadIdx.x + k * UP_NT;           \
    if (i < nstage) sin[i] = sreg[k];                \
  }

// the pixel's logits: a[c] of head 0 and, with two heads, b[c] of head 1 (else -inf), the multiply-adds in the order of up8_fwd_kernel;
// woff / soff are the lane's LDS offsets.  Groups of four classes in basic blocks of their own (see pixel_losses).
#define MCD_UP8_LOGITS(a, b)                                                                                     \
  _Pragma("unroll") for (int c0 = 0; c0 < NCMAX; c0 += 4) {                                                      \
    MCD_OPAQUE_TRUE(go);                                                                                         \
    if (go) {                                                                                                    \
      _Pragma("unroll") for (int c = c0; c < c0 + 4; ++c) {                                                      \
        if (c >= NCMAX) continue;                                                                                \
        b[c] = -INFINITY;                                                                                        \
        _Pragma("unroll") for (int h = 0; h < HEADS; ++h) {                                                      \
          const float4 wv = *reinterpret_cast<const float4*>(wl + woff + (h * NCMAX + c) * 256);                 \
          const float4 sv = *reinterpret_cast<const float4*>(sin + soff + (h * NCMAX + c) * (UP_JP * 4));        \
          float o = 0.f;                                                                                         \
          o = fmaf(sv.x, wv.x, o);                                                                               \
          o = fmaf(sv.y, wv.y, o);                                                                               \
          o = fmaf(sv.z, wv.z, o);                                                                               \
          o = fmaf(sv.w, wv.w, o);                                                                               \
          if (h == 0)                                                                                            \
            a[c] = o;                                                                                            \
          else                                                                                                   \
            b[c] = o;                                                                                            \
        }                                                                                                        \
      }                                                                                                          \
    }                                                                                                            \
  }
