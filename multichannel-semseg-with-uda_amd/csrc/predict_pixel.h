// The pixel tail of the inference kernels, as text: shared by predict_kernel (csrc/loss.hip) and predict_up8_kernel (csrc/infer.hip),
// each compiled with its own file's flags (adapt_tester.py:101-124, util.py:44-48).  A macro, not a function, for the reason given at
// the head of up8_patch.h: behind a __device__ function both kernels compile to other code (up to 100 more scalar registers spilled).
//   MCD_PREDICT_PIXEL(a, best, ent)   float a[NCMAX]: the pixel's logits (-inf past C), left as exp(a - max); int best = argmax over
//                                     the first C_used classes (the first of equals); float ent += sum_c p_c log(p_c + 1e-6) over ALL
//                                     C classes.  Names the kernel's NCMAX, C and C_used; declares nothing outside its own braces.
#pragma once

#define MCD_PREDICT_PIXEL(a, best, ent)                     \
  {                                                         \
    float m = a[0], mu = a[0];                              \
    best = 0;                                               \
    _Pragma("unroll") for (int c = 1; c < NCMAX; ++c) {     \
      m = fmaxf(m, a[c]);                                   \
      if (c < C_used && a[c] > mu) {                        \
        mu = a[c];                                          \
        best = c;                                           \
      }                                                     \
    }                                                       \
    float sum = 0.f;                                        \
    _Pragma("unroll") for (int c = 0; c < NCMAX; ++c) {     \
      a[c] = (c < C) ? expf(a[c] - m) : 0.f;                \
      sum += a[c];                                          \
    }                                                       \
    const float r = 1.f / sum;                              \
    _Pragma("unroll") for (int c = 0; c < NCMAX; ++c) {     \
      if (c < C) {                                          \
        const float pc = a[c] * r;                          \
        ent += pc * logf(pc + 1e-6f);                       \
      }                                                     \
    }                                                       \
  }
