// Operand-split policies of the matrix-pipe convolutions (conv_gemm_split.hip, conv_wgrad_split.hip, bn.hip), and at the end of the file
// what their weight-gradient kernels share: the transposing LDS reads, the companion-piece descriptor, the piece stride, the CU count.
//
// gfx950 has no fp32-grade matrix instruction faster than the vector rate (no xf32/TF32), so an fp32 product a*b is
// carried through the 16-bit MFMA pipe as a sum of exact piece products:
//
//   SplitBf16x6   a = a1 + a2 + a3 with bf16 pieces (8+8+8 significant bits, fp32's exponent range: no scaling needed),
//                 six cross terms a1b1 + a1b2 + a2b1 + a2b2 + a1b3 + a3b1 on v_mfma_f32_32x32x16_bf16;
//   SplitF16x3    a = s * (h1 + h2) with fp16 pieces (11+11 significant bits) and a power-of-two scale s per TENSOR,
//                 three cross terms h1h1' + h1h2' + h2h1' on v_mfma_f32_32x32x16_f16 -- half the matrix instructions
//                 and two thirds of the operand bytes of the bf16 form for the same measured accuracy against the
//                 reference's fp64 gradients (tools/split_numerics.py; tests/test_model_gpu.py).
//
// fp16 has 5 exponent bits, so SplitF16x3 needs the scale: s = 2^(e-15) where 2^e >= B and B is an UPPER BOUND of |x| over
// the tensor, known before the tensor is written (BatchNorm outputs: Samuelson's inequality |xhat| <= sqrt(n-1), see bn.hip;
// weights and foreign tensors: a measured absolute maximum).  Then |x/s| <= 2^15 < 65504: no finite value overflows.  An
// element keeps 22 significant bits while |x/s| >= 2^-3 and an ABSOLUTE error of 2^-25 s below that (fp16 subnormals are
// kept by v_cvt_f16_f32 and by the MFMA: tools/probes/f16_denorm.hip) -- for a dot product it is the absolute error relative
// to the TYPICAL magnitude that counts, and typical values sit within 2^13 of the bound for every tensor of the network.
// Non-finite values stay non-finite: inf becomes NaN in the remainder (inf - inf), as in the bf16 split.
#pragma once
#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// scale of a tensor whose absolute values are bounded by `bound`: 2^(e-15) with 2^e >= bound; 1 for an empty / all-zero /
// non-finite bound (non-finite data then overflows into inf/NaN, which is the contract)
__host__ __device__ __forceinline__ float mcd_scale_of_bound(float bound) {
  if (!(bound > 0.f) || !(bound <= 3.0e38f)) return 1.f;
  int e;
  (void)frexpf(bound, &e);  // bound = m * 2^e, 0.5 <= m < 1
  e -= 15;
  if (e < -100) e = -100;
  if (e > 100) e = 100;
  return ldexpf(1.f, e);
}

struct SplitBf16x6 {
  static constexpr bool HALF_OUT = false;  // (16-bit channel-blocked epilogues: the one-term arithmetic only)
  static constexpr int KDEEP = 1;          // (K-steps of 16 channels per barrier interval of the ping-pong kernels)
  static constexpr int NP = 3;
  static constexpr int NPU = 3;  // pieces a kernel stages into LDS (all of them)
  static constexpr int NTERMS = 6;
  static constexpr bool SCALED = false;
  typedef __bf16 elem;
  typedef bf16x8 frag;
  // cross terms (piece of A, piece of B), smallest first
  static constexpr int TA[6] = {2, 0, 1, 1, 0, 0};
  static constexpr int TB[6] = {0, 2, 1, 0, 1, 0};
  __device__ __forceinline__ static f32x16 mfma(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  __device__ __forceinline__ static void split(float v, float /*inv_scale*/, elem (&p)[NP]) {
    const __bf16 a = (__bf16)v;
    const float r1 = v - (float)a;  // exact
    const __bf16 b = (__bf16)r1;
    p[0] = a;
    p[1] = b;
    p[2] = (__bf16)(r1 - (float)b);
  }
};

struct SplitF16x3 {
  static constexpr bool HALF_OUT = false;
  static constexpr int KDEEP = 1;
  static constexpr int NP = 2;
  static constexpr int NPU = 2;
  static constexpr int NTERMS = 3;
  static constexpr bool SCALED = true;
  typedef _Float16 elem;
  typedef f16x8 frag;
  static constexpr int TA[3] = {1, 0, 0};
  static constexpr int TB[3] = {0, 1, 0};
  __device__ __forceinline__ static f32x16 mfma(frag a, frag b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  __device__ __forceinline__ static void split(float v, float inv_scale, elem (&p)[NP]) {
    const float q = v * inv_scale;  // exact: the scale is a power of two
    const _Float16 h = (_Float16)q;
    p[0] = h;
    p[1] = (_Float16)(q - (float)h);
  }
};

// SplitF16x1: the REDUCED-PRECISION arithmetic (BASELINE config 5 "bf16"; bench.py --dtype f16): the operands are stored exactly
// as SplitF16x3 stores them (two scaled fp16 pieces -- same companions, weight images, bounds, producers), but a product keeps
// only the leading term h1 h1': one MFMA instead of three, operands rounded to fp16's 11 significant bits (bf16 would keep 8).
struct SplitF16x1 : SplitF16x3 {
  static constexpr bool HALF_OUT = true;  // its convolutions can write 16-bit channel-blocked tensors (round 6: 2-byte activation storage)
  static constexpr int NPU = 1;  // pieces a kernel has to STAGE (the second piece is stored but never multiplied)
  static constexpr int NTERMS = 1;
  static constexpr int TA[1] = {0};
  static constexpr int TB[1] = {0};
};

// SplitF16x1D: the same arithmetic for the 8-wave ping-pong convolution with TWO K-steps of 16 channels per barrier interval.  A K-step
// of the one-term arithmetic is 8 matrix instructions per wave (256 cycles) against the three-term form's 24, while its barriers, counted
// waits and DMA issue cost what they cost: the kernels balanced for three terms reach 0.30 of the matrix peak with one (round 5).  Here
// the LDS slots of the (never staged) second piece hold the NEXT K-step's operands: the stage image, the fragment reads and the DMA count
// are the three-term kernel's, 16 matrix instructions per interval.  Same products in the same order: bit for bit SplitF16x1's results.
struct SplitF16x1D : SplitF16x1 {
  static constexpr int KDEEP = 2;
};

// split 8 values into NP fragments
template <class P>
__device__ __forceinline__ void split_frag(const float (&v)[8], float inv_scale, typename P::frag (&out)[P::NP]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    typename P::elem q[P::NP];
    P::split(v[e], inv_scale, q);
#pragma unroll
    for (int pc = 0; pc < P::NP; ++pc) out[pc][e] = q[pc];
  }
}

// scale of an operand from its bound pointer (NULL for the unscaled policy)
template <class P>
__device__ __forceinline__ float operand_scale(const float* bound) {
  if constexpr (P::SCALED) return mcd_scale_of_bound(*bound);
  return 1.f;
}

// one unit of a companion in the channel-blocked layout cb[piece NP][N][C/8][HW][8 x 16 bit] (bn.hip, "cb" variants): the split of 8
// channels of one pixel, one 16-byte store per piece; idx16 = (n * C/8 + g) * HW + pixel
template <class P>
__device__ __forceinline__ void split_store(const float (&v)[8], float inv_scale, typename P::elem* __restrict__ cb, size_t piece_stride,
                                            size_t idx16) {
  typename P::frag pieces[P::NP];
  split_frag<P>(v, inv_scale, pieces);
#pragma unroll
  for (int pc = 0; pc < P::NP; ++pc) *reinterpret_cast<typename P::frag*>(cb + pc * piece_stride + idx16 * 8) = pieces[pc];
}

static inline int mcd_math_pieces(int math) { return (math == 3 || math == 1) ? 2 : 3; }  // MCDSEG_MATH_F16X3 / _F16X1 : MCDSEG_MATH_BF16X6
// the arithmetic whose STORAGE (companions, weight images, bounds) a math shares: F16X1 multiplies F16X3's operands
static inline int mcd_storage_math(int math) { return math == 1 ? 3 : math; }
static inline bool mcd_math_known(int math) { return math == 1 || math == 3 || math == 6; }

// what every entry point that reads or writes a companion refuses before it launches (`math`: the storage math, mcd_storage_math)
static inline int cb_check(const char* who, int32_t math, const float* bound, int32_t N, int32_t C, int32_t HW) {
  MCD_REQUIRE(math == MCDSEG_MATH_BF16X6 || math == MCDSEG_MATH_F16X3, "%s: unknown math %d", who, math);
  MCD_REQUIRE(math != MCDSEG_MATH_F16X3 || bound != nullptr, "%s: the f16x3 split needs the bound scalar of the tensor", who);
  MCD_REQUIRE(N > 0 && C > 0 && HW > 0 && (C % 8) == 0, "%s: C must be a positive multiple of 8", who);
  MCD_REQUIRE((int64_t)N * (C / 8) <= 65535, "%s: N*C/8 exceeds the grid limit", who);
  return 0;
}

// ---- transposing LDS reads (ds_read_b64_tr_b16): the MFMA fragments of the weight-gradient kernels whose operands sit in LDS as in
// memory, 16-byte units of 8 channels x 1 pixel (conv_wgrad_split.hip, conv_wgrad_split_pp.hip) ----------------------------------
typedef short mcd_s16x4 __attribute__((ext_vector_type(4)));
typedef short mcd_s16x8 __attribute__((ext_vector_type(8)));

// the LDS byte address of (a place in) a __shared__ array: what a ds_ instruction written as inline assembly takes
__device__ __forceinline__ unsigned mcd_lds_addr(const void* shared) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (unsigned)(size_t)(__attribute__((address_space(3))) const unsigned char*)shared;
#else
  (void)shared;
  return 0;
#endif
}

// One transposing read at base + OFF (a compile-time offset).  Inline assembly: for a compiler-visible LDS load the wait-count pass
// puts an s_waitcnt vmcnt(0) in front whenever an LDS-DMA may be pending (it cannot tell that the DMA targets another stage), which
// would drain the prefetch at the head of every read phase.  The read completes at the lgkmcnt(0) of the wait that closes the
// caller's read phase; the caller then re-defines the registers behind that wait (`settle`: asm volatile("" : "+v"(f))) so that no
// matrix instruction can be scheduled ahead of it.
template <int OFF>
__device__ __forceinline__ mcd_s16x4 mcd_tr_read_at(unsigned base) {
  mcd_s16x4 v;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(base), "n"(OFF) : "memory");
#else
  (void)base;
  v = mcd_s16x4{};
#endif
  return v;
}

// The same read through the builtin, for the kernels whose reads the compiler may see (no LDS-DMA the wait-count pass knows of is
// pending when they read: conv_wgrad_split_tr64_kernel hides its DMAs, conv_wgrad_thin_tr.hip has drained them).
__device__ __forceinline__ mcd_s16x4 mcd_tr_read(const unsigned char* lds) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) mcd_s16x4*)(lds));
#else
  (void)lds;
  return mcd_s16x4{};
#endif
}

// two 4-pixel reads -> the 8 k slots of a fragment: 0-3 from the lane's first quad, 4-7 from its second
template <class F>
__device__ __forceinline__ F mcd_frag_pack(mcd_s16x4 lo, mcd_s16x4 hi) {
  const mcd_s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(F, v);
}
template <class F, int LO, int HI>
__device__ __forceinline__ F mcd_tr_frag(unsigned base) {
  const mcd_s16x4 lo = mcd_tr_read_at<LO>(base);
  const mcd_s16x4 hi = mcd_tr_read_at<HI>(base);
  return mcd_frag_pack<F>(lo, hi);
}

// The buffer descriptor a wave stages companion pieces through: `bytes` of the companion `cb` from byte `first` on (a whole piece, or
// several with the stride between them).  It starts `bias` = mcd_piece_bias(pad) bytes below that so that the SGPR offset (tile + tap
// shift, + bias) is never negative; the launchers admit a kernel only while what one descriptor covers stays below 2 GiB.
__device__ __forceinline__ int mcd_piece_bias(int pad) { return pad * 16 + 16; }
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mcd_piece_rsrc(const void* cb, long long first, int bytes, int bias) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)cb + first - bias), 0, bytes + bias, 0x00020000);
}

// bytes between the pieces of a companion of `per_image` 16-bit values per image: the companions' own batch (mcdseg_conv_desc.Ncb) apart;
// 0 for F16X1, which reads piece 0 only
static inline long long mcd_piece_stride(const mcdseg_conv_desc* d, int math, long long per_image) {
  return math == MCDSEG_MATH_F16X1 ? 0 : (long long)(d->Ncb ? d->Ncb : d->N) * per_image * 2;
}

// CUs of the current device (256, the MI355X's, where the query fails): defined in conv_gemm_split_pp.hip
int mcdseg_internal_device_cus();
