// Ensembling of saved predictions -- the reference's tools/ensemble_predict_from_npy.py:17-56 on the device.
//
//  * ensemble_probs        -- K maps [N][C][H][W] of the same images, each where its upload left it (K device pointers, no [K,C,H,W]
//                             copy), combined per element and arg-maxed per pixel in ONE pass:
//                               averaging  sum(probs) / len(probs) as numpy evaluates it (:24): ((0 + p0) + p1) + ... left to right in
//                                          fp32 -- the leading 0 is Python's, so a -0.0 leaves as +0.0 -- then one IEEE division by K;
//                               nms        np.max(probs, 0) (:26): m = m > p ? m : p left to right, so of +0 and -0 the later one stays
//                                          (what numpy's maximum gives), and a NaN wins.
//                             A NaN result leaves as the canonical quiet NaN 0x7FC00000 (the payload of a NaN that an addition makes is
//                             the host's business in numpy: 0xFFC00000 on x86, 0x7FC00000 elsewhere); under nms too, where numpy
//                             would hand an input NaN's payload through: input payloads are not preserved.
//                             label = argmax over c < n_used by numpy's rule (:32): the first maximum, a NaN counts as the maximum and
//                             the first NaN wins, +0 == -0.  The library is compiled with -ffp-contract=off; nothing here is contracted.
//  * label_resize_colorize -- Image.resize(out_shape, NEAREST) of the label map (:33-35) and of its palette image (:50-56) as one gather:
//                             NEAREST of the palette image and the palette of the NEAREST label are the same picture.  A label beyond
//                             the palette is black (Colorize.__call__, transform.py:155-165).
// Both are single-pass streams with plain stores and no atomics: the same bits run to run, nothing written outside the outputs.
#include "common.h"
#include "nearest_index.h"

namespace {

struct EnsembleMaps {
  const float* p[MCDSEG_ENSEMBLE_MAX_K];
};

template <int VEC>
struct Px;
template <>
struct Px<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* a) { v[0] = *a; }
  __device__ __forceinline__ void store(float* a) const { *a = v[0]; }
};
template <>
struct Px<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* a) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(a);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  }
  __device__ __forceinline__ void store(float* a) const {
    f32x4 t;
    t.x = v[0], t.y = v[1], t.z = v[2], t.w = v[3];
    *reinterpret_cast<f32x4*>(a) = t;
  }
};

// VEC pixels of one image per thread, every class of them in turn; STORE = the combined map is wanted (then all C classes are formed,
// else only the n_used the label needs, from registers)
template <int VEC, bool NMS, bool STORE>
__global__ __launch_bounds__(256) void ensemble_probs_kernel(EnsembleMaps maps, int K, float* __restrict__ out,
                                                             uint8_t* __restrict__ labels, int n_used, int C, int64_t HW) {
  const int n = blockIdx.y;
  const int64_t groups = HW / VEC;
  const int cs = STORE ? C : n_used;
  const float kf = (float)K;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
    float best[VEC];
    int bi[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) best[j] = 0.0f, bi[j] = 0;
    for (int c = 0; c < cs; ++c) {
      const size_t off = ((size_t)n * C + c) * (size_t)HW + (size_t)g * VEC;
      Px<VEC> acc, t;
      t.load(maps.p[0] + off);
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc.v[j] = NMS ? t.v[j] : 0.0f + t.v[j];
#pragma unroll 4  // four members' loads in flight before the first add: 0.161 against 0.228 ms per image at K = 16, nothing at K = 3
      for (int k = 1; k < K; ++k) {
        t.load(maps.p[k] + off);
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc.v[j] = NMS ? ((acc.v[j] > t.v[j] || acc.v[j] != acc.v[j]) ? acc.v[j] : t.v[j]) : acc.v[j] + t.v[j];
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float a = NMS ? acc.v[j] : acc.v[j] / kf;
        a = a != a ? __builtin_bit_cast(float, 0x7FC00000u) : a;
        acc.v[j] = a;
        if (c == 0) {
          best[j] = a;
        } else if (c < n_used && best[j] == best[j] && (a > best[j] || a != a)) {
          best[j] = a, bi[j] = c;
        }
      }
      if (STORE) acc.store(out + off);
    }
    uint8_t* l = labels + (size_t)n * (size_t)HW + (size_t)g * VEC;
    if (VEC == 4) {
      *reinterpret_cast<uint32_t*>(l) = (uint32_t)bi[0] | ((uint32_t)bi[1] << 8) | ((uint32_t)bi[2] << 16) | ((uint32_t)bi[3] << 24);
    } else {
      l[0] = (uint8_t)bi[0];
    }
  }
}

__global__ __launch_bounds__(256) void label_resize_colorize_kernel(const uint8_t* __restrict__ src, const int* __restrict__ ix,
                                                                    const int* __restrict__ iy, const uint8_t* __restrict__ palette,
                                                                    int n_pal, uint8_t* __restrict__ label_out, uint8_t* __restrict__ vis,
                                                                    int N, int H, int W, int OH, int OW) {
  const int64_t total = (int64_t)N * OH * OW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % OW);
    const int64_t r = i / OW;
    const int y = (int)(r % OH), n = (int)(r / OH);
    const int l = src[((size_t)n * H + iy[y]) * W + ix[x]];
    if (label_out) label_out[i] = (uint8_t)l;
    if (vis) {
      const bool in = l < n_pal;
      vis[3 * i + 0] = in ? palette[3 * l + 0] : (uint8_t)0;
      vis[3 * i + 1] = in ? palette[3 * l + 1] : (uint8_t)0;
      vis[3 * i + 2] = in ? palette[3 * l + 2] : (uint8_t)0;
    }
  }
}

template <int VEC, bool NMS>
void launch_ensemble(const EnsembleMaps& maps, int K, float* out, uint8_t* labels, int n_used, int N, int C, int64_t HW, hipStream_t st) {
  const dim3 grid((unsigned)ceil_div64(HW / VEC, 256, 4096), (unsigned)N);
  if (out)
    hipLaunchKernelGGL((ensemble_probs_kernel<VEC, NMS, true>), grid, dim3(256), 0, st, maps, K, out, labels, n_used, C, HW);
  else
    hipLaunchKernelGGL((ensemble_probs_kernel<VEC, NMS, false>), grid, dim3(256), 0, st, maps, K, out, labels, n_used, C, HW);
}

}  // namespace

extern "C" int mcdseg_ensemble_probs(const float* const* maps, int32_t K, int32_t method, float* out, uint8_t* labels, int32_t n_used,
                                     int32_t N, int32_t C, int32_t H, int32_t W, void* stream) {
  MCD_REQUIRE(maps && labels, "ensemble_probs: null pointer");
  MCD_REQUIRE(K >= 2 && K <= MCDSEG_ENSEMBLE_MAX_K, "ensemble_probs: K = %d maps, outside [2, %d]", K, MCDSEG_ENSEMBLE_MAX_K);
  MCD_REQUIRE(method == MCDSEG_ENSEMBLE_AVERAGING || method == MCDSEG_ENSEMBLE_NMS, "ensemble_probs: unknown method %d", method);
  MCD_REQUIRE(N > 0 && N <= 65535 && C > 0 && H > 0 && W > 0, "ensemble_probs: bad dims");
  MCD_REQUIRE(n_used >= 1 && n_used <= C && n_used <= 256, "ensemble_probs: n_used = %d outside [1, min(C = %d, 256)]", n_used, C);
  const int64_t HW = (int64_t)H * W;
  MCD_REQUIRE(HW < ((int64_t)1 << 31) && (int64_t)N * C * HW < ((int64_t)1 << 40), "ensemble_probs: maps too large");
  EnsembleMaps m;
  uintptr_t bits = reinterpret_cast<uintptr_t>(out);  // (a null `out` adds nothing)
  for (int k = 0; k < MCDSEG_ENSEMBLE_MAX_K; ++k) {
    m.p[k] = k < K ? maps[k] : nullptr;
    MCD_REQUIRE(k >= K || m.p[k], "ensemble_probs: map %d is null", k);
    bits |= reinterpret_cast<uintptr_t>(m.p[k]);
  }
  MCD_REQUIRE((bits & 3) == 0, "ensemble_probs: a map or out is not 4-byte aligned");
  bits |= reinterpret_cast<uintptr_t>(labels);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = W % 4 == 0 && (bits & 15) == 0;  // (then H*W % 4 == 0 and every row of four pixels, labels included, is aligned)
  const bool nms = method == MCDSEG_ENSEMBLE_NMS;
  if (vec && nms) launch_ensemble<4, true>(m, K, out, labels, n_used, N, C, HW, st);
  else if (vec) launch_ensemble<4, false>(m, K, out, labels, n_used, N, C, HW, st);
  else if (nms) launch_ensemble<1, true>(m, K, out, labels, n_used, N, C, HW, st);
  else launch_ensemble<1, false>(m, K, out, labels, n_used, N, C, HW, st);
  MCD_LAUNCH_CHECK("ensemble_probs");
  return 0;
}

extern "C" size_t mcdseg_label_resize_colorize_workspace_bytes(int32_t OH, int32_t OW) {
  return OH > 0 && OW > 0 ? ((size_t)OH + (size_t)OW) * sizeof(int) : 0;
}

extern "C" int mcdseg_label_resize_colorize(const uint8_t* labels, const uint8_t* palette, int32_t n_pal, uint8_t* label_out,
                                            uint8_t* vis_out, int32_t N, int32_t H, int32_t W, int32_t OH, int32_t OW, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(labels && workspace, "label_resize_colorize: null pointer");
  MCD_REQUIRE(label_out || vis_out, "label_resize_colorize: no output");
  MCD_REQUIRE(!vis_out || (palette && n_pal >= 1 && n_pal <= 256), "label_resize_colorize: vis needs a palette of 1..256 colours");
  MCD_REQUIRE(N > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "label_resize_colorize: bad dims");
  MCD_REQUIRE((int64_t)N * H * W < ((int64_t)1 << 40) && (int64_t)N * OH * OW < ((int64_t)1 << 40), "label_resize_colorize: maps too large");
  MCD_REQUIRE(workspace_bytes >= mcdseg_label_resize_colorize_workspace_bytes(OH, OW), "label_resize_colorize: workspace too small");
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "label_resize_colorize: workspace must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int* ix = (int*)workspace;
  int* iy = ix + OW;
  hipLaunchKernelGGL(nearest_index_kernel, dim3(1), dim3(64), 0, st, W, OW, ix);
  hipLaunchKernelGGL(nearest_index_kernel, dim3(1), dim3(64), 0, st, H, OH, iy);
  hipLaunchKernelGGL(label_resize_colorize_kernel, dim3((unsigned)ceil_div64((int64_t)N * OH * OW, 256, 8192)), dim3(256), 0, st, labels, ix,
                     iy, palette, n_pal, label_out, vis_out, N, H, W, OH, OW);
  MCD_LAUNCH_CHECK("label_resize_colorize");
  return 0;
}
