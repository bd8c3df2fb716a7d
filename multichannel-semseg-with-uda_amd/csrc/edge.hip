// The edge maps of the reference's tools/edge_detect.py:33-53 -- what sample_scripts/refine_seg_by_boundary.sh:6 refines label maps by
// (BOUNDARY_DIR = .../edges/canny) -- on the device: the luma plane, cv2.Laplacian + 128, the Sobel magnitude and cv2.Canny (aperture 3,
// L1 gradient) of 8-bit RGB images.  The definition is OpenCV's PUBLISHED 8-bit algorithm as DESIGN.md section 4.15 states it; all of
// it is integer arithmetic and tests/edge_ref.py is its yardstick, bit for bit.  No OpenCV build was at hand: byte equality with a
// particular OpenCV build is neither claimed nor tested.
//
// edge_maps -- ONE launch for whatever is asked; one workgroup per 32 x 32 tile (the geometry of refine_tile_kernel):
//     stage    the luma Y = (4899 R + 9617 G + 1868 B + 8192) >> 14 of the tile plus a 2-pixel ring goes to LDS -- IN-IMAGE pixels
//              only.  The ring serves two border rules at once: the Laplacian and the Sobel map read a neighbour outside the image by
//              BORDER_REFLECT_101 (-1 -> 1, L -> L - 2; a dimension of length 1 -> 0), Canny's gradient by BORDER_REPLICATE.  So no
//              staged value stands for an off-image position: a neighbour's COORDINATE is mapped by the rule of the map being formed
//              when it is read, and the mapped coordinate always lies inside the staged window (|offset| <= 1 from a pixel of the tile
//              or of its 1-pixel ring).  Rows of 3-byte pixels start at any byte alignment, so the pixels are fetched as bytes;
//              neighbouring lanes fetch neighbouring bytes.
//     mag      |dx| + |dy| (REPLICATE) of the tile plus a 1-pixel ring goes to LDS; a ring position OUTSIDE the image holds 0, not
//              the gradient of replicated pixels
//     emit     luma, Laplacian, Sobel, and Canny's classes after the non-maximum suppression: 0 / 1 (weak) / 2 (strong)
//
// canny_hysteresis -- an edge is a candidate (class 1 or 2) whose 8-connected component of candidates holds a class 2 pixel: connected
// components by the union-find of csrc/union_find.h, in the five passes of boundary_regions (csrc/refine.hip):
//     tile     one workgroup per 32 x 32 tile: union-find in LDS over the candidates; each pixel leaves with the global index of its
//              tile-local root (a pixel that is no candidate with its own index)
//     seam     every pair of candidates that straddles a tile border, the four corner diagonals included, unions the two global
//              trees; agent-scope atomics only
//     flatten  every pixel chases to its root and stores it
//     mark     every class 2 pixel stores -1 at its root
//     emit     255 where a candidate's root holds -1, else 0
// Passes hand over through kernel boundaries only.  Roots are the smallest row-major index of a component, marks are idempotent
// stores: the same bits run to run.  An image of one tile needs no seam and no flatten pass.
#include "common.h"
#include "union_find.h"

namespace {

constexpr int ED_TILE = 32;                // tile edge
constexpr int ED_TILE_PIX = ED_TILE * ED_TILE;
constexpr int ED_YW = ED_TILE + 4;         // the staged luma window: the tile and a 2-pixel ring
constexpr int ED_MW = ED_TILE + 2;         // the magnitude window: the tile and a 1-pixel ring

__device__ __forceinline__ int ed_reflect101(int i, int L) {  // for i in [-1, L]
  if (L == 1) return 0;
  return i < 0 ? -i : (i >= L ? 2 * L - 2 - i : i);
}

__device__ __forceinline__ int ed_replicate(int i, int L) { return i < 0 ? 0 : (i >= L ? L - 1 : i); }

struct EdgeTile {
  const uint8_t* y;  // the staged window
  int y0, x0;        // image coordinates of its first element
  __device__ __forceinline__ int at(int gy, int gx) const { return y[(gy - y0) * ED_YW + (gx - x0)]; }  // (gy, gx) inside the image
};

// the 3 x 3 Sobel pair at (gy, gx): rows / columns -1, 0, +1 already mapped into the image by the caller's border rule
__device__ __forceinline__ void ed_sobel(const EdgeTile& t, const int ry[3], const int rx[3], int* dx, int* dy) {
  const int a = t.at(ry[0], rx[0]), b = t.at(ry[0], rx[1]), c = t.at(ry[0], rx[2]);
  const int d = t.at(ry[1], rx[0]), f = t.at(ry[1], rx[2]);
  const int g = t.at(ry[2], rx[0]), h = t.at(ry[2], rx[1]), i = t.at(ry[2], rx[2]);
  *dx = (c - a) + 2 * (f - d) + (i - g);
  *dy = (g - a) + 2 * (h - b) + (i - c);
}

__device__ __forceinline__ void ed_canny_grad(const EdgeTile& t, int gy, int gx, int H, int W, int* dx, int* dy) {
  const int ry[3] = {ed_replicate(gy - 1, H), gy, ed_replicate(gy + 1, H)};
  const int rx[3] = {ed_replicate(gx - 1, W), gx, ed_replicate(gx + 1, W)};
  ed_sobel(t, ry, rx, dx, dy);
}

__device__ __forceinline__ int ed_abs(int v) { return v < 0 ? -v : v; }

// floor(sqrt(s)) for 0 <= s <= 2 * 1020^2: sqrtf is exact enough over the whole range, the one-step correction stays anyway
__device__ __forceinline__ int ed_isqrt(int s) {
  int r = (int)sqrtf((float)s);
  if (r * r > s) --r;
  if ((r + 1) * (r + 1) <= s) ++r;
  return r;
}

__global__ __launch_bounds__(256) void edge_maps_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ luma,
                                                        uint8_t* __restrict__ laplacian, uint8_t* __restrict__ sobel,
                                                        uint8_t* __restrict__ canny_cls, int low, int high, int H, int W) {
  __shared__ uint8_t ybuf[ED_YW * ED_YW];
  __shared__ uint16_t mag[ED_MW * ED_MW];  // at most 2 * 1020
  const size_t img = (size_t)blockIdx.z * H * W;
  const int x0 = blockIdx.x * ED_TILE, y0 = blockIdx.y * ED_TILE;
  const EdgeTile t = {ybuf, y0 - 2, x0 - 2};
  for (int i = threadIdx.x; i < ED_YW * ED_YW; i += blockDim.x) {
    const int gy = t.y0 + i / ED_YW, gx = t.x0 + i % ED_YW;
    int v = 0;  // off-image: never read
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const uint8_t* p = rgb + (img + (size_t)gy * W + gx) * 3;
      v = (4899 * (int)p[0] + 9617 * (int)p[1] + 1868 * (int)p[2] + 8192) >> 14;
    }
    ybuf[i] = (uint8_t)v;
  }
  __syncthreads();
  if (canny_cls) {
    for (int i = threadIdx.x; i < ED_MW * ED_MW; i += blockDim.x) {
      const int gy = y0 - 1 + i / ED_MW, gx = x0 - 1 + i % ED_MW;
      int m = 0;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        int dx, dy;
        ed_canny_grad(t, gy, gx, H, W, &dx, &dy);
        m = ed_abs(dx) + ed_abs(dy);
      }
      mag[i] = (uint16_t)m;
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < ED_TILE_PIX; i += blockDim.x) {
    const int ly = i / ED_TILE, lx = i % ED_TILE;
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy >= H || gx >= W) continue;
    const size_t o = img + (size_t)gy * W + gx;
    if (luma) luma[o] = (uint8_t)t.at(gy, gx);
    if (laplacian || sobel) {
      const int ry[3] = {ed_reflect101(gy - 1, H), gy, ed_reflect101(gy + 1, H)};
      const int rx[3] = {ed_reflect101(gx - 1, W), gx, ed_reflect101(gx + 1, W)};
      if (laplacian) {
        const int v = t.at(ry[0], gx) + t.at(ry[2], gx) + t.at(gy, rx[0]) + t.at(gy, rx[2]) - 4 * t.at(gy, gx) + 128;
        laplacian[o] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
      }
      if (sobel) {
        int dx, dy;
        ed_sobel(t, ry, rx, &dx, &dy);
        const int r = ed_isqrt(dx * dx + dy * dy);
        sobel[o] = (uint8_t)(r > 255 ? 255 : r);
      }
    }
    if (canny_cls) {
      const uint16_t* mc = mag + (ly + 1) * ED_MW + (lx + 1);
      const int m = mc[0];
      int cls = 0;
      if (m > low) {
        int dx, dy;
        ed_canny_grad(t, gy, gx, H, W, &dx, &dy);
        const int x = ed_abs(dx), y = ed_abs(dy) << 15;
        const int t22 = x * 13573, t67 = t22 + (x << 16);
        bool keep;
        if (y < t22) {
          keep = m > mc[-1] && m >= mc[1];
        } else if (y > t67) {
          keep = m > mc[-ED_MW] && m >= mc[ED_MW];
        } else {
          const int s = (dx ^ dy) < 0 ? -1 : 1;
          keep = m > mc[-ED_MW - s] && m > mc[ED_MW + s];
        }
        if (keep) cls = m > high ? 2 : 1;
      }
      canny_cls[o] = (uint8_t)cls;
    }
  }
}

__device__ __forceinline__ bool ed_cand(int c) { return c == 1 || c == 2; }

__global__ __launch_bounds__(256) void canny_tile_kernel(const uint8_t* __restrict__ cls, int* __restrict__ labels, int H, int W) {
  __shared__ int lab[ED_TILE_PIX];
  __shared__ uint8_t cand[ED_TILE_PIX];  // 1 = a candidate inside the image
  const size_t img = (size_t)blockIdx.z * H * W;
  const int x0 = blockIdx.x * ED_TILE, y0 = blockIdx.y * ED_TILE;
  for (int i = threadIdx.x; i < ED_TILE_PIX; i += blockDim.x) {
    const int gy = y0 + i / ED_TILE, gx = x0 + i % ED_TILE;
    cand[i] = (gy < H && gx < W) ? (uint8_t)ed_cand(cls[img + (size_t)gy * W + gx]) : (uint8_t)0;
    lab[i] = i;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ED_TILE_PIX; i += blockDim.x) {
    if (!cand[i]) continue;
    const int ly = i / ED_TILE, lx = i % ED_TILE;
    if (lx > 0 && cand[i - 1]) rf_union_lds(lab, i, i - 1);
    if (ly > 0) {
      if (cand[i - ED_TILE]) rf_union_lds(lab, i, i - ED_TILE);
      if (lx > 0 && cand[i - ED_TILE - 1]) rf_union_lds(lab, i, i - ED_TILE - 1);
      if (lx < ED_TILE - 1 && cand[i - ED_TILE + 1]) rf_union_lds(lab, i, i - ED_TILE + 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ED_TILE_PIX; i += blockDim.x) {
    const int gy = y0 + i / ED_TILE, gx = x0 + i % ED_TILE;
    if (gy >= H || gx >= W) continue;
    const int r = rf_find_lds(lab, i);  // a pixel that is no candidate was never linked: its own index
    labels[img + (size_t)gy * W + gx] = (y0 + r / ED_TILE) * W + (x0 + r % ED_TILE);
  }
}

// one thread per pixel; a candidate on a seam looks at its left, upper and two upper diagonal neighbours across the tile border
__global__ __launch_bounds__(256) void canny_seam_kernel(const uint8_t* __restrict__ cls, int* labels, int H, int W) {
  const int HW = H * W;
  const uint8_t* c = cls + (size_t)blockIdx.y * HW;
  int* label = labels + (size_t)blockIdx.y * HW;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < HW; q += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)q;
    const int y = p / W, x = p - y * W;
    const bool left_seam = x % ED_TILE == 0, up_seam = y % ED_TILE == 0, right_seam = x % ED_TILE == ED_TILE - 1;
    if (!(left_seam || up_seam || right_seam) || !ed_cand(c[p])) continue;
    if (left_seam && x > 0 && ed_cand(c[p - 1])) rf_union(label, p, p - 1);
    if (y > 0) {
      if (up_seam && ed_cand(c[p - W])) rf_union(label, p, p - W);
      if ((left_seam || up_seam) && x > 0 && ed_cand(c[p - W - 1])) rf_union(label, p, p - W - 1);
      if ((right_seam || up_seam) && x < W - 1 && ed_cand(c[p - W + 1])) rf_union(label, p, p - W + 1);
    }
  }
}

__global__ __launch_bounds__(256) void canny_flatten_kernel(int* labels, int HW) {
  int* label = labels + (size_t)blockIdx.y * HW;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < HW; q += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)q;
    const int r = rf_find(label, p);  // a root's entry never changes in this pass; any other entry read is an ancestor, old or new
    if (r != p) rf_store(label + p, r);
  }
}

__global__ __launch_bounds__(256) void canny_mark_kernel(const uint8_t* __restrict__ cls, int* labels, int HW) {
  const uint8_t* c = cls + (size_t)blockIdx.y * HW;
  int* label = labels + (size_t)blockIdx.y * HW;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < HW; q += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)q;
    if (c[p] != 2) continue;
    const int r = rf_load(label + p);  // its root, or -1 where p is a root that another thread has marked already
    if (r >= 0) rf_store(label + r, -1);
  }
}

// roots are not written here, and a pixel that is not a root holds its root's index since the flatten pass
__global__ __launch_bounds__(256) void canny_emit_kernel(const uint8_t* __restrict__ cls, const int* __restrict__ labels,
                                                         uint8_t* __restrict__ edges, int HW) {
  const size_t img = (size_t)blockIdx.y * HW;
  const int* label = labels + img;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < HW; q += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)q;
    bool edge = false;
    if (ed_cand(cls[img + p])) {
      const int r = label[p];
      edge = r < 0 || (r != p && label[r] < 0);
    }
    edges[img + p] = edge ? (uint8_t)255 : (uint8_t)0;
  }
}

// the bounds of rf_check_dims (csrc/refine.hip)
int ed_check_dims(const char* what, int N, int H, int W) {
  MCD_REQUIRE(N > 0 && H > 0 && W > 0, "%s: bad dims", what);
  MCD_REQUIRE((int64_t)N * H * W < (1ll << 31), "%s: N*H*W must fit 32 bits", what);
  MCD_REQUIRE(N <= 65535, "%s: at most 65535 images per call", what);
  MCD_REQUIRE(ceil_div(H, ED_TILE) <= 65535, "%s: image too tall", what);
  return 0;
}

int ed_blocks(int HW) {
  const int b = ceil_div(HW, 256);
  return b > 4096 ? 4096 : b;
}

}  // namespace

extern "C" int mcdseg_edge_maps(const uint8_t* rgb, uint8_t* luma, uint8_t* laplacian, uint8_t* sobel, uint8_t* canny_cls, int32_t low,
                                int32_t high, int32_t N, int32_t H, int32_t W, void* stream) {
  MCD_REQUIRE(rgb, "edge_maps: null rgb");
  MCD_REQUIRE(luma || laplacian || sobel || canny_cls, "edge_maps: no output asked for");
  if (int rc = ed_check_dims("edge_maps", N, H, W)) return rc;
  if (canny_cls && low > high) { const int32_t t = low; low = high; high = t; }
  hipLaunchKernelGGL(edge_maps_kernel, dim3(ceil_div(W, ED_TILE), ceil_div(H, ED_TILE), N), dim3(256), 0, (hipStream_t)stream, rgb, luma,
                     laplacian, sobel, canny_cls, low, high, H, W);
  MCD_LAUNCH_CHECK("edge_maps");
  return 0;
}

extern "C" size_t mcdseg_canny_hysteresis_workspace_bytes(int32_t N, int32_t H, int32_t W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * H * W * sizeof(int);
}

extern "C" int mcdseg_canny_hysteresis(const uint8_t* cls, uint8_t* edges, int32_t N, int32_t H, int32_t W, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  MCD_REQUIRE(cls && edges, "canny_hysteresis: null pointer");
  MCD_REQUIRE(cls != edges, "canny_hysteresis: edges must not be cls (the passes read cls after edges is written)");
  if (int rc = ed_check_dims("canny_hysteresis", N, H, W)) return rc;
  MCD_REQUIRE(workspace, "canny_hysteresis: null workspace");
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "canny_hysteresis: workspace must be 4-byte aligned");
  MCD_REQUIRE(workspace_bytes >= mcdseg_canny_hysteresis_workspace_bytes(N, H, W),
              "canny_hysteresis: workspace too small (%zu bytes, mcdseg_canny_hysteresis_workspace_bytes asks for %zu)", workspace_bytes,
              mcdseg_canny_hysteresis_workspace_bytes(N, H, W));
  const int tx = ceil_div(W, ED_TILE), ty = ceil_div(H, ED_TILE);
  hipStream_t st = (hipStream_t)stream;
  int* labels = (int*)workspace;
  const int HW = H * W;
  const dim3 grid(ed_blocks(HW), N);
  hipLaunchKernelGGL(canny_tile_kernel, dim3(tx, ty, N), dim3(256), 0, st, cls, labels, H, W);
  if (tx > 1 || ty > 1) {
    hipLaunchKernelGGL(canny_seam_kernel, grid, dim3(256), 0, st, cls, labels, H, W);
    hipLaunchKernelGGL(canny_flatten_kernel, grid, dim3(256), 0, st, labels, HW);
  }
  hipLaunchKernelGGL(canny_mark_kernel, grid, dim3(256), 0, st, cls, labels, HW);
  hipLaunchKernelGGL(canny_emit_kernel, grid, dim3(256), 0, st, cls, labels, edges, HW);
  MCD_LAUNCH_CHECK("canny_hysteresis");
  return 0;
}
