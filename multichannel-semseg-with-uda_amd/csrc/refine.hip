// "Postprocess using Boundary Detection output" of the reference (sample_scripts/refine_seg_by_boundary.sh:15-17), on the device:
//   * tools/binalize_boundary.py:9-20      m = b > thre, with a frame of ones around it
//   * tools/apply_bwboundary.m:10-15       bwboundaries(m): 8-connected objects, their holes labelled too, frame cropped off
//   * tools/refine_seg_by_bwboundary.py:31-42  every region of min_thre < pixels < max_thre (but the frame object, k != 1) takes the
//                                          most common label inside it
// All integer, no tolerance.  Two halves, separately usable:
//
// boundary_regions -- connected-component labelling by a lock-free union-find.  p and q are joined iff m[p] == m[q] and they are
// 4-adjacent, or diagonal neighbours with m == 1 (objects connect 8-wise, holes 4-wise: the duality of bwboundaries).  A pixel's
// parent is always a pixel of SMALLER row-major index of its component (a root points to itself), every link goes from the larger
// root to the smaller by an integer atomicMin, so the final root of a component is its smallest index whatever the schedule: the
// canonical id, bit-reproducible.  The label array is `regions` itself; nothing else is allocated.
//     tile     one workgroup per 32 x 32 tile: union-find in LDS, each pixel leaves with the global index of its tile-local root
//     seam     every adjacent pair that straddles a tile border (the corner diagonals included) unions the two global trees:
//              find, find, atomicMin(&label[larger root], smaller root), go on from the value returned.  Other workgroups rewrite
//              label[] meanwhile and a CU's L1 / another XCD's L2 are not refreshed by their stores, so EVERY access of this pass is
//              an agent-scope atomic; a retry strictly lowers a label, so the loop ends, and nobody waits for anybody
//     flatten  every pixel chases to its root and stores it
//     mark     every mask pixel of the image border writes -1 at its root (the frame object: whatever touches the frame of ones)
//     frame    every pixel whose root holds -1 becomes -1
// Passes hand over through kernel boundaries only.
//
// refine_labels_by_regions -- the vote, for ANY region map with ids in [-1, H*W) (an id outside is read as -1):
//     init     count[id] = 0, the vote table = {0, INT_MAX}
//     count    count[id] += pixels
//     compact  eligible ids (min_thre < count < max_thre) take a dense slot, count[id] becomes the slot or -1.  At most
//              H*W / (max(min_thre, 0) + 1) ids can be eligible, which is the table's size; a slot beyond it is refused, not written
//     vote     table[slot][label] = {pixels, first row-major index}
//     winner   per slot the label of most pixels, ties to the earliest first index (Counter.most_common()[0] on Python >= 3.7)
//     apply    out = winner[slot] where the pixel's id is eligible, else seg
// count and vote group the lanes of a wave by key (one ballot per distinct key of the wave) before the atomic: one same-address atomic
// per key and wave, not per pixel -- a region may put 79 000 pixels into one bin.  Integer add / min only: the result does not depend
// on the order of execution.  The slot NUMBERS do (an atomic counter hands them out), the output does not.
#include <limits.h>
#include "common.h"
#include "union_find.h"

namespace {

constexpr int RF_TILE = 32;                       // tile edge of the LDS pass
constexpr int RF_TILE_PIX = RF_TILE * RF_TILE;
constexpr int RF_BINS = 256;                      // one per uint8 label value

__global__ __launch_bounds__(256) void refine_tile_kernel(const uint8_t* __restrict__ boundary, int thre, int* __restrict__ regions, int H,
                                                          int W) {
  __shared__ int lab[RF_TILE_PIX];
  __shared__ uint8_t msk[RF_TILE_PIX];  // 0 / 1 = the mask, 2 = outside the image (equal to no pixel's mask)
  const size_t img = (size_t)blockIdx.z * H * W;
  const int x0 = blockIdx.x * RF_TILE, y0 = blockIdx.y * RF_TILE;
  for (int i = threadIdx.x; i < RF_TILE_PIX; i += blockDim.x) {
    const int gy = y0 + i / RF_TILE, gx = x0 + i % RF_TILE;
    msk[i] = (gy < H && gx < W) ? (uint8_t)((int)boundary[img + (size_t)gy * W + gx] > thre) : (uint8_t)2;
    lab[i] = i;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < RF_TILE_PIX; i += blockDim.x) {
    const int m = msk[i];
    if (m == 2) continue;
    const int ly = i / RF_TILE, lx = i % RF_TILE;
    if (lx > 0 && msk[i - 1] == m) rf_union_lds(lab, i, i - 1);
    if (ly > 0 && msk[i - RF_TILE] == m) rf_union_lds(lab, i, i - RF_TILE);
    if (m == 1 && ly > 0) {
      if (lx > 0 && msk[i - RF_TILE - 1] == 1) rf_union_lds(lab, i, i - RF_TILE - 1);
      if (lx < RF_TILE - 1 && msk[i - RF_TILE + 1] == 1) rf_union_lds(lab, i, i - RF_TILE + 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < RF_TILE_PIX; i += blockDim.x) {
    if (msk[i] == 2) continue;
    const int r = rf_find_lds(lab, i);  // the smallest local index of the component = its smallest global index inside the tile
    regions[img + (size_t)(y0 + i / RF_TILE) * W + (x0 + i % RF_TILE)] = (y0 + r / RF_TILE) * W + (x0 + r % RF_TILE);
  }
}

// one thread per pixel; it looks at its left, upper and (mask pixels) two upper diagonal neighbours and unions across a tile border
__global__ __launch_bounds__(256) void refine_seam_kernel(const uint8_t* __restrict__ boundary, int thre, int* regions, int H, int W) {
  const int HW = H * W;
  const uint8_t* b = boundary + (size_t)blockIdx.y * HW;
  int* label = regions + (size_t)blockIdx.y * HW;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < HW; q += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)q;
    const int y = p / W, x = p - y * W;
    const bool left_seam = x % RF_TILE == 0, up_seam = y % RF_TILE == 0, right_seam = x % RF_TILE == RF_TILE - 1;
    if (!(left_seam || up_seam || right_seam)) continue;
    const int m = (int)b[p] > thre;
    if (left_seam && x > 0 && ((int)b[p - 1] > thre) == m) rf_union(label, p, p - 1);
    if (up_seam && y > 0 && ((int)b[p - W] > thre) == m) rf_union(label, p, p - W);
    if (m == 1 && y > 0) {
      if ((left_seam || up_seam) && x > 0 && (int)b[p - W - 1] > thre) rf_union(label, p, p - W - 1);
      if ((right_seam || up_seam) && x < W - 1 && (int)b[p - W + 1] > thre) rf_union(label, p, p - W + 1);
    }
  }
}

__global__ __launch_bounds__(256) void refine_flatten_kernel(int* regions, int HW) {
  int* label = regions + (size_t)blockIdx.y * HW;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < HW; q += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)q;
    const int r = rf_find(label, p);  // a root's entry never changes in this pass; any other entry read is an ancestor, old or new
    if (r != p) rf_store(label + p, r);
  }
}

// the image border, one thread per border position (corners seen twice: the same store)
__global__ __launch_bounds__(256) void refine_mark_kernel(const uint8_t* __restrict__ boundary, int thre, int* regions, int H, int W) {
  const int HW = H * W;
  const uint8_t* b = boundary + (size_t)blockIdx.y * HW;
  int* label = regions + (size_t)blockIdx.y * HW;
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= 2 * ((int64_t)W + H)) return;
  int64_t p;
  if (i < W) p = i;
  else if (i < 2 * (int64_t)W) p = (int64_t)(H - 1) * W + (i - W);
  else if (i < 2 * (int64_t)W + H) p = (i - 2 * (int64_t)W) * W;
  else p = (i - 2 * (int64_t)W - H) * W + (W - 1);
  if (!((int)b[p] > thre)) return;
  const int r = rf_load(label + p);  // its root, or -1 where p is a root that another thread has marked already
  if (r >= 0) rf_store(label + r, -1);
}

// roots are not written here and nobody but its own thread reads a non-root's entry
__global__ __launch_bounds__(256) void refine_frame_kernel(int* regions, int HW) {
  int* label = regions + (size_t)blockIdx.y * HW;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < HW; q += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)q;
    const int r = label[p];
    if (r >= 0 && r != p && label[r] < 0) label[p] = -1;
  }
}

// ---- the vote ---------------------------------------------------------------------------------------------------------------

// Groups the lanes of a wave that hold equal (a, b), adjacent or not: true on the lowest lane of each group, *n = the group's size.
// Lanes with valid == false belong to no group.  Every lane of the wave must call; the loop runs once per distinct key of the wave
// (wave-uniform: ballots live in scalar registers).  Equality along a row is not enough: where one-pixel walls and corridors
// alternate, every lane is a run of its own and a run-length rule would issue one atomic per pixel after all.
__device__ __forceinline__ bool rf_group_head(int a, int b, bool valid, int* n) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  bool head = false;
  *n = 0;
  while (todo) {
    const int leader = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(todo));
    const int la = __builtin_amdgcn_readlane(a, leader), lb = __builtin_amdgcn_readlane(b, leader);
    const unsigned long long same = __ballot(valid && a == la && b == lb);
    if (lane == leader) {
      head = true;
      *n = __popcll(same);
    }
    todo &= ~same;
  }
  return head;
}

struct RefineWs {
  int* count;      // [N][HW]   pixels per id, then the id's slot or -1
  int* used;       // [N]       slots handed out
  uint8_t* winner; // [N][slots]
  int* table;      // [N][slots][256][2]  {pixels, first index}
};

__global__ __launch_bounds__(256) void refine_init_kernel(RefineWs ws, int64_t counts, int N, int64_t bins) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < counts; i += stride) ws.count[i] = 0;
  for (int64_t i = t0; i < N; i += stride) ws.used[i] = 0;
  for (int64_t i = t0; i < bins; i += stride) {
    ws.table[2 * i] = 0;
    ws.table[2 * i + 1] = INT_MAX;
  }
}

__global__ __launch_bounds__(256) void refine_count_kernel(const int32_t* __restrict__ regions, RefineWs ws, int HW) {
  const int32_t* reg = regions + (size_t)blockIdx.y * HW;
  int* count = ws.count + (size_t)blockIdx.y * HW;
  const int64_t per_round = (int64_t)gridDim.x * blockDim.x;
  const int rounds = (int)((HW + per_round - 1) / per_round);  // whole waves stay in the loop together
  for (int k = 0; k < rounds; ++k) {
    const int64_t p = k * per_round + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int r = p < HW ? reg[p] : -1;
    if (r >= HW) r = -1;
    int len;
    if (rf_group_head(r, 0, r >= 0, &len)) atomicAdd(count + r, len);
  }
}

__global__ __launch_bounds__(256) void refine_compact_kernel(RefineWs ws, int HW, int min_thre, int max_thre, int slots) {
  int* count = ws.count + (size_t)blockIdx.y * HW;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < HW; q += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)q;
    const int c = count[r];
    int slot = -1;
    if (c > min_thre && c < max_thre) {
      slot = atomicAdd(ws.used + blockIdx.y, 1);
      if (slot >= slots) slot = -1;  // (cannot happen: `slots` is the most ids that can be eligible)
    }
    count[r] = slot;
  }
}

__global__ __launch_bounds__(256) void refine_vote_kernel(const uint8_t* __restrict__ seg, const int32_t* __restrict__ regions, RefineWs ws,
                                                          int HW, int slots) {
  const int32_t* reg = regions + (size_t)blockIdx.y * HW;
  const uint8_t* s = seg + (size_t)blockIdx.y * HW;
  const int* slot_of = ws.count + (size_t)blockIdx.y * HW;
  int* table = ws.table + (size_t)blockIdx.y * slots * RF_BINS * 2;
  const int64_t per_round = (int64_t)gridDim.x * blockDim.x;
  const int rounds = (int)((HW + per_round - 1) / per_round);
  for (int k = 0; k < rounds; ++k) {
    const int64_t p = k * per_round + blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int slot = -1, v = 0;
    if (p < HW) {
      const int r = reg[p];
      if (r >= 0 && r < HW) slot = slot_of[r];
      v = s[p];
    }
    int len;
    if (rf_group_head(slot, v, slot >= 0, &len)) {
      int* bin = table + ((size_t)slot * RF_BINS + v) * 2;
      atomicAdd(bin, len);
      atomicMin(bin + 1, (int)p);  // the head is the group's lowest lane: its smallest index
    }
  }
}

// one workgroup per slot, one thread per label value: most pixels, then the earliest first index
__global__ __launch_bounds__(RF_BINS) void refine_winner_kernel(RefineWs ws, int slots) {
  __shared__ unsigned long long best[RF_BINS / 64];
  const int slot = blockIdx.x;
  if (slot >= ws.used[blockIdx.y] || slot >= slots) return;  // (uniform per workgroup)
  const int* bin = ws.table + (((size_t)blockIdx.y * slots + slot) * RF_BINS + threadIdx.x) * 2;
  const int c = bin[0], first = bin[1];
  // an empty bin is key 0; first indices of non-empty bins are different pixels, so non-empty keys are distinct
  const unsigned long long key = ((unsigned long long)(unsigned)c << 32) | (unsigned)(INT_MAX - first);
  unsigned long long m = key;
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_xor(m, d);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0) best[threadIdx.x >> 6] = m;
  __syncthreads();
  for (int w = 0; w < RF_BINS / 64; ++w) m = best[w] > m ? best[w] : m;
  if (c > 0 && key == m) ws.winner[(size_t)blockIdx.y * slots + slot] = (uint8_t)threadIdx.x;
}

__global__ __launch_bounds__(256) void refine_apply_kernel(const uint8_t* __restrict__ seg, const int32_t* __restrict__ regions,
                                                           uint8_t* __restrict__ out, RefineWs ws, int HW, int slots) {
  const size_t img = (size_t)blockIdx.y * HW;
  const int* slot_of = ws.count + img;
  const uint8_t* winner = ws.winner + (size_t)blockIdx.y * slots;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < HW; q += (int64_t)gridDim.x * blockDim.x) {
    const int p = (int)q;
    const int r = regions[img + p];
    const int slot = (r >= 0 && r < HW) ? slot_of[r] : -1;
    out[img + p] = slot >= 0 ? winner[slot] : seg[img + p];
  }
}

int64_t rf_slots(int64_t HW, int min_thre) { return HW / ((int64_t)(min_thre > 0 ? min_thre : 0) + 1); }

size_t rf_pad16(size_t b) { return (b + 15) & ~(size_t)15; }

int rf_check_dims(const char* what, int N, int H, int W) {
  MCD_REQUIRE(N > 0 && H > 0 && W > 0, "%s: bad dims", what);
  MCD_REQUIRE((int64_t)N * H * W < (1ll << 31), "%s: N*H*W must fit 32 bits", what);
  MCD_REQUIRE(N <= 65535, "%s: at most 65535 images per call", what);
  return 0;
}

int rf_blocks(int HW) {
  const int b = ceil_div(HW, 256);
  return b > 4096 ? 4096 : b;
}

}  // namespace

extern "C" size_t mcdseg_refine_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t min_thre) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  const int64_t HW = (int64_t)H * W, slots = rf_slots(HW, min_thre);
  return rf_pad16((size_t)N * HW * sizeof(int)) + rf_pad16((size_t)N * sizeof(int)) + rf_pad16((size_t)N * slots) +
         (size_t)N * slots * RF_BINS * 2 * sizeof(int);
}

extern "C" int mcdseg_boundary_regions(const uint8_t* boundary, int32_t thre, int32_t* regions, int32_t N, int32_t H, int32_t W, void* ws,
                                       size_t ws_bytes, void* stream) {
  (void)ws, (void)ws_bytes;  // the labels are resolved inside `regions`
  MCD_REQUIRE(boundary && regions, "boundary_regions: null pointer");
  if (int rc = rf_check_dims("boundary_regions", N, H, W)) return rc;
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(regions) & 3) == 0, "boundary_regions: regions must be 4-byte aligned");
  const int tx = ceil_div(W, RF_TILE), ty = ceil_div(H, RF_TILE);
  MCD_REQUIRE(ty <= 65535, "boundary_regions: image too tall");
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  const dim3 grid(rf_blocks(HW), N);
  hipLaunchKernelGGL(refine_tile_kernel, dim3(tx, ty, N), dim3(256), 0, st, boundary, thre, regions, H, W);
  if (tx > 1 || ty > 1) {
    hipLaunchKernelGGL(refine_seam_kernel, grid, dim3(256), 0, st, boundary, thre, regions, H, W);
    hipLaunchKernelGGL(refine_flatten_kernel, grid, dim3(256), 0, st, regions, HW);
  }
  hipLaunchKernelGGL(refine_mark_kernel, dim3((unsigned)ceil_div64(2 * ((int64_t)W + H), 256), N), dim3(256), 0, st, boundary, thre, regions, H, W);
  hipLaunchKernelGGL(refine_frame_kernel, grid, dim3(256), 0, st, regions, HW);
  MCD_LAUNCH_CHECK("boundary_regions");
  return 0;
}

extern "C" int mcdseg_refine_labels_by_regions(const uint8_t* seg, const int32_t* regions, uint8_t* out, int32_t N, int32_t H, int32_t W,
                                               int32_t min_thre, int32_t max_thre, void* ws, size_t ws_bytes, void* stream) {
  MCD_REQUIRE(seg && regions && out && ws, "refine_labels_by_regions: null pointer");
  if (int rc = rf_check_dims("refine_labels_by_regions", N, H, W)) return rc;
  MCD_REQUIRE(ws_bytes >= mcdseg_refine_workspace_bytes(N, H, W, min_thre),
              "refine_labels_by_regions: workspace too small (%zu bytes, mcdseg_refine_workspace_bytes asks for %zu)", ws_bytes,
              mcdseg_refine_workspace_bytes(N, H, W, min_thre));
  MCD_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3) == 0 && (reinterpret_cast<uintptr_t>(regions) & 3) == 0,
              "refine_labels_by_regions: workspace and regions must be 4-byte aligned");
  const int HW = H * W;
  const int64_t slots64 = rf_slots(HW, min_thre);
  const int slots = (int)slots64;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(rf_blocks(HW), N);
  if (slots == 0) {  // min_thre >= H*W: no region can be eligible
    if (out != seg) (void)hipMemcpyAsync(out, seg, (size_t)N * HW, hipMemcpyDeviceToDevice, st);
    return 0;
  }
  RefineWs w;
  char* base = (char*)ws;
  w.count = (int*)base;
  base += rf_pad16((size_t)N * HW * sizeof(int));
  w.used = (int*)base;
  base += rf_pad16((size_t)N * sizeof(int));
  w.winner = (uint8_t*)base;
  base += rf_pad16((size_t)N * slots);
  w.table = (int*)base;
  const int64_t counts = (int64_t)N * HW, bins = (int64_t)N * slots * RF_BINS;
  int64_t ib = ceil_div64(counts > bins ? counts : bins, 256);
  if (ib > 8192) ib = 8192;
  hipLaunchKernelGGL(refine_init_kernel, dim3((unsigned)ib), dim3(256), 0, st, w, counts, N, bins);
  hipLaunchKernelGGL(refine_count_kernel, grid, dim3(256), 0, st, regions, w, HW);
  hipLaunchKernelGGL(refine_compact_kernel, grid, dim3(256), 0, st, w, HW, min_thre, max_thre, slots);
  hipLaunchKernelGGL(refine_vote_kernel, grid, dim3(256), 0, st, seg, regions, w, HW, slots);
  // the number of slots in use lives on the device: one workgroup per POSSIBLE slot, the unused ones leave at once
  hipLaunchKernelGGL(refine_winner_kernel, dim3(slots, N), dim3(RF_BINS), 0, st, w, slots);
  hipLaunchKernelGGL(refine_apply_kernel, grid, dim3(256), 0, st, seg, regions, out, w, HW, slots);
  MCD_LAUNCH_CHECK("refine_labels_by_regions");
  return 0;
}
