// Label-map post-processing of the reference's get_post_transforms (src/definer.py:679-694) on the GPU: the two steps
// behind --cleaning_areas and --replace_value (src/arguments_inference.py:61-70), applied by Engine.evaluate to the
// thresholded ensemble mean (learning/engine.py:244-259).  Labels are uint8 [N][D][H][W], one sample at a time,
// worked on in place; every decision is taken on the device (no host synchronisation, no allocation).
//
// cc_*   KeepLargestConnectedComponent / get_largest_component (utils/transforms.py:209-230,579-600): 26-connected
//        components of labels != 0 by union-find over flat voxel indices.  parent[i] <= i always holds and only ever
//        decreases (links and path compression are device-scope atomicMin), so every value a load returns -- however
//        stale -- is an ancestor and each root is its component's smallest index.  Each workgroup labels its
//        8 x 8 x 32 brick in LDS first, so the global pass only merges across brick faces: a long thin component costs
//        chains of bricks, not of voxels.  Sizes are integer atomics on the root; "largest only" is one 64-bit atomicMax
//        per sample of (size << 32 | ~root), which also reproduces the reference's tie rule (first component in C order).
// rare_* ReplaceWithClosestValue / replace_w_closest_value_3d (utils/transforms.py:233-268,603-647): a value that occurs
//        at most `max_count` times in the sample is rare; in every slice along `axis` each rare pixel takes the value of
//        the nearest non-rare pixel of that slice (exact squared Euclidean distance in pixel units; ties: the first such
//        pixel in the slice's row-major order).  Histogram -> per-line nearest non-rare column -> per-rare-pixel scan
//        over the slice's rows: O(voxels + rare pixels x rows), independent of the threshold.
#include "common.hpp"

namespace {

constexpr int BX = 32, BY = 8, BZ = 8, BVOX = BX * BY * BZ;  // brick of one workgroup (256 threads = 32 x 8 columns)

// the 13 "backward" neighbours (dz, dy, dx) < (0, 0, 0) in C order: each pair of 26-neighbours is linked once, always from
// the larger flat index to the smaller one
__constant__ int8_t kNb[13][3] = {{-1, -1, -1}, {-1, -1, 0}, {-1, -1, 1}, {-1, 0, -1}, {-1, 0, 0}, {-1, 0, 1}, {-1, 1, -1},
                                  {-1, 1, 0},   {-1, 1, 1},  {0, -1, -1}, {0, -1, 0},  {0, -1, 1}, {0, 0, -1}};

inline int grid_for(size_t work, int cap) {
  size_t b = (work + 255) / 256;
  return (int)(b < 1 ? 1 : (b > (size_t)cap ? (size_t)cap : b));
}

// ---- union-find, LDS flavour (one brick) ------------------------------------------------------------------------------
DEVI int lds_ld(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

DEVI int lds_find(int* p, int x) {  // path halving; parents only decrease
  while (true) {
    const int px = lds_ld(p + x);
    if (px == x) return x;
    const int ppx = lds_ld(p + px);
    if (ppx == px) return px;
    __hip_atomic_fetch_min(p + x, ppx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    x = ppx;
  }
}

DEVI void lds_unite(int* p, int a, int b) {
  while (true) {
    a = lds_find(p, a);
    b = lds_find(p, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(p + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == b) return;  // b was a root and now hangs below a
    b = old;               // b had been linked meanwhile: unite a with what b pointed to
  }
}

// ---- union-find, global flavour (across bricks) -----------------------------------------------------------------------
// Loads bypass this CU's L1 (agent scope); a value that is stale anyway is still an ancestor, and the atomic's returned
// value decides every link, so a stale "root" only costs another round of the loop in g_unite.
DEVI int g_ld(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

DEVI int g_find(int* p, int x) {
  while (true) {
    const int px = g_ld(p + x);
    if (px == x) return x;
    const int ppx = g_ld(p + px);
    if (ppx == px) return px;
    __hip_atomic_fetch_min(p + x, ppx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = ppx;
  }
}

DEVI void g_unite(int* p, int a, int b) {
  while (true) {
    a = g_find(p, a);
    b = g_find(p, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(p + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == b) return;
    b = old;
  }
}

struct Brick {
  int n, z0, y0, x0, tx, ty, x, y;
  DEVI Brick(int D) {
    const int nbz = (D + BZ - 1) / BZ;
    n = blockIdx.z / nbz;
    z0 = (blockIdx.z % nbz) * BZ;
    y0 = blockIdx.y * BY;
    x0 = blockIdx.x * BX;
    tx = threadIdx.x % BX;
    ty = threadIdx.x / BX;
    x = x0 + tx;
    y = y0 + ty;
  }
};

// 1. label every brick in LDS; parent[i] = flat index of the brick-local root (the brick's C order is the volume's, so this
//    root is the smallest index of the local component and parent[i] <= i); zero size[] at foreground voxels
__global__ __launch_bounds__(256) void cc_local_kernel(const uint8_t* __restrict__ lab, int* __restrict__ parent,
                                                       unsigned* __restrict__ size, unsigned long long* __restrict__ best, int N,
                                                       int D, int H, int W) {
  __shared__ int sp[BVOX];
  const Brick b(D);
  const size_t base = (size_t)b.n * D * H * W;
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
    for (int i = threadIdx.x; i < N; i += blockDim.x) best[i] = 0;
  for (int lz = 0; lz < BZ; ++lz) {
    const int z = b.z0 + lz, l = (lz * BY + b.ty) * BX + b.tx;
    bool fg = false;
    if (z < D && b.y < H && b.x < W) {
      const size_t g = base + ((size_t)z * H + b.y) * W + b.x;
      fg = lab[g] != 0;
      if (fg) size[g] = 0;
    }
    sp[l] = fg ? l : -1;  // outside the volume counts as background
  }
  __syncthreads();
  for (int lz = 0; lz < BZ; ++lz) {
    const int l = (lz * BY + b.ty) * BX + b.tx;
    if (lds_ld(sp + l) < 0) continue;  // (foreground entries never become negative)
    for (int k = 0; k < 13; ++k) {
      const int qz = lz + kNb[k][0], qy = b.ty + kNb[k][1], qx = b.tx + kNb[k][2];
      if (qz < 0 || qy < 0 || qy >= BY || qx < 0 || qx >= BX) continue;  // outside the brick: cc_merge_kernel
      const int q = (qz * BY + qy) * BX + qx;
      if (lds_ld(sp + q) >= 0) lds_unite(sp, l, q);
    }
  }
  __syncthreads();
  for (int lz = 0; lz < BZ; ++lz) {
    const int z = b.z0 + lz, l = (lz * BY + b.ty) * BX + b.tx;
    if (lds_ld(sp + l) < 0) continue;
    const int r = lds_find(sp, l);
    const int rz = r / (BX * BY), ry = (r / BX) % BY, rx = r % BX;
    parent[base + ((size_t)z * H + b.y) * W + b.x] = (int)(base + ((size_t)(b.z0 + rz) * H + b.y0 + ry) * W + b.x0 + rx);
  }
}

// 2. merge across brick faces: every foreground voxel unites with its foreground backward neighbours outside its brick
__global__ __launch_bounds__(256) void cc_merge_kernel(const uint8_t* __restrict__ lab, int* parent, int D, int H, int W) {
  const Brick b(D);
  if (b.x >= W || b.y >= H) return;
  const size_t base = (size_t)b.n * D * H * W;
  const bool edge_yx = b.ty == 0 || b.ty == BY - 1 || b.tx == 0 || b.tx == BX - 1;
  for (int lz = 0; lz < BZ; ++lz) {
    const int z = b.z0 + lz;
    if (z >= D) break;
    if (lz != 0 && !edge_yx) continue;  // every backward neighbour lies inside the brick
    const size_t g = base + ((size_t)z * H + b.y) * W + b.x;
    if (!lab[g]) continue;
    for (int k = 0; k < 13; ++k) {
      const int qz = lz + kNb[k][0], qy = b.ty + kNb[k][1], qx = b.tx + kNb[k][2];
      if (qz >= 0 && qy >= 0 && qy < BY && qx >= 0 && qx < BX) continue;  // inside the brick: done in LDS
      const int z2 = z + kNb[k][0], y2 = b.y + kNb[k][1], x2 = b.x + kNb[k][2];
      if (z2 < 0 || y2 < 0 || y2 >= H || x2 < 0 || x2 >= W) continue;   // no wrap-around, no crossing into another sample
      const size_t g2 = base + ((size_t)z2 * H + y2) * W + x2;
      if (lab[g2]) g_unite(parent, (int)g, (int)g2);
    }
  }
}

// 3. compress every foreground voxel onto its root and count the component sizes on the roots (one atomic per distinct root
//    of a wave)
__global__ __launch_bounds__(256) void cc_resolve_kernel(const uint8_t* __restrict__ lab, int* parent, unsigned* __restrict__ size,
                                                         size_t total) {
  const int lane = __lane_id();
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const bool fg = lab[i] != 0;
    int r = -1;
    if (fg) {
      const int p0 = g_ld(parent + i);
      r = g_find(parent, p0);
      if (r != p0) __hip_atomic_fetch_min(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    unsigned long long pending = __ballot(fg);
    while (pending) {
      const int src = __ffsll((unsigned long long)pending) - 1;
      const int r0 = __shfl(r, src);
      const unsigned long long same = __ballot(fg && r == r0);
      if (lane == src) atomicAdd(size + r0, (unsigned)__popcll(same));
      pending &= ~same;
    }
  }
}

// 4. (largest only) best[n] = max over the roots of sample n of (size << 32 | 0xFFFFFFFF - root): largest size, then the
//    smallest root = the component that comes first in C order (skimage's numbering + np.argmax's first maximum)
__global__ __launch_bounds__(256) void cc_best_kernel(const uint8_t* __restrict__ lab, const int* __restrict__ parent,
                                                      const unsigned* __restrict__ size, unsigned long long* best, size_t V,
                                                      size_t total) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    if (!lab[i] || parent[i] != (int)i) continue;
    const size_t n = i / V;
    const unsigned local = (unsigned)(i - n * V);
    atomicMax(best + n, ((unsigned long long)size[i] << 32) | (0xFFFFFFFFu - local));
  }
}

// 5. zero every foreground voxel of a dropped component (min_size >= 0: keep size > min_size; -1: keep best[n] only)
__global__ __launch_bounds__(256) void cc_filter_kernel(uint8_t* __restrict__ lab, const int* __restrict__ parent,
                                                        const unsigned* __restrict__ size, const unsigned long long* __restrict__ best,
                                                        size_t V, size_t total, int min_size) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    if (!lab[i]) continue;
    const int r = parent[i];
    bool keep;
    if (min_size >= 0) {
      keep = size[r] > (unsigned)min_size;
    } else {
      const size_t n = i / V;
      keep = (unsigned)(best[n] & 0xFFFFFFFFull) == 0xFFFFFFFFu - (unsigned)((size_t)r - n * V);
    }
    if (!keep) lab[i] = 0;
  }
}

// ---- rare-label fill ---------------------------------------------------------------------------------------------------
// hist[n][v] = number of voxels of sample n holding value v (LDS bins, one global atomic per bin and workgroup; the
// values 0..7 are counted in registers first so the common background value does not serialise on one LDS bank)
__global__ __launch_bounds__(256) void rare_hist_kernel(const uint8_t* __restrict__ lab, unsigned* __restrict__ hist, size_t V) {
  __shared__ unsigned sh[256];
  sh[threadIdx.x] = 0;
  __syncthreads();
  const uint8_t* p = lab + (size_t)blockIdx.y * V;
  unsigned c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (size_t)gridDim.x * blockDim.x) {
    const unsigned x = p[v];
    if (x < 8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) c[k] += x == (unsigned)k;
    } else {
      atomicAdd(sh + x, 1u);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    unsigned s = c[k];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (__lane_id() == 0 && s) atomicAdd(sh + k, s);
  }
  __syncthreads();
  if (sh[threadIdx.x]) atomicAdd(hist + (size_t)blockIdx.y * 256 + threadIdx.x, sh[threadIdx.x]);
}

// rare[v] for the block's sample (256 threads); false when no NON-ZERO value is rare: then the map stays as it is (the
// reference's `values_to_replace.any()`), and the whole block returns
DEVI bool load_rare(const unsigned* __restrict__ hist, int n, int max_count, bool* rare) {
  const unsigned c = hist[(size_t)n * 256 + threadIdx.x];
  const bool r = c > 0 && (long long)c <= (long long)max_count;
  rare[threadIdx.x] = r;
  return __syncthreads_or(r && threadIdx.x > 0) != 0;
}

struct SliceGeo {  // slice axis a, first in-plane ("row") axis ra < second in-plane ("column") axis ca
  int len[3];
  size_t st[3];
  int a, ra, ca;
  DEVI SliceGeo(int D, int H, int W, int axis) {
    len[0] = D; len[1] = H; len[2] = W;
    st[0] = (size_t)H * W; st[1] = (size_t)W; st[2] = 1;
    a = axis;
    ra = axis == 0 ? 1 : 0;
    ca = axis == 2 ? 1 : 2;
  }
};

// near[pixel] = column of the nearest non-rare pixel in the pixel's line along the column axis (ties: the smaller column),
// -1 for a line without one.  One lane per line; lanes lie on consecutive lines along the faster of the two axes that are
// not scanned, so a wave's loads are consecutive bytes when that axis is W.
__global__ __launch_bounds__(256) void rare_near_kernel(const uint8_t* __restrict__ lab, const unsigned* __restrict__ hist,
                                                        int16_t* __restrict__ near, int D, int H, int W, int axis, int max_count) {
  __shared__ bool rare[256];
  const int n = blockIdx.y;
  if (!load_rare(hist, n, max_count, rare)) return;
  const SliceGeo g(D, H, W, axis);
  const int fa = g.a > g.ra ? g.a : g.ra, sa = g.a > g.ra ? g.ra : g.a;  // fast / slow line axes
  const size_t lines = (size_t)g.len[fa] * g.len[sa];
  const int C = g.len[g.ca];
  const size_t sc = g.st[g.ca];
  const size_t base = (size_t)n * D * H * W;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < lines; t += (size_t)gridDim.x * blockDim.x) {
    const size_t off = base + (t / g.len[fa]) * g.st[sa] + (t % g.len[fa]) * g.st[fa];
    int last = -1;
    for (int c = 0; c < C; ++c) {
      if (!rare[lab[off + c * sc]]) last = c;
      near[off + c * sc] = (int16_t)last;
    }
    int next = -1;
    for (int c = C - 1; c >= 0; --c) {
      if (!rare[lab[off + c * sc]]) next = c;
      const int l = near[off + c * sc];
      if (next >= 0 && (l < 0 || next - c < c - l)) near[off + c * sc] = (int16_t)next;
    }
  }
}

// every rare pixel (i, j) of slice s: min over rows r of (i - r)^2 + (j - near[s][r][j])^2, first minimum in r, and takes
// that pixel's value; 0 when no row of the slice holds a non-rare pixel.  Sources are never rare, so in place is safe.
__global__ __launch_bounds__(256) void rare_fill_kernel(uint8_t* lab, const unsigned* __restrict__ hist,
                                                        const int16_t* __restrict__ near, int D, int H, int W, int axis,
                                                        int max_count) {
  __shared__ bool rare[256];
  const int n = blockIdx.y;
  if (!load_rare(hist, n, max_count, rare)) return;
  const SliceGeo g(D, H, W, axis);
  const size_t V = (size_t)D * H * W, base = (size_t)n * V;
  const int R = g.len[g.ra];
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (size_t)gridDim.x * blockDim.x) {
    if (!rare[lab[base + v]]) continue;
    const int co[3] = {(int)(v / g.st[0]), (int)((v / W) % H), (int)(v % W)};
    const int i = co[g.ra], j = co[g.ca];
    const size_t slice = base + (size_t)co[g.a] * g.st[g.a];
    unsigned bd = 0xFFFFFFFFu;
    size_t src = 0;
    for (int r = 0; r < R; ++r) {
      const size_t row = slice + (size_t)r * g.st[g.ra];
      const int c = near[row + (size_t)j * g.st[g.ca]];
      if (c < 0) continue;
      const unsigned d2 = (unsigned)((i - r) * (i - r)) + (unsigned)((j - c) * (j - c));
      if (d2 < bd) {
        bd = d2;
        src = row + (size_t)c * g.st[g.ca];
      }
    }
    lab[base + v] = bd == 0xFFFFFFFFu ? 0 : lab[src];
  }
}

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

bool shape_ok(int N, int D, int H, int W) { return N > 0 && D > 0 && H > 0 && W > 0; }

}  // namespace

extern "C" size_t brats_cc_ws_bytes(int N, int D, int H, int W) {
  if (!shape_ok(N, D, H, W)) return 0;
  const size_t total = (size_t)N * D * H * W;
  return align256((size_t)N * sizeof(unsigned long long)) + total * (sizeof(int) + sizeof(unsigned));
}

extern "C" int brats_cc_filter(uint8_t* labels, int N, int D, int H, int W, int min_size, void* ws, brats_stream_t s) {
  if (!labels || !ws || !shape_ok(N, D, H, W) || min_size < -1) BRATS_FAIL(BRATS_E_ARG, "cc_filter: bad argument");
  const size_t V = (size_t)D * H * W, total = (size_t)N * V;
  if (total >= (size_t)INT32_MAX) BRATS_FAIL(BRATS_E_UNSUPPORTED, "cc_filter: %zu voxels do not fit int32 indices", total);
  unsigned long long* best = (unsigned long long*)ws;
  int* parent = (int*)((char*)ws + align256((size_t)N * sizeof(unsigned long long)));
  unsigned* size = (unsigned*)(parent + total);
  hipStream_t st = (hipStream_t)s;
  const dim3 bricks((W + BX - 1) / BX, (H + BY - 1) / BY, N * ((D + BZ - 1) / BZ));
  hipLaunchKernelGGL(cc_local_kernel, bricks, dim3(256), 0, st, labels, parent, size, best, N, D, H, W);
  BRATS_CHECK_LAUNCH();
  hipLaunchKernelGGL(cc_merge_kernel, bricks, dim3(256), 0, st, labels, parent, D, H, W);
  BRATS_CHECK_LAUNCH();
  const int gx = grid_for(total, 8192);
  hipLaunchKernelGGL(cc_resolve_kernel, dim3(gx), dim3(256), 0, st, labels, parent, size, total);
  BRATS_CHECK_LAUNCH();
  if (min_size < 0) {
    hipLaunchKernelGGL(cc_best_kernel, dim3(gx), dim3(256), 0, st, labels, parent, size, best, V, total);
    BRATS_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(cc_filter_kernel, dim3(gx), dim3(256), 0, st, labels, parent, size, best, V, total, min_size);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t brats_rare_fill_ws_bytes(int N, int D, int H, int W) {
  if (!shape_ok(N, D, H, W)) return 0;
  return align256((size_t)N * 256 * sizeof(unsigned)) + (size_t)N * D * H * W * sizeof(int16_t);
}

extern "C" int brats_rare_fill(uint8_t* labels, int N, int D, int H, int W, int axis, int max_count, void* ws,
                               brats_stream_t s) {
  if (!labels || !ws || !shape_ok(N, D, H, W) || axis < 0 || axis > 2) BRATS_FAIL(BRATS_E_ARG, "rare_fill: bad argument");
  if (D > INT16_MAX || H > INT16_MAX || W > INT16_MAX)
    BRATS_FAIL(BRATS_E_UNSUPPORTED, "rare_fill: lines longer than %d pixels", (int)INT16_MAX);
  const size_t V = (size_t)D * H * W;
  unsigned* hist = (unsigned*)ws;
  int16_t* near = (int16_t*)((char*)ws + align256((size_t)N * 256 * sizeof(unsigned)));
  hipStream_t st = (hipStream_t)s;
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)N * 256 * sizeof(unsigned), st);
  if (e != hipSuccess) BRATS_FAIL(BRATS_E_HIP, "rare_fill: memset: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(rare_hist_kernel, dim3(grid_for(V / 16, 1024), N), dim3(256), 0, st, labels, hist, V);
  BRATS_CHECK_LAUNCH();
  const size_t lines = V / (axis == 2 ? H : W);
  hipLaunchKernelGGL(rare_near_kernel, dim3(grid_for(lines, 4096), N), dim3(256), 0, st, labels, hist, near, D, H, W, axis,
                     max_count);
  BRATS_CHECK_LAUNCH();
  hipLaunchKernelGGL(rare_fill_kernel, dim3(grid_for(V, 4096), N), dim3(256), 0, st, labels, hist, near, D, H, W, axis,
                     max_count);
  BRATS_CHECK_LAUNCH();
  return 0;
}
