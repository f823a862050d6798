// Hausdorff distance of the reference's validation metrics (utils/metrics.py:35-134 -> MONAI 0.6.0
// HausdorffDistanceMetric / compute_hausdorff_distance / get_mask_edges / get_surface_distance) on the GPU, for 0/1 float
// masks pred, target [NK][D][H][W].  Everything is decided on the device: no host synchronisation, no allocation.
//
// Per (n, k):
//   1. box    union bounding box of (pred == 1) | (target == 1) (integer atomicMax on zeroed memory)
//   2. edges  fg ^ erosion(fg) inside the box, where the erosion is the 6-neighbour cross with outside = 0, restricted to
//             the axes along which the box is more than one voxel thick (MONAI crops to the box and np.squeeze()s the
//             crop, so scipy erodes a 2-D / 1-D / 0-d array there); edge counts and the (z, x) projection of the edges
//   3. exact squared Euclidean distance of every voxel of the box to the nearest edge voxel of the OTHER map, separably:
//        w-pass  nearest edge in the row (one wave per row, prefix max / min over lanes), squared
//        z-pass  lower envelope of parabolas (Meijster et al.) along D, one lane per (y, x) line
//        y-pass  the same along H, only for (z, x) lines that hold a source edge, evaluated at the source edges only:
//                each squared distance goes into a per-(n, k, direction) histogram (LDS bins below 256)
//      All integer: squared distances are at most (D-1)^2 + (H-1)^2 + (W-1)^2.  The envelope stacks live in the pass's
//      output (z-pass) / in the consumed row buffer (y-pass), so nothing beyond the two int32 fields is needed.
//   4. finalise  per (n, k): the two order statistics of np.percentile's linear method by a scan over the histogram,
//                sqrt and numpy's _lerp in double, max over the two directions with Python's max(), one rounding to f32.
//
// Direction 0 is pred -> target (source = pred edges), direction 1 target -> pred.
#include "common.hpp"
#include "envelope.hpp"

namespace {

constexpr int HDR = 16;           // ints of per-(n, k) header: box[6], edge counts[2], max d^2 [2]
constexpr int LBINS = 256;        // low histogram bins kept per workgroup in LDS
constexpr int MAX_EXTENT = ENVELOPE_MAX_EXTENT;

struct Box {
  int z0, y0, x0, z1, y1, x1, bd, bh, bw;
  bool empty;
  DEVI Box(const int* h, int D, int H, int W) {
    z0 = D - 1 - h[0]; y0 = H - 1 - h[1]; x0 = W - 1 - h[2];
    z1 = h[3] - 1; y1 = h[4] - 1; x1 = h[5] - 1;
    empty = h[3] == 0;
    bd = z1 - z0 + 1; bh = y1 - y0 + 1; bw = x1 - x0 + 1;
  }
};

DEVI int wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
DEVI unsigned wave_sum(unsigned v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// 1. hdr[0..2] = max(D-1-z, H-1-y, W-1-x), hdr[3..5] = max(z+1, y+1, x+1) over the union's voxels (all 0: empty union)
__global__ __launch_bounds__(256) void hd_box_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                     int* __restrict__ hdr, int D, int H, int W) {
  const int nk = blockIdx.y;
  const size_t V = (size_t)D * H * W;
  const float* p = pred + (size_t)nk * V;
  const float* t = target + (size_t)nk * V;
  int a[6] = {0, 0, 0, 0, 0, 0};
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (size_t)gridDim.x * blockDim.x) {
    if (p[v] == 1.f || t[v] == 1.f) {
      const int z = (int)(v / ((size_t)H * W)), y = (int)((v / W) % H), x = (int)(v % W);
      a[0] = max(a[0], D - z); a[1] = max(a[1], H - y); a[2] = max(a[2], W - x);  // (D-1-z)+1: 0 stays "nothing seen"
      a[3] = max(a[3], z + 1); a[4] = max(a[4], y + 1); a[5] = max(a[5], x + 1);
    }
  }
  __shared__ int sh[4][6];
  const int wv = threadIdx.x / 64;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int m = wave_max(a[i]);
    if (__lane_id() == 0) sh[wv][i] = m;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int m = max(max(sh[0][threadIdx.x], sh[1][threadIdx.x]), max(sh[2][threadIdx.x], sh[3][threadIdx.x]));
    // the three "min" entries were stored + 1 so that 0 means empty; a non-empty union has all six > 0
    if (m > 0) atomicMax(hdr + (size_t)nk * HDR + threadIdx.x, threadIdx.x < 3 ? m - 1 : m);
  }
}

DEVI bool fg_at(const float* m, size_t g) { return m[g] == 1.f; }

// 2. edge[g] bit 0 = pred edge, bit 1 = target edge (written inside the box only); hdr[6], hdr[7] = edge counts;
//    proj[nk][z][x] |= the bits of every edge of the (z, x) line
__global__ __launch_bounds__(256) void hd_edge_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                      int* __restrict__ hdr, uint8_t* __restrict__ edge,
                                                      unsigned* __restrict__ proj, int D, int H, int W) {
  const int nk = blockIdx.y;
  int* h = hdr + (size_t)nk * HDR;
  const Box b(h, D, H, W);
  unsigned cp = 0, ct = 0;
  if (!b.empty) {
    const size_t V = (size_t)D * H * W, HW = (size_t)H * W, base = (size_t)nk * V;
    const size_t bvol = (size_t)b.bd * b.bh * b.bw;
    // an axis along which the box is one voxel thick is squeezed away before the erosion: no neighbours along it
    const bool ez = b.bd > 1, ey = b.bh > 1, ex = b.bw > 1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < bvol; i += (size_t)gridDim.x * blockDim.x) {
      const int z = b.z0 + (int)(i / ((size_t)b.bh * b.bw)), y = b.y0 + (int)((i / b.bw) % b.bh), x = b.x0 + (int)(i % b.bw);
      const size_t g = base + (size_t)z * HW + (size_t)y * W + x;
      unsigned bits = 0;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const float* m = mi == 0 ? pred : target;
        if (!fg_at(m, g)) continue;
        // a neighbour outside the volume is background; one outside the box is background by construction of the box
        const bool e = (ex && (x == 0 || !fg_at(m, g - 1))) || (ex && (x == W - 1 || !fg_at(m, g + 1))) ||
                       (ey && (y == 0 || !fg_at(m, g - W))) || (ey && (y == H - 1 || !fg_at(m, g + W))) ||
                       (ez && (z == 0 || !fg_at(m, g - HW))) || (ez && (z == D - 1 || !fg_at(m, g + HW)));
        if (e) bits |= 1u << mi;
      }
      edge[g] = (uint8_t)bits;
      if (bits) atomicOr(proj + ((size_t)nk * D + z) * W + x, bits);
      cp += bits & 1u;
      ct += bits >> 1;
    }
  }
  cp = wave_sum(cp);
  ct = wave_sum(ct);
  if (__lane_id() == 0 && (cp | ct)) {
    atomicAdd((unsigned*)h + 6, cp);
    atomicAdd((unsigned*)h + 7, ct);
  }
}

// 3a. w-pass, one wave per row of the box: rd[nk][dir][voxel] = squared distance to the nearest edge of the other map in
//     the row (dir 0: target edges, dir 1: pred edges), INF where the row has none.  Forward sweep: last edge at or left of
//     x (prefix max over lanes, carried across 64-wide chunks), stored as a distance; backward sweep: next edge at or right
//     of x (prefix min), combined.
__global__ __launch_bounds__(256) void hd_row_kernel(const int* __restrict__ hdr, const uint8_t* __restrict__ edge,
                                                     int* __restrict__ rd, int D, int H, int W) {
  const int nk = blockIdx.y;
  const Box b(hdr + (size_t)nk * HDR, D, H, W);
  if (b.empty) return;
  const size_t V = (size_t)D * H * W;
  const int lane = __lane_id();
  const int rows = b.bd * b.bh, chunks = (b.bw + 63) / 64;
  for (int r = blockIdx.x * 4 + threadIdx.x / 64; r < rows; r += gridDim.x * 4) {
    const int z = b.z0 + r / b.bh, y = b.y0 + r % b.bh;
    const size_t row = (size_t)nk * V + ((size_t)z * H + y) * W;
    int* r0 = rd + (size_t)nk * 2 * V + ((size_t)z * H + y) * W;  // dir 0
    int* r1 = r0 + V;                                                // dir 1
    int c0 = -1, c1 = -1;                                            // last target / pred edge so far (-1: none)
    for (int c = 0; c < chunks; ++c) {
      const int x = b.x0 + c * 64 + lane;
      const bool ok = x <= b.x1;
      const unsigned e = ok ? edge[row + x] : 0u;
      int l0 = (e & 2u) ? x : -1, l1 = (e & 1u) ? x : -1;
      for (int o = 1; o < 64; o <<= 1) {
        const int u0 = __shfl_up(l0, o), u1 = __shfl_up(l1, o);
        if (lane >= o) { l0 = max(l0, u0); l1 = max(l1, u1); }
      }
      l0 = max(l0, c0);
      l1 = max(l1, c1);
      c0 = __shfl(l0, 63);
      c1 = __shfl(l1, 63);
      if (ok) {
        r0[x] = l0 >= 0 ? x - l0 : INF;
        r1[x] = l1 >= 0 ? x - l1 : INF;
      }
    }
    c0 = INF; c1 = INF;  // next target / pred edge so far
    for (int c = chunks - 1; c >= 0; --c) {
      const int x = b.x0 + c * 64 + lane;
      const bool ok = x <= b.x1;
      const unsigned e = ok ? edge[row + x] : 0u;
      int n0 = (e & 2u) ? x : INF, n1 = (e & 1u) ? x : INF;
      for (int o = 1; o < 64; o <<= 1) {
        const int u0 = __shfl_down(n0, o), u1 = __shfl_down(n1, o);
        if (lane + o < 64) { n0 = min(n0, u0); n1 = min(n1, u1); }
      }
      n0 = min(n0, c0);
      n1 = min(n1, c1);
      c0 = __shfl(n0, 0);
      c1 = __shfl(n1, 0);
      if (ok) {
        int d0 = r0[x], d1 = r1[x];
        if (n0 != INF) d0 = min(d0, n0 - x);
        if (n1 != INF) d1 = min(d1, n1 - x);
        r0[x] = d0 != INF ? d0 * d0 : INF;
        r1[x] = d1 != INF ? d1 * d1 : INF;
      }
    }
  }
}

// 3b. z-pass over every (y, x) line of the box: g2[p] = min_i rd[i] + (p - i)^2 along D.  The stack lives in g2 itself: the
//     backward scan writes position u only once every stack entry it still needs lies below u.
__global__ __launch_bounds__(256) void hd_zpass_kernel(const int* __restrict__ hdr, const int* __restrict__ rd, int* g2, int D,
                                                       int H, int W) {
  const int nkd = blockIdx.y, nk = nkd >> 1;
  const Box b(hdr + (size_t)nk * HDR, D, H, W);
  if (b.empty) return;
  const size_t V = (size_t)D * H * W, HW = (size_t)H * W;
  const int lines = b.bh * b.bw;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < lines; t += gridDim.x * blockDim.x) {
    const int y = b.y0 + t / b.bw, x = b.x0 + t % b.bw;
    const size_t off = (size_t)nkd * V + (size_t)b.z0 * HW + (size_t)y * W + x;
    const int* in = rd + off;
    int* out = g2 + off;
    int tv = 0, tt = 0, tf = 0;
    int k = envelope(in, out, HW, b.bd, tv, tt, tf);
    for (int u = b.bd - 1; u >= 0; --u) {
      const int a = u - tv;
      out[(size_t)u * HW] = k >= 0 ? a * a + tf : INF;
      if (k >= 0 && u == tt && --k >= 0) {
        const int e = out[(size_t)k * HW];
        tv = e & 0xFFFF;
        tt = e >> 16;
        tf = in[(size_t)tv * HW];
      }
    }
  }
}

// 3c. y-pass over the (z, x) lines of the box that hold a source edge: the squared distance at every source edge voxel goes
//     into hist[nkd][d2] (bins < LBINS counted in LDS first, flushed once per workgroup), the largest into hdr[8 + dir].
//     The stack reuses rd (consumed by the z-pass).
__global__ __launch_bounds__(256) void hd_ypass_kernel(int* __restrict__ hdr, const int* __restrict__ g2, int* rd,
                                                       const uint8_t* __restrict__ edge, const unsigned* __restrict__ proj,
                                                       unsigned* __restrict__ hist, int nbins, int directed, int D, int H,
                                                       int W) {
  const int nkd = blockIdx.y, nk = nkd >> 1, dir = nkd & 1;
  int* h = hdr + (size_t)nk * HDR;
  const Box b(h, D, H, W);
  // nothing to count when a side has no edge (finalise decides those cases from the counts)
  if (b.empty || (directed && dir == 1) || h[6] == 0 || h[7] == 0) return;
  __shared__ unsigned lh[LBINS];
  lh[threadIdx.x] = 0;
  __syncthreads();
  const size_t V = (size_t)D * H * W, HW = (size_t)H * W;
  const unsigned sbit = dir == 0 ? 1u : 2u;  // source: pred edges (dir 0), target edges (dir 1)
  unsigned* hg = hist + (size_t)nkd * nbins;
  int mx = 0;
  const int lines = b.bd * b.bw;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < lines; t += gridDim.x * blockDim.x) {
    const int z = b.z0 + t / b.bw, x = b.x0 + t % b.bw;
    if (!(proj[((size_t)nk * D + z) * W + x] & sbit)) continue;
    const size_t off = (size_t)z * HW + (size_t)b.y0 * W + x;
    const int* in = g2 + (size_t)nkd * V + off;
    int* stk = rd + (size_t)nkd * V + off;
    const uint8_t* e = edge + (size_t)nk * V + off;
    int tv = 0, tt = 0, tf = 0;
    int k = envelope(in, stk, W, b.bh, tv, tt, tf);  // k >= 0: the other map has an edge, so every z-pass value is finite
    for (int u = b.bh - 1; u >= 0 && k >= 0; --u) {
      if (e[(size_t)u * W] & sbit) {
        const int a = u - tv, d2 = a * a + tf;
        mx = max(mx, d2);
        if (d2 < LBINS) atomicAdd(lh + d2, 1u);
        else atomicAdd(hg + d2, 1u);
      }
      if (u == tt && --k >= 0) {
        const int s = stk[(size_t)k * W];
        tv = s & 0xFFFF;
        tt = s >> 16;
        tf = in[(size_t)tv * W];
      }
    }
  }
  mx = wave_max(mx);
  if (__lane_id() == 0 && mx > 0) atomicMax(h + 8 + dir, mx);
  __syncthreads();
  if (lh[threadIdx.x]) atomicAdd(hg + threadIdx.x, lh[threadIdx.x]);
}

// value (bin) of the 0-based rank `r` of the histogram hist[0..nb) -- one workgroup of 256 threads, all must call
DEVI int rank_bin(const unsigned* __restrict__ hist, int nb, unsigned long long r, unsigned long long* sh, int* res) {
  const int chunk = (nb + 255) / 256, lo = threadIdx.x * chunk, hi = min(nb, lo + chunk);
  unsigned long long s = 0;
  for (int i = lo; i < hi; ++i) s += hist[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long run = 0;
    for (int i = 0; i < 256; ++i) {
      const unsigned long long c = sh[i];
      sh[i] = run;
      run += c;
    }
  }
  __syncthreads();
  unsigned long long run = sh[threadIdx.x];
  if (r >= run && r < run + s) {
    for (int i = lo; i < hi; ++i) {
      run += hist[i];
      if (r < run) { *res = i; break; }
    }
  }
  __syncthreads();
  const int v = *res;
  __syncthreads();
  return v;
}

// np.percentile(d, pct) of one direction (linear method, numpy's _lerp), or max(d) for pct < 0; NaN / inf for the empty
// cases as MONAI's get_surface_distance + compute_percent_hausdorff_distance produce them
DEVI double directed_hd(const unsigned* __restrict__ hist, unsigned n_src, unsigned n_dst, int maxd2, double pct,
                        unsigned long long* sh, int* res) {
  if (n_src == 0 && n_dst == 0) return __builtin_nan("");     // no distances at all
  if (n_src == 0 || n_dst == 0) return pct < 0 ? __builtin_inf() : __builtin_nan("");  // all inf: lerp(inf, inf) = nan
  if (pct < 0) return sqrt((double)maxd2);
  const double vi = (double)(n_src - 1) * (pct / 100.0);
  unsigned long long r0, r1;
  double g;
  if (vi >= (double)(n_src - 1)) {  // numpy: both neighbours are the last element, gamma = vi - (-1)
    r0 = r1 = n_src - 1;
    g = vi + 1.0;
  } else {
    const double f = floor(vi);
    r0 = (unsigned long long)f;
    r1 = r0 + 1;
    g = vi - f;
  }
  const int nb = maxd2 + 1;
  const double a = sqrt((double)rank_bin(hist, nb, r0, sh, res));
  const double b = r1 == r0 ? a : sqrt((double)rank_bin(hist, nb, r1, sh, res));
  const double diff = b - a;
  return g >= 0.5 ? b - diff * (1.0 - g) : a + diff * g;
}

// 4. one workgroup per (n, k)
__global__ __launch_bounds__(256) void hd_finalize_kernel(const int* __restrict__ hdr, const unsigned* __restrict__ hist,
                                                          int nbins, double pct, int directed, float* __restrict__ out) {
  __shared__ unsigned long long sh[256];
  __shared__ int res;
  const int nk = blockIdx.x;
  const int* h = hdr + (size_t)nk * HDR;
  const unsigned np = (unsigned)h[6], nt = (unsigned)h[7];
  const double d0 = directed_hd(hist + (size_t)(2 * nk) * nbins, np, nt, h[8], pct, sh, &res);
  double d = d0;
  if (!directed) {
    const double d1 = directed_hd(hist + (size_t)(2 * nk + 1) * nbins, nt, np, h[9], pct, sh, &res);
    d = d1 > d0 ? d1 : d0;  // Python's max(d0, d1): the first argument unless the second is strictly larger
  }
  if (threadIdx.x == 0) out[nk] = (float)d;
}

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

bool shape_ok(int NK, int D, int H, int W) {
  return NK > 0 && D > 0 && H > 0 && W > 0 && D <= MAX_EXTENT && H <= MAX_EXTENT && W <= MAX_EXTENT;
}

int n_bins(int D, int H, int W) { return (D - 1) * (D - 1) + (H - 1) * (H - 1) + (W - 1) * (W - 1) + 1; }

struct Ws {
  int* hdr;
  unsigned* proj;
  uint8_t* edge;
  int *rd, *g2;
  unsigned* hist;
  size_t hdr_bytes, proj_bytes, hist_bytes, total;
  Ws(void* base, int NK, int D, int H, int W) {
    const size_t V = (size_t)D * H * W;
    hdr_bytes = align256((size_t)NK * HDR * sizeof(int));
    proj_bytes = align256((size_t)NK * D * W * sizeof(unsigned));
    hist_bytes = align256((size_t)NK * 2 * n_bins(D, H, W) * sizeof(unsigned));
    const size_t edge_bytes = align256((size_t)NK * V), field = align256((size_t)NK * 2 * V * sizeof(int));
    char* p = (char*)base;
    hdr = (int*)p;                             // hdr, proj and hist are contiguous: one memset
    proj = (unsigned*)(p + hdr_bytes);
    hist = (unsigned*)(p + hdr_bytes + proj_bytes);
    edge = (uint8_t*)(p + hdr_bytes + proj_bytes + hist_bytes);
    rd = (int*)((char*)edge + edge_bytes);
    g2 = (int*)((char*)rd + field);
    total = hdr_bytes + proj_bytes + hist_bytes + edge_bytes + 2 * field;
  }
};

inline int grid_cap(size_t work, int per_block, int cap) {
  const size_t b = (work + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : (b > (size_t)cap ? (size_t)cap : b));
}

}  // namespace

extern "C" size_t brats_hausdorff_ws_bytes(int NK, int D, int H, int W) {
  if (!shape_ok(NK, D, H, W)) return 0;
  return Ws(nullptr, NK, D, H, W).total;
}

extern "C" int brats_hausdorff(const float* pred, const float* target, int NK, int D, int H, int W, double percentile,
                               int directed, float* out, void* ws, brats_stream_t s) {
  if (!pred || !target || !out || !ws || NK <= 0 || D <= 0 || H <= 0 || W <= 0 || !(percentile <= 100.0))
    BRATS_FAIL(BRATS_E_ARG, "hausdorff: bad argument");
  if (!shape_ok(NK, D, H, W))
    BRATS_FAIL(BRATS_E_UNSUPPORTED, "hausdorff: spatial extents above %d are not supported", MAX_EXTENT);
  const Ws w(ws, NK, D, H, W);
  const int nb = n_bins(D, H, W);
  const size_t V = (size_t)D * H * W;
  hipStream_t st = (hipStream_t)s;
  hipError_t e = hipMemsetAsync(w.hdr, 0, w.hdr_bytes + w.proj_bytes + w.hist_bytes, st);
  if (e != hipSuccess) BRATS_FAIL(BRATS_E_HIP, "hausdorff: memset: %s", hipGetErrorString(e));
  // grids are sized for a box as large as the volume; the kernels read the actual box and stride over it
  hipLaunchKernelGGL(hd_box_kernel, dim3(grid_cap(V, 256 * 8, 1024), NK), dim3(256), 0, st, pred, target, w.hdr, D, H, W);
  BRATS_CHECK_LAUNCH();
  hipLaunchKernelGGL(hd_edge_kernel, dim3(grid_cap(V, 256 * 4, 1024), NK), dim3(256), 0, st, pred, target, w.hdr, w.edge,
                     w.proj, D, H, W);
  BRATS_CHECK_LAUNCH();
  hipLaunchKernelGGL(hd_row_kernel, dim3(grid_cap((size_t)D * H, 4, 2048), NK), dim3(256), 0, st, w.hdr, w.edge, w.rd, D, H,
                     W);
  BRATS_CHECK_LAUNCH();
  hipLaunchKernelGGL(hd_zpass_kernel, dim3(grid_cap((size_t)H * W, 256, 1024), NK * 2), dim3(256), 0, st, w.hdr, w.rd, w.g2,
                     D, H, W);
  BRATS_CHECK_LAUNCH();
  hipLaunchKernelGGL(hd_ypass_kernel, dim3(grid_cap((size_t)D * W, 256, 1024), NK * 2), dim3(256), 0, st, w.hdr, w.g2, w.rd,
                     w.edge, w.proj, w.hist, nb, directed ? 1 : 0, D, H, W);
  BRATS_CHECK_LAUNCH();
  hipLaunchKernelGGL(hd_finalize_kernel, dim3(NK), dim3(256), 0, st, w.hdr, w.hist, nb, percentile, directed ? 1 : 0, out);
  BRATS_CHECK_LAUNCH();
  return 0;
}
