// Exact Euclidean distance transform (scipy.ndimage.distance_transform_edt, unit sampling) of `planes` independent volumes
// mask [planes][D][H][W] -> f32 field, and the signed boundary map of one_hot2dist / OneHotToDist built on it
// (learning/losses.py:59-95, utils/transforms.py:95-122).  Everything is decided on the device: no host synchronisation, no
// allocation, no atomics -- deterministic and graph-capturable.
//
// One DIRECTION = the squared distance of every voxel to the nearest SOURCE voxel (direction 0: sources are the background
// voxels, direction 1: the foreground voxels), separably and in exact int32 like the Hausdorff metric (metrics.hip):
//   w-pass  nearest source in the row: one wave per row, prefix max / suffix min over lanes carried across 64-wide chunks (any
//           W, ragged last chunk), squared; INF where the row has none                             mask -> rd
//   z-pass  lower envelope of parabolas along D, one lane per (y, x) line (adjacent lanes on adjacent x: coalesced), the
//           stack inside its own output                                                            rd -> g2
//   y-pass  the same along H, one lane per (z, x) line, the stack in the consumed rd; the result leaves as f32:
//           sqrt in double, rounded once (= scipy's f64 field cast to f32)                         g2 -> out
// A squared distance of 0 marks a source voxel, INF after the y-pass a plane without any source -- so the passes need no look
// at the mask again and no "has foreground" flag:
//   mode 0 (direction 0 only)   out = sqrt(d2); a plane without background (INF) takes scipy's value there, the distance to a
//                               virtual background voxel at index (-1, 0, 0): d2 = (z + 1)^2 + y^2 + x^2
//   mode 2                      mode 0 truncated to an integer: one_hot2hd_dist writes scipy's field into np.zeros_like(seg),
//                               and for the prediction seg is the int32 one-hot of probs2one_hot (learning/losses.py:37,88,158)
//   mode 1 (both directions, one after the other through the same two int32 fields)
//          direction 0 writes the foreground voxels (d2 > 0):  0 - (sqrt(d2) - 1)      (INF: the virtual voxel as above)
//          direction 1 writes the background voxels (d2 > 0):  sqrt(d2); INF = no foreground in the plane: 0 everywhere
//
// Bytes per voxel and direction (the bound of the three passes; the envelope stacks are written and popped within a line that
// the same lane has just streamed, i.e. they add at most one more int32 write + read to the z- and the y-pass):
//   w-pass  mask (4 f32 / 1 u8) + 4 written; rows longer than one chunk read the mask and their own output once more
//   z-pass  4 read + 4 written         y-pass  4 read + 4 written (f32)
//   = 20 B (u8 mask: 17 B) per voxel and direction, 40 B (34 B) for mode 1; 28 / 56 B with full stack traffic.
#include "common.hpp"
#include "envelope.hpp"

namespace {

template <typename T> DEVI bool is_fg(T v) { return v != (T)0; }

// w-pass, one wave per row: rd = squared distance to the nearest source of the row, INF where the row has none.  Forward
// sweep: last source at or left of x (prefix max over lanes, carried across chunks), stored as a distance; backward sweep:
// next source at or right of x (suffix min), combined and squared.
template <typename T>
__global__ __launch_bounds__(256) void edt_row_kernel(const T* __restrict__ mask, int* __restrict__ rd, int rows, int W, int dir) {
  const int lane = __lane_id();
  const int chunks = (W + 63) / 64;
  const bool src_fg = dir != 0;
  for (int r = blockIdx.x * 4 + threadIdx.x / 64; r < rows; r += gridDim.x * 4) {
    const size_t row = ((size_t)blockIdx.y * rows + r) * W;
    const T* m = mask + row;
    int* o = rd + row;
    int cl = -1;  // last source so far (-1: none)
    for (int c = 0; c < chunks; ++c) {
      const int x = c * 64 + lane;
      const bool ok = x < W;
      int l = (ok && is_fg(m[x]) == src_fg) ? x : -1;
      for (int s = 1; s < 64; s <<= 1) {
        const int u = __shfl_up(l, s);
        if (lane >= s) l = max(l, u);
      }
      l = max(l, cl);
      cl = __shfl(l, 63);
      if (ok) o[x] = l >= 0 ? x - l : INF;
    }
    int cn = INF;  // next source so far
    for (int c = chunks - 1; c >= 0; --c) {
      const int x = c * 64 + lane;
      const bool ok = x < W;
      int n = (ok && is_fg(m[x]) == src_fg) ? x : INF;
      for (int s = 1; s < 64; s <<= 1) {
        const int u = __shfl_down(n, s);
        if (lane + s < 64) n = min(n, u);
      }
      n = min(n, cn);
      cn = __shfl(n, 0);
      if (ok) {
        int d = o[x];
        if (n != INF) d = min(d, n - x);
        o[x] = d != INF ? d * d : INF;
      }
    }
  }
}

// z-pass over every (y, x) line: g2[p] = min_i rd[i] + (p - i)^2 along D.  The stack lives in g2 itself: the backward scan
// writes position u only once every stack entry it still needs lies below u.
__global__ __launch_bounds__(256) void edt_zpass_kernel(const int* __restrict__ rd, int* g2, int D, int H, int W) {
  const size_t HW = (size_t)H * W, V = (size_t)D * HW;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= H * W) return;
  const size_t off = (size_t)blockIdx.y * V + t;
  const int* in = rd + off;
  int* out = g2 + off;
  int tv = 0, tt = 0, tf = 0;
  int k = envelope(in, out, HW, D, tv, tt, tf);
  for (int u = D - 1; u >= 0; --u) {
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

// y-pass over every (z, x) line, stack in rd (consumed by the z-pass); the squared distance leaves as the mode's f32 value
__global__ __launch_bounds__(256) void edt_ypass_kernel(const int* __restrict__ g2, int* rd, float* __restrict__ out, int D, int H,
                                                        int W, int mode, int dir) {
  const size_t HW = (size_t)H * W, V = (size_t)D * HW;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= D * W) return;
  const int z = t / W, x = t % W;
  const size_t off = (size_t)blockIdx.y * V + (size_t)z * HW + x;
  const int* in = g2 + off;
  float* o = out + off;
  int tv = 0, tt = 0, tf = 0;
  int k = envelope(in, rd + off, W, H, tv, tt, tf);
  const bool none = k < 0;  // no source anywhere in the plane (every z-pass value of the line is INF only then)
  for (int u = H - 1; u >= 0; --u) {
    const int a = u - tv;
    // no background at all: the virtual background voxel at (-1, 0, 0)
    const int d2 = none ? (z + 1) * (z + 1) + u * u + x * x : a * a + tf;
    if (mode != 1) {
      const double r = sqrt((double)d2);
      o[(size_t)u * W] = (float)(mode == 2 ? floor(r) : r);
    } else if (dir == 0) {
      if (d2 > 0) o[(size_t)u * W] = (float)(0.0 - (sqrt((double)d2) - 1.0));
    } else {
      if (none) o[(size_t)u * W] = 0.f;
      else if (d2 > 0) o[(size_t)u * W] = (float)sqrt((double)d2);
    }
    if (!none && u == tt && --k >= 0) {
      const int e = rd[off + (size_t)k * W];
      tv = e & 0xFFFF;
      tt = e >> 16;
      tf = in[(size_t)tv * W];
    }
  }
}

inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }

bool shape_ok(int planes, int D, int H, int W) {
  return planes > 0 && planes <= 65535 && D > 0 && H > 0 && W > 0 && D <= ENVELOPE_MAX_EXTENT && H <= ENVELOPE_MAX_EXTENT &&
         W <= ENVELOPE_MAX_EXTENT;
}

}  // namespace

extern "C" size_t brats_edt_ws_bytes(int planes, int D, int H, int W) {
  if (!shape_ok(planes, D, H, W)) return 0;
  return 2 * align256((size_t)planes * D * H * W * sizeof(int));
}

extern "C" int brats_edt(const void* mask, int mask_kind, int planes, int D, int H, int W, int mode, float* out, void* ws,
                         brats_stream_t s) {
  if (!mask || !out || !ws || (mask_kind != BRATS_MASK_F32 && mask_kind != BRATS_MASK_U8) || mode < 0 || mode > 2)
    BRATS_FAIL(BRATS_E_ARG, "edt: bad argument");
  if (!shape_ok(planes, D, H, W))
    BRATS_FAIL(BRATS_E_ARG, "edt: planes must be 1..65535 and D, H, W 1..%d", ENVELOPE_MAX_EXTENT);
  hipStream_t st = (hipStream_t)s;
  int* rd = (int*)ws;
  int* g2 = (int*)((char*)ws + align256((size_t)planes * D * H * W * sizeof(int)));
  const int rows = D * H;
  const int row_blocks = (rows + 3) / 4 < 2048 ? (rows + 3) / 4 : 2048;
  for (int dir = 0; dir <= (mode == 1 ? 1 : 0); ++dir) {
    if (mask_kind == BRATS_MASK_F32)
      hipLaunchKernelGGL(edt_row_kernel<float>, dim3(row_blocks, planes), dim3(256), 0, st, (const float*)mask, rd, rows, W, dir);
    else
      hipLaunchKernelGGL(edt_row_kernel<uint8_t>, dim3(row_blocks, planes), dim3(256), 0, st, (const uint8_t*)mask, rd, rows, W,
                         dir);
    BRATS_CHECK_LAUNCH();
    hipLaunchKernelGGL(edt_zpass_kernel, dim3((H * W + 255) / 256, planes), dim3(256), 0, st, rd, g2, D, H, W);
    BRATS_CHECK_LAUNCH();
    hipLaunchKernelGGL(edt_ypass_kernel, dim3((D * W + 255) / 256, planes), dim3(256), 0, st, g2, rd, out, D, H, W, mode, dir);
    BRATS_CHECK_LAUNCH();
  }
  return 0;
}
