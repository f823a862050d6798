// 2x2x2 max / max+avg pooling and align_corners=True trilinear up-sampling (forward + adjoint), NDHWC.
// All HBM-bound: 16-byte channel vectors per thread, coalesced along the channel-minor layout.
// Reference: nn.MaxPool3d(2,2) networks/equiunet2020.py:433; MONAI MaxAvgPool networks/equiunet2021.py:261
// (cat([max, avg], dim=1)); nn.Upsample(trilinear, align_corners=True) networks/equiunet2020.py:439.
#include "twin_begin.hpp"
#include "common.hpp"

constexpr int POOL_MAX_BLOCKS = 8192;  // of the grid-stride passes (stream_grid)

// ---- pooling -----------------------------------------------------------------------------------
// argmax (optional): one byte per (pooled voxel, channel) = the window index 0..7 (d, h, w order) of torch's first arg-max;
// brats_maxpool2_bwd_idx reads these instead of the window
template <typename T>
__global__ void maxpool2_fwd_kernel(const T* __restrict__ x, int xpitch, T* __restrict__ y, int ypitch, int N, int C,
                                    int D, int H, int W, int with_avg, uint8_t* __restrict__ argmax) {
  constexpr int VW = 16 / sizeof(T);
  const int cv = C / VW, Do = D / 2, Ho = H / 2, Wo = W / 2;
  const size_t total = (size_t)N * Do * Ho * Wo * cv;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(it % cv) * VW;
    size_t v = it / cv;
    const int xo = v % Wo; v /= Wo;
    const int yo = v % Ho; v /= Ho;
    const int zo = v % Do;
    const int n = (int)(v / Do);
    float mx[VW], sm[VW];
    int am[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) { mx[j] = -INFINITY; sm[j] = 0.f; am[j] = 0; }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int z = 2 * zo + (k >> 2), yy = 2 * yo + ((k >> 1) & 1), xx = 2 * xo + (k & 1);
      float a[VW];
      Vec<T, VW>::load(x + ((((size_t)n * D + z) * H + yy) * W + xx) * xpitch + c0, a);
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        if (a[j] > mx[j] || a[j] != a[j]) { mx[j] = a[j]; am[j] = k; }
        sm[j] += a[j];
      }
    }
    const size_t pvox = (((size_t)n * Do + zo) * Ho + yo) * Wo + xo;
    T* yo_p = y + pvox * ypitch;
    if (argmax) {
      uint32_t* ap = (uint32_t*)(argmax + pvox * C + c0);
#pragma unroll
      for (int q = 0; q < VW / 4; ++q) ap[q] = am[4 * q] | (am[4 * q + 1] << 8) | (am[4 * q + 2] << 16) | (am[4 * q + 3] << 24);
    }
    Vec<T, VW>::store(yo_p + c0, mx);
    if (with_avg) {
#pragma unroll
      for (int j = 0; j < VW; ++j) sm[j] *= 0.125f;
      Vec<T, VW>::store(yo_p + C + c0, sm);
    }
  }
}

// one thread per pooled voxel x channel vector: recompute the first arg-max (torch tie rule:
// strict '>' in d,h,w scan order) and write all 8 input-gradient voxels of the window.
template <typename T>
__global__ void maxpool2_bwd_kernel(const T* __restrict__ x, int xpitch, const T* __restrict__ dy, int dypitch,
                                    const T* __restrict__ dxs, int dxspitch, T* __restrict__ dx, int dxpitch, int N, int C,
                                    int D, int H, int W, int with_avg) {
  constexpr int VW = 16 / sizeof(T);
  const int cv = C / VW, Do = D / 2, Ho = H / 2, Wo = W / 2;
  const size_t total = (size_t)N * Do * Ho * Wo * cv;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(it % cv) * VW;
    size_t v = it / cv;
    const int xo = v % Wo; v /= Wo;
    const int yo = v % Ho; v /= Ho;
    const int zo = v % Do;
    const int n = (int)(v / Do);
    float a[8][VW];
    float mx[VW];
    int am[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) { mx[j] = -INFINITY; am[j] = 0; }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int z = 2 * zo + (k >> 2), yy = 2 * yo + ((k >> 1) & 1), xx = 2 * xo + (k & 1);
      Vec<T, VW>::load(x + ((((size_t)n * D + z) * H + yy) * W + xx) * xpitch + c0, a[k]);
#pragma unroll
      for (int j = 0; j < VW; ++j)
        if (a[k][j] > mx[j] || a[k][j] != a[k][j]) { mx[j] = a[k][j]; am[j] = k; }
    }
    const T* dyp = dy + ((((size_t)n * Do + zo) * Ho + yo) * Wo + xo) * dypitch;
    float g[VW], ga[VW];
    Vec<T, VW>::load(dyp + c0, g);
#pragma unroll
    for (int j = 0; j < VW; ++j) ga[j] = 0.f;
    if (with_avg) {
      Vec<T, VW>::load(dyp + C + c0, ga);
#pragma unroll
      for (int j = 0; j < VW; ++j) ga[j] *= 0.125f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int z = 2 * zo + (k >> 2), yy = 2 * yo + ((k >> 1) & 1), xx = 2 * xo + (k & 1);
      const size_t vox = (((size_t)n * D + z) * H + yy) * W + xx;
      float o[VW];
#pragma unroll
      for (int j = 0; j < VW; ++j) o[j] = ga[j] + (am[j] == k ? g[j] : 0.f);
      if (dxs) {
        float sk[VW];
        Vec<T, VW>::load(dxs + vox * dxspitch + c0, sk);
#pragma unroll
        for (int j = 0; j < VW; ++j) o[j] += sk[j];
      }
      Vec<T, VW>::store(dx + vox * dxpitch + c0, o);
    }
  }
}

// The same backward from a RECORDED arg-max (one byte per pooled voxel and channel, written by brats_affine_act_pool_fwd): the
// 8 window voxels of x (403 MB at 2 x 48 x 128^3) are not read again.  A thread owns one x position x one 16-byte channel
// vector and the 2 x 2 (z, y) voxels above it: its 4 skip-gradient loads and 4 stores are contiguous runs of a row across the
// lanes; the pooled gradient and the arg-max bytes are read by both threads of an x pair.  Same arithmetic as
// maxpool2_bwd_kernel ((avg / 8 + [k == argmax] * dy) + skip): bit-identical.
template <typename T>
__global__ void __launch_bounds__(256) maxpool2_bwd_idx_kernel(const uint8_t* __restrict__ argmax, const T* __restrict__ dy, int dypitch,
                                                               const T* __restrict__ dxs, int dxspitch, T* __restrict__ dx, int dxpitch,
                                                               int C, int D, int H, int W, int with_avg) {
  constexpr int VW = 16 / sizeof(T);
  const int n = blockIdx.y;
  const int cv = C / VW;
  int xb = blockDim.x / cv;
  if (xb > W) xb = W;
  const int mycv = threadIdx.x % cv, myvl = threadIdx.x / cv, c0 = mycv * VW;
  const int Do = D / 2, Ho = H / 2, Wo = W / 2;
  const int segs = (W + xb - 1) / xb;
  const size_t items = (size_t)Do * Ho * segs, voxels = (size_t)D * H * W, pvoxels = (size_t)Do * Ho * Wo;
  if (myvl >= xb) return;
  const T* dyb = dy + (size_t)n * pvoxels * dypitch + c0;
  const T* sb = dxs ? dxs + (size_t)n * voxels * dxspitch + c0 : nullptr;
  T* ob = dx + (size_t)n * voxels * dxpitch + c0;
  const uint8_t* ab = argmax + (size_t)n * pvoxels * C + c0;
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int seg = (int)(item % segs);
    const size_t rp = item / segs;
    const int yo = (int)(rp % Ho), zo = (int)(rp / Ho);
    const int x = seg * xb + myvl;
    if (x >= W) continue;
    const size_t pvox = ((size_t)zo * Ho + yo) * Wo + (x >> 1);
    float sk[4][VW];
    size_t vox[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      vox[k] = ((size_t)(2 * zo + (k >> 1)) * H + (2 * yo + (k & 1))) * W + x;
      if (sb) Vec<T, VW>::load(sb + vox[k] * dxspitch, sk[k]);
    }
    uint32_t aw[VW / 4];
#pragma unroll
    for (int q = 0; q < VW / 4; ++q) aw[q] = ((const uint32_t*)(ab + pvox * C))[q];
    float g[VW], ga[VW];
    Vec<T, VW>::load(dyb + pvox * dypitch, g);
#pragma unroll
    for (int j = 0; j < VW; ++j) ga[j] = 0.f;
    if (with_avg) {
      Vec<T, VW>::load(dyb + pvox * dypitch + C, ga);
#pragma unroll
      for (int j = 0; j < VW; ++j) ga[j] *= 0.125f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int kk = 2 * k + (x & 1);  // the voxel's index in the window, d, h, w order
      float o[VW];
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        const int am = (aw[j >> 2] >> (8 * (j & 3))) & 0xff;
        o[j] = ga[j] + (am == kk ? g[j] : 0.f);
        if (sb) o[j] += sk[k][j];
      }
      Vec<T, VW>::store(ob + vox[k] * dxpitch, o);
    }
  }
}

extern "C" int BRATS_API(brats_maxpool2_bwd_idx)(const unsigned char* argmax, const void* dy, int dypitch, const void* dx_skip,
                                      int dxskip_pitch, void* dx, int dxpitch, int dtype, int N, int C, int D, int H, int W,
                                      int with_avg, brats_stream_t s) {
  const int vw = vec_width(dtype);
  if (!argmax || !dy || !dx || C % vw || dypitch % vw || dxpitch % vw || (dx_skip && dxskip_pitch % vw) || ((D | H | W) & 1) ||
      C / vw > 256)
    BRATS_FAIL(BRATS_E_ARG, "maxpool2_bwd_idx: bad argument");
  int xb = 256 / (C / vw);
  if (xb > W) xb = W;
  const size_t items = (size_t)(D / 2) * (H / 2) * ((W + xb - 1) / xb);
  dim3 grid(stream_grid(items, 1, POOL_MAX_BLOCKS), N);
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(maxpool2_bwd_idx_kernel<T>, grid, dim3(256), 0, (hipStream_t)s, argmax, (const T*)dy, dypitch, (const T*)dx_skip,
                       dxskip_pitch, (T*)dx, dxpitch, C, D, H, W, with_avg);
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int BRATS_API(brats_maxpool2_fwd)(const void* x, int xpitch, void* y, int ypitch, unsigned char* argmax, int dtype, int N,
                                  int C, int D, int H, int W, int with_avg, brats_stream_t s) {
  const int vw = vec_width(dtype);
  if (!x || !y || C % vw || xpitch % vw || ypitch % vw || (D | H | W) & 1)
    BRATS_FAIL(BRATS_E_ARG, "maxpool2_fwd: C/pitch multiple of %d and even spatial dims required", vw);
  const size_t total = (size_t)N * (D / 2) * (H / 2) * (W / 2) * (C / vw);
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(maxpool2_fwd_kernel<T>, dim3(stream_grid(total, 256, POOL_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)s, (const T*)x,
                       xpitch, (T*)y, ypitch, N, C, D, H, W, with_avg, argmax);
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int BRATS_API(brats_maxpool2_bwd)(const void* x, int xpitch, const void* y, int ypitch, const void* dy, int dypitch,
                                  const void* dx_skip, int dxskip_pitch, void* dx, int dxpitch, int dtype, int N, int C,
                                  int D, int H, int W, int with_avg, brats_stream_t s) {
  (void)y; (void)ypitch;  // arg-max is recomputed from x
  const int vw = vec_width(dtype);
  if (!x || !dy || !dx || C % vw || xpitch % vw || dypitch % vw || dxpitch % vw || (dx_skip && dxskip_pitch % vw) ||
      (D | H | W) & 1)
    BRATS_FAIL(BRATS_E_ARG, "maxpool2_bwd: bad argument");
  const size_t total = (size_t)N * (D / 2) * (H / 2) * (W / 2) * (C / vw);
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(maxpool2_bwd_kernel<T>, dim3(stream_grid(total, 128, POOL_MAX_BLOCKS)), dim3(128), 0, (hipStream_t)s, (const T*)x,
                       xpitch, (const T*)dy, dypitch, (const T*)dx_skip, dxskip_pitch, (T*)dx, dxpitch, N, C, D, H, W, with_avg);
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

// ---- trilinear, align_corners=True -------------------------------------------------------------
// torch semantics (UpSample.h area_pixel_compute_source_index, align_corners): scale = (in-1)/(out-1)
// in f32, src = scale*dst, i0 = (int)src, i1 = i0 + (i0 < in-1), lambda1 = src - i0.
struct Lerp { int i0, i1; float w0, w1; };
DEVI Lerp lerp_coef(int o, int in_len, float scale) {
  const float src = scale * (float)o;
  Lerp l;
  l.i0 = (int)src;
  if (l.i0 > in_len - 1) l.i0 = in_len - 1;
  l.i1 = l.i0 + (l.i0 < in_len - 1 ? 1 : 0);
  l.w1 = fminf(fmaxf(src - (float)l.i0, 0.f), 1.f);
  l.w0 = 1.f - l.w1;
  return l;
}
static inline float ac_scale(int in_len, int out_len) { return out_len > 1 ? (float)(in_len - 1) / (float)(out_len - 1) : 0.f; }

// One block = one output row (n, zo, yo): the z / y interpolation coefficients and the four source-row pointers are
// scalar; a thread handles (xo, channel vector) items of the row (no per-element div / mod chains).
template <typename T>
__global__ void __launch_bounds__(256) upsample_fwd_kernel(const T* __restrict__ x, int xpitch, T* __restrict__ y, int ypitch,
                                                           int N, int C, int D, int H, int W, int sc, float sd, float sh,
                                                           float sw) {
  constexpr int VW = 16 / sizeof(T);
  const int cv = C / VW, Do = D * sc, Ho = H * sc, Wo = W * sc;
  for (size_t row = blockIdx.x; row < (size_t)N * Do * Ho; row += gridDim.x) {
    const int yo = (int)(row % Ho);
    const int zo = (int)((row / Ho) % Do);
    const int n = (int)(row / ((size_t)Ho * Do));
    const Lerp lz = lerp_coef(zo, D, sd), ly = lerp_coef(yo, H, sh);
    const T* xb = x + (size_t)n * D * H * W * xpitch;
    const T* r00 = xb + (size_t)(lz.i0 * H + ly.i0) * W * xpitch;
    const T* r01 = xb + (size_t)(lz.i0 * H + ly.i1) * W * xpitch;
    const T* r10 = xb + (size_t)(lz.i1 * H + ly.i0) * W * xpitch;
    const T* r11 = xb + (size_t)(lz.i1 * H + ly.i1) * W * xpitch;
    T* yb = y + row * Wo * ypitch;
    for (int it = threadIdx.x; it < Wo * cv; it += blockDim.x) {
      const int xo = it / cv, c0 = (it % cv) * VW;
      const Lerp lx = lerp_coef(xo, W, sw);
      float o[VW];
#pragma unroll
      for (int j = 0; j < VW; ++j) o[j] = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const T* r = (k & 4) ? ((k & 2) ? r11 : r10) : ((k & 2) ? r01 : r00);
        const int xx = (k & 1) ? lx.i1 : lx.i0;
        // same association as ATen's upsample_trilinear3d: w_z * (w_y * (w_x * v ...)) -> use product of weights
        const float w = ((k & 4) ? lz.w1 : lz.w0) * ((k & 2) ? ly.w1 : ly.w0) * ((k & 1) ? lx.w1 : lx.w0);
        float a[VW];
        Vec<T, VW>::load(r + (size_t)xx * xpitch + c0, a);
#pragma unroll
        for (int j = 0; j < VW; ++j) o[j] += w * a[j];
      }
      Vec<T, VW>::store(yb + (size_t)xo * ypitch + c0, o);
    }
  }
}

// scale 2 (the decoder's up-sampling): one block = 2 output z-planes x 4 output y-rows of one sample, a thread = one (xo,
// channel vector) column of that 2 x 4 patch.  The 8 outputs read the same 3 input planes x 4 input rows, so a thread does
// 24 gathers for 8 outputs instead of 64 (the row-per-block kernel above is bound by its 8 gathers per 16-byte store), and
// every store instruction still writes a contiguous x-row.  Weights of absent (plane, row) pairs are zero; same f32
// coefficients as lerp_coef, summed x first, then y, then z.
// LDSX: the 3 planes x 4 rows the block reads are first copied into LDS with dense 16-byte loads (every input element
// fetched once per block: 18 load instructions per thread instead of 72 gathers); 12 x W x C elements must fit (73.7 KB at
// every decoder level of the bf16 networks: W x C = 3072).
template <typename T, bool NT = false, bool LDSX = false>
__global__ void __launch_bounds__(256) upsample2_fwd_kernel(const T* __restrict__ x, int xpitch, T* __restrict__ y, int ypitch,
                                                            int C, int D, int H, int W, float sd, float sh, float sw) {
  constexpr int VW = 16 / sizeof(T);
  extern __shared__ __attribute__((aligned(16))) char up_lds[];
  const int cv = C / VW, Do = 2 * D, Ho = 2 * H, Wo = 2 * W;
  const int yq = blockIdx.x, zp = blockIdx.y, n = blockIdx.z;
  const int zo0 = 2 * zp, yo0 = 4 * yq;
  Lerp lz[2], ly[4];
#pragma unroll
  for (int a = 0; a < 2; ++a) lz[a] = lerp_coef(zo0 + a, D, sd);
#pragma unroll
  for (int b = 0; b < 4; ++b) ly[b] = lerp_coef(yo0 + b, H, sh);
  const int zb = lz[0].i0, yb = ly[0].i0;
  float wz[2][3], wy[4][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int pz = 0; pz < 3; ++pz) wz[a][pz] = (lz[a].i0 == zb + pz ? lz[a].w0 : 0.f) + (lz[a].i1 == zb + pz ? lz[a].w1 : 0.f);
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) wy[b][r] = (ly[b].i0 == yb + r ? ly[b].w0 : 0.f) + (ly[b].i1 == yb + r ? ly[b].w1 : 0.f);
  const T* xb = x + (size_t)n * D * H * W * xpitch;
  T* yb_ = y + (size_t)n * Do * Ho * Wo * ypitch;
  if constexpr (LDSX) {
    const int row_pieces = W * cv;
    for (int q = threadIdx.x; q < 12 * row_pieces; q += blockDim.x) {
      const int rr = q / row_pieces, w = q % row_pieces;
      const int zi = zb + rr / 4 < D ? zb + rr / 4 : D - 1, yi = yb + rr % 4 < H ? yb + rr % 4 : H - 1;
      *(u32x4*)(up_lds + (size_t)q * 16) =
          *(const u32x4*)(xb + ((size_t)(zi * H + yi) * W + w / cv) * xpitch + (w % cv) * VW);
    }
    __syncthreads();
  }
  // pairs of channels through explicit v_pk_fma_f32: with separate multiplies and adds (the build's -ffp-contract=off) the
  // ~1400 packed ops per 8 outputs made this kernel VALU-bound at 2.3 TB/s
  typedef __attribute__((ext_vector_type(2))) float f2;
  auto fma2 = [](float w, f2 v, f2 acc) { return __builtin_elementwise_fma(f2{w, w}, v, acc); };
  constexpr int V2 = VW / 2;
  for (int it = threadIdx.x; it < Wo * cv; it += blockDim.x) {
    const int xo = it / cv, c0 = (it % cv) * VW;
    const Lerp lx = lerp_coef(xo, W, sw);
    f2 o[2][4][V2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int j = 0; j < V2; ++j) o[a][b][j] = f2{0.f, 0.f};
#pragma unroll
    for (int pz = 0; pz < 3; ++pz) {
      const int zi = zb + pz < D ? zb + pz : D - 1;   // (a clamped plane / row carries zero weight)
      f2 t[4][V2];                                    // y-interpolated rows of this plane, per output row b
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int j = 0; j < V2; ++j) t[b][j] = f2{0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int yi = yb + r < H ? yb + r : H - 1;
        float v0[VW], v1[VW];
        if constexpr (LDSX) {
          const T* row = (const T*)up_lds + (size_t)(pz * 4 + r) * W * C + c0;
          Vec<T, VW>::load(row + (size_t)lx.i0 * C, v0);
          Vec<T, VW>::load(row + (size_t)lx.i1 * C, v1);
        } else {
          const T* row = xb + (size_t)(zi * H + yi) * W * xpitch + c0;
          Vec<T, VW>::load(row + (size_t)lx.i0 * xpitch, v0);
          Vec<T, VW>::load(row + (size_t)lx.i1 * xpitch, v1);
        }
#pragma unroll
        for (int j = 0; j < V2; ++j) {
          const f2 xl = fma2(lx.w1, f2{v1[2 * j], v1[2 * j + 1]}, lx.w0 * f2{v0[2 * j], v0[2 * j + 1]});
#pragma unroll
          for (int b = 0; b < 4; ++b) t[b][j] = fma2(wy[b][r], xl, t[b][j]);
        }
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
          for (int j = 0; j < V2; ++j) o[a][b][j] = fma2(wz[a][pz], t[b][j], o[a][b][j]);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        float of[VW];
#pragma unroll
        for (int j = 0; j < V2; ++j) { of[2 * j] = o[a][b][j][0]; of[2 * j + 1] = o[a][b][j][1]; }
        vstore<T, VW, NT>(yb_ + ((size_t)((zo0 + a) * Ho + yo0 + b) * Wo + xo) * ypitch + c0, of);
      }
  }
}

extern "C" int BRATS_API(brats_upsample_fwd)(const void* x, int xpitch, void* y, int ypitch, int dtype, int N, int C, int D, int H,
                                  int W, int scale, brats_stream_t s) {
  const int vw = vec_width(dtype);
  if (!x || !y || C % vw || xpitch % vw || ypitch % vw || scale < 1)
    BRATS_FAIL(BRATS_E_ARG, "upsample_fwd: C/pitch must be multiples of %d", vw);
  const size_t rows = (size_t)N * D * scale * H * scale;
  const unsigned grid = (unsigned)(rows > 65536 ? 65536 : rows);
  const float sd = ac_scale(D, D * scale), sh = ac_scale(H, H * scale), sw = ac_scale(W, W * scale);
  if (scale == 2 && H % 2 == 0 && N <= 65535 && D <= 65535) {
    const dim3 g2(H / 2, D, N);  // (Ho / 4, Do / 2, N)
    const size_t ldsx = (size_t)12 * W * C * 2;
    const bool big = big_tensor16(dtype, (size_t)N * D * H * W * 8 * C);  // output beyond the Infinity Cache: non-temporal stores
    auto go = [&](auto t, auto nt, auto in_lds) {
      using T = typename decltype(t)::type;
      constexpr bool LDSX = decltype(in_lds)::value;
      hipLaunchKernelGGL((upsample2_fwd_kernel<T, decltype(nt)::value, LDSX>), g2, dim3(256), LDSX ? ldsx : 0, (hipStream_t)s, (const T*)x,
                         xpitch, (T*)y, ypitch, C, D, H, W, sd, sh, sw);
    };
    if (dtype == BRATS_BF16 && ldsx <= 80 * 1024) {  // two blocks per CU with their input rows in LDS
      static std::atomic<uint64_t> attr_a{0}, attr_b{0};
      BRATS_ENSURE_LDS_ATTR((upsample2_fwd_kernel<bf16_t, true, true>), 80 * 1024, attr_a);
      BRATS_ENSURE_LDS_ATTR((upsample2_fwd_kernel<bf16_t, false, true>), 80 * 1024, attr_b);
      with_flag(big, [&](auto nt) { go(type_tag<bf16_t>{}, nt, std::true_type{}); });
    } else {
      with_stream16(dtype, big, [&](auto t, auto nt) { go(t, nt, std::false_type{}); });
    }
    BRATS_CHECK_LAUNCH();
    return 0;
  }
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(upsample_fwd_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)s, (const T*)x, xpitch, (T*)y, ypitch, N, C, D, H, W,
                       scale, sd, sh, sw);
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

// acc[j] = the stored sum of the adjoint's value and an addend: the value rounded to the storage type first, then the f32 sum
// of the two stored values, rounded once by the store -- what a separate elementwise add of the two tensors computes
template <typename T, int VW>
DEVI void add_stored(float* acc, const T* addp) {
  float b[VW];
  if constexpr (VW == 1) b[0] = to_f<T>(addp[0]);
  else Vec<T, VW>::load(addp, b);
#pragma unroll
  for (int j = 0; j < VW; ++j) acc[j] = to_f<T>(from_f<T>(acc[j])) + b[j];
}

// 1-D adjoint of the lerp along one axis of a tensor viewed as [outer][L][inner_vox][C(+pitch)]:
// out[o][i][v][c] = sum_{l : i0(l)==i} w0(l)*in[o][l][v][c] + sum_{l : i1(l)==i, i1!=i0} w1(l)*in[..l..].
// Candidates l are re-derived with the *forward's own* f32 expression, so forward and adjoint are
// exactly transposes of each other.
template <typename TI, typename TO, int VW, bool ADD = false>
__global__ void lerp_adjoint_kernel(const TI* __restrict__ in, int in_pitch, TO* __restrict__ out, int out_pitch,
                                    size_t outer, int Lout /*len of in*/, int Lin /*len of out*/, size_t inner_vox, int C,
                                    float scale, const TO* __restrict__ add = nullptr /* ADD: out = stored(adjoint) + add */,
                                    int add_pitch = 0) {
  const int cv = C / VW;
  const size_t total = outer * Lin * inner_vox * cv;
  const float inv = scale > 0.f ? 1.f / scale : 0.f;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (size_t)gridDim.x * blockDim.x) {
    const int c0 = (int)(it % cv) * VW;
    size_t v = it / cv;
    const size_t iv = v % inner_vox; v /= inner_vox;
    const int i = (int)(v % Lin);
    const size_t o = v / Lin;
    int lo = (int)floorf((float)(i - 1) * inv) - 1, hi = (int)ceilf((float)(i + 1) * inv) + 1;
    if (scale <= 0.f) { lo = 0; hi = Lout - 1; }
    lo = lo < 0 ? 0 : lo;
    hi = hi > Lout - 1 ? Lout - 1 : hi;
    float acc[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) acc[j] = 0.f;
    for (int l = lo; l <= hi; ++l) {
      const Lerp c = lerp_coef(l, Lin, scale);
      float w = 0.f;
      if (c.i0 == i) w += c.w0;
      if (c.i1 == i) w += c.w1;  // when i1 == i0 (clamped end) both weights land on the same index
      if (w != 0.f) {
        float a[VW];
        if constexpr (VW == 1) a[0] = to_f<TI>(in[((o * Lout + l) * inner_vox + iv) * in_pitch + c0]);
        else Vec<TI, VW>::load(in + ((o * Lout + l) * inner_vox + iv) * in_pitch + c0, a);
#pragma unroll
        for (int j = 0; j < VW; ++j) acc[j] += w * a[j];
      }
    }
    if constexpr (ADD) add_stored<TO, VW>(acc, add + ((o * Lin + i) * inner_vox + iv) * add_pitch + c0);
    if constexpr (VW == 1) out[((o * Lin + i) * inner_vox + iv) * out_pitch + c0] = from_f<TO>(acc[0]);
    else Vec<TO, VW>::store(out + ((o * Lin + i) * inner_vox + iv) * out_pitch + c0, acc);
  }
}

// exported for head.hip: f32 planes [outer][L][inner] adjoint along one axis (the three-pass form, for what the tile form
// below does not take)
int brats_lerp_adjoint_f32_planes(const float* in, float* out, size_t outer, int Lout, int Lin, size_t inner,
                                  hipStream_t st) {
  const size_t total = outer * Lin * inner;
  if (inner % 4 == 0 && (((size_t)in | (size_t)out) & 15) == 0) {
    // four neighbouring inner elements per thread (16-byte loads): these planes are bound by the NUMBER of vector-memory
    // instructions (one per candidate l per thread), not by their bytes
    hipLaunchKernelGGL((lerp_adjoint_kernel<float, float, 4>), dim3(stream_grid(total / 4, 256, POOL_MAX_BLOCKS)), dim3(256), 0, st, in, 4,
                       out, 4, outer, Lout, Lin, inner / 4, 4, ac_scale(Lin, Lout));
    BRATS_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL((lerp_adjoint_kernel<float, float, 1>), dim3(stream_grid(total, 256, POOL_MAX_BLOCKS)), dim3(256), 0, st, in, 1, out, 1,
                     outer, Lout, Lin, inner, 1, ac_scale(Lin, Lout));
  BRATS_CHECK_LAUNCH();
  return 0;
}

// ---- the three axes of the adjoint in ONE launch --------------------------------------------------------------------------
// The three-pass form moves every tensor through HBM again between the axes (x2 at 2 x 48 x 128^3: 403 -> 201 -> 100 -> 50 MB,
// 1.06 GB for 0.45 GB of input and output; each pass is at bandwidth, the structure is the cost).  Here a workgroup owns a
// coarse tile, walks the fine planes that feed it once in ascending z with the D reduction in registers, and does the H and W
// reductions of every finished coarse plane out of LDS; only the coarse tile is written.
// Bit-identity with the three-pass form: per axis the same f32 sum over ascending fine index l of w(l) * v(l) with
// w = [i0 == i] w0 + [i1 == i] w1 from the forward's own lerp_coef (zero weights skipped), and the value is rounded to the
// storage type between the axes exactly where that form stores t1 and t2.
// A fine plane l feeds the coarse planes i0(l) and i1(l) <= i0 + 1 only, so the walk keeps two accumulators per column: `cur`
// (coarse plane i) and `nxt` (i + 1).  Step i takes the planes with i0 == i: they end cur's sum (w0, plus w1 at a clamped end)
// and begin nxt's (w1) -- for every coarse plane that is ascending l, the planes with i1 == i first.  A z chunk starts one
// step early (the planes with i0 == za - 1 carry w1 into za); that step's own plane is dropped.
// (Earlier forms that kept the temporaries in HBM or gathered again from it did not pay: profiles/r03_lerp_adjoint_two_axis_negative.txt,
//  profiles/r04_upsample_adjoint_stream_negative.txt.)

// first / last fine index that can carry weight into the coarse range [a, a + cnt): found with the forward's own expression,
// starting from a conservative estimate
DEVI void lerp_fine_range(int a, int cnt, int Lin, int Lout, float scale, int& lo, int& hi) {
  const float inv = scale > 0.f ? 1.f / scale : 0.f;
  lo = (int)floorf((float)(a - 1) * inv) - 2;
  hi = (int)ceilf((float)(a + cnt) * inv) + 2;
  if (scale <= 0.f) { lo = 0; hi = Lout - 1; }
  lo = lo < 0 ? 0 : lo;
  hi = hi > Lout - 1 ? Lout - 1 : hi;
  while (lo < hi && lerp_coef(lo, Lin, scale).i1 < a) ++lo;
  while (hi > lo && lerp_coef(hi, Lin, scale).i0 > a + cnt - 1) --hi;
}
// w(l) for coarse index i (the three-pass kernel's expression)
DEVI float lerp_weight_to(int l, int i, int Lin, float scale) {
  const Lerp c = lerp_coef(l, Lin, scale);
  float w = 0.f;
  if (c.i0 == i) w += c.w0;
  if (c.i1 == i) w += c.w1;
  return w;
}

// 16-bit NDHWC, scale 2: coarse tile = (cd planes) x 4 rows x 8 columns on a slice of 48 channels, 512 threads, two workgroups
// per CU (31 KB of LDS, <= 128 VGPRs each) so that one loads while the other reduces.  The fine rows / columns that reach c
// coarse ones lie in a closed interval of (c + 1) / scale: <= 19.3 for c = 8 (extents >= 16; the whole axis, 16, at extent 8)
// and <= 11.7 for c = 4, hence the 12 x 20 footprint.  Re-read of the input: 11 / 8 x 19 / 16 x (2 cd + 2) / (2 cd) = 1.7 at
// cd = 16; the workgroup ids are dealt out so that the tiles of one z chunk run on one XCD and share their halo lines in its L2
// (measured: 449 MB fetched from HBM for the 403 MB of a 2 x 48 x 128^3 gradient, profiles/memory_passes_pmc.txt).
// The loads of step i + 1 are issued before the LDS passes of step i, so they are in flight while the workgroup is there.
constexpr int UBF_TH = 4, UBF_TW = 8, UBF_FH = 12, UBF_FW = 20, UBF_CS = 48, UBF_CV = UBF_CS / 8, UBF_THREADS = 512, UBF_KC = 3, UBF_MAXP = 2;
static_assert(UBF_FH * UBF_FW * UBF_CV <= UBF_THREADS * UBF_KC, "every column of the fine footprint needs a thread slot");
// acc[0..7] += w * (8 x 16-bit at p)
DEVI void ubf_add(float* acc, float w, const bf16_t* p) {
  float a[8];
  Vec<bf16_t, 8>::load(p, a);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] += w * a[j];
}
struct UbfStep { int l[UBF_MAXP]; float wc[UBF_MAXP], wn[UBF_MAXP]; int np; };
// ADD: dx = stored(adjoint) + add (an addend of dx's extent, pitch addpitch; may be the gradient another consumer produced)
template <bool ADD>
__global__ void __launch_bounds__(UBF_THREADS, 4) upsample2_bwd_fused_kernel(const bf16_t* __restrict__ dy, int dypitch, bf16_t* __restrict__ dx,
                                                                          int dxpitch, int C, int D, int H, int W, int cd, float sd,
                                                                          float sh, float sw, const bf16_t* __restrict__ add, int addpitch) {
  __shared__ __attribute__((aligned(16))) bf16_t slab[UBF_FH * UBF_FW * UBF_CS];  // the finished coarse plane, D-reduced: [fh][fw][48]
  __shared__ __attribute__((aligned(16))) bf16_t t2s[UBF_TH * UBF_FW * UBF_CS];   // ... H-reduced: [4][fw][48]
  __shared__ float wys[UBF_TH][UBF_FH], wxs[UBF_TW][UBF_FW];
  __shared__ int yrng[UBF_TH][2], xrng[UBF_TW][2];
  const int Do = 2 * D, Ho = 2 * H, Wo = 2 * W;
  const int nsl = C / UBF_CS, tiles_x = W / UBF_TW, tiles_y = H / UBF_TH, nz = D / cd;
  // workgroup ids go round the 8 XCDs: give every XCD a contiguous run of tiles (one z chunk's tiles are neighbours there)
  int bid = blockIdx.x;
  if (gridDim.x % 8 == 0) bid = (bid % 8) * (gridDim.x / 8) + bid / 8;
  const int sl = bid % nsl, tx = (bid / nsl) % tiles_x, ty = (bid / (nsl * tiles_x)) % tiles_y;
  const int zc = (bid / (nsl * tiles_x * tiles_y)) % nz, n = bid / (nsl * tiles_x * tiles_y * nz);
  const int za = zc * cd, ya = ty * UBF_TH, xa = tx * UBF_TW;
  const int tid = threadIdx.x;
  int yl, yh, xl, xh;
  lerp_fine_range(ya, UBF_TH, H, Ho, sh, yl, yh);
  lerp_fine_range(xa, UBF_TW, W, Wo, sw, xl, xh);
  if (yh - yl + 1 > UBF_FH) yh = yl + UBF_FH - 1;  // (cannot happen for the extents the host admits; keeps LDS in bounds)
  if (xh - xl + 1 > UBF_FW) xh = xl + UBF_FW - 1;
  const int fh = yh - yl + 1, fw = xh - xl + 1;
  // weight tables of the H and W reductions
  if (tid < UBF_TH * UBF_FH) {
    const int t = tid / UBF_FH, f = tid % UBF_FH;
    wys[t][f] = f < fh ? lerp_weight_to(yl + f, ya + t, H, sh) : 0.f;
  } else if (tid >= 64 && tid < 64 + UBF_TW * UBF_FW) {
    const int t = (tid - 64) / UBF_FW, f = (tid - 64) % UBF_FW;
    wxs[t][f] = f < fw ? lerp_weight_to(xl + f, xa + t, W, sw) : 0.f;
  }
  __syncthreads();
  if (tid < UBF_TH + UBF_TW) {  // first / last fine index with weight, per coarse row / column
    const int ax = tid >= UBF_TH, t = ax ? tid - UBF_TH : tid, fn = ax ? fw : fh;
    const float* wt = ax ? wxs[t] : wys[t];
    int a = 0, b = fn - 1;
    while (a < b && wt[a] == 0.f) ++a;
    while (b > a && wt[b] == 0.f) --b;
    (ax ? xrng : yrng)[t][0] = a;
    (ax ? xrng : yrng)[t][1] = b;
  }
  // this thread's columns (fine y, fine x, channel vector) of the footprint
  const int ncol = fh * fw * UBF_CV;
  const bf16_t* src = dy + (size_t)n * Do * Ho * Wo * dypitch + (size_t)sl * UBF_CS;
  const size_t plane = (size_t)Ho * Wo * dypitch;
  size_t coloff[UBF_KC];
  bool colok[UBF_KC];
#pragma unroll
  for (int k = 0; k < UBF_KC; ++k) {
    const int col = tid + k * UBF_THREADS;
    colok[k] = col < ncol;
    const int cvi = col % UBF_CV, xx = (col / UBF_CV) % fw, yy = colok[k] ? col / (UBF_CV * fw) : 0;
    coloff[k] = ((size_t)(yl + yy) * Wo + (xl + xx)) * dypitch + cvi * 8;
  }
  // the z walk
  const int i_first = za > 0 ? za - 1 : 0, i_last = za + cd - 1;
  int lcur, lend;
  lerp_fine_range(i_first, 1, D, Do, sd, lcur, lend);
  while (lcur < Do && lerp_coef(lcur, D, sd).i0 < i_first) ++lcur;
  auto plan = [&](int i, UbfStep& st) {  // up to UBF_MAXP planes with i0 == i, from lcur on
    st.np = 0;
#pragma unroll
    for (int p = 0; p < UBF_MAXP; ++p) {
      st.l[p] = 0; st.wc[p] = 0.f; st.wn[p] = 0.f;
      if (st.np == p && lcur < Do) {
        const Lerp c = lerp_coef(lcur, D, sd);
        if (c.i0 == i) {
          st.l[p] = lcur;
          st.wc[p] = c.i1 == i ? c.w0 + c.w1 : c.w0;
          st.wn[p] = c.i1 == i + 1 ? c.w1 : 0.f;
          st.np = p + 1;
          ++lcur;
        }
      }
    }
  };
  u32x4 raw[UBF_MAXP][UBF_KC];
  auto issue = [&](const UbfStep& st) {
#pragma unroll
    for (int p = 0; p < UBF_MAXP; ++p)
      if (p < st.np) {
#pragma unroll
        for (int k = 0; k < UBF_KC; ++k)
          raw[p][k] = colok[k] ? *(const u32x4*)(src + (size_t)st.l[p] * plane + coloff[k]) : u32x4{0u, 0u, 0u, 0u};
      }
  };
  // (scalar f32 multiplies and adds on purpose: the same sums as f32x2 pairs -- v_pk_mul_f32 + v_pk_add_f32 -- measured
  //  slower, 190 -> 215 us at 2 x 48 x 128^3, for the register pairing they need)
  float cur[UBF_KC][8], nxt[UBF_KC][8];
#pragma unroll
  for (int k = 0; k < UBF_KC; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) { cur[k][j] = 0.f; nxt[k][j] = 0.f; }
  auto accumulate = [&](const UbfStep& st) {
#pragma unroll
    for (int p = 0; p < UBF_MAXP; ++p)
      if (p < st.np) {
#pragma unroll
        for (int k = 0; k < UBF_KC; ++k) {
          float a[8];
#pragma unroll
          for (int q = 0; q < 4; ++q) unpack2(raw[p][k][q], a[2 * q], a[2 * q + 1]);
          if (st.wc[p] != 0.f) {
#pragma unroll
            for (int j = 0; j < 8; ++j) cur[k][j] += st.wc[p] * a[j];
          }
          if (st.wn[p] != 0.f) {
#pragma unroll
            for (int j = 0; j < 8; ++j) nxt[k][j] += st.wn[p] * a[j];
          }
        }
      }
  };
  UbfStep st;
  plan(i_first, st);
  issue(st);
  bf16_t* dst = dx + (size_t)n * D * H * W * dxpitch + (size_t)sl * UBF_CS;
  for (int i = i_first; i <= i_last; ++i) {
    accumulate(st);
    while (st.np == UBF_MAXP) {  // more planes with the same i0 than one batch holds
      plan(i, st);
      issue(st);
      accumulate(st);
    }
    if (i >= za) {
#pragma unroll
      for (int k = 0; k < UBF_KC; ++k)
        if (colok[k]) Vec<bf16_t, 8>::store(slab + (size_t)(tid + k * UBF_THREADS) * 8, cur[k]);
    }
#pragma unroll
    for (int k = 0; k < UBF_KC; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) { cur[k][j] = nxt[k][j]; nxt[k][j] = 0.f; }
    if (i < i_last) {  // the next step's planes: in flight during the LDS passes below
      plan(i + 1, st);
      issue(st);
    } else {
      st.np = 0;
    }
    __syncthreads();
    if (i < za) continue;
    // H: [fh][fw][48] -> [4][fw][48], rounded to the storage type
    const int rowv = fw * UBF_CV;
    for (int it = tid; it < UBF_TH * rowv; it += UBF_THREADS) {
      const int h = it / rowv, r = it % rowv;
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
      for (int f = yrng[h][0]; f <= yrng[h][1]; ++f) {
        const float w = wys[h][f];
        if (w != 0.f) ubf_add(acc, w, slab + ((size_t)f * rowv + r) * 8);
      }
      Vec<bf16_t, 8>::store(t2s + (size_t)it * 8, acc);
    }
    __syncthreads();
    // W: [4][fw][48] -> the coarse tile's plane i
    for (int it = tid; it < UBF_TH * UBF_TW * UBF_CV; it += UBF_THREADS) {
      const int cvi = it % UBF_CV, xc = (it / UBF_CV) % UBF_TW, h = it / (UBF_CV * UBF_TW);
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
      for (int f = xrng[xc][0]; f <= xrng[xc][1]; ++f) {
        const float w = wxs[xc][f];
        if (w != 0.f) ubf_add(acc, w, t2s + ((size_t)(h * fw + f) * UBF_CV + cvi) * 8);
      }
      if constexpr (ADD)
        add_stored<bf16_t, 8>(acc, add + (size_t)n * D * H * W * addpitch + (size_t)sl * UBF_CS +
                                       (((size_t)i * H + ya + h) * W + xa + xc) * addpitch + cvi * 8);
      Vec<bf16_t, 8>::store(dst + (((size_t)i * H + ya + h) * W + xa + xc) * dxpitch + cvi * 8, acc);
    }
  }
}

static int g_upsample_bwd_fused = -1;  // brats_upsample_bwd_set_fused(): -1 = default (on where the tile form applies), 0 = off, 1 = on
extern "C" int BRATS_API(brats_upsample_bwd_set_fused)(int mode) {
  const int old = g_upsample_bwd_fused;
  g_upsample_bwd_fused = mode < 0 ? -1 : (mode ? 1 : 0);
  return old;
}
// the z chunk of the tile form, 0 = this problem goes through the three passes (scale 4 / 8, f32, extents that do not tile)
static int upsample_bwd_fused_cd(int N, int C, int D, int H, int W, int sc) {
  if (g_upsample_bwd_fused == 0 || sc != 2 || C % UBF_CS || H % UBF_TH || W % UBF_TW || D % 4) return 0;
  const size_t per_z = (size_t)N * (H / UBF_TH) * (W / UBF_TW) * (C / UBF_CS);
  int cd = 16;
  while (cd > 4 && (D % cd || per_z * (D / cd) < 1024)) cd /= 2;  // two rounds of two workgroups per CU where the tensor is large enough
  if (per_z * (D / cd) > 0x7fffffffull) return 0;
  return cd;
}

// ---- f32 planes [P][Do][Ho][Wo] -> [P][D][H][W] (the deep-supervision heads, scale 2 / 4 / 8; head.hip) in one launch ------
// The same walk on planes without a channel axis: a workgroup owns cd coarse planes x th coarse rows of one plane stack over
// the full width, a thread's columns are (fine y, four fine x).  f32 throughout, so there is no rounding between the axes and
// the D-reduced tile stays in LDS for all cd planes: the fine planes are streamed B at a time (KC x B 16-byte loads in flight
// per thread), a coarse plane is put down when the walk passes it, and the H and W reductions run once per workgroup.  The
// order of the additions per axis is that of lerp_adjoint_kernel, with its weights derived on the fly over its conservative
// candidate range.  LDS: cd x (fmax + th) x Wo floats.
constexpr int PAF_THREADS = 256;
template <int KC, int B>
__global__ void __launch_bounds__(PAF_THREADS) planes_adjoint_fused_kernel(const float* __restrict__ in, float* __restrict__ out, int D, int H, int W,
                                                                           int sc, int cd, int th, int fmax, float sd, float sh, float sw) {
  extern __shared__ __attribute__((aligned(16))) float paf_lds[];
  const int Do = D * sc, Ho = H * sc, Wo = W * sc, W4 = Wo / 4;
  float* t1s = paf_lds;                            // [cd][fmax][Wo]
  float* t2s = paf_lds + (size_t)cd * fmax * Wo;   // [cd][th][Wo]
  const int ya = blockIdx.x * th, za = blockIdx.y * cd;
  const size_t pl = blockIdx.z;
  const int tid = threadIdx.x;
  int yl, yh;
  lerp_fine_range(ya, th, H, Ho, sh, yl, yh);
  if (yh - yl + 1 > fmax) yh = yl + fmax - 1;  // (the host sizes fmax for the closed interval of (th + 1) / scale; keeps LDS in bounds)
  const int fh = yh - yl + 1;
  const int ncol = fh * W4;
  const float* src = in + pl * Do * Ho * Wo + (size_t)yl * Wo;
  const size_t plane = (size_t)Ho * Wo;
  // the planes with i0 in [i_first, i_last]; i_first = za - 1 carries its w1 into za and is itself dropped
  const int i_first = za > 0 ? za - 1 : 0, i_last = za + cd - 1;
  int lstart, lend;
  lerp_fine_range(i_first, i_last - i_first + 1, D, Do, sd, lstart, lend);
  while (lstart < lend && lerp_coef(lstart, D, sd).i0 < i_first) ++lstart;
  f32x4 cur[KC], nxt[KC];
#pragma unroll
  for (int k = 0; k < KC; ++k) { cur[k] = f32x4{0.f, 0.f, 0.f, 0.f}; nxt[k] = cur[k]; }
  int i = i_first;  // the coarse plane `cur` belongs to
  auto flush = [&]() {
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      const int col = tid + k * PAF_THREADS;
      if (i >= za && col < ncol) *(f32x4*)(t1s + ((size_t)(i - za) * fmax * W4 + col) * 4) = cur[k];
      cur[k] = nxt[k];
      nxt[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    ++i;
  };
  for (int l0 = lstart; l0 <= lend; l0 += B) {
    f32x4 raw[B][KC];
#pragma unroll
    for (int b = 0; b < B; ++b)
      if (l0 + b <= lend) {
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          const int col = tid + k * PAF_THREADS;
          raw[b][k] = col < ncol ? *(const f32x4*)(src + (size_t)(l0 + b) * plane + (size_t)col * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
#pragma unroll
    for (int b = 0; b < B; ++b)
      if (l0 + b <= lend) {
        const Lerp c = lerp_coef(l0 + b, D, sd);
        while (i < c.i0 && i <= i_last) flush();
        const float wc = c.i1 == i ? c.w0 + c.w1 : c.w0, wn = c.i1 == i + 1 ? c.w1 : 0.f;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          if (wc != 0.f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) cur[k][j] += wc * raw[b][k][j];
          }
          if (wn != 0.f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) nxt[k][j] += wn * raw[b][k][j];
          }
        }
      }
  }
  while (i <= i_last) flush();
  __syncthreads();
  const float invh = sh > 0.f ? 1.f / sh : 0.f, invw = sw > 0.f ? 1.f / sw : 0.f;
  // H: [cd][fh][Wo] -> [cd][th][Wo]
  for (int it = tid; it < cd * th * W4; it += PAF_THREADS) {
    const int x4 = it % W4, h = (it / W4) % th, z = it / (W4 * th), ic = ya + h;
    int lo = (int)floorf((float)(ic - 1) * invh) - 1, hi = (int)ceilf((float)(ic + 1) * invh) + 1;
    if (sh <= 0.f) { lo = 0; hi = Ho - 1; }
    lo = lo < yl ? yl : lo;
    hi = hi > yh ? yh : hi;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int l = lo; l <= hi; ++l) {
      const float w = lerp_weight_to(l, ic, H, sh);
      if (w != 0.f) {
        const f32x4 a = *(const f32x4*)(t1s + ((size_t)(z * fmax + l - yl) * W4 + x4) * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += w * a[j];
      }
    }
    *(f32x4*)(t2s + (size_t)it * 4) = acc;
  }
  __syncthreads();
  // W: [cd][th][Wo] -> [cd][th][W] of the coarse planes za..
  for (int it = tid; it < cd * th * W; it += PAF_THREADS) {
    const int xc = it % W, h = (it / W) % th, z = it / (W * th);
    int lo = (int)floorf((float)(xc - 1) * invw) - 1, hi = (int)ceilf((float)(xc + 1) * invw) + 1;
    if (sw <= 0.f) { lo = 0; hi = Wo - 1; }
    lo = lo < 0 ? 0 : lo;
    hi = hi > Wo - 1 ? Wo - 1 : hi;
    float acc = 0.f;
    for (int l = lo; l <= hi; ++l) {
      const float w = lerp_weight_to(l, xc, W, sw);
      if (w != 0.f) acc += w * t2s[(size_t)(z * th + h) * Wo + l];
    }
    out[((pl * D + za + z) * H + ya + h) * (size_t)W + xc] = acc;
  }
}

// exported for head.hip: the three axes of the f32 plane adjoint, [P][D sc][H sc][W sc] -> [P][D][H][W], one launch.
// Returns 1 without launching where the tile form does not apply (width no multiple of 4, rows too wide for LDS): the caller
// runs the three passes (brats_lerp_adjoint_f32_planes) then.
int brats_planes_adjoint_f32(const float* in, float* out, size_t P, int D, int H, int W, int sc, hipStream_t st) {
  const int Wo = W * sc;
  if (Wo % 4 || (((size_t)in | (size_t)out) & 15) || P > 65535 || D > 65535) return 1;
  // tile: 2 - 4 coarse planes x 2 - 4 coarse rows (about 16 x 8 fine planes x rows per workgroup): small enough for
  // several workgroups per CU and a grid of many hundreds, the halo re-read ((cd + 1) / cd x (th + 1) / th = 1.6 at scale
  // 2, 2.25 at scale 8) comes out of the caches the producer of the 50 MB planes has just filled
  int cd = 16 / sc < 2 ? 2 : (16 / sc > 4 ? 4 : 16 / sc), th = 8 / sc < 2 ? 2 : (8 / sc > 4 ? 4 : 8 / sc);
  while (cd > 1 && D % cd) cd /= 2;
  while (th > 1 && H % th) th /= 2;
  // fine rows that reach th coarse ones: the closed interval of (th + 1) / scale, scale = (H - 1) / (H sc - 1)
  const float scale_h = H > 1 ? (float)(H - 1) / (float)(H * sc - 1) : 0.f;
  int fmax = scale_h > 0.f ? (int)ceilf((float)(th + 1) / scale_h) + 2 : H * sc;
  if (fmax > H * sc) fmax = H * sc;
  const size_t lds = (size_t)cd * (fmax + th) * Wo * sizeof(float);
  const int kc = (fmax * (Wo / 4) + PAF_THREADS - 1) / PAF_THREADS;
  if (lds > 64 * 1024 || kc > 6) return 1;
  const dim3 grid(H / th, D / cd, (unsigned)P);
#define PAF_LAUNCH(KC, B) hipLaunchKernelGGL((planes_adjoint_fused_kernel<KC, B>), grid, dim3(PAF_THREADS), lds, st, in, out, D, H, W, sc, cd, th, \
                                             fmax, ac_scale(D, D * sc), ac_scale(H, H * sc), ac_scale(W, W * sc))
  if (kc <= 2) PAF_LAUNCH(2, 8);
  else if (kc <= 4) PAF_LAUNCH(4, 4);
  else PAF_LAUNCH(6, 2);
#undef PAF_LAUNCH
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t BRATS_API(brats_upsample_bwd_ws_bytes)(int dtype, int N, int C, int D, int H, int W, int scale) {
  const size_t esz = dtype == BRATS_BF16 ? 2 : 4;
  const size_t a = (size_t)N * D * (H * scale) * (W * scale) * C;  // after the D pass
  const size_t b = (size_t)N * D * H * (W * scale) * C;            // after the H pass
  return ((a * esz + 255) / 256 * 256) + ((b * esz + 255) / 256 * 256);
}

template <typename T>
static int upsample_bwd_t(const T* dy, int dypitch, T* dx, int dxpitch, char* tmp, int N, int C, int D, int H, int W, int sc,
                          hipStream_t st, const T* add = nullptr, int addpitch = 0) {
  constexpr int VW = 16 / sizeof(T);
  const int Do = D * sc, Ho = H * sc, Wo = W * sc;
  if constexpr (sizeof(T) == 2) {
    if (const int cd = upsample_bwd_fused_cd(N, C, D, H, W, sc)) {  // one launch, nothing through tmp
      const dim3 grid((unsigned)((size_t)N * (H / UBF_TH) * (W / UBF_TW) * (C / UBF_CS) * (D / cd)));
      if (add)
        hipLaunchKernelGGL(upsample2_bwd_fused_kernel<true>, grid, dim3(UBF_THREADS), 0, st, dy, dypitch, dx, dxpitch, C, D, H, W, cd,
                           ac_scale(D, Do), ac_scale(H, Ho), ac_scale(W, Wo), add, addpitch);
      else
        hipLaunchKernelGGL(upsample2_bwd_fused_kernel<false>, grid, dim3(UBF_THREADS), 0, st, dy, dypitch, dx, dxpitch, C, D, H, W, cd,
                           ac_scale(D, Do), ac_scale(H, Ho), ac_scale(W, Wo), (const bf16_t*)nullptr, 0);
      BRATS_CHECK_LAUNCH();
      return 0;
    }
  }
  const size_t a_elems = (size_t)N * D * Ho * Wo * C;
  T* t1 = (T*)tmp;
  T* t2 = (T*)(tmp + ((a_elems * sizeof(T) + 255) / 256 * 256));
  // D axis: [N][Do][Ho*Wo][C] -> [N][D][Ho*Wo][C]
  size_t total = (size_t)N * D * Ho * Wo * (C / VW);
  hipLaunchKernelGGL((lerp_adjoint_kernel<T, T, VW>), dim3(stream_grid(total, 256, POOL_MAX_BLOCKS)), dim3(256), 0, st, dy, dypitch, t1, C,
                     (size_t)N, Do, D, (size_t)Ho * Wo, C, ac_scale(D, Do));
  // H axis: [N*D][Ho][Wo][C] -> [N*D][H][Wo][C]
  total = (size_t)N * D * H * Wo * (C / VW);
  hipLaunchKernelGGL((lerp_adjoint_kernel<T, T, VW>), dim3(stream_grid(total, 256, POOL_MAX_BLOCKS)), dim3(256), 0, st, (const T*)t1, C, t2, C,
                     (size_t)N * D, Ho, H, (size_t)Wo, C, ac_scale(H, Ho));
  // W axis: [N*D*H][Wo][1][C] -> [N*D*H][W][1][C(pitch)]
  total = (size_t)N * D * H * W * (C / VW);
  if (add)
    hipLaunchKernelGGL((lerp_adjoint_kernel<T, T, VW, true>), dim3(stream_grid(total, 256, POOL_MAX_BLOCKS)), dim3(256), 0, st, (const T*)t2, C,
                       dx, dxpitch, (size_t)N * D * H, Wo, W, (size_t)1, C, ac_scale(W, Wo), add, addpitch);
  else
    hipLaunchKernelGGL((lerp_adjoint_kernel<T, T, VW>), dim3(stream_grid(total, 256, POOL_MAX_BLOCKS)), dim3(256), 0, st, (const T*)t2, C, dx,
                       dxpitch, (size_t)N * D * H, Wo, W, (size_t)1, C, ac_scale(W, Wo), (const T*)nullptr, 0);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int BRATS_API(brats_upsample_bwd)(const void* dy, int dypitch, void* dx, int dxpitch, void* tmp, int dtype, int N, int C,
                                  int D, int H, int W, int scale, brats_stream_t s) {
  const int vw = vec_width(dtype);
  if (!dy || !dx || !tmp || C % vw || dypitch % vw || dxpitch % vw) BRATS_FAIL(BRATS_E_ARG, "upsample_bwd: bad argument");
  return with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return upsample_bwd_t<T>((const T*)dy, dypitch, (T*)dx, dxpitch, (char*)tmp, N, C, D, H, W, scale, (hipStream_t)s);
  });
}
// dx = stored(adjoint of dy) + add, bit-equal to brats_upsample_bwd followed by an elementwise add of the two tensors (the f32
// sum of the two stored values, rounded once); add has dx's extent and must not overlap dx
extern "C" int BRATS_API(brats_upsample_bwd_add)(const void* dy, int dypitch, const void* add, int addpitch, void* dx, int dxpitch,
                                                 void* tmp, int dtype, int N, int C, int D, int H, int W, int scale, brats_stream_t s) {
  const int vw = vec_width(dtype);
  if (!dy || !add || !dx || !tmp || C % vw || dypitch % vw || dxpitch % vw || addpitch % vw)
    BRATS_FAIL(BRATS_E_ARG, "upsample_bwd_add: bad argument");
  return with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return upsample_bwd_t<T>((const T*)dy, dypitch, (T*)dx, dxpitch, (char*)tmp, N, C, D, H, W, scale, (hipStream_t)s, (const T*)add,
                             addpitch);
  });
}
#include "twin_end.hpp"
