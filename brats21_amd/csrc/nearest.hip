// Nearest-neighbour up-sampling (nn.Upsample(scale_factor=s) in its default mode, networks/unet_family.py:43,170-172) and its
// adjoint: x2 on NDHWC activations (UpConv), x2 / x4 / x8 on f32 NCDHW planes (the deep-supervision logits).
// All four are streaming passes: every input byte is read once and every output byte written once, 16 bytes per lane along C
// (NDHWC) or s floats per lane along W (planes).  The forward passes do no arithmetic; the adjoints sum the s^3 children of a
// coarse element in one fixed order in f32 (no atomics, no workspace).
#include "common.hpp"

namespace {

constexpr int NEAR_MAX_BLOCKS = 1 << 20;  // of the grid-stride passes

// ---- 16-byte vectors of the three storage types <-> float registers --------------------------------------------------
// (this translation unit is built once: inside it bf16 is common.hpp's 16-bit type, fp16 is converted here)
template <int DT> struct St;
template <> struct St<BRATS_F32> {
  static constexpr int VW = 4;
  static DEVI void unpack(u32x4 v, float* o) {
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = __uint_as_float(v[i]);
  }
  static DEVI u32x4 pack(const float* o) { return u32x4{__float_as_uint(o[0]), __float_as_uint(o[1]), __float_as_uint(o[2]), __float_as_uint(o[3])}; }
};
template <> struct St<BRATS_BF16> {
  static constexpr int VW = 8;
  static DEVI void unpack(u32x4 v, float* o) {
#pragma unroll
    for (int i = 0; i < 4; ++i) unpack2(v[i], o[2 * i], o[2 * i + 1]);
  }
  static DEVI u32x4 pack(const float* o) {
    u32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = pack2(o[2 * i], o[2 * i + 1]);
    return v;
  }
};
typedef __attribute__((ext_vector_type(2))) _Float16 near_h2;
template <> struct St<BRATS_F16> {
  static constexpr int VW = 8;
  static DEVI void unpack(u32x4 v, float* o) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t w = v[i];
      const near_h2 h = __builtin_bit_cast(near_h2, w);
      o[2 * i] = (float)h[0];
      o[2 * i + 1] = (float)h[1];
    }
  }
  static DEVI u32x4 pack(const float* o) {
    u32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x2_ f = {o[2 * i], o[2 * i + 1]};
      v[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, near_h2));  // RNE
    }
    return v;
  }
};

template <bool NT> DEVI u32x4 ld16(const u32x4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT> DEVI void st16(u32x4* p, u32x4 v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// ---- NDHWC x2 ---------------------------------------------------------------------------------------------------------
// Pointers and pitches in 16-byte vectors; cv = vectors per voxel.  One workgroup per coarse row (n, z, y) and turn: lane i of
// the row takes fine voxel j = i / cv and channel vector c, reads x[j / 2][c] (the two lanes that share it hit the same line) and
// writes the four fine rows (2z + a, 2y + b) at [j][c] -- every store instruction covers a contiguous stretch of a fine row.
template <bool NT>
__global__ void __launch_bounds__(256) nearest2_fwd_kernel(const u32x4* __restrict__ x, int xpitch, u32x4* __restrict__ y, int ypitch, int cv,
                                                           int D, int H, int W, size_t rows) {
  const int items = 2 * W * cv;
  const size_t ystep = (size_t)2 * W * ypitch, zstep = (size_t)2 * H * ystep;
  for (size_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const int yy = (int)(r % H);
    const size_t q = r / H;
    const int z = (int)(q % D);
    const size_t n = q / D;
    const u32x4* xr = x + r * W * xpitch;
    u32x4* yr = y + ((n * 2 * D + 2 * z) * 2 * H + 2 * yy) * ystep;
    for (int i = threadIdx.x; i < items; i += 256) {
      const int j = i / cv, c = i - j * cv;
      const u32x4 v = xr[(size_t)(j >> 1) * xpitch + c];
      u32x4* o = yr + (size_t)j * ypitch + c;
      st16<NT>(o, v);
      st16<NT>(o + ystep, v);
      st16<NT>(o + zstep, v);
      st16<NT>(o + zstep + ystep, v);
    }
  }
}

// dx[n][z][y][x][:] = sum of the 8 children of dy in the order (a, b, e) = (z, y, x offset), e fastest: f32, rounded once.
// ADD: the sum rounded to the storage type, plus the addend in f32, stored once -- what an elementwise add of the two stored
// tensors computes.
template <int DT, bool ADD, bool NT>
__global__ void __launch_bounds__(256) nearest2_bwd_kernel(const u32x4* __restrict__ dy, int dypitch, const u32x4* __restrict__ add, int addpitch,
                                                           u32x4* __restrict__ dx, int dxpitch, int cv, int D, int H, int W, size_t rows) {
  using S = St<DT>;
  constexpr int VW = S::VW;
  const int items = W * cv;
  const size_t ystep = (size_t)2 * W * dypitch, zstep = (size_t)2 * H * ystep;
  for (size_t r = blockIdx.x; r < rows; r += gridDim.x) {
    const int yy = (int)(r % H);
    const size_t q = r / H;
    const int z = (int)(q % D);
    const size_t n = q / D;
    const u32x4* dyr = dy + ((n * 2 * D + 2 * z) * 2 * H + 2 * yy) * ystep;
    for (int i = threadIdx.x; i < items; i += 256) {
      const int j = i / cv, c = i - j * cv;
      const u32x4* p = dyr + (size_t)(2 * j) * dypitch + c;
      u32x4 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = ld16<NT>(p + (k >> 2) * zstep + ((k >> 1) & 1) * ystep + (size_t)(k & 1) * dypitch);
      float acc[VW], t[VW];
      S::unpack(v[0], acc);
#pragma unroll
      for (int k = 1; k < 8; ++k) {
        S::unpack(v[k], t);
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[e] += t[e];
      }
      if constexpr (ADD) {
        S::unpack(S::pack(acc), acc);
        S::unpack(add[(r * W + j) * addpitch + c], t);
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[e] += t[e];
      }
      dx[(r * W + j) * dxpitch + c] = S::pack(acc);
    }
  }
}

// ---- f32 NCDHW planes, scale S in {2, 4, 8} -----------------------------------------------------------------------------
// One lane per coarse element (p, z, y, x): its S^3 block is S * S fine rows of S contiguous floats, moved as vectors of
// min(S, 4) floats (S = 2: the fine row length 2 W need not be a multiple of 4) -- adjacent lanes cover adjacent stretches.
template <int S> struct PlaneVec { typedef f32x4 type; static constexpr int N = 4; };
template <> struct PlaneVec<2> { typedef f32x2 type; static constexpr int N = 2; };

template <int S>
__global__ void __launch_bounds__(256) planes_nearest_fwd_kernel(const float* __restrict__ low, float* __restrict__ out, size_t total, int H, int W) {
  using V = typename PlaneVec<S>::type;
  constexpr int VN = PlaneVec<S>::N;
  const size_t Wo = (size_t)W * S, Ho = (size_t)H * S;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(it % W);
    size_t q = it / W;
    const int y = (int)(q % H);
    q /= H;  // p * D + z
    const float f = low[it];
    V v;
#pragma unroll
    for (int e = 0; e < VN; ++e) v[e] = f;
    float* o = out + ((q * S) * Ho + (size_t)y * S) * Wo + (size_t)x * S;
    for (int a = 0; a < S; ++a)
#pragma unroll
      for (int b = 0; b < S; ++b)
#pragma unroll
        for (int e = 0; e < S / VN; ++e) *(V*)(o + (a * Ho + b) * Wo + e * VN) = v;
  }
}

// dlow[p][z][y][x] = sum of the S^3 block of dout in the order (a, b, e), e fastest, in f32
template <int S>
__global__ void __launch_bounds__(256) planes_nearest_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dlow, size_t total, int H, int W) {
  using V = typename PlaneVec<S>::type;
  constexpr int VN = PlaneVec<S>::N;
  const size_t Wo = (size_t)W * S, Ho = (size_t)H * S;
  for (size_t it = (size_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(it % W);
    size_t q = it / W;
    const int y = (int)(q % H);
    q /= H;
    const float* p = dout + ((q * S) * Ho + (size_t)y * S) * Wo + (size_t)x * S;
    float acc = 0.f;
    for (int a = 0; a < S; ++a)
#pragma unroll
      for (int b = 0; b < S; ++b)
#pragma unroll
        for (int e = 0; e < S / VN; ++e) {
          const V v = *(const V*)(p + (a * Ho + b) * Wo + e * VN);
#pragma unroll
          for (int k = 0; k < VN; ++k) acc += v[k];
        }
    dlow[it] = acc;
  }
}

// storage type of a dtype code (the split-precision codes are f32 tensors); -1: unknown
int storage_of(int dtype) {
  if (dtype == BRATS_F32 || dtype == BRATS_X3_BF16 || dtype == BRATS_X3_F16) return BRATS_F32;
  return (dtype == BRATS_BF16 || dtype == BRATS_F16) ? dtype : -1;
}

// nonzero (after BRATS_FAIL) when the shape / pitches of an NDHWC x2 call are not what the kernels take
int nearest_check(const char* who, int dtype, int N, int C, int D, int H, int W, int scale, const int* pitches, int np) {
  const int st = storage_of(dtype);
  if (st < 0) BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: dtype %d (F32 | BF16 | F16)", who, dtype);
  if (scale != 2) BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: scale %d (the NDHWC pair is built for scale 2)", who, scale);
  if (N < 1 || C < 1 || D < 1 || H < 1 || W < 1) BRATS_FAIL(BRATS_E_ARG, "%s: N=%d C=%d D=%d H=%d W=%d", who, N, C, D, H, W);
  const int vw = st == BRATS_F32 ? 4 : 8;
  if (C % vw) BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: C = %d must be a multiple of %d (16-byte channel vectors)", who, C, vw);
  for (int i = 0; i < np; ++i)
    if (pitches[i] < C || pitches[i] % vw) BRATS_FAIL(BRATS_E_ARG, "%s: pitch %d (>= C = %d, a multiple of %d)", who, pitches[i], C, vw);
  if ((size_t)2 * W * (C / vw) > (size_t)INT32_MAX) BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: a fine row of %d x %d channels is too long", who, 2 * W, C);
  return 0;
}

int planes_check(const char* who, int planes, int D, int H, int W, int scale) {
  if (scale != 2 && scale != 4 && scale != 8) BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: scale %d (2, 4 or 8)", who, scale);
  if (planes < 1 || D < 1 || H < 1 || W < 1) BRATS_FAIL(BRATS_E_ARG, "%s: planes=%d D=%d H=%d W=%d", who, planes, D, H, W);
  return 0;
}

}  // namespace

extern "C" int brats_upsample_nearest_fwd(const void* x, int xpitch, void* y, int ypitch, int dtype, int N, int C, int D, int H, int W, int scale,
                                          brats_stream_t s) {
  if (!x || !y) BRATS_FAIL(BRATS_E_ARG, "upsample_nearest_fwd: null pointer");
  const int pitches[2] = {xpitch, ypitch};
  if (const int rc = nearest_check("upsample_nearest_fwd", dtype, N, C, D, H, W, scale, pitches, 2)) return rc;
  const int vw = storage_of(dtype) == BRATS_F32 ? 4 : 8, es = 16 / vw;
  const size_t rows = (size_t)N * D * H;
  const bool nt = stream_nt(rows * W * 8 * C * es);  // the output cannot stay in the Infinity Cache: non-temporal stores
  const dim3 grid((unsigned)(rows > (size_t)NEAR_MAX_BLOCKS ? (size_t)NEAR_MAX_BLOCKS : rows));
  with_flag(nt, [&](auto f) {
    hipLaunchKernelGGL((nearest2_fwd_kernel<decltype(f)::value>), grid, dim3(256), 0, (hipStream_t)s, (const u32x4*)x, xpitch / vw, (u32x4*)y,
                       ypitch / vw, C / vw, D, H, W, rows);
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_upsample_nearest_bwd(const void* dy, int dypitch, const void* add, int addpitch, void* dx, int dxpitch, int dtype, int N, int C,
                                          int D, int H, int W, int scale, brats_stream_t s) {
  if (!dy || !dx) BRATS_FAIL(BRATS_E_ARG, "upsample_nearest_bwd: null pointer");
  const int pitches[3] = {dypitch, dxpitch, addpitch};
  if (const int rc = nearest_check("upsample_nearest_bwd", dtype, N, C, D, H, W, scale, pitches, add ? 3 : 2)) return rc;
  const int st = storage_of(dtype), vw = st == BRATS_F32 ? 4 : 8, es = 16 / vw;
  const size_t rows = (size_t)N * D * H;
  const bool nt = stream_nt(rows * W * 8 * C * es);  // dy is streamed once and is too large to have stayed in the cache
  const dim3 grid((unsigned)(rows > (size_t)NEAR_MAX_BLOCKS ? (size_t)NEAR_MAX_BLOCKS : rows));
  auto go = [&](auto dt, auto with_add, auto f) {
    hipLaunchKernelGGL((nearest2_bwd_kernel<decltype(dt)::value, decltype(with_add)::value, decltype(f)::value>), grid, dim3(256), 0,
                       (hipStream_t)s, (const u32x4*)dy, dypitch / vw, (const u32x4*)add, addpitch / vw, (u32x4*)dx, dxpitch / vw, C / vw, D, H, W,
                       rows);
  };
  with_flag(add != nullptr, [&](auto with_add) {
    with_flag(nt, [&](auto f) {
      if (st == BRATS_F32) go(std::integral_constant<int, BRATS_F32>{}, with_add, f);
      else if (st == BRATS_BF16) go(std::integral_constant<int, BRATS_BF16>{}, with_add, f);
      else go(std::integral_constant<int, BRATS_F16>{}, with_add, f);
    });
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_planes_nearest_fwd(const float* low, float* out, int planes, int D, int H, int W, int scale, brats_stream_t s) {
  if (!low || !out) BRATS_FAIL(BRATS_E_ARG, "planes_nearest_fwd: null pointer");
  if (const int rc = planes_check("planes_nearest_fwd", planes, D, H, W, scale)) return rc;
  const size_t total = (size_t)planes * D * H * W;
  const dim3 grid(stream_grid(total, 256, NEAR_MAX_BLOCKS));
  hipStream_t st = (hipStream_t)s;
  if (scale == 2) hipLaunchKernelGGL(planes_nearest_fwd_kernel<2>, grid, dim3(256), 0, st, low, out, total, H, W);
  else if (scale == 4) hipLaunchKernelGGL(planes_nearest_fwd_kernel<4>, grid, dim3(256), 0, st, low, out, total, H, W);
  else hipLaunchKernelGGL(planes_nearest_fwd_kernel<8>, grid, dim3(256), 0, st, low, out, total, H, W);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_planes_nearest_bwd(const float* dout, float* dlow, int planes, int D, int H, int W, int scale, brats_stream_t s) {
  if (!dout || !dlow) BRATS_FAIL(BRATS_E_ARG, "planes_nearest_bwd: null pointer");
  if (const int rc = planes_check("planes_nearest_bwd", planes, D, H, W, scale)) return rc;
  const size_t total = (size_t)planes * D * H * W;
  const dim3 grid(stream_grid(total, 256, NEAR_MAX_BLOCKS));
  hipStream_t st = (hipStream_t)s;
  if (scale == 2) hipLaunchKernelGGL(planes_nearest_bwd_kernel<2>, grid, dim3(256), 0, st, dout, dlow, total, H, W);
  else if (scale == 4) hipLaunchKernelGGL(planes_nearest_bwd_kernel<4>, grid, dim3(256), 0, st, dout, dlow, total, H, W);
  else hipLaunchKernelGGL(planes_nearest_bwd_kernel<8>, grid, dim3(256), 0, st, dout, dlow, total, H, W);
  BRATS_CHECK_LAUNCH();
  return 0;
}
