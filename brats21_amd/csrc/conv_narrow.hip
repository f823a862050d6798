// Narrow-output 3x3x3 convolution: C (any multiple of 8) input channels -> K <= 16 output planes, zero padding, dilation 1,
//   out[n][k][z][y][x] (f32, NCDHW) = add[n][k][z][y][x] (optional) + bias[k] (optional) + sum_taps sum_c w[k][c][tap] * x[n][z+dz][y+dy][x+dx][c]
// with x NDHWC (bf16, fp16 or f32; a channel slice with a pitch is fine) and f32 accumulation.  Two users (networks/equiunet.py,
// the refinement stage): the last convolution of RefUnet, f0 -> num_classes, whose residual `add` is the unrefined logits -- the
// refined logits leave in one pass, as f32 planes, without a padded 16-bit intermediate and without rounding the residual -- and
// the input gradient of RefUnet's first convolution (the same shape: the pack step transposes the weights and flips the taps),
// whose `add` is the gradient that reaches the unrefined logits from the loss.
//
// The implicit-GEMM kernels (conv_igemm.hpp) have 16 x 8 or wider output-channel fragments and write NDHWC in the storage
// type; with 1 - 16 rows in use this shape is bound by the 2 C bytes per voxel it reads.  Form: a workgroup owns an 8 x 8 x 16
// output tile; per chunk of 8 channels its 10 x 10 x 18 halo is staged ONCE into LDS and every tap reads from there.
//   * bf16 / fp16 (one template parameter, no twin build): 16 class rows x 16 voxels per v_mfma_f32_16x16x32, contracting over
//     (tap, channel) groups -- conv_narrow_mfma_kernel below;
//   * f32 (the exact mode and the split-precision mode, whose tensors are f32): plain f32 FMAs in a fixed order -- a thread owns four
//     consecutive x of one row and keeps the 6 x 8 inputs of a (dz, dy) row pair in registers across the three dx taps; the
//     weights are wave-uniform: packed [chunk][tap][c][KT] they are read through the scalar cache and enter the FMAs as scalar
//     operands, pairs of classes per packed FMA, nothing per element from LDS.
#include "common.hpp"

namespace {
constexpr int NT_Z = 8, NT_Y = 8, NT_X = 16;               // output tile
constexpr int NH_Y = NT_Y + 2, NH_X = NT_X + 2;            // halo extents (z: NT_Z + 2)
constexpr int NH_VOX = (NT_Z + 2) * NH_Y * NH_X;           // 1800 halo voxels x 8 channels x 4 bytes = 57 600 bytes of LDS
constexpr int N_CH = 8;                                    // channels per chunk
constexpr int N_KMAX = 16;

// class tile: the smallest even instantiation that holds K
inline int narrow_kt(int K) { return K <= 2 ? 2 : K <= 4 ? 4 : K <= 6 ? 6 : K <= 8 ? 8 : K <= 12 ? 12 : 16; }

template <int KT>
__global__ void __launch_bounds__(256) conv_narrow_kernel(const float* __restrict__ x, int C, int xpitch, const float* __restrict__ wp,
                                                          const float* __restrict__ bias, const float* __restrict__ add,
                                                          float* __restrict__ out, int K, int D, int H, int W, int tiles_x, int tiles_y,
                                                          int vec) {
  __shared__ __attribute__((aligned(16))) float halo[NH_VOX * N_CH];
  const int n = blockIdx.y;
  int t = blockIdx.x;
  const int bx = t % tiles_x; t /= tiles_x;
  const int by = t % tiles_y;
  const int bz = t / tiles_y;
  const int z0 = bz * NT_Z, y0 = by * NT_Y, x0 = bx * NT_X;
  const int tid = threadIdx.x, xg = tid & 3, ty = (tid >> 2) & 7, tz = tid >> 5;
  const float* xn = x + (size_t)n * D * H * W * xpitch;

  f32x2 acc[KT / 2][4];
#pragma unroll
  for (int kp = 0; kp < KT / 2; ++kp)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[kp][j] = f32x2{0.f, 0.f};

  const int nchunks = C / N_CH;
  for (int ch = 0; ch < nchunks; ++ch) {
    __syncthreads();  // (the previous chunk's readers are done)
    for (int i = tid; i < NH_VOX; i += 256) {
      const int hx = i % NH_X, hy = (i / NH_X) % NH_Y, hz = i / (NH_X * NH_Y);
      const int gz = z0 + hz - 1, gy = y0 + hy - 1, gx = x0 + hx - 1;
      f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
      if (gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const f32x4* src = (const f32x4*)(xn + (((size_t)gz * H + gy) * W + gx) * xpitch + (size_t)ch * N_CH);
        lo = src[0];
        hi = src[1];
      }
      f32x4* dst = (f32x4*)(halo + i * N_CH);
      dst[0] = lo;
      dst[1] = hi;
    }
    __syncthreads();
    const float* wc = wp + (size_t)ch * 27 * N_CH * KT;
#pragma unroll 1
    for (int dzy = 0; dzy < 9; ++dzy) {
      const int dz = dzy / 3, dy = dzy % 3;
      const float* row = halo + (((tz + dz) * NH_Y + ty + dy) * NH_X + xg * 4) * N_CH;
      float xs[6][N_CH];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const f32x4 a = ((const f32x4*)(row + i * N_CH))[0], b = ((const f32x4*)(row + i * N_CH))[1];
#pragma unroll
        for (int c = 0; c < 4; ++c) { xs[i][c] = a[c]; xs[i][4 + c] = b[c]; }
      }
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const float* wt = wc + (dzy * 3 + dx) * N_CH * KT;  // wave-uniform: scalar loads
#pragma unroll
        for (int c = 0; c < N_CH; ++c)
#pragma unroll
          for (int kp = 0; kp < KT / 2; ++kp) {
            const f32x2 wv = {wt[c * KT + 2 * kp], wt[c * KT + 2 * kp + 1]};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const f32x2 xv = {xs[j + dx][c], xs[j + dx][c]};
              acc[kp][j] = __builtin_elementwise_fma(wv, xv, acc[kp][j]);
            }
          }
      }
    }
  }

  const int gz = z0 + tz, gy = y0 + ty, gx = x0 + xg * 4;
  if (gz >= D || gy >= H || gx >= W) return;
  const size_t plane = (size_t)D * H * W;
  const size_t off = ((size_t)gz * H + gy) * W + gx;
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    if (k >= K) continue;
    const size_t o = ((size_t)n * K + k) * plane + off;
    const float b = bias ? bias[k] : 0.f;
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = acc[k >> 1][j][k & 1];
    if (vec) {  // W % 4 == 0 and 16-byte aligned planes: gx + 3 < W
      if (add) {
        const f32x4 a = *(const f32x4*)(add + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = a[j] + b + r[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = b + r[j];
      }
      *(f32x4*)(out + o) = f32x4{r[0], r[1], r[2], r[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (gx + j < W) out[o + j] = (add ? add[o + j] + b : b) + r[j];
    }
  }
}

// 16-bit storage: the same tile on the matrix pipe.  One v_mfma_f32_16x16x32 holds 16 class rows x 16 voxels (one x row of the tile)
// and contracts over 32 = 4 groups of (tap, 8 channels): per chunk of 8 channels the 27 taps are 7 steps (the 28th group has zero
// weights and a zeroed operand).  Lane (v, q) reads voxel v's 8 channels at tap 4 step + q as ONE 16-byte LDS read and holds row
// v of the packed weights [chunk][step][lane][8] (16-bit, 16 bytes per lane from global / L2, seven fragments per chunk kept in
// registers).  A wave owns 16 of the tile's 64 rows; the accumulator lane (v, q) ends with classes 4q .. 4q + 3 of voxel v.
constexpr int NM_STEPS = 7;
typedef __attribute__((ext_vector_type(8))) __bf16 nbf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 nf16x8;
template <int DT> DEVI f32x4 narrow_mfma(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (DT == BRATS_BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(nbf16x8, a), __builtin_bit_cast(nbf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(nf16x8, a), __builtin_bit_cast(nf16x8, b), c, 0, 0, 0);
}

template <int DT>
__global__ void __launch_bounds__(256) conv_narrow_mfma_kernel(const void* __restrict__ x, int C, int xpitch, const u32x4* __restrict__ wa,
                                                               const float* __restrict__ bias, const float* __restrict__ add,
                                                               float* __restrict__ out, int K, int D, int H, int W, int tiles_x, int tiles_y) {
  __shared__ u32x4 halo[NH_VOX];  // 8 channels of the storage type per halo voxel: 28 800 bytes
  const int n = blockIdx.y;
  int t = blockIdx.x;
  const int bx = t % tiles_x; t /= tiles_x;
  const int by = t % tiles_y;
  const int bz = t / tiles_y;
  const int z0 = bz * NT_Z, y0 = by * NT_Y, x0 = bx * NT_X;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, v = lane & 15, q = lane >> 4;
  const char* xn = (const char*)x + (size_t)n * D * H * W * xpitch * 2;
  int toff[NM_STEPS];
#pragma unroll
  for (int s = 0; s < NM_STEPS; ++s) {
    const int g = 4 * s + q, tap = g < 27 ? g : 0;
    toff[s] = ((tap / 9) * NH_Y + (tap / 3) % 3) * NH_X + tap % 3;
  }
  f32x4 acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  // staging: thread tid owns the halo voxels tid + 256 j.  Their global offsets do not depend on the chunk, and the loads of chunk
  // ch + 1 are issued before the MFMA phase of chunk ch, so that their latency is covered by it
  constexpr int NSTG = (NH_VOX + 255) / 256;
  size_t goff[NSTG];
  unsigned inb = 0;
#pragma unroll
  for (int j = 0; j < NSTG; ++j) {
    const int i = tid + 256 * j;
    const int hx = i % NH_X, hy = (i / NH_X) % NH_Y, hz = i / (NH_X * NH_Y);
    const int gz = z0 + hz - 1, gy = y0 + hy - 1, gx = x0 + hx - 1;
    const bool in = i < NH_VOX && gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W;
    goff[j] = in ? (((size_t)gz * H + gy) * W + gx) * xpitch * 2 : 0;
    inb |= in ? 1u << j : 0u;
  }
  u32x4 pre[NSTG];
  auto fetch = [&](int ch) {
#pragma unroll
    for (int j = 0; j < NSTG; ++j) {
      pre[j] = u32x4{0u, 0u, 0u, 0u};
      if (inb >> j & 1u) pre[j] = *(const u32x4*)(xn + goff[j] + (size_t)ch * N_CH * 2);
    }
  };
  fetch(0);
  const int nchunks = C / N_CH;
  for (int ch = 0; ch < nchunks; ++ch) {
    __syncthreads();  // (the previous chunk's readers are done)
#pragma unroll
    for (int j = 0; j < NSTG; ++j)
      if (tid + 256 * j < NH_VOX) halo[tid + 256 * j] = pre[j];
    u32x4 a[NM_STEPS];
#pragma unroll
    for (int s = 0; s < NM_STEPS; ++s) a[s] = wa[((size_t)ch * NM_STEPS + s) * 64 + lane];
    __syncthreads();
    if (ch + 1 < nchunks) fetch(ch + 1);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int rho = wave * 16 + i;
      const int base = ((rho >> 3) * NH_Y + (rho & 7)) * NH_X + v;
#pragma unroll
      for (int s = 0; s < NM_STEPS; ++s) {
        u32x4 b = halo[base + toff[s]];
        if (s == NM_STEPS - 1 && q == 3) b = u32x4{0u, 0u, 0u, 0u};  // the 28th group: no tap
        acc[i] = narrow_mfma<DT>(a[s], b, acc[i]);
      }
    }
  }
  const size_t plane = (size_t)D * H * W;
  const int gx = x0 + v;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int rho = wave * 16 + i;
    const int gz = z0 + (rho >> 3), gy = y0 + (rho & 7);
    if (gz >= D || gy >= H || gx >= W) continue;
    const size_t off = ((size_t)gz * H + gy) * W + gx;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 4 * q + r;
      if (k >= K) continue;
      const size_t o = ((size_t)n * K + k) * plane + off;
      const float b = bias ? bias[k] : 0.f;
      out[o] = (add ? add[o] + b : b) + acc[i][r];
    }
  }
}

// packed [C / 8][27][8][KT] f32 from torch-layout w [cout_w][cin_w][27].  BRATS_PACK_FWD: class row k = output channel, channel
// c = input channel (K = cout_w, C = cin_w).  BRATS_PACK_DGRAD: class row k = INPUT channel, c = output channel, tap 26 - tap
// (K = cin_w, C = cout_w): the input gradient as a convolution of dy.  Rows k >= K are zero.
__global__ void conv_narrow_pack_kernel(const float* __restrict__ w, float* __restrict__ packed, int mode, int cout_w, int cin_w, int C, int KT,
                                        int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int k = i % KT, c = (i / KT) % N_CH, tap = (i / (KT * N_CH)) % 27, ch = i / (KT * N_CH * 27);
  const int cc = ch * N_CH + c;
  const int K = mode == BRATS_PACK_FWD ? cout_w : cin_w;
  float v = 0.f;
  if (k < K && cc < C)
    v = mode == BRATS_PACK_FWD ? w[((size_t)k * cin_w + cc) * 27 + tap] : w[((size_t)cc * cin_w + k) * 27 + (26 - tap)];
  packed[i] = v;
}

// the MFMA fragments [C / 8][7][64 lanes][8] of the same weights, rounded to bf16 (section 0) and to fp16 (section 1): lane (r, q) of
// step s holds class row r, tap 4 s + q, the chunk's 8 channels
__global__ void conv_narrow_pack16_kernel(const float* __restrict__ w, uint16_t* __restrict__ frag, int mode, int cout_w, int cin_w, int C,
                                          int total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = i % 8, lane = (i / 8) % 64, s = (i / 512) % NM_STEPS, ch = i / (512 * NM_STEPS);
  const int r = lane & 15, tap = 4 * s + (lane >> 4), cc = ch * N_CH + j;
  const int K = mode == BRATS_PACK_FWD ? cout_w : cin_w;
  float v = 0.f;
  if (r < K && tap < 27)
    v = mode == BRATS_PACK_FWD ? w[((size_t)r * cin_w + cc) * 27 + tap] : w[((size_t)cc * cin_w + r) * 27 + (26 - tap)];
  frag[i] = __builtin_bit_cast(uint16_t, (__bf16)v);
  frag[(size_t)total + i] = __builtin_bit_cast(uint16_t, (_Float16)v);
}

bool narrow_dims(int mode, int cout_w, int cin_w, int* C, int* K) {
  if (mode != BRATS_PACK_FWD && mode != BRATS_PACK_DGRAD) return false;
  *C = mode == BRATS_PACK_FWD ? cin_w : cout_w;
  *K = mode == BRATS_PACK_FWD ? cout_w : cin_w;
  return *C >= N_CH && *C % N_CH == 0 && *K >= 1 && *K <= N_KMAX;
}
}  // namespace

// f32 section [C / 8][27][8][KT], then the bf16 and the fp16 MFMA fragments ([C / 8][7][64][8] each)
static size_t narrow_f32_floats(int C, int K) { return (size_t)C * 27 * narrow_kt(K); }
static size_t narrow_frag_elems(int C) { return (size_t)(C / N_CH) * NM_STEPS * 64 * 8; }
extern "C" size_t brats_conv3d_narrow_packed_bytes(int C, int K) {
  if (C < N_CH || C % N_CH || K < 1 || K > N_KMAX) return 0;
  return narrow_f32_floats(C, K) * sizeof(float) + 2 * narrow_frag_elems(C) * sizeof(uint16_t);
}

extern "C" int brats_conv3d_narrow_pack(const float* w, float* packed, int mode, int cout_w, int cin_w, brats_stream_t s) {
  int C, K;
  if (!w || !packed || !narrow_dims(mode, cout_w, cin_w, &C, &K))
    BRATS_FAIL(BRATS_E_ARG, "conv3d_narrow_pack: bad argument (channels a multiple of 8, 1 - 16 class rows; cout_w=%d cin_w=%d mode=%d)", cout_w, cin_w, mode);
  const int kt = narrow_kt(K), total = C * 27 * kt;
  hipLaunchKernelGGL(conv_narrow_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)s, w, packed, mode, cout_w, cin_w, C, kt, total);
  const int ftotal = (int)narrow_frag_elems(C);
  hipLaunchKernelGGL(conv_narrow_pack16_kernel, dim3((ftotal + 255) / 256), dim3(256), 0, (hipStream_t)s, w, (uint16_t*)(packed + narrow_f32_floats(C, K)),
                     mode, cout_w, cin_w, C, ftotal);
  BRATS_CHECK_LAUNCH();
  return 0;
}

static int narrow_launch(int kt, dim3 grid, hipStream_t st, const float* x, int C, int xpitch, const float* wp, const float* bias, const float* add,
                         float* out, int K, int D, int H, int W, int tx, int ty, int vec) {
#define NARROW_CASE(KT) case KT: hipLaunchKernelGGL(conv_narrow_kernel<KT>, grid, dim3(256), 0, st, x, C, xpitch, wp, bias, add, out, K, D, H, W, tx, ty, vec); break
  switch (kt) {
    NARROW_CASE(2);
    NARROW_CASE(4);
    NARROW_CASE(6);
    NARROW_CASE(8);
    NARROW_CASE(12);
    NARROW_CASE(16);
  }
#undef NARROW_CASE
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_conv3d_narrow_fwd(const void* x, int C, int xpitch, const float* packed_w, const float* bias, const float* add, float* out,
                                       int dtype, int K, int N, int D, int H, int W, brats_stream_t s) {
  if (!x || !packed_w || !out || C < N_CH || C % N_CH || xpitch < C || xpitch % N_CH || K < 1 || K > N_KMAX || N < 1 || D < 1 || H < 1 || W < 1 ||
      ((size_t)x & 15) || out == add)
    BRATS_FAIL(BRATS_E_ARG, "conv3d_narrow_fwd: bad argument (C and pitch multiples of 8, 1 <= K <= 16, x 16-byte aligned, out != add)");
  if (dtype != BRATS_F32 && dtype != BRATS_BF16 && dtype != BRATS_F16) BRATS_FAIL(BRATS_E_ARG, "conv3d_narrow_fwd: dtype %d", dtype);
  const int tx = ceil_div(W, NT_X), ty = ceil_div(H, NT_Y), tz = ceil_div(D, NT_Z);
  const long long tiles = (long long)tx * ty * tz;
  if (tiles > 0x7fffffffLL || N > 65535) BRATS_FAIL(BRATS_E_UNSUPPORTED, "conv3d_narrow_fwd: volume too large");
  const int vec = W % 4 == 0 && !((size_t)out & 15) && !((size_t)add & 15);
  const dim3 grid((unsigned)tiles, (unsigned)N);
  hipStream_t st = (hipStream_t)s;
  const int kt = narrow_kt(K);
  if (dtype == BRATS_F32) return narrow_launch(kt, grid, st, (const float*)x, C, xpitch, packed_w, bias, add, out, K, D, H, W, tx, ty, vec);
  const uint16_t* frag = (const uint16_t*)(packed_w + narrow_f32_floats(C, K));
  if (dtype == BRATS_BF16)
    hipLaunchKernelGGL(conv_narrow_mfma_kernel<BRATS_BF16>, grid, dim3(256), 0, st, x, C, xpitch, (const u32x4*)frag, bias, add, out, K, D, H, W, tx, ty);
  else
    hipLaunchKernelGGL(conv_narrow_mfma_kernel<BRATS_F16>, grid, dim3(256), 0, st, x, C, xpitch, (const u32x4*)(frag + narrow_frag_elems(C)), bias, add, out,
                       K, D, H, W, tx, ty);
  BRATS_CHECK_LAUNCH();
  return 0;
}
