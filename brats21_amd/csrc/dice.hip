// Fused sigmoid-Dice / Jaccard statistics and gradient for deep supervision.
// Semantics = monai.losses.DiceLoss(sigmoid, squared_pred, batch=True) as configured at src/definer.py:184-203,
// averaged over heads as in learning/engine.py:322-330.  Per head (brats_dice_stats / brats_dice_grad) the scalar algebra on the
// [classes] sums stays in torch and these kernels only do the two HBM-bound passes over the [N][K][V] f32 logits; for all heads
// of a step at once (brats_dice_*_multi, brats_dice_finish, at the end of this file) the algebra is a kernel too:
//   stats : sums[k] = { sum t*p, sum p*p, sum t*t }      (p = sigmoid(x), over n and voxels)
//   grad  : dx = (a_k * t + b_k * 2p) * p * (1 - p)        (a_k = dL/dI_k, b_k = dL/dP2_k, read from device memory)
#include "common.hpp"

// The per-element arithmetic, shared by the one-head and the all-heads kernels so that both compile to the same operations
// (no contraction: every product and sum is rounded on its own, whatever the translation unit is built with).
DEVI float dice_sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }
DEVI float dice_grad_elem(float a, float b2, float t, float p) {
#pragma clang fp contract(off)
  return (a * t + b2 * p) * p * (1.f - p);
}
// r[.][0] = sum of r[.][0..255] for S rows, the tree every Dice statistics kernel ends with
template <int S>
DEVI void dice_block_tree(float (*r)[256]) {
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if ((int)threadIdx.x < m) {
#pragma unroll
      for (int q = 0; q < S; ++q) r[q][threadIdx.x] += r[q][threadIdx.x + m];
    }
    __syncthreads();
  }
}

__global__ void dice_stats_kernel(const float* __restrict__ x, const float* __restrict__ t, float* __restrict__ part, int K,
                                  size_t voxels) {
  // grid: (blocks, N*K); each block reduces a slice of one (n, k) plane
  const int nk = blockIdx.y, k = nk % K;
  const float* xp = x + (size_t)nk * voxels;
  const float* tp = t + (size_t)nk * voxels;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  // the 16-byte path only where every plane starts on a 16-byte boundary; else v4 = 0 and all blocks share the scalar loop
  const size_t v4 = (voxels % 4 == 0 && (((size_t)x | (size_t)t) & 15) == 0) ? voxels / 4 : 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < v4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 xv = ((const f32x4*)xp)[i], tv = ((const f32x4*)tp)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p = dice_sigmoid(xv[j]);
      s0 += tv[j] * p;
      s1 += p * p;
      s2 += tv[j] * tv[j];
    }
  }
  for (size_t i = v4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < voxels; i += (size_t)gridDim.x * blockDim.x) {
    const float p = dice_sigmoid(xp[i]);
    s0 += tp[i] * p; s1 += p * p; s2 += tp[i] * tp[i];
  }
  __shared__ float r[3][256];
  r[0][threadIdx.x] = s0; r[1][threadIdx.x] = s1; r[2][threadIdx.x] = s2;
  dice_block_tree<3>(r);
  // one partial per block: part[(n * gridDim.x + blockIdx.x)][K][3]; brats_ordered_sum adds them in block order
  if (threadIdx.x < 3) part[(((size_t)(nk / K) * gridDim.x + blockIdx.x) * K + k) * 3 + threadIdx.x] = r[threadIdx.x][0];
}

// out[i] = sum over nb partial vectors, 8 entries x 32 slices per block, slices added in order
__global__ void __launch_bounds__(256) ordered_sum_kernel(const float* __restrict__ part, float* __restrict__ out, int nb, int total,
                                                          float* __restrict__ out2 /* entries >= n1 go here (may be NULL) */, int n1) {
  const int e = threadIdx.x & 7, g = threadIdx.x >> 3;
  const int i = blockIdx.x * 8 + e;
  float s = 0.f;
  if (i < total) {
    // eight partials in flight, added in block order (hipcc turns the plain loop into load - wait - add, one round trip each)
    const float* src = part + i;
    int b = g;
    for (; b + 7 * 32 < nb; b += 8 * 32) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(b + 32 * u) * total];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; b < nb; b += 32) s += src[(size_t)b * total];
  }
  __shared__ float sm[32][8];
  sm[g][e] = s;
  __syncthreads();
  if (g == 0 && i < total) {
#pragma unroll
    for (int k = 1; k < 32; ++k) s += sm[k][e];
    if (out2 && i >= n1) out2[i - n1] = s;
    else out[i] = s;
  }
}

int brats_ordered_sum(const float* part, float* out, int nb, int total, hipStream_t st) {
  hipLaunchKernelGGL(ordered_sum_kernel, dim3((total + 7) / 8), dim3(256), 0, st, part, out, nb, total, (float*)nullptr, 0);
  return 0;
}
// the first n1 totals to out1, the rest to out2 (two result tensors, one launch, no copies)
int brats_ordered_sum2(const float* part, float* out1, int n1, float* out2, int nb, int total, hipStream_t st) {
  hipLaunchKernelGGL(ordered_sum_kernel, dim3((total + 7) / 8), dim3(256), 0, st, part, out1, nb, total, out2, n1);
  return 0;
}

__global__ void dice_grad_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ coef,
                                 float* __restrict__ dx, int K, size_t voxels) {
  const int nk = blockIdx.y, k = nk % K;
  const float a = coef[k * 2], b2 = 2.f * coef[k * 2 + 1];
  const float* xp = x + (size_t)nk * voxels;
  const float* tp = t + (size_t)nk * voxels;
  float* dp = dx + (size_t)nk * voxels;
  const size_t v4 = (voxels % 4 == 0 && (((size_t)x | (size_t)t | (size_t)dx) & 15) == 0) ? voxels / 4 : 0;  // (as in dice_stats_kernel)
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < v4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 xv = ((const f32x4*)xp)[i], tv = ((const f32x4*)tp)[i];
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p = dice_sigmoid(xv[j]);
      o[j] = dice_grad_elem(a, b2, tv[j], p);
    }
    ((f32x4*)dp)[i] = o;
  }
  for (size_t i = v4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < voxels; i += (size_t)gridDim.x * blockDim.x) {
    const float p = dice_sigmoid(xp[i]);
    dp[i] = dice_grad_elem(a, b2, tp[i], p);
  }
}

constexpr int DICE_MAX_BLOCKS = 512;
extern "C" size_t brats_dice_ws_floats(int N, int K) { return (size_t)N * DICE_MAX_BLOCKS * K * 3; }

extern "C" int brats_dice_stats(const float* logits, const float* target, float* sums /*[K][3]*/, float* ws, int N, int K,
                                size_t voxels, brats_stream_t s) {
  if (!logits || !target || !sums || !ws || N <= 0 || K <= 0) BRATS_FAIL(BRATS_E_ARG, "dice_stats: bad argument");
  hipStream_t st = (hipStream_t)s;
  size_t gx = (voxels / 4 + 255) / 256 / 4;
  gx = gx < 1 ? 1 : (gx > DICE_MAX_BLOCKS ? DICE_MAX_BLOCKS : gx);
  hipLaunchKernelGGL(dice_stats_kernel, dim3((unsigned)gx, N * K), dim3(256), 0, st, logits, target, ws, K, voxels);
  brats_ordered_sum(ws, sums, N * (int)gx, K * 3, st);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_dice_grad(const float* logits, const float* target, const float* coef /*[K][2] = dL/dI, dL/dP2*/,
                               float* dlogits, int N, int K, size_t voxels, brats_stream_t s) {
  if (!logits || !target || !coef || !dlogits) BRATS_FAIL(BRATS_E_ARG, "dice_grad: null pointer");
  size_t gx = (voxels / 4 + 255) / 256 / 4;
  gx = gx < 1 ? 1 : (gx > 2048 ? 2048 : gx);
  hipLaunchKernelGGL(dice_grad_kernel, dim3((unsigned)gx, N * K), dim3(256), 0, (hipStream_t)s, logits, target, coef, dlogits, K, voxels);
  BRATS_CHECK_LAUNCH();
  return 0;
}

// ---- all heads of a deep-supervision step in three launches -----------------------------------------------------------------
// The heads share one target, so the per-head passes above read it H times per pass and leave H ordered sums and the
// [heads][classes] algebra (about twenty 15-float torch launches) between them.  Here: one statistics launch (target vector
// loaded once, H logit vectors beside it), one finisher (ordered sums of all heads + the algebra + the loss) and one gradient
// launch.  Every per-block partial, total, coefficient and gradient element is the value the per-head entries give: a thread
// walks the same elements in the same order per head, the block tree and the slice order of ordered_sum_kernel are the same.
// The head pointers travel by value in the kernel arguments: no table upload, nothing a graph capture cannot hold.
constexpr int DICE_MAX_HEADS = 8;
struct DiceHeadsIn { const float* x[DICE_MAX_HEADS]; };
struct DiceHeadsOut { float* dx[DICE_MAX_HEADS]; };

template <int H>
__global__ void __launch_bounds__(256) dice_stats_multi_kernel(DiceHeadsIn hp, const float* __restrict__ t, float* __restrict__ part,
                                                               size_t head_stride, int K, size_t voxels, int vec_ok) {
  const int nk = blockIdx.y, k = nk % K;
  const size_t plane = (size_t)nk * voxels;
  const float* tp = t + plane;
  float s0[H], s1[H], s2 = 0.f;  // (sum t*t is the same sum for every head: formed once, written H times)
#pragma unroll
  for (int h = 0; h < H; ++h) { s0[h] = 0.f; s1[h] = 0.f; }
  const size_t v4 = vec_ok ? voxels / 4 : 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < v4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 tv = ((const f32x4*)tp)[i];
    f32x4 xv[H];
#pragma unroll
    for (int h = 0; h < H; ++h) xv[h] = ((const f32x4*)(hp.x[h] + plane))[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int h = 0; h < H; ++h) {
        const float p = dice_sigmoid(xv[h][j]);
        s0[h] += tv[j] * p;
        s1[h] += p * p;
      }
      s2 += tv[j] * tv[j];
    }
  }
  for (size_t i = v4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < voxels; i += (size_t)gridDim.x * blockDim.x) {
    const float tt = tp[i];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      const float p = dice_sigmoid(hp.x[h][plane + i]);
      s0[h] += tt * p;
      s1[h] += p * p;
    }
    s2 += tt * tt;
  }
  __shared__ float r[2 * H + 1][256];
#pragma unroll
  for (int h = 0; h < H; ++h) { r[2 * h][threadIdx.x] = s0[h]; r[2 * h + 1][threadIdx.x] = s1[h]; }
  r[2 * H][threadIdx.x] = s2;
  dice_block_tree<2 * H + 1>(r);
  // part[h][(n * gridDim.x + blockIdx.x)][K][3]: per head the layout of dice_stats_kernel
  if (threadIdx.x < 3 * H) {
    const int h = threadIdx.x / 3, q = threadIdx.x % 3;
    part[h * head_stride + (((size_t)(nk / K) * gridDim.x + blockIdx.x) * K + k) * 3 + q] = r[q == 2 ? 2 * H : 2 * h + q][0];
  }
}

// One workgroup: the totals of all H * K * 3 entries (eight entries x 32 slices per 256 threads, four such groups side by
// side; per entry the additions of ordered_sum_kernel in its order), then per (head, class) what _FusedDiceFn.forward computed
// with torch's elementwise f32 kernels, operation for operation:  x / python_scalar is x * (1.f / scalar),  scalar / x is
// (1.f / x) * scalar,  x ** 2 is x * x.  The loss is torch's mean of the H * K values (see dice_mean).
constexpr int DICE_FIN_THREADS = 1024, DICE_MAX_CLASSES = 16;
// torch's mean of n <= 128 contiguous f32 values, in the order its reduction kernel adds them on this hardware (probed for
// n = 1 .. 48 against emulations of the candidate orders: bit-equal in every trial): bw = the largest power of two <= n (at
// most a wavefront) lanes; lane j adds f[j] and f[j + bw] into two accumulators that start at 0 and folds its four accumulators
// left to right; the lanes are combined by shuffle-down steps of 1, 2, 4, ...; the total is multiplied by fl(1 / n).
// One thread, tl = scratch of 64 floats.
DEVI float dice_mean(const float* f, int n, float* tl) {
#pragma clang fp contract(off)
  int bw = 1;
  while (bw * 2 <= n && bw < 64) bw *= 2;
  for (int j = 0; j < bw; ++j) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int i = 0;
    for (int idx = j; idx < n; idx += bw, ++i) {
      const float v = f[idx];
      if ((i & 3) == 0) a0 += v;
      else if ((i & 3) == 1) a1 += v;
      else if ((i & 3) == 2) a2 += v;
      else a3 += v;
    }
    tl[j] = ((a0 + a1) + a2) + a3;
  }
  for (int off = 1; off < bw; off <<= 1)
    for (int j = 0; j + off < bw; ++j) tl[j] += tl[j + off];
  return tl[0] * (1.f / (float)n);
}
__global__ void __launch_bounds__(DICE_FIN_THREADS) dice_finish_kernel(const float* __restrict__ part, size_t head_stride, int nb, int H, int K,
                                                                       float eps, int jaccard, float* __restrict__ sums,
                                                                       float* __restrict__ coef, float* __restrict__ loss) {
#pragma clang fp contract(off)
  __shared__ float sm[DICE_FIN_THREADS / 256][32][8];
  __shared__ float tot[DICE_MAX_HEADS * DICE_MAX_CLASSES * 3], fv[DICE_MAX_HEADS * DICE_MAX_CLASSES];
  const int K3 = K * 3, total = H * K3;
  const int c = threadIdx.x >> 8, e = threadIdx.x & 7, g = (threadIdx.x & 255) >> 3;
  for (int base = 0; base < total; base += DICE_FIN_THREADS / 32) {
    const int i = base + c * 8 + e;
    float s = 0.f;
    if (i < total) {
      const float* src = part + (size_t)(i / K3) * head_stride + i % K3;
      int b = g;
      for (; b + 7 * 32 < nb; b += 8 * 32) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(b + 32 * u) * K3];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
      }
      for (; b < nb; b += 32) s += src[(size_t)b * K3];
    }
    sm[c][g][e] = s;
    __syncthreads();
    if (g == 0 && i < total) {
#pragma unroll
      for (int k = 1; k < 32; ++k) s += sm[c][k][e];
      tot[i] = s;
      sums[i] = s;
    }
    __syncthreads();
  }
  const int hk = H * K;
  if ((int)threadIdx.x < hk) {
    const float inter = tot[threadIdx.x * 3], p2 = tot[threadIdx.x * 3 + 1], t2 = tot[threadIdx.x * 3 + 2];
    const float inv_hk = 1.f / (float)hk;
    const float num = 2.f * inter + eps;
    float c0, c1, de;
    if (jaccard) {
      de = 2.f * (t2 + p2 - inter) + eps;
      const float dden = num / (de * de);
      c0 = ((1.f / de) * -2.f - 2.f * dden) * inv_hk;
      c1 = (2.f * dden) * inv_hk;
    } else {
      de = t2 + p2 + eps;
      c0 = ((1.f / de) * -2.f) * inv_hk;
      c1 = (num / (de * de)) * inv_hk;
    }
    coef[threadIdx.x * 2] = c0;
    coef[threadIdx.x * 2 + 1] = c1;
    fv[threadIdx.x] = 1.f - num / de;
  }
  __syncthreads();
  if (threadIdx.x == 0) *loss = dice_mean(fv, hk, &sm[0][0][0]);
}

template <int H>
__global__ void __launch_bounds__(256) dice_grad_multi_kernel(DiceHeadsIn hp, const float* __restrict__ t, const float* __restrict__ coef,
                                                              const float* __restrict__ g, DiceHeadsOut op, int K, size_t voxels,
                                                              int vec_ok) {
  const int nk = blockIdx.y, k = nk % K;
  const size_t plane = (size_t)nk * voxels;
  const float* tp = t + plane;
  const float up = g[0];
  float a[H], b2[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {  // fl(coef * g): what (coef * g).contiguous() handed to dice_grad_kernel
    a[h] = coef[(h * K + k) * 2] * up;
    b2[h] = 2.f * (coef[(h * K + k) * 2 + 1] * up);
  }
  const size_t v4 = vec_ok ? voxels / 4 : 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < v4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 tv = ((const f32x4*)tp)[i];
    f32x4 xv[H];
#pragma unroll
    for (int h = 0; h < H; ++h) xv[h] = ((const f32x4*)(hp.x[h] + plane))[i];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = dice_grad_elem(a[h], b2[h], tv[j], dice_sigmoid(xv[h][j]));
      ((f32x4*)(op.dx[h] + plane))[i] = o;
    }
  }
  for (size_t i = v4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < voxels; i += (size_t)gridDim.x * blockDim.x) {
    const float tt = tp[i];
#pragma unroll
    for (int h = 0; h < H; ++h) op.dx[h][plane + i] = dice_grad_elem(a[h], b2[h], tt, dice_sigmoid(hp.x[h][plane + i]));
  }
}

// dispatch on the head count: the accumulators and the vectors in flight are registers
#define DICE_FOR_HEADS(H, CALL) \
  switch (H) {                  \
    case 1: { CALL(1); } break; \
    case 2: { CALL(2); } break; \
    case 3: { CALL(3); } break; \
    case 4: { CALL(4); } break; \
    case 5: { CALL(5); } break; \
    case 6: { CALL(6); } break; \
    case 7: { CALL(7); } break; \
    default: { CALL(8); } break; \
  }

static size_t dice_stats_blocks(size_t voxels) {  // (the rule of brats_dice_stats: the partials depend on it)
  const size_t gx = (voxels / 4 + 255) / 256 / 4;
  return gx < 1 ? 1 : (gx > DICE_MAX_BLOCKS ? DICE_MAX_BLOCKS : gx);
}

extern "C" size_t brats_dice_multi_ws_floats(int H, int N, int K) { return (size_t)H * brats_dice_ws_floats(N, K); }

extern "C" int brats_dice_stats_multi(const float* const* heads, int H, const float* target, float* ws, int N, int K, size_t voxels,
                                      brats_stream_t s) {
  if (!heads || !target || !ws || H < 1 || H > DICE_MAX_HEADS || N <= 0 || K <= 0 || (size_t)N * K > 65535)
    BRATS_FAIL(BRATS_E_ARG, "dice_stats_multi: bad argument (1 <= heads <= %d)", DICE_MAX_HEADS);
  DiceHeadsIn hp = {};
  size_t bits = (size_t)target;
  for (int h = 0; h < H; ++h) {
    if (!heads[h]) BRATS_FAIL(BRATS_E_ARG, "dice_stats_multi: null head pointer");
    hp.x[h] = heads[h];
    bits |= (size_t)heads[h];
  }
  const int vec_ok = voxels % 4 == 0 && (bits & 15) == 0;  // one path for all heads: the target vector is loaded once
  const dim3 grid((unsigned)dice_stats_blocks(voxels), N * K);
  const size_t stride = brats_dice_ws_floats(N, K);
#define DICE_CALL(HH) hipLaunchKernelGGL((dice_stats_multi_kernel<HH>), grid, dim3(256), 0, (hipStream_t)s, hp, target, ws, stride, K, voxels, vec_ok)
  DICE_FOR_HEADS(H, DICE_CALL)
#undef DICE_CALL
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_dice_finish(const float* ws, int H, int N, int K, size_t voxels, float eps, int jaccard, float* sums /*[H][K][3]*/,
                                 float* coef /*[H][K][2]*/, float* loss, brats_stream_t s) {
  if (!ws || !sums || !coef || !loss || H < 1 || H > DICE_MAX_HEADS || N <= 0 || K <= 0 || K > DICE_MAX_CLASSES)
    BRATS_FAIL(BRATS_E_ARG, "dice_finish: bad argument (1 <= heads <= %d, 1 <= classes <= %d)", DICE_MAX_HEADS, DICE_MAX_CLASSES);
  hipLaunchKernelGGL(dice_finish_kernel, dim3(1), dim3(DICE_FIN_THREADS), 0, (hipStream_t)s, ws, brats_dice_ws_floats(N, K),
                     N * (int)dice_stats_blocks(voxels), H, K, eps, jaccard, sums, coef, loss);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_dice_grad_multi(const float* const* heads, int H, const float* target, const float* coef /*[H][K][2]*/,
                                     const float* g /*device scalar*/, float* const* dlogits, int N, int K, size_t voxels,
                                     brats_stream_t s) {
  if (!heads || !target || !coef || !g || !dlogits || H < 1 || H > DICE_MAX_HEADS || N <= 0 || K <= 0 || (size_t)N * K > 65535)
    BRATS_FAIL(BRATS_E_ARG, "dice_grad_multi: bad argument (1 <= heads <= %d)", DICE_MAX_HEADS);
  DiceHeadsIn hp = {};
  DiceHeadsOut op = {};
  size_t bits = (size_t)target;
  for (int h = 0; h < H; ++h) {
    if (!heads[h] || !dlogits[h]) BRATS_FAIL(BRATS_E_ARG, "dice_grad_multi: null head pointer");
    hp.x[h] = heads[h];
    op.dx[h] = dlogits[h];
    bits |= (size_t)heads[h] | (size_t)dlogits[h];
  }
  const int vec_ok = voxels % 4 == 0 && (bits & 15) == 0;
  size_t gx = (voxels / 4 + 255) / 256 / 4;
  gx = gx < 1 ? 1 : (gx > 2048 ? 2048 : gx);
#define DICE_CALL(HH) hipLaunchKernelGGL((dice_grad_multi_kernel<HH>), dim3((unsigned)gx, N * K), dim3(256), 0, (hipStream_t)s, hp, target, coef, g, op, K, voxels, vec_ok)
  DICE_FOR_HEADS(H, DICE_CALL)
#undef DICE_CALL
  BRATS_CHECK_LAUNCH();
  return 0;
}
