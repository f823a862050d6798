// Exclusive-class segmentation: softmax Dice + cross-entropy statistics and gradient, softmax planes and arg-max labels.
// Semantics = the reference's DiceCELoss(softmax=True, to_onehot_y=True) (learning/losses.py over monai DiceLoss and
// torch.nn.CrossEntropyLoss(ignore_index)); the scalar algebra on the [N][K] sums stays in torch (brats21_amd/losses.py),
// these kernels do the HBM-bound passes over the [N][K][V] f32 logits and the [N][V] uint8 label map:
//   stats : per sample  I_k = sum m t_k p_k,  P2_k = sum m p_k^2,  P1_k = sum m p_k,  CE = sum m (lse - x_y)      (4K + 1 bytes / voxel)
//   grad  : dx_k = m [ p_k (g_k - sum_j g_j p_j) + c (p_k - t_k) ],  g_j = a_j t_j + b_j (s0 + s1 p_j)             (8K + 1 bytes / voxel)
// with p = softmax over the K planes of a voxel, t_k = [y == k], m = [y < K]: a label >= K (255 = unlabelled) takes the voxel
// out of every sum and gives it a zero gradient.  The label is only ever COMPARED, never used as an index.
// K (2..16) is a template argument: the K logits of a voxel live in registers, every loop over them is unrolled, and the
// per-thread accumulators are named registers too (no scratch: DESIGN.md quotes the compiler's resource usage).  W = 4
// voxels per thread and 16-byte accesses (statistics and gradient above 8 classes: W = 2, wide_voxels) where every plane
// starts on a 16-byte boundary and V % 4 == 0, W = 1 otherwise.
#include "class_planes.hpp"  // the grid, the plane loads and stores, the workgroup sums

// f(std::integral_constant<int, K>) for the run-time K in 2..16
template <typename F> static inline int with_classes(int K, F&& f) {
  switch (K) {
#define SM_CASE(k) case k: return f(std::integral_constant<int, k>{});
    SM_CASE(2) SM_CASE(3) SM_CASE(4) SM_CASE(5) SM_CASE(6) SM_CASE(7) SM_CASE(8) SM_CASE(9)
    SM_CASE(10) SM_CASE(11) SM_CASE(12) SM_CASE(13) SM_CASE(14) SM_CASE(15) SM_CASE(16)
#undef SM_CASE
  }
  return BRATS_E_ARG;
}

// voxels per thread of the wide form of the statistics and gradient passes: 4 (16-byte loads) up to 8 classes, 2 (8-byte loads)
// above -- with 16 classes four voxels hold 64 logits beside the 49 accumulators, 169 registers and two waves per SIMD;
// two voxels: 125 and four waves (2 x 16 x 128^3: statistics 0.066 -> 0.054 ms, gradient 0.134 -> 0.119 ms)
static constexpr int wide_voxels(int K) { return K > 8 ? 2 : 4; }

// p = softmax(x) in place, the maximum subtracted first (logits of +-100 at one voxel stay finite); returns log(sum exp(x - max))
// and leaves x_k - max in d
template <int K> DEVI float softmax_reg(const float (&x)[K], float (&d)[K], float (&p)[K]) {
  float mx = x[0];
#pragma unroll
  for (int k = 1; k < K; ++k) mx = fmaxf(mx, x[k]);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    d[k] = x[k] - mx;
    p[k] = __expf(d[k]);
    s += p[k];
  }
  const float inv = 1.f / s;
#pragma unroll
  for (int k = 0; k < K; ++k) p[k] *= inv;
  return __logf(s);
}

// grid (blocks, N); part[block][n][3K + 1] = {I_k, P2_k, P1_k}_k, CE
template <int K, int W> __global__ void __launch_bounds__(SM_BLOCK) softmax_stats_kernel(const float* __restrict__ x, const uint8_t* __restrict__ y,
                                                                                         float* __restrict__ part, size_t V) {
  constexpr int T = 3 * K + 1;
  const int n = blockIdx.y;
  const float* xp = x + (size_t)n * K * V;
  const uint8_t* yp = y + (size_t)n * V;
  float acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = 0.f;
  const size_t groups = V / W;
  for (size_t i = (size_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < groups; i += (size_t)gridDim.x * SM_BLOCK) {
    float xv[K][W];
    load_planes<K, W>(xp, V, i, xv);
    const uint32_t labs = load_labels<W>(yp, i);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const uint32_t lab = (labs >> (8 * j)) & 255u;
      float xs[K], d[K], p[K];
#pragma unroll
      for (int k = 0; k < K; ++k) xs[k] = xv[k][j];
      const float logsum = softmax_reg<K>(xs, d, p);
      const bool valid = lab < (uint32_t)K;
      float dy = 0.f;  // x_y - max
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const bool hit = lab == (uint32_t)k;
        dy = hit ? d[k] : dy;
        acc[3 * k] += hit ? p[k] : 0.f;
        acc[3 * k + 1] += valid ? p[k] * p[k] : 0.f;
        acc[3 * k + 2] += valid ? p[k] : 0.f;
      }
      acc[3 * K] += valid ? logsum - dy : 0.f;
    }
  }
  block_sums<T>(acc, part + ((size_t)blockIdx.x * gridDim.y + n) * T);
}

// grid (blocks, N); coef[n][2K + 1] = {a_k, b_k}_k, c
template <int K, int W> __global__ void __launch_bounds__(SM_BLOCK) softmax_grad_kernel(const float* __restrict__ x, const uint8_t* __restrict__ y,
                                                                                        const float* __restrict__ coef, float* __restrict__ dx,
                                                                                        size_t V, float s0, float s1) {
  const int n = blockIdx.y;
  const float* xp = x + (size_t)n * K * V;
  const uint8_t* yp = y + (size_t)n * V;
  float* dp = dx + (size_t)n * K * V;
  const float* cf = coef + (size_t)n * (2 * K + 1);
  float a[K], b[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { a[k] = cf[2 * k]; b[k] = cf[2 * k + 1]; }
  const float c = cf[2 * K];
  const size_t groups = V / W;
  for (size_t i = (size_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < groups; i += (size_t)gridDim.x * SM_BLOCK) {
    float xv[K][W];
    load_planes<K, W>(xp, V, i, xv);
    const uint32_t labs = load_labels<W>(yp, i);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const uint32_t lab = (labs >> (8 * j)) & 255u;
      float xs[K], d[K], p[K], g[K];
#pragma unroll
      for (int k = 0; k < K; ++k) xs[k] = xv[k][j];
      softmax_reg<K>(xs, d, p);
      const bool valid = lab < (uint32_t)K;
      float dot = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        g[k] = (lab == (uint32_t)k ? a[k] : 0.f) + b[k] * (s0 + s1 * p[k]);
        dot += g[k] * p[k];
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float t = lab == (uint32_t)k ? 1.f : 0.f;
        xv[k][j] = valid ? p[k] * (g[k] - dot) + c * (p[k] - t) : 0.f;
      }
    }
    store_planes<K, W>(dp, V, i, xv);
  }
}

// grid (blocks, N); out may be x
template <int K, int W> __global__ void __launch_bounds__(SM_BLOCK) softmax_planes_kernel(const float* x, float* out, size_t V) {
  const int n = blockIdx.y;
  const float* xp = x + (size_t)n * K * V;
  float* op = out + (size_t)n * K * V;
  const size_t groups = V / W;
  for (size_t i = (size_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < groups; i += (size_t)gridDim.x * SM_BLOCK) {
    float xv[K][W];
    load_planes<K, W>(xp, V, i, xv);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      float xs[K], d[K], p[K];
#pragma unroll
      for (int k = 0; k < K; ++k) xs[k] = xv[k][j];
      softmax_reg<K>(xs, d, p);
#pragma unroll
      for (int k = 0; k < K; ++k) xv[k][j] = p[k];
    }
    store_planes<K, W>(op, V, i, xv);
  }
}

// grid (blocks, N); part[block][n][17] = voxels of label 0..15, voxels of a label < K
template <int W> __global__ void __launch_bounds__(SM_BLOCK) label_stats_kernel(const uint8_t* __restrict__ y, float* __restrict__ part, int K, size_t V) {
  constexpr int T = SM_MAX_K + 1;
  const int n = blockIdx.y;
  const uint8_t* yp = y + (size_t)n * V;
  int cnt[T];
#pragma unroll
  for (int t = 0; t < T; ++t) cnt[t] = 0;
  const size_t groups = V / W;
  for (size_t i = (size_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < groups; i += (size_t)gridDim.x * SM_BLOCK) {
    const uint32_t labs = load_labels<W>(yp, i);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const uint32_t lab = (labs >> (8 * j)) & 255u;
#pragma unroll
      for (int k = 0; k < SM_MAX_K; ++k) cnt[k] += lab == (uint32_t)k ? 1 : 0;
      cnt[SM_MAX_K] += lab < (uint32_t)K ? 1 : 0;
    }
  }
  float acc[T];  // a workgroup sees fewer than 2^24 voxels of a sample up to 2^34 voxels: the counts are exact in f32
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = (float)cnt[t];
  block_sums<T>(acc, part + ((size_t)blockIdx.x * gridDim.y + n) * T);
}
// counts[n][k] (k < K) = totals[n][k], counts[n][K] = totals[n][16]
__global__ void label_stats_pick_kernel(const float* __restrict__ totals, float* __restrict__ counts, int N, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * (K + 1)) return;
  const int n = i / (K + 1), k = i % (K + 1);
  counts[i] = totals[n * (SM_MAX_K + 1) + (k < K ? k : SM_MAX_K)];
}

// grid (blocks, N): labels[n][v] = arg-max over k of sum[n][k][v] (the first maximum: ties to the lowest class), 0 where every
// image channel is 0
template <int W> __global__ void __launch_bounds__(SM_BLOCK) argmax_labels_kernel(const float* __restrict__ sum, const float* __restrict__ img,
                                                                                  uint8_t* __restrict__ labels, int K, int C, size_t V) {
  const int n = blockIdx.y;
  const float* sp = sum + (size_t)n * K * V;
  const float* ip = img ? img + (size_t)n * C * V : nullptr;
  uint8_t* lp = labels + (size_t)n * V;
  const size_t groups = V / W;
  for (size_t i = (size_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < groups; i += (size_t)gridDim.x * SM_BLOCK) {
    float best[W];
    uint32_t arg[W];
    bool fg[W];
#pragma unroll
    for (int j = 0; j < W; ++j) { best[j] = 0.f; arg[j] = 0; fg[j] = ip == nullptr; }
    for (int k = 0; k < K; ++k) {
      float v[1][W];
      load_planes<1, W>(sp + (size_t)k * V, V, i, v);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const bool better = k == 0 || v[0][j] > best[j];
        best[j] = better ? v[0][j] : best[j];
        arg[j] = better ? (uint32_t)k : arg[j];
      }
    }
    for (int c = 0; c < C && ip; ++c) {
      float v[1][W];
      load_planes<1, W>(ip + (size_t)c * V, V, i, v);
#pragma unroll
      for (int j = 0; j < W; ++j) fg[j] = fg[j] || v[0][j] != 0.f;
    }
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) packed |= (fg[j] ? arg[j] : 0u) << (8 * j);
    if constexpr (W == 4) ((uint32_t*)lp)[i] = packed;
    else lp[i] = (uint8_t)packed;
  }
}

static int check_classes(const char* what, int N, int K, size_t voxels) {
  if (N <= 0 || N > 65535 || voxels == 0) BRATS_FAIL(BRATS_E_ARG, "%s: bad batch or voxel count", what);
  if (K < 2 || K > SM_MAX_K) BRATS_FAIL(BRATS_E_ARG, "%s: %d classes (2 .. %d are built)", what, K, SM_MAX_K);
  return 0;
}

extern "C" size_t brats_softmax_ws_floats(int N, int K) {
  if (N <= 0 || K < 2 || K > SM_MAX_K) return 0;
  return (size_t)SM_MAX_BLOCKS * N * (3 * K + 1);
}

extern "C" int brats_softmax_stats(const float* logits, const uint8_t* labels, float* sums /*[N][3K+1]*/, float* ws, int N, int K,
                                   size_t voxels, brats_stream_t s) {
  if (!logits || !labels || !sums || !ws) BRATS_FAIL(BRATS_E_ARG, "softmax_stats: null pointer");
  if (int rc = check_classes("softmax_stats", N, K, voxels)) return rc;
  hipStream_t st = (hipStream_t)s;
  const bool vec = voxels % 4 == 0 && aligned_to(logits, 16) && aligned_to(labels, 4);
  const int w = vec ? wide_voxels(K) : 1;
  const unsigned gx = sm_grid(voxels, w, N);
  with_classes(K, [&](auto k) {
    constexpr int KK = decltype(k)::value;
    constexpr int WW = wide_voxels(KK);
    if (vec) hipLaunchKernelGGL((softmax_stats_kernel<KK, WW>), dim3(gx, N), dim3(SM_BLOCK), 0, st, logits, labels, ws, voxels);
    else hipLaunchKernelGGL((softmax_stats_kernel<KK, 1>), dim3(gx, N), dim3(SM_BLOCK), 0, st, logits, labels, ws, voxels);
    return 0;
  });
  brats_ordered_sum(ws, sums, (int)gx, N * (3 * K + 1), st);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_softmax_grad(const float* logits, const uint8_t* labels, const float* coef /*[N][2K+1]*/, float* dlogits, int N,
                                  int K, size_t voxels, int squared_pred, brats_stream_t s) {
  if (!logits || !labels || !coef || !dlogits) BRATS_FAIL(BRATS_E_ARG, "softmax_grad: null pointer");
  if (int rc = check_classes("softmax_grad", N, K, voxels)) return rc;
  hipStream_t st = (hipStream_t)s;
  const bool vec = voxels % 4 == 0 && aligned_to(logits, 16) && aligned_to(dlogits, 16) && aligned_to(labels, 4);
  const int w = vec ? wide_voxels(K) : 1;
  const unsigned gx = sm_grid(voxels, w, N);
  const float s0 = squared_pred ? 0.f : 1.f, s1 = squared_pred ? 2.f : 0.f;  // dP/dp_j = s0 + s1 p_j
  with_classes(K, [&](auto k) {
    constexpr int KK = decltype(k)::value;
    constexpr int WW = wide_voxels(KK);
    if (vec) hipLaunchKernelGGL((softmax_grad_kernel<KK, WW>), dim3(gx, N), dim3(SM_BLOCK), 0, st, logits, labels, coef, dlogits, voxels, s0, s1);
    else hipLaunchKernelGGL((softmax_grad_kernel<KK, 1>), dim3(gx, N), dim3(SM_BLOCK), 0, st, logits, labels, coef, dlogits, voxels, s0, s1);
    return 0;
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t brats_label_stats_ws_floats(int N) { return N <= 0 ? 0 : (size_t)(SM_MAX_BLOCKS + 1) * N * (SM_MAX_K + 1); }

extern "C" int brats_label_stats(const uint8_t* labels, float* counts /*[N][K+1]*/, float* ws, int N, int K, size_t voxels,
                                 brats_stream_t s) {
  if (!labels || !counts || !ws) BRATS_FAIL(BRATS_E_ARG, "label_stats: null pointer");
  if (int rc = check_classes("label_stats", N, K, voxels)) return rc;
  hipStream_t st = (hipStream_t)s;
  const bool vec = voxels % 4 == 0 && aligned_to(labels, 4);
  const unsigned gx = sm_grid(voxels, vec ? 4 : 1, N);
  const int T = SM_MAX_K + 1;
  float* totals = ws + (size_t)SM_MAX_BLOCKS * N * T;
  if (vec) hipLaunchKernelGGL(label_stats_kernel<4>, dim3(gx, N), dim3(SM_BLOCK), 0, st, labels, ws, K, voxels);
  else hipLaunchKernelGGL(label_stats_kernel<1>, dim3(gx, N), dim3(SM_BLOCK), 0, st, labels, ws, K, voxels);
  brats_ordered_sum(ws, totals, (int)gx, N * T, st);
  hipLaunchKernelGGL(label_stats_pick_kernel, dim3(ceil_div(N * (K + 1), 256)), dim3(256), 0, st, (const float*)totals, counts, N, K);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_softmax_planes(const float* logits, float* out, int N, int K, size_t voxels, brats_stream_t s) {
  if (!logits || !out) BRATS_FAIL(BRATS_E_ARG, "softmax_planes: null pointer");
  if (int rc = check_classes("softmax_planes", N, K, voxels)) return rc;
  hipStream_t st = (hipStream_t)s;
  const bool vec = voxels % 4 == 0 && aligned_to(logits, 16) && aligned_to(out, 16);
  const unsigned gx = sm_grid(voxels, vec ? 4 : 1, N);
  with_classes(K, [&](auto k) {
    constexpr int KK = decltype(k)::value;
    if (vec) hipLaunchKernelGGL((softmax_planes_kernel<KK, 4>), dim3(gx, N), dim3(SM_BLOCK), 0, st, logits, out, voxels);
    else hipLaunchKernelGGL((softmax_planes_kernel<KK, 1>), dim3(gx, N), dim3(SM_BLOCK), 0, st, logits, out, voxels);
    return 0;
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_argmax_labels(const float* sum, const float* img /* may be NULL */, uint8_t* labels, int N, int K, int C,
                                   size_t voxels, brats_stream_t s) {
  if (!sum || !labels) BRATS_FAIL(BRATS_E_ARG, "argmax_labels: null pointer");
  if (N <= 0 || N > 65535 || voxels == 0 || K < 1 || K > 255 || (img && C <= 0)) BRATS_FAIL(BRATS_E_ARG, "argmax_labels: bad argument");
  const bool vec = voxels % 4 == 0 && aligned_to(sum, 16) && aligned_to(labels, 4) && (!img || aligned_to(img, 16));
  const unsigned gx = sm_grid(voxels, vec ? 4 : 1, N);
  if (vec) hipLaunchKernelGGL(argmax_labels_kernel<4>, dim3(gx, N), dim3(SM_BLOCK), 0, (hipStream_t)s, sum, img, labels, K, C, voxels);
  else hipLaunchKernelGGL(argmax_labels_kernel<1>, dim3(gx, N), dim3(SM_BLOCK), 0, (hipStream_t)s, sum, img, labels, K, C, voxels);
  BRATS_CHECK_LAUNCH();
  return 0;
}
