// Multi-label criteria over sigmoid probabilities: the statistics and the gradient of dice_ce, dice_focal, focal and tversky
// (src/definer.py:204-245: the reference's DiceCELoss(sigmoid=True), learning/losses.py:470-595, and monai 0.6.0 DiceFocalLoss,
// FocalLoss and TverskyLoss).  The scalar algebra on the [N][K] sums stays in torch (brats21_amd/losses.py); these kernels do the
// HBM-bound passes over the [N][K][V] f32 logits x and target t, p = sigmoid(x):
//   prepare: per plane  T1 = sum t, T2 = sum t^2;  y[n][v] = arg-max_k t (ties to the lowest channel)       (4K (+ 1) bytes / voxel)
//   stats  : per plane  I = sum p t, P2 = sum p^2, P1 = sum p, F = sum focal(x, t);  per sample CE = sum (lse_k x - x_y)
//                                                                                                   (8K (+ 1 with CE) bytes / voxel)
//   grad   : dx = p (1 - p) (A t + 2 B p + C) + Fc dfocal/dx + c (softmax_k x - [k == y])           (12K (+ 1 with CE) bytes / voxel)
// focal(x, t) = exp(gamma q) bce, q = logsigmoid(-x (2t - 1)), bce = x - x t + softplus(-x): monai's FocalLoss; for a binary
// target it is (1 - p_t)^gamma BCE.  dfocal/dx = exp(gamma q) [p - t - gamma bce (2t - 1) sigmoid(x (2t - 1))].
// Two forms of each pass, chosen by the term mask:
//   * plane form (no CE term): every class is on its own, so a workgroup streams ONE plane (grid (blocks, N, K)), four voxels per
//     thread whatever K is, four sums per thread; FOCAL is a template argument -- without it the kernel has no logarithm in it.
//     (All K planes of a voxel in registers, as the CE form has them, cost the focal statistics 256 VGPRs at K = 16.)
//   * voxel form (CE term): the softmax needs the K logits of a voxel together; K (1..16) is a template argument as in
//     softmax_loss.hip, the planes of a voxel group and the 3K + 1 accumulators are registers.  Only this form reads the class map.
// Every exponential has an argument <= 0 (exp(-|x|), exp(x_k - max)), so logits of +-100 at one voxel stay finite; 1 - p is
// e / (1 + e), never a subtraction.  The class map is only ever COMPARED, never used as an index.
#include "class_planes.hpp"

// f(std::integral_constant<int, K>) for the run-time K in 1..16
template <typename F> static inline int with_planes(int K, F&& f) {
  switch (K) {
#define SIG_CASE(k) case k: return f(std::integral_constant<int, k>{});
    SIG_CASE(1) SIG_CASE(2) SIG_CASE(3) SIG_CASE(4) SIG_CASE(5) SIG_CASE(6) SIG_CASE(7) SIG_CASE(8) SIG_CASE(9)
    SIG_CASE(10) SIG_CASE(11) SIG_CASE(12) SIG_CASE(13) SIG_CASE(14) SIG_CASE(15) SIG_CASE(16)
#undef SIG_CASE
  }
  return BRATS_E_ARG;
}
// voxels per thread of the wide voxel form: two planes (x and t) per class are in registers, so 4 (16-byte accesses) up to 4
// classes and 2 (8-byte accesses) above; DESIGN.md quotes the compiler's resource usage
static constexpr int sig_voxels(int K) { return K > 4 ? 2 : 4; }

// e = exp(-|x|), a = 1 / (1 + e): sigmoid(|x|) = a, sigmoid(-|x|) = e a -- p and q = 1 - p without a cancelling subtraction
DEVI void sigmoid_parts(float x, float& e, float& a, float& p, float& q) {
  e = __expf(-fabsf(x));
  a = 1.f / (1.f + e);
  const float b = e * a;
  p = x >= 0.f ? a : b;
  q = x >= 0.f ? b : a;
}
// the focal element of (x, t), e and a from sigmoid_parts(x): w = exp(gamma q), bce, u = 2t - 1, spos = sigmoid(x u).  With a
// binary target |x u| = |x|, so the exponential, the reciprocal and the logarithm of x serve z = x u as well; a soft target
// takes the branch that computes its own.  gamma == 2 (the reference's setting): w = sigmoid(-z)^2 without another exponential.
DEVI void focal_parts(float x, float t, float e, float a, float gamma, float& w, float& bce, float& u, float& spos) {
  const float l = __logf(1.f + e);  // softplus(-|x|)
  bce = x - x * t + fmaxf(-x, 0.f) + l;
  u = 2.f * t - 1.f;
  const float z = x * u;
  float ez = e, az = a, lz = l;
  if (t != 0.f && t != 1.f) {
    ez = __expf(-fabsf(z));
    az = 1.f / (1.f + ez);
    lz = __logf(1.f + ez);
  }
  const float lo = ez * az;  // sigmoid(-|z|); az = sigmoid(|z|)
  const float sneg = z >= 0.f ? lo : az;
  spos = z >= 0.f ? az : lo;
  const float q = -(fmaxf(z, 0.f) + lz);  // logsigmoid(-z)
  w = gamma == 2.f ? sneg * sneg : __expf(gamma * q);
}
// exp(x_k - max) of the K logits of a voxel into ex, their sum returned; dy = x_y - max for the class y (0 where y >= K)
template <int K> DEVI float softmax_parts(const float (&x)[K], uint32_t lab, float (&ex)[K], float& dy) {
  float mx = x[0];
#pragma unroll
  for (int k = 1; k < K; ++k) mx = fmaxf(mx, x[k]);
  float s = 0.f;
  dy = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float d = x[k] - mx;
    dy = lab == (uint32_t)k ? d : dy;
    ex[k] = __expf(d);
    s += ex[k];
  }
  return s;
}

// grid (blocks, N); part[block][n][2K] = {T1_k, T2_k}_k; y (MAP): the class map.  One plane after the other: the running
// maximum and its channel are all that stays in registers beside the 2K sums
template <int K, int W, bool MAP> __global__ void __launch_bounds__(SM_BLOCK) sigmoid_prepare_kernel(const float* __restrict__ t, uint8_t* __restrict__ y,
                                                                                            float* __restrict__ part, size_t V) {
  const int n = blockIdx.y;
  const float* tp = t + (size_t)n * K * V;
  float acc[2 * K];
#pragma unroll
  for (int a = 0; a < 2 * K; ++a) acc[a] = 0.f;
  const size_t groups = V / W;
  for (size_t i = (size_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < groups; i += (size_t)gridDim.x * SM_BLOCK) {
    float best[W];
    uint32_t arg[W];
#pragma unroll
    for (int j = 0; j < W; ++j) { best[j] = 0.f; arg[j] = 0; }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float tv[1][W];
      load_planes<1, W>(tp + (size_t)k * V, V, i, tv);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const float v = tv[0][j];
        acc[2 * k] += v;
        acc[2 * k + 1] += v * v;
        const bool better = k == 0 || v > best[j];  // strict: the first maximum wins, as torch.argmax
        best[j] = better ? v : best[j];
        arg[j] = better ? (uint32_t)k : arg[j];
      }
    }
    if constexpr (MAP) {
      uint32_t packed = 0;
#pragma unroll
      for (int j = 0; j < W; ++j) packed |= arg[j] << (8 * j);
      uint8_t* yp = y + (size_t)n * V;
      if constexpr (W == 4) ((uint32_t*)yp)[i] = packed;
      else yp[i] = (uint8_t)packed;
    }
  }
  block_sums<2 * K>(acc, part + ((size_t)blockIdx.x * gridDim.y + n) * (2 * K));
}

// ---- plane form.  grid (blocks, N, K); part[block][n][4K + 1]: this workgroup's {I, P2, P1, F} of plane (n, k), F = 0 without
// FOCAL; the workgroups of plane 0 write the CE column (0: not asked for)
template <int W, bool FOCAL> __global__ void __launch_bounds__(SM_BLOCK) sigmoid_plane_stats_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                                           float* __restrict__ part, size_t V, float gamma) {
  const int n = blockIdx.y, k = blockIdx.z, K = gridDim.z;
  const float* xp = x + ((size_t)n * K + k) * V;
  const float* tp = t + ((size_t)n * K + k) * V;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const size_t groups = V / W;
  for (size_t i = (size_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < groups; i += (size_t)gridDim.x * SM_BLOCK) {
    float xv[1][W], tv[1][W];
    load_planes<1, W>(xp, V, i, xv);
    load_planes<1, W>(tp, V, i, tv);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float xx = xv[0][j], tt = tv[0][j];
      float e, a, p, q;
      sigmoid_parts(xx, e, a, p, q);
      acc[0] += p * tt;
      acc[1] += p * p;
      acc[2] += p;
      if constexpr (FOCAL) {
        float w, bce, u, spos;
        focal_parts(xx, tt, e, a, gamma, w, bce, u, spos);
        acc[3] += w * bce;
      }
    }
  }
  float* row = part + ((size_t)blockIdx.x * gridDim.y + n) * (4 * K + 1);
  block_sums<4>(acc, row + 4 * k);
  if (k == 0 && threadIdx.x == 0) row[4 * K] = 0.f;
}

// grid (blocks, N, K); coef[n][4K + 1] = {A_k, B_k, C_k, Fc_k}_k, c (c is not read)
template <int W, bool FOCAL> __global__ void __launch_bounds__(SM_BLOCK) sigmoid_plane_grad_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                                          const float* __restrict__ coef, float* __restrict__ dx,
                                                                                          size_t V, float gamma) {
  const int n = blockIdx.y, k = blockIdx.z, K = gridDim.z;
  const float* xp = x + ((size_t)n * K + k) * V;
  const float* tp = t + ((size_t)n * K + k) * V;
  float* dp = dx + ((size_t)n * K + k) * V;
  const float* cf = coef + (size_t)n * (4 * K + 1) + 4 * k;
  const float A = cf[0], B2 = 2.f * cf[1], C = cf[2], Fc = cf[3];
  const size_t groups = V / W;
  for (size_t i = (size_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < groups; i += (size_t)gridDim.x * SM_BLOCK) {
    float xv[1][W], tv[1][W];
    load_planes<1, W>(xp, V, i, xv);
    load_planes<1, W>(tp, V, i, tv);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float xx = xv[0][j], tt = tv[0][j];
      float e, a, p, q;
      sigmoid_parts(xx, e, a, p, q);
      float g = p * q * (A * tt + B2 * p + C);
      if constexpr (FOCAL) {
        float w, bce, u, spos;
        focal_parts(xx, tt, e, a, gamma, w, bce, u, spos);
        g += Fc * (w * (p - tt - gamma * bce * u * spos));
      }
      xv[0][j] = g;
    }
    store_planes<1, W>(dp, V, i, xv);
  }
}

// ---- voxel form (Dice sums + CE).  3K + 1 per-thread sums -> one row {I, P2, P1, F = 0}_k, CE of 4K + 1 per workgroup: the lanes
// of a wave by DPP, the four waves through LDS in wave order
template <int K> DEVI void ce_stats_row(const float (&acc)[3 * K + 1], float* __restrict__ row) {
  constexpr int T = 3 * K + 1;
  __shared__ float sm[SM_BLOCK / 64][T];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const float v = wave_sum_lane63(acc[t]);
    if (lane == 63) sm[wave][t] = v;
  }
  __syncthreads();
  const int c = threadIdx.x;  // the column of the row
  if (c < 4 * K + 1) {
    float s = 0.f;
    if ((c & 3) < 3 || c == 4 * K) {
      const int src = c == 4 * K ? 3 * K : 3 * (c >> 2) + (c & 3);
      s = sm[0][src];
#pragma unroll
      for (int w = 1; w < SM_BLOCK / 64; ++w) s += sm[w][src];
    }
    row[c] = s;
  }
}

// grid (blocks, N); part[block][n][4K + 1]
template <int K, int W> __global__ void __launch_bounds__(SM_BLOCK) sigmoid_ce_stats_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                                   const uint8_t* __restrict__ y, float* __restrict__ part, size_t V) {
  constexpr int T = 3 * K + 1;
  const int n = blockIdx.y;
  const float* xp = x + (size_t)n * K * V;
  const float* tp = t + (size_t)n * K * V;
  const uint8_t* yp = y + (size_t)n * V;
  float acc[T];
#pragma unroll
  for (int a = 0; a < T; ++a) acc[a] = 0.f;
  const size_t groups = V / W;
  for (size_t i = (size_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < groups; i += (size_t)gridDim.x * SM_BLOCK) {
    float xv[K][W], tv[K][W];
    load_planes<K, W>(xp, V, i, xv);
    load_planes<K, W>(tp, V, i, tv);
    const uint32_t labs = load_labels<W>(yp, i);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      float xs[K], ex[K], dy;
#pragma unroll
      for (int k = 0; k < K; ++k) xs[k] = xv[k][j];
      const float s = softmax_parts<K>(xs, (labs >> (8 * j)) & 255u, ex, dy);
      acc[3 * K] += __logf(s) - dy;  // logsumexp - x_y, the maximum cancelled before the subtraction
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float e, a, p, q;
        sigmoid_parts(xs[k], e, a, p, q);
        acc[3 * k] += p * tv[k][j];
        acc[3 * k + 1] += p * p;
        acc[3 * k + 2] += p;
      }
    }
  }
  ce_stats_row<K>(acc, part + ((size_t)blockIdx.x * gridDim.y + n) * (4 * K + 1));
}

// grid (blocks, N); coef[n][4K + 1] = {A_k, B_k, C_k, Fc_k}_k, c (Fc is not read)
template <int K, int W> __global__ void __launch_bounds__(SM_BLOCK) sigmoid_ce_grad_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                                  const uint8_t* __restrict__ y, const float* __restrict__ coef,
                                                                                  float* __restrict__ dx, size_t V) {
  const int n = blockIdx.y;
  const float* xp = x + (size_t)n * K * V;
  const float* tp = t + (size_t)n * K * V;
  const uint8_t* yp = y + (size_t)n * V;
  float* dp = dx + (size_t)n * K * V;
  const float* cf = coef + (size_t)n * (4 * K + 1);
  float A[K], B2[K], C[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { A[k] = cf[4 * k]; B2[k] = 2.f * cf[4 * k + 1]; C[k] = cf[4 * k + 2]; }
  const float c = cf[4 * K];
  const size_t groups = V / W;
  for (size_t i = (size_t)blockIdx.x * SM_BLOCK + threadIdx.x; i < groups; i += (size_t)gridDim.x * SM_BLOCK) {
    float xv[K][W], tv[K][W];
    load_planes<K, W>(xp, V, i, xv);
    load_planes<K, W>(tp, V, i, tv);
    const uint32_t labs = load_labels<W>(yp, i);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const uint32_t lab = (labs >> (8 * j)) & 255u;
      float xs[K], ex[K], dy;
#pragma unroll
      for (int k = 0; k < K; ++k) xs[k] = xv[k][j];
      const float inv = 1.f / softmax_parts<K>(xs, lab, ex, dy);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float e, a, p, q;
        sigmoid_parts(xs[k], e, a, p, q);
        xv[k][j] = p * q * (A[k] * tv[k][j] + B2[k] * p + C[k]) + c * (ex[k] * inv - (lab == (uint32_t)k ? 1.f : 0.f));
      }
    }
    store_planes<K, W>(dp, V, i, xv);
  }
}

static int check_planes(const char* what, int N, int K, size_t voxels) {
  if (N <= 0 || N > 65535 || voxels == 0) BRATS_FAIL(BRATS_E_ARG, "%s: bad batch or voxel count", what);
  if (K < 1 || K > SM_MAX_K) BRATS_FAIL(BRATS_E_ARG, "%s: %d classes (1 .. %d are built)", what, K, SM_MAX_K);
  return 0;
}
static int check_terms(const char* what, int terms, const uint8_t* classmap) {
  if (terms & ~(BRATS_SIG_FOCAL | BRATS_SIG_CE)) BRATS_FAIL(BRATS_E_ARG, "%s: unknown bits in the term mask %d", what, terms);
  if (terms == (BRATS_SIG_FOCAL | BRATS_SIG_CE))
    BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: the focal and the CE term together are not built (no criterion of the reference has both)", what);
  if ((terms & BRATS_SIG_CE) && !classmap) BRATS_FAIL(BRATS_E_ARG, "%s: the CE term needs the class map", what);
  return 0;
}

extern "C" size_t brats_sigmoid_loss_ws_floats(int N, int K) {
  if (N <= 0 || K < 1 || K > SM_MAX_K) return 0;
  return (size_t)SM_MAX_BLOCKS * N * (4 * K + 1);
}

extern "C" int brats_sigmoid_target_prepare(const float* target, float* tsums /*[N][2K]*/, uint8_t* classmap, float* ws, int N, int K,
                                            size_t voxels, brats_stream_t s) {
  if (!target || !tsums || !ws) BRATS_FAIL(BRATS_E_ARG, "sigmoid_target_prepare: null pointer");
  if (int rc = check_planes("sigmoid_target_prepare", N, K, voxels)) return rc;
  hipStream_t st = (hipStream_t)s;
  const bool vec = voxels % 4 == 0 && aligned_to(target, 16) && (!classmap || aligned_to(classmap, 4));
  const unsigned gx = sm_grid(voxels, vec ? 4 : 1, N);
  with_planes(K, [&](auto k) {
    constexpr int KK = decltype(k)::value;
    if (vec && classmap) hipLaunchKernelGGL((sigmoid_prepare_kernel<KK, 4, true>), dim3(gx, N), dim3(SM_BLOCK), 0, st, target, classmap, ws, voxels);
    else if (vec) hipLaunchKernelGGL((sigmoid_prepare_kernel<KK, 4, false>), dim3(gx, N), dim3(SM_BLOCK), 0, st, target, classmap, ws, voxels);
    else if (classmap) hipLaunchKernelGGL((sigmoid_prepare_kernel<KK, 1, true>), dim3(gx, N), dim3(SM_BLOCK), 0, st, target, classmap, ws, voxels);
    else hipLaunchKernelGGL((sigmoid_prepare_kernel<KK, 1, false>), dim3(gx, N), dim3(SM_BLOCK), 0, st, target, classmap, ws, voxels);
    return 0;
  });
  brats_ordered_sum(ws, tsums, (int)gx, N * 2 * K, st);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_sigmoid_loss_stats(const float* logits, const float* target, const uint8_t* classmap, float* sums /*[N][4K+1]*/,
                                        float* ws, int N, int K, size_t voxels, int terms, float gamma, brats_stream_t s) {
  if (!logits || !target || !sums || !ws) BRATS_FAIL(BRATS_E_ARG, "sigmoid_loss_stats: null pointer");
  if (int rc = check_planes("sigmoid_loss_stats", N, K, voxels)) return rc;
  if (int rc = check_terms("sigmoid_loss_stats", terms, classmap)) return rc;
  hipStream_t st = (hipStream_t)s;
  bool vec = voxels % 4 == 0 && aligned_to(logits, 16) && aligned_to(target, 16);
  unsigned gx;
  if (terms & BRATS_SIG_CE) {
    vec = vec && aligned_to(classmap, 4);
    gx = sm_grid(voxels, vec ? sig_voxels(K) : 1, N);
    with_planes(K, [&](auto k) {
      constexpr int KK = decltype(k)::value;
      if (vec) hipLaunchKernelGGL((sigmoid_ce_stats_kernel<KK, sig_voxels(KK)>), dim3(gx, N), dim3(SM_BLOCK), 0, st, logits, target, classmap, ws, voxels);
      else hipLaunchKernelGGL((sigmoid_ce_stats_kernel<KK, 1>), dim3(gx, N), dim3(SM_BLOCK), 0, st, logits, target, classmap, ws, voxels);
      return 0;
    });
  } else {
    gx = sm_grid(voxels, vec ? 4 : 1, N * K);  // about 2048 workgroups over the N * K planes
    const dim3 grid(gx, N, K);
    if (terms & BRATS_SIG_FOCAL) {
      if (vec) hipLaunchKernelGGL((sigmoid_plane_stats_kernel<4, true>), grid, dim3(SM_BLOCK), 0, st, logits, target, ws, voxels, gamma);
      else hipLaunchKernelGGL((sigmoid_plane_stats_kernel<1, true>), grid, dim3(SM_BLOCK), 0, st, logits, target, ws, voxels, gamma);
    } else {
      if (vec) hipLaunchKernelGGL((sigmoid_plane_stats_kernel<4, false>), grid, dim3(SM_BLOCK), 0, st, logits, target, ws, voxels, gamma);
      else hipLaunchKernelGGL((sigmoid_plane_stats_kernel<1, false>), grid, dim3(SM_BLOCK), 0, st, logits, target, ws, voxels, gamma);
    }
  }
  brats_ordered_sum(ws, sums, (int)gx, N * (4 * K + 1), st);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_sigmoid_loss_grad(const float* logits, const float* target, const uint8_t* classmap, const float* coef /*[N][4K+1]*/,
                                       float* dlogits, int N, int K, size_t voxels, int terms, float gamma, brats_stream_t s) {
  if (!logits || !target || !coef || !dlogits) BRATS_FAIL(BRATS_E_ARG, "sigmoid_loss_grad: null pointer");
  if (int rc = check_planes("sigmoid_loss_grad", N, K, voxels)) return rc;
  if (int rc = check_terms("sigmoid_loss_grad", terms, classmap)) return rc;
  hipStream_t st = (hipStream_t)s;
  bool vec = voxels % 4 == 0 && aligned_to(logits, 16) && aligned_to(target, 16) && aligned_to(dlogits, 16);
  if (terms & BRATS_SIG_CE) {
    vec = vec && aligned_to(classmap, 4);
    const unsigned gx = sm_grid(voxels, vec ? sig_voxels(K) : 1, N);
    with_planes(K, [&](auto k) {
      constexpr int KK = decltype(k)::value;
      if (vec) hipLaunchKernelGGL((sigmoid_ce_grad_kernel<KK, sig_voxels(KK)>), dim3(gx, N), dim3(SM_BLOCK), 0, st, logits, target, classmap, coef, dlogits, voxels);
      else hipLaunchKernelGGL((sigmoid_ce_grad_kernel<KK, 1>), dim3(gx, N), dim3(SM_BLOCK), 0, st, logits, target, classmap, coef, dlogits, voxels);
      return 0;
    });
  } else {
    const dim3 grid(sm_grid(voxels, vec ? 4 : 1, N * K), N, K);
    if (terms & BRATS_SIG_FOCAL) {
      if (vec) hipLaunchKernelGGL((sigmoid_plane_grad_kernel<4, true>), grid, dim3(SM_BLOCK), 0, st, logits, target, coef, dlogits, voxels, gamma);
      else hipLaunchKernelGGL((sigmoid_plane_grad_kernel<1, true>), grid, dim3(SM_BLOCK), 0, st, logits, target, coef, dlogits, voxels, gamma);
    } else {
      if (vec) hipLaunchKernelGGL((sigmoid_plane_grad_kernel<4, false>), grid, dim3(SM_BLOCK), 0, st, logits, target, coef, dlogits, voxels, gamma);
      else hipLaunchKernelGGL((sigmoid_plane_grad_kernel<1, false>), grid, dim3(SM_BLOCK), 0, st, logits, target, coef, dlogits, voxels, gamma);
    }
  }
  BRATS_CHECK_LAUNCH();
  return 0;
}
