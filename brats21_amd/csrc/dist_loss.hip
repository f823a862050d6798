// Distance-map losses of learning/losses.py as src/definer.py:246-282 configures them (sigmoid, reduction mean) on f32
// logits x [N][K][voxels], p = sigmoid(x):
//   onehot : probs2one_hot (learning/losses.py:43-56), the arg-max over the channels of p as uint8 [N][K][voxels]
//   hd     : HausdorffLoss   sum (p - t)^2 w,  w = tdm^alpha + pdm^alpha      dx = 2 (p - t) w p (1 - p) scale
//   bnd    : SurfaceLoss     sum p dist                                         dx = dist p (1 - p) scale
// The fields (edt.hip) carry no gradient.  Each loss is one statistics pass (one partial per block, added in block order by
// brats_ordered_sum: bitwise reproducible) and one gradient pass; `scale` is a device scalar (upstream gradient / count), so
// nothing here reads the host.  Bytes per element: hd 16 read (x, t, tdm, pdm) forward, 16 read + 4 written backward -- w is
// recomputed from the two fields, since writing it once and rereading it moves the same 36 B and holds one more tensor per
// head; bnd 8 read forward, 8 read + 4 written backward; onehot 4 read + 1 written.
#include "common.hpp"

namespace {

constexpr int MAX_BLOCKS = 2048;

// p = sigmoid(x) and q = 1 - p, neither by a cancelling subtraction; saturates like torch.sigmoid (p == 1 from x ~ 17 on)
DEVI void sigmoid_pq(float x, float& p, float& q) {
  const float e = __expf(-fabsf(x)), a = 1.f / (1.f + e), b = e * a;
  p = x >= 0.f ? a : b;
  q = x >= 0.f ? b : a;
}
// p - t without cancellation for a 0/1 target: (1 - t) - q where p is close to 1
DEVI float p_minus_t(float x, float p, float q, float t) { return x >= 0.f ? (1.f - t) - q : p - t; }

template <bool SQ> DEVI float hd_weight(float tdm, float pdm, float alpha) {
  return SQ ? tdm * tdm + pdm * pdm : powf(tdm, alpha) + powf(pdm, alpha);
}

__global__ __launch_bounds__(256) void argmax_onehot_kernel(const float* __restrict__ x, uint8_t* __restrict__ oh, int K, size_t voxels) {
  const size_t base = (size_t)blockIdx.y * K * voxels;
  for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < voxels; v += (size_t)gridDim.x * blockDim.x) {
    int best = 0;
    float pb = -1.f;
    for (int k = 0; k < K; ++k) {
      float p, q;
      sigmoid_pq(x[base + (size_t)k * voxels + v], p, q);
      if (p > pb) { pb = p; best = k; }  // strictly greater: ties stay with the lowest channel
    }
    for (int k = 0; k < K; ++k) oh[base + (size_t)k * voxels + v] = k == best ? 1 : 0;
  }
}

// one partial per block at part[blockIdx.x]
DEVI void block_partial(float s, float* __restrict__ part) {
  __shared__ float r[256];
  r[threadIdx.x] = s;
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if ((int)threadIdx.x < m) r[threadIdx.x] += r[threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = r[0];
}

template <bool SQ>
__global__ __launch_bounds__(256) void hd_stats_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                       const float* __restrict__ tdm, const float* __restrict__ pdm, float alpha,
                                                       float* __restrict__ part, size_t total) {
  float s = 0.f;
  auto term = [&](float xv, float tv, float a, float b) {
    float p, q;
    sigmoid_pq(xv, p, q);
    const float d = p_minus_t(xv, p, q, tv);
    s += d * d * hd_weight<SQ>(a, b, alpha);
  };
  const size_t n4 = total / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 xv = ((const f32x4*)x)[i], tv = ((const f32x4*)t)[i], av = ((const f32x4*)tdm)[i], bv = ((const f32x4*)pdm)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) term(xv[j], tv[j], av[j], bv[j]);
  }
  if (blockIdx.x == 0)
    for (size_t i = n4 * 4 + threadIdx.x; i < total; i += blockDim.x) term(x[i], t[i], tdm[i], pdm[i]);
  block_partial(s, part);
}

template <bool SQ>
__global__ __launch_bounds__(256) void hd_grad_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                      const float* __restrict__ tdm, const float* __restrict__ pdm, float alpha,
                                                      const float* __restrict__ scale, float* __restrict__ dx, size_t total) {
  const float sc = 2.f * scale[0];
  auto grad = [&](float xv, float tv, float a, float b) {
    float p, q;
    sigmoid_pq(xv, p, q);
    return sc * p_minus_t(xv, p, q, tv) * hd_weight<SQ>(a, b, alpha) * (p * q);
  };
  const size_t n4 = total / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 xv = ((const f32x4*)x)[i], tv = ((const f32x4*)t)[i], av = ((const f32x4*)tdm)[i], bv = ((const f32x4*)pdm)[i];
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = grad(xv[j], tv[j], av[j], bv[j]);
    ((f32x4*)dx)[i] = o;
  }
  if (blockIdx.x == 0)
    for (size_t i = n4 * 4 + threadIdx.x; i < total; i += blockDim.x) dx[i] = grad(x[i], t[i], tdm[i], pdm[i]);
}

__global__ __launch_bounds__(256) void bnd_stats_kernel(const float* __restrict__ x, const float* __restrict__ dist,
                                                        float* __restrict__ part, size_t total) {
  float s = 0.f;
  auto term = [&](float xv, float dv) {
    float p, q;
    sigmoid_pq(xv, p, q);
    s += p * dv;
  };
  const size_t n4 = total / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 xv = ((const f32x4*)x)[i], dv = ((const f32x4*)dist)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) term(xv[j], dv[j]);
  }
  if (blockIdx.x == 0)
    for (size_t i = n4 * 4 + threadIdx.x; i < total; i += blockDim.x) term(x[i], dist[i]);
  block_partial(s, part);
}

__global__ __launch_bounds__(256) void bnd_grad_kernel(const float* __restrict__ x, const float* __restrict__ dist,
                                                       const float* __restrict__ scale, float* __restrict__ dx, size_t total) {
  const float sc = scale[0];
  auto grad = [&](float xv, float dv) {
    float p, q;
    sigmoid_pq(xv, p, q);
    return sc * dv * (p * q);
  };
  const size_t n4 = total / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 xv = ((const f32x4*)x)[i], dv = ((const f32x4*)dist)[i];
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = grad(xv[j], dv[j]);
    ((f32x4*)dx)[i] = o;
  }
  if (blockIdx.x == 0)
    for (size_t i = n4 * 4 + threadIdx.x; i < total; i += blockDim.x) dx[i] = grad(x[i], dist[i]);
}

inline unsigned blocks_for(size_t total) {
  const size_t b = (total / 4 + 255) / 256 / 4;
  return (unsigned)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}
inline bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

}  // namespace

extern "C" size_t brats_dist_loss_ws_floats(void) { return MAX_BLOCKS; }

extern "C" int brats_sigmoid_argmax_onehot(const float* logits, uint8_t* onehot, int N, int K, size_t voxels, brats_stream_t s) {
  if (!logits || !onehot || N <= 0 || N > 65535 || K <= 0 || voxels == 0) BRATS_FAIL(BRATS_E_ARG, "sigmoid_argmax_onehot: bad argument");
  const size_t b = (voxels + 255) / 256;
  hipLaunchKernelGGL(argmax_onehot_kernel, dim3((unsigned)(b > 4096 ? 4096 : b), N), dim3(256), 0, (hipStream_t)s, logits, onehot, K,
                     voxels);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_hd_loss_stats(const float* logits, const float* target, const float* tdm, const float* pdm, float alpha,
                                   float* sum, float* ws, size_t total, brats_stream_t s) {
  if (!logits || !target || !tdm || !pdm || !sum || !ws || total == 0 || !(alpha > 0.f))
    BRATS_FAIL(BRATS_E_ARG, "hd_loss_stats: bad argument");
  if (!aligned16(logits) || !aligned16(target) || !aligned16(tdm) || !aligned16(pdm))
    BRATS_FAIL(BRATS_E_ARG, "hd_loss_stats: tensors must be 16-byte aligned");
  hipStream_t st = (hipStream_t)s;
  const unsigned gx = blocks_for(total);
  if (alpha == 2.f) hipLaunchKernelGGL(hd_stats_kernel<true>, dim3(gx), dim3(256), 0, st, logits, target, tdm, pdm, alpha, ws, total);
  else hipLaunchKernelGGL(hd_stats_kernel<false>, dim3(gx), dim3(256), 0, st, logits, target, tdm, pdm, alpha, ws, total);
  brats_ordered_sum(ws, sum, (int)gx, 1, st);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_hd_loss_grad(const float* logits, const float* target, const float* tdm, const float* pdm, float alpha,
                                  const float* scale, float* dlogits, size_t total, brats_stream_t s) {
  if (!logits || !target || !tdm || !pdm || !scale || !dlogits || total == 0 || !(alpha > 0.f))
    BRATS_FAIL(BRATS_E_ARG, "hd_loss_grad: bad argument");
  if (!aligned16(logits) || !aligned16(target) || !aligned16(tdm) || !aligned16(pdm) || !aligned16(dlogits))
    BRATS_FAIL(BRATS_E_ARG, "hd_loss_grad: tensors must be 16-byte aligned");
  hipStream_t st = (hipStream_t)s;
  const unsigned gx = blocks_for(total);
  if (alpha == 2.f)
    hipLaunchKernelGGL(hd_grad_kernel<true>, dim3(gx), dim3(256), 0, st, logits, target, tdm, pdm, alpha, scale, dlogits, total);
  else
    hipLaunchKernelGGL(hd_grad_kernel<false>, dim3(gx), dim3(256), 0, st, logits, target, tdm, pdm, alpha, scale, dlogits, total);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_boundary_loss_stats(const float* logits, const float* dist, float* sum, float* ws, size_t total,
                                         brats_stream_t s) {
  if (!logits || !dist || !sum || !ws || total == 0) BRATS_FAIL(BRATS_E_ARG, "boundary_loss_stats: bad argument");
  if (!aligned16(logits) || !aligned16(dist)) BRATS_FAIL(BRATS_E_ARG, "boundary_loss_stats: tensors must be 16-byte aligned");
  hipStream_t st = (hipStream_t)s;
  const unsigned gx = blocks_for(total);
  hipLaunchKernelGGL(bnd_stats_kernel, dim3(gx), dim3(256), 0, st, logits, dist, ws, total);
  brats_ordered_sum(ws, sum, (int)gx, 1, st);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_boundary_loss_grad(const float* logits, const float* dist, const float* scale, float* dlogits, size_t total,
                                        brats_stream_t s) {
  if (!logits || !dist || !scale || !dlogits || total == 0) BRATS_FAIL(BRATS_E_ARG, "boundary_loss_grad: bad argument");
  if (!aligned16(logits) || !aligned16(dist) || !aligned16(dlogits))
    BRATS_FAIL(BRATS_E_ARG, "boundary_loss_grad: tensors must be 16-byte aligned");
  hipLaunchKernelGGL(bnd_grad_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)s, logits, dist, scale, dlogits, total);
  BRATS_CHECK_LAUNCH();
  return 0;
}
