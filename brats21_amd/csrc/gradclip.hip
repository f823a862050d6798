// Multi-tensor gradient clipping: global-norm clipping (torch.nn.utils.clip_grad_norm_, the reference's --gradient_clipping,
// learning/engine.py:442-452) and adaptive gradient clipping (the reference's AGC, learning/lr_scheduler.py:114-215, its
// --adaptive_gradient_clipping).  The reference walks the parameters in Python with about a dozen small torch ops and two
// host-to-device uploads per tensor; here one call is at most three launches over ALL tensors, none of which touches the host:
//   gradclip_stats    : one WG per unit (unitwise_norm's unit: an output-channel slice of a 4/5-D weight, a column of a 2/3-D
//                       one, a whole 0/1-D tensor): (sum p^2, sum g^2) -> stats[unit]
//   gradclip_finalise : total_norm = sqrt(sum over units of sum g^2) / grad_scale, clip_coef = min(1, max_norm / (total_norm + 1e-6))
//   gradclip_apply    : one WG per 2048-element chunk, in place: g <- g * clip_coef * f_unit
// Every reduction has a fixed order and no atomics: the result is the same bit pattern at every run.
// Pure f32 streaming: the stats pass reads 8 B/param (4 without AGC), the apply pass reads and writes 4 B/param each.
#include "common.hpp"

static constexpr int GRADCLIP_CHUNK = 2048;

// The GradScaler pair of ranger.hip: grad_scale = the loss scale the gradients still carry (NULL = already unscaled), found_inf =
// non-zero when a gradient overflowed -- then every kernel returns at once and writes nothing.
struct ClipAmp {
  const float* grad_scale;
  const float* found_inf;
  __device__ bool skip() const { return found_inf && *found_inf != 0.f; }
  __device__ float inv() const { return grad_scale ? 1.f / *grad_scale : 1.f; }
};

// 256 partial sums -> red[0]: the 8-level tree of ranger.hip (thread t adds t + m)
__device__ __forceinline__ void tree256(float* red) {
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
    __syncthreads();
  }
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <bool WITH_P>
__global__ void __launch_bounds__(256) gradclip_stats_kernel(const brats_gradclip_tensor* __restrict__ tab, const int* __restrict__ units,
                                                             float* __restrict__ stats /* [nunits][2] */, ClipAmp amp) {
  if (amp.skip()) return;
  const int t = units[blockIdx.x * 2], u = units[blockIdx.x * 2 + 1];
  const brats_gradclip_tensor T = tab[t];
  const int n = T.unit_len;
  float sp = 0.f, sg = 0.f;
  if (T.unit_stride > 1) {  // a column of a 2-D / 3-D tensor: element j of unit u lies at u + j * stride
    const float* __restrict__ g = (const float*)T.grad + u;
    const float* __restrict__ p = (const float*)T.param + u;
    for (int j = threadIdx.x; j < n; j += 256) {
      const size_t o = (size_t)j * T.unit_stride;
      const float gv = g[o];
      sg += gv * gv;
      if (WITH_P) { const float pv = p[o]; sp += pv * pv; }
    }
  } else {
    const float* __restrict__ g = (const float*)T.grad + (size_t)u * n;
    const float* __restrict__ p = (const float*)T.param + (size_t)u * n;
    if ((n & 3) == 0 && aligned16(g) && (!WITH_P || aligned16(p))) {
      // 16-byte loads, four running sums per operand so that a thread's chain of additions stays n / 1024 long
      const float4* __restrict__ g4 = (const float4*)g;
      const float4* __restrict__ p4 = (const float4*)p;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
      for (int j = threadIdx.x; j < (n >> 2); j += 256) {
        const float4 gv = g4[j];
        a0 += gv.x * gv.x; a1 += gv.y * gv.y; a2 += gv.z * gv.z; a3 += gv.w * gv.w;
        if (WITH_P) {
          const float4 pv = p4[j];
          b0 += pv.x * pv.x; b1 += pv.y * pv.y; b2 += pv.z * pv.z; b3 += pv.w * pv.w;
        }
      }
      sg = (a0 + a1) + (a2 + a3);
      sp = (b0 + b1) + (b2 + b3);
    } else {
      for (int j = threadIdx.x; j < n; j += 256) {
        const float gv = g[j];
        sg += gv * gv;
        if (WITH_P) { const float pv = p[j]; sp += pv * pv; }
      }
    }
  }
  __shared__ float rg[256], rp[256];
  rg[threadIdx.x] = sg;
  tree256(rg);
  if (WITH_P) {
    rp[threadIdx.x] = sp;
    tree256(rp);
  }
  if (threadIdx.x == 0) {
    float* out = stats + (size_t)(T.unit_base + u) * 2;
    if (WITH_P) out[0] = rp[0];
    out[1] = rg[0];
  }
}

// One WG: thread t adds units t, t + 256, ... in f64, then the same fixed tree in f64.  max_norm < 0: no global clipping, the
// coefficient is 1 (the total norm is still reported).
__global__ void __launch_bounds__(256) gradclip_finalise_kernel(const float* __restrict__ stats, int nunits, float max_norm,
                                                                float* __restrict__ pair /* {total_norm, clip_coef} */, ClipAmp amp) {
  if (amp.skip()) return;
  double s = 0.0;
  for (int u = threadIdx.x; u < nunits; u += 256) s += (double)stats[(size_t)u * 2 + 1];
  __shared__ double red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float total = (float)(sqrt(red[0]) * (double)amp.inv());
    pair[0] = total;
    pair[1] = max_norm >= 0.f ? fminf(1.f, max_norm / (total + 1e-6f)) : 1.f;  // torch.nn.utils.clip_grad_norm_'s formula
  }
}

// AGC's factor of one unit (learning/lr_scheduler.py:203-213) from its sums, on the globally clipped, UNSCALED gradient
__device__ __forceinline__ float agc_factor(const float* __restrict__ stats, int unit, float coef, float ginv, float clipping, float eps) {
  const float gn = coef * sqrtf(stats[(size_t)unit * 2 + 1]) * ginv;
  const float pn = fmaxf(sqrtf(stats[(size_t)unit * 2]), eps);
  const float mx = pn * clipping;
  return gn > mx ? mx / fmaxf(gn, 1e-6f) : 1.f;
}

// g <- g * clip_coef * f_unit, in place (the gradient keeps its loss scale).  pair == NULL: clip_coef = 1; agc_clipping < 0: f = 1.
__global__ void __launch_bounds__(256) gradclip_apply_kernel(const brats_gradclip_tensor* __restrict__ tab, const int* __restrict__ chunks,
                                                             const float* __restrict__ stats, const float* __restrict__ pair,
                                                             float agc_clipping, float agc_eps, ClipAmp amp) {
  if (amp.skip()) return;
  const float coef = pair ? pair[1] : 1.f;
  const bool agc = agc_clipping >= 0.f;
  if (!agc && coef == 1.f) return;  // nothing to scale (torch multiplies by 1 here: the same bits)
  const float ginv = amp.inv();
  const int t = chunks[blockIdx.x * 2];
  const brats_gradclip_tensor T = tab[t];
  const unsigned numel = (unsigned)T.numel;  // (< 2^31: checked by the host)
  const unsigned base = (unsigned)chunks[blockIdx.x * 2 + 1] * GRADCLIP_CHUNK;
  const unsigned end = base + GRADCLIP_CHUNK < numel ? base + GRADCLIP_CHUNK : numel;
  float* __restrict__ g = (float*)T.grad;
  const unsigned ulen = (unsigned)T.unit_len, ustride = (unsigned)T.unit_stride;
  const bool strided = ustride > 1;
  if (!strided && (ulen & 3) == 0 && aligned16(g)) {
    // (numel is a multiple of ulen, so of 4: whole float4s, each inside one unit)
    float4* __restrict__ g4 = (float4*)g;
    int last = -1;
    float f = 1.f;
    for (unsigned i = (base >> 2) + threadIdx.x; i < (end >> 2); i += 256) {
      if (agc) {
        const int unit = T.unit_base + (int)((i << 2) / ulen);
        if (unit != last) { f = agc_factor(stats, unit, coef, ginv, agc_clipping, agc_eps); last = unit; }
      }
      float4 v = g4[i];
      v.x = v.x * coef * f; v.y = v.y * coef * f; v.z = v.z * coef * f; v.w = v.w * coef * f;
      g4[i] = v;
    }
  } else {
    int last = -1;
    float f = 1.f;
    for (unsigned i = base + threadIdx.x; i < end; i += 256) {
      if (agc) {
        const int unit = T.unit_base + (int)(strided ? i % ustride : i / ulen);
        if (unit != last) { f = agc_factor(stats, unit, coef, ginv, agc_clipping, agc_eps); last = unit; }
      }
      g[i] = g[i] * coef * f;
    }
  }
}

extern "C" int brats_gradclip_chunk(void) { return GRADCLIP_CHUNK; }

extern "C" int brats_gradclip(const brats_gradclip_tensor* table, int ntensors, const int* units, int nunits, const int* chunks,
                              int nchunks, float* stats, float* pair, float max_norm, float agc_clipping, float agc_eps,
                              const float* grad_scale, const float* found_inf, brats_stream_t s) {
  const ClipAmp amp{grad_scale, found_inf};
  if (!table || ntensors <= 0 || !units || nunits <= 0 || !chunks || nchunks <= 0 || !stats)
    BRATS_FAIL(BRATS_E_ARG, "gradclip: empty tensor / unit / chunk table or no stats workspace");
  const bool agc = agc_clipping >= 0.f;
  if (!agc && !pair) BRATS_FAIL(BRATS_E_ARG, "gradclip: neither global-norm clipping (pair) nor AGC (agc_clipping >= 0) asked for");
  if (max_norm >= 0.f && !pair) BRATS_FAIL(BRATS_E_ARG, "gradclip: global-norm clipping needs the {total_norm, clip_coef} pair");
  if (agc && !(agc_eps >= 0.f)) BRATS_FAIL(BRATS_E_ARG, "gradclip: agc_eps must be >= 0");
  hipStream_t st = (hipStream_t)s;
  if (agc) hipLaunchKernelGGL(gradclip_stats_kernel<true>, dim3(nunits), dim3(256), 0, st, table, units, stats, amp);
  else hipLaunchKernelGGL(gradclip_stats_kernel<false>, dim3(nunits), dim3(256), 0, st, table, units, stats, amp);
  BRATS_CHECK_LAUNCH();
  if (pair) {
    hipLaunchKernelGGL(gradclip_finalise_kernel, dim3(1), dim3(256), 0, st, (const float*)stats, nunits, max_norm, pair, amp);
    BRATS_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(gradclip_apply_kernel, dim3(nchunks), dim3(256), 0, st, table, chunks, (const float*)stats, (const float*)pair,
                     agc_clipping, agc_eps, amp);
  BRATS_CHECK_LAUNCH();
  return 0;
}
