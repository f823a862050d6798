// Additive attention gate of the reference's AttUnet / R2AttUnet (AttentionBlock, networks/unet_family.py:104-131) on NDHWC
// tensors of f32, bf16 or fp16 storage:
//   g1 = BN_g(W_g g + b_g),  x1 = BN_x(W_x x + b_x)      1x1x1 convolutions to f_int channels, BatchNorm3d
//   s  = g1 + x1,  p = act(s)
//   q  = w_psi . p (+ b_psi),  alpha = sigmoid(BN_1(q))   one channel, BatchNorm3d(1)
//   out = x alpha
// The two f_int-wide convolutions (forward, input and weight gradients) and their batch statistics are the library's own
// kernels; this file holds what lies between them and the gate itself.  The raw convolution outputs g1raw / x1raw and the f32 plane
// q (WITHOUT b_psi: it cancels in the training-mode normalisation and is carried by the finaliser's tables otherwise, so the
// variance of the plane loses no digits to it) are all that is stored: s, p and alpha are recomputed wherever they are needed.
// The batch is walked as ONE sample of M = N * voxels voxels (BatchNorm's statistics run over all of them; NDHWC with a channel
// pitch is contiguous in the voxel index across samples), with 64-bit voxel indices.
// Every reduction goes through per-workgroup partials that are added in a fixed order: no floating-point atomics, the same
// bits at every run.  The per-voxel sums over channels are added in channel-vector order from LDS; the sums over voxels are
// accumulated in f64 (plane statistics) or f32 per thread and f64 across lanes and workgroups.
// Small tables (all f32):
//   ss_g / ss_x [C][2]  scale, shift of BN_g / BN_x as brats_gn_finalize writes them (eval mode: from the running buffers)
//   mr_g / mr_x [C][2]  mean, rstd of the same
//   st1 [8]             BN_1: {mean of q + b_psi, biased variance, rstd, sub, a, b, -, -} with qhat = (q - sub) rstd and
//                       BN_1(q) = a q + b; training: sub = mean of the plane, eval: sub = running_mean - b_psi
//   bw1 [4]             BN_1 backward: {sum dqn qhat, sum dqn, m1, m2}: dq = a (dqn - m1 - qhat m2); m1 = m2 = 0 in eval mode
//   coef [3][C]         BN_g / BN_x backward: mean ds, mean ds ghat, mean ds xhat (zeros in eval mode)
//   sums [4 C + 1]      sum ds, sum ds ghat, sum ds xhat, sum dq p (each [C]), sum dq
// Limits: C (f_int padded, or the channels of x) a multiple of the 16-byte channel vector and at most 256 vectors (1024 channels
// in f32, 2048 in 16-bit storage); any N and voxels whose product fits size_t (voxels < 2^31 per sample).
#include "twin_begin.hpp"
#include "common.hpp"
#include "act.hpp"
#include <math.h>

namespace {

constexpr int AG_MAX_BLOCKS = 2048;
constexpr int AG_K = 4;  // voxels a lane has in flight in the passes that reduce over channels

DEVI float ag_sigm(float a) { return 1.f / (1.f + __expf(-a)); }

// workgroups of a pass over M voxels of C channels (all passes are grid-stride: any count is correct, this one sizes the partials)
int ag_blocks(int vw, int C, size_t M) {
  const int vl = 256 / (C / vw);
  const size_t b = (M + (size_t)vl * AG_K - 1) / ((size_t)vl * AG_K);
  return (int)(b < 1 ? 1 : (b > (size_t)AG_MAX_BLOCKS ? (size_t)AG_MAX_BLOCKS : b));
}

// sum over the 256 threads in a fixed tree; red: 256 doubles of LDS
DEVI double ag_block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// The walk of the passes that reduce over the channels of a voxel: 256 threads = cv channel vectors x vl voxel lanes, AG_K voxels
// per lane and step.  partial(vox) = this thread's share of the voxel's sum (its own channel vector); the cv shares go through
// LDS and are added in channel-vector order by one thread per voxel, which hands the sum to finish(vox, sum).
template <typename P, typename F>
DEVI void ag_voxel_sums(size_t M, int cv, float* red, P&& partial, F&& finish) {
  const int vl = 256 / cv;
  const int mycv = threadIdx.x % cv, myvl = threadIdx.x / cv;
  const bool live = myvl < vl;
  const size_t span = (size_t)AG_K * vl;
  for (size_t base = (size_t)blockIdx.x * span; base < M; base += (size_t)gridDim.x * span) {
    float d[AG_K];
#pragma unroll
    for (int k = 0; k < AG_K; ++k) {
      const size_t vox = base + (size_t)k * vl + myvl;
      d[k] = (live && vox < M) ? partial(vox) : 0.f;
    }
    if (live) {
#pragma unroll
      for (int k = 0; k < AG_K; ++k) red[(k * vl + myvl) * cv + mycv] = d[k];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < AG_K * vl; t += 256) {
      const size_t vox = base + t;
      if (vox < M) {
        float s = 0.f;
        for (int i = 0; i < cv; ++i) s += red[t * cv + i];
        finish(vox, s);
      }
    }
    __syncthreads();
  }
}

// ---- forward: q = w_psi . act(BN_g(g1raw) + BN_x(x1raw)), the plane and (training) its per-workgroup (sum, sum of squares)
template <typename T, bool HEAVY>
__global__ void __launch_bounds__(256) ag_psi_fwd_kernel(const T* __restrict__ g1, int gpitch, const T* __restrict__ x1, int xpitch,
                                                         const float* __restrict__ ssg, const float* __restrict__ ssx,
                                                         const float* __restrict__ wpsi, float* __restrict__ q, double* __restrict__ part,
                                                         int act, float slope, size_t M, int C) {
  constexpr int VW = 16 / sizeof(T);
  __shared__ float red[AG_K * 256];
  __shared__ double dred[256];
  const int cv = C / VW, c0 = ((int)threadIdx.x % cv) * VW;
  float scg[VW], scx[VW], sh[VW], w[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    scg[j] = ssg[(c0 + j) * 2];
    scx[j] = ssx[(c0 + j) * 2];
    sh[j] = ssg[(c0 + j) * 2 + 1] + ssx[(c0 + j) * 2 + 1];
    w[j] = wpsi[c0 + j];
  }
  double s1 = 0.0, s2 = 0.0;
  ag_voxel_sums(M, cv, red,
                [&](size_t vox) {
                  float a[VW], b[VW];
                  Vec<T, VW>::load(g1 + vox * gpitch + c0, a);
                  Vec<T, VW>::load(x1 + vox * xpitch + c0, b);
                  float d = 0.f;
#pragma unroll
                  for (int j = 0; j < VW; ++j) d += w[j] * act_fwd<HEAVY>(a[j] * scg[j] + b[j] * scx[j] + sh[j], act, slope);
                  return d;
                },
                [&](size_t vox, float s) {
                  q[vox] = s;
                  s1 += (double)s;
                  s2 += (double)s * (double)s;
                });
  if (part) {
    const double r1 = ag_block_sum(s1, dred), r2 = ag_block_sum(s2, dred);
    if (threadIdx.x == 0) {
      part[2 * (size_t)blockIdx.x] = r1;
      part[2 * (size_t)blockIdx.x + 1] = r2;
    }
  }
}

// ---- BN_1's finaliser: one workgroup adds the partials in a fixed order and writes st1
__global__ void __launch_bounds__(256) ag_bn1_kernel(const double* __restrict__ part, int nb, double count, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ bpsi,
                                                     const float* __restrict__ rmean, const float* __restrict__ rvar, float eps,
                                                     float* __restrict__ st1) {
  __shared__ double dred[256];
  double s1 = 0.0, s2 = 0.0;
  if (!rmean) {
    for (int i = threadIdx.x; i < nb; i += 256) {
      s1 += part[2 * (size_t)i];
      s2 += part[2 * (size_t)i + 1];
    }
    s1 = ag_block_sum(s1, dred);
    s2 = ag_block_sum(s2, dred);
  }
  if (threadIdx.x == 0) {
    double mean, var, sub;
    if (rmean) {
      mean = rmean[0];
      var = rvar[0];
      sub = mean - (double)bpsi[0];
    } else {
      sub = s1 / count;
      var = s2 / count - sub * sub;
      var = var > 0.0 ? var : 0.0;
      mean = sub + (double)bpsi[0];
    }
    const double rstd = 1.0 / sqrt(var + (double)eps);
    const double a = (double)gamma[0] * rstd;
    st1[0] = (float)mean;
    st1[1] = (float)var;
    st1[2] = (float)rstd;
    st1[3] = (float)sub;
    st1[4] = (float)a;
    st1[5] = (float)((double)beta[0] - sub * a);
    st1[6] = 0.f;
    st1[7] = 0.f;
  }
}

// the gate term of one voxel's channel vector: v <- v alpha (+ r), alpha = sigmoid(a q + b).  ONE statement of it: the apply
// passes and the fused dx + un-pooling pass below form the same bits
template <int VW, bool ADD>
DEVI void ag_gate_term(float a, float b, float qv, float* v, const float* r) {
  const float al = ag_sigm(a * qv + b);
#pragma unroll
  for (int j = 0; j < VW; ++j) v[j] = ADD ? v[j] * al + r[j] : v[j] * al;
}

// ---- out = x sigmoid(a q + b) / dx = dout sigmoid(a q + b) + t: a thread owns one 16-byte channel vector and walks voxels
template <typename T, bool ADD>
__global__ void __launch_bounds__(256) ag_apply_kernel(const T* __restrict__ x, int xpitch, const T* __restrict__ add, int addpitch,
                                                       const float* __restrict__ q, const float* __restrict__ st1, T* __restrict__ out,
                                                       int opitch, size_t M, int C) {
  constexpr int VW = 16 / sizeof(T);
  const int cv = C / VW, vl = 256 / cv;
  const int mycv = threadIdx.x % cv, myvl = threadIdx.x / cv, c0 = mycv * VW;
  if (myvl >= vl) return;
  const float a = st1[4], b = st1[5];
  auto one = [&](size_t vox, float* v, const float* r) { ag_gate_term<VW, ADD>(a, b, q[vox], v, r); };
  const size_t stride = (size_t)gridDim.x * vl;
  size_t vox = (size_t)blockIdx.x * vl + myvl;
  for (; vox + stride < M; vox += 2 * stride) {
    float v0[VW], v1[VW], r0[VW], r1[VW];
    Vec<T, VW>::load(x + vox * xpitch + c0, v0);
    Vec<T, VW>::load(x + (vox + stride) * xpitch + c0, v1);
    if constexpr (ADD) {
      Vec<T, VW>::load(add + vox * addpitch + c0, r0);
      Vec<T, VW>::load(add + (vox + stride) * addpitch + c0, r1);
    }
    one(vox, v0, r0);
    one(vox + stride, v1, r1);
    Vec<T, VW>::store(out + vox * opitch + c0, v0);
    Vec<T, VW>::store(out + (vox + stride) * opitch + c0, v1);
  }
  if (vox < M) {
    float v0[VW], r0[VW];
    Vec<T, VW>::load(x + vox * xpitch + c0, v0);
    if constexpr (ADD) Vec<T, VW>::load(add + vox * addpitch + c0, r0);
    one(vox, v0, r0);
    Vec<T, VW>::store(out + vox * opitch + c0, v0);
  }
}

// ---- the gate's dx and the un-pooling of the level it belongs to in one pass (R2AttUnet's skip gradients):
//   out = ([k == argmax] d_pooled) + round_T(dout sigmoid(a q + b) + t)
// what brats_maxpool2_bwd_idx(argmax, d_pooled, dx_skip = the output of brats_attgate_dx) writes, without the dx tensor in
// between.  The walk is maxpool2_bwd_idx_kernel's (pool_up.hip): grid.y = sample, a thread owns one x position x one 16-byte
// channel vector and the 2 x 2 (z, y) voxels above it; q is indexed by the batch-wide voxel n voxels + vox.  The gate term is
// ag_gate_term's, rounded to the storage type before the sum, and the sum is written as that kernel writes it ((0 + sel) +
// skip): the two passes' bits.
template <typename T>
__global__ void __launch_bounds__(256) ag_dx_unpool_kernel(const T* __restrict__ dout, int dopitch, const T* __restrict__ t, int tpitch,
                                                           const float* __restrict__ q, const float* __restrict__ st1,
                                                           const uint8_t* __restrict__ argmax, const T* __restrict__ dy, int dypitch,
                                                           T* __restrict__ out, int opitch, int C, int D, int H, int W) {
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
  const float a = st1[4], b = st1[5];
  const T* db = dout + (size_t)n * voxels * dopitch + c0;
  const T* tb = t + (size_t)n * voxels * tpitch + c0;
  const float* qb = q + (size_t)n * voxels;
  const T* dyb = dy + (size_t)n * pvoxels * dypitch + c0;
  T* ob = out + (size_t)n * voxels * opitch + c0;
  const uint8_t* ab = argmax + (size_t)n * pvoxels * C + c0;
  for (size_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int seg = (int)(item % segs);
    const size_t rp = item / segs;
    const int yo = (int)(rp % Ho), zo = (int)(rp / Ho);
    const int x = seg * xb + myvl;
    if (x >= W) continue;
    const size_t pvox = ((size_t)zo * Ho + yo) * Wo + (x >> 1);
    float sk[4][VW], r[4][VW], qv[4];
    size_t vox[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      vox[k] = ((size_t)(2 * zo + (k >> 1)) * H + (2 * yo + (k & 1))) * W + x;
      Vec<T, VW>::load(db + vox[k] * dopitch, sk[k]);
      Vec<T, VW>::load(tb + vox[k] * tpitch, r[k]);
      qv[k] = qb[vox[k]];
    }
    uint32_t aw[VW / 4];
#pragma unroll
    for (int i = 0; i < VW / 4; ++i) aw[i] = ((const uint32_t*)(ab + pvox * C))[i];
    float g[VW];
    Vec<T, VW>::load(dyb + pvox * dypitch, g);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int kk = 2 * k + (x & 1);  // the voxel's index in the window, d, h, w order
      ag_gate_term<VW, true>(a, b, qv[k], sk[k], r[k]);
      float o[VW];
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        const int am = (aw[j >> 2] >> (8 * (j & 3))) & 0xff;
        o[j] = 0.f + (am == kk ? g[j] : 0.f);
        o[j] += to_f<T>(from_f<T>(sk[k][j]));
      }
      Vec<T, VW>::store(ob + vox[k] * opitch, o);
    }
  }
}

// ---- backward of the apply pass: dqn = (sum_c dout x) alpha (1 - alpha), the plane and per-workgroup (sum dqn, sum dqn qhat)
template <typename T>
__global__ void __launch_bounds__(256) ag_apply_bwd_kernel(const T* __restrict__ dout, int dopitch, const T* __restrict__ x, int xpitch,
                                                           const float* __restrict__ q, const float* __restrict__ st1,
                                                           float* __restrict__ dqn, double* __restrict__ part, size_t M, int C) {
  constexpr int VW = 16 / sizeof(T);
  __shared__ float red[AG_K * 256];
  __shared__ double dred[256];
  const int cv = C / VW, c0 = ((int)threadIdx.x % cv) * VW;
  const float rstd = st1[2], sub = st1[3], a = st1[4], b = st1[5];
  double s1 = 0.0, s2 = 0.0;
  ag_voxel_sums(M, cv, red,
                [&](size_t vox) {
                  float u[VW], v[VW];
                  Vec<T, VW>::load(dout + vox * dopitch + c0, u);
                  Vec<T, VW>::load(x + vox * xpitch + c0, v);
                  float d = 0.f;
#pragma unroll
                  for (int j = 0; j < VW; ++j) d += u[j] * v[j];
                  return d;
                },
                [&](size_t vox, float s) {
                  const float qv = q[vox];
                  const float al = ag_sigm(a * qv + b);
                  const float d = s * al * (1.f - al);
                  dqn[vox] = d;
                  s1 += (double)d;
                  s2 += (double)d * (double)((qv - sub) * rstd);
                });
  const double r1 = ag_block_sum(s1, dred), r2 = ag_block_sum(s2, dred);
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = r1;
    part[2 * (size_t)blockIdx.x + 1] = r2;
  }
}

__global__ void __launch_bounds__(256) ag_bn1_bwd_kernel(const double* __restrict__ part, int nb, double count, int training,
                                                         float* __restrict__ bw1) {
  __shared__ double dred[256];
  double s1 = 0.0, s2 = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) {
    s1 += part[2 * (size_t)i];
    s2 += part[2 * (size_t)i + 1];
  }
  s1 = ag_block_sum(s1, dred);
  s2 = ag_block_sum(s2, dred);
  if (threadIdx.x == 0) {
    bw1[0] = (float)s2;
    bw1[1] = (float)s1;
    bw1[2] = training ? (float)(s1 / count) : 0.f;
    bw1[3] = training ? (float)(s2 / count) : 0.f;
  }
}

// ---- backward between the plane and the two raw convolution outputs.  Both passes recompute s, p and act'(s) from g1raw / x1raw
// and form dq = BN_1's backward of dqn and ds = w_psi dq act'(s).
template <int VW> struct AgTables {
  float scg[VW], scx[VW], sh[VW], w[VW], mg[VW], rg[VW], mx[VW], rx[VW];
  float a1, sub, rstd1, m1, m2;
  DEVI void load(const float* ssg, const float* ssx, const float* mrg, const float* mrx, const float* wpsi, const float* st1,
                 const float* bw1, int c0) {
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      scg[j] = ssg[(c0 + j) * 2];
      scx[j] = ssx[(c0 + j) * 2];
      sh[j] = ssg[(c0 + j) * 2 + 1] + ssx[(c0 + j) * 2 + 1];
      w[j] = wpsi[c0 + j];
      mg[j] = mrg[(c0 + j) * 2];
      rg[j] = mrg[(c0 + j) * 2 + 1];
      mx[j] = mrx[(c0 + j) * 2];
      rx[j] = mrx[(c0 + j) * 2 + 1];
    }
    rstd1 = st1[2], sub = st1[3], a1 = st1[4], m1 = bw1[2], m2 = bw1[3];
  }
  DEVI float dq(float qv, float dqnv) const { return a1 * (dqnv - m1 - (qv - sub) * rstd1 * m2); }
};

template <typename T, bool HEAVY>
__global__ void __launch_bounds__(256) ag_psi_bwd_stats_kernel(const T* __restrict__ g1, int gpitch, const T* __restrict__ x1, int xpitch,
                                                               const float* __restrict__ q, const float* __restrict__ dqn,
                                                               const float* __restrict__ ssg, const float* __restrict__ ssx,
                                                               const float* __restrict__ mrg, const float* __restrict__ mrx,
                                                               const float* __restrict__ wpsi, const float* __restrict__ st1,
                                                               const float* __restrict__ bw1, float* __restrict__ part, int act,
                                                               float slope, size_t M, int C) {
  constexpr int VW = 16 / sizeof(T);
  __shared__ float red[256 * VW];
  const int cv = C / VW, vl = 256 / cv;
  const int mycv = threadIdx.x % cv, myvl = threadIdx.x / cv, c0 = mycv * VW;
  const bool live = myvl < vl;
  AgTables<VW> tb;
  tb.load(ssg, ssx, mrg, mrx, wpsi, st1, bw1, c0);
  float acc[4][VW], accq = 0.f;
#pragma unroll
  for (int j = 0; j < VW; ++j) acc[0][j] = acc[1][j] = acc[2][j] = acc[3][j] = 0.f;
  auto body = [&](const float* a, const float* b, float qv, float dqnv) {
    const float dq = tb.dq(qv, dqnv);
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const float s = a[j] * tb.scg[j] + b[j] * tb.scx[j] + tb.sh[j];
      const float ds = tb.w[j] * dq * act_grad<HEAVY>(s, act, slope);
      acc[0][j] += ds;
      acc[1][j] += ds * ((a[j] - tb.mg[j]) * tb.rg[j]);
      acc[2][j] += ds * ((b[j] - tb.mx[j]) * tb.rx[j]);
      acc[3][j] += dq * act_fwd<HEAVY>(s, act, slope);
    }
    if (mycv == 0) accq += dq;
  };
  // two voxels (four vector loads) in flight per lane
  const size_t stride = (size_t)gridDim.x * vl;
  size_t vox = live ? (size_t)blockIdx.x * vl + myvl : M;
  for (; vox + stride < M; vox += 2 * stride) {
    float a0[VW], b0[VW], a1[VW], b1[VW];
    Vec<T, VW>::load(g1 + vox * gpitch + c0, a0);
    Vec<T, VW>::load(x1 + vox * xpitch + c0, b0);
    Vec<T, VW>::load(g1 + (vox + stride) * gpitch + c0, a1);
    Vec<T, VW>::load(x1 + (vox + stride) * xpitch + c0, b1);
    const float q0 = q[vox], d0 = dqn[vox], q1 = q[vox + stride], d1 = dqn[vox + stride];
    body(a0, b0, q0, d0);
    body(a1, b1, q1, d1);
  }
  if (vox < M) {
    float a0[VW], b0[VW];
    Vec<T, VW>::load(g1 + vox * gpitch + c0, a0);
    Vec<T, VW>::load(x1 + vox * xpitch + c0, b0);
    body(a0, b0, q[vox], dqn[vox]);
  }
  // the voxel lanes are added in lane order, in f64
  float* row = part + (size_t)blockIdx.x * (4 * C + 4);
  for (int k = 0; k < 4; ++k) {
    if (live) {
#pragma unroll
      for (int j = 0; j < VW; ++j) red[myvl * C + c0 + j] = acc[k][j];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
      double s = 0.0;
      for (int l = 0; l < vl; ++l) s += (double)red[l * C + c];
      row[k * C + c] = (float)s;
    }
    __syncthreads();
  }
  if (live && mycv == 0) red[myvl] = accq;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int l = 0; l < vl; ++l) s += (double)red[l];
    row[4 * C] = (float)s;
  }
}

// sums[i] = the partials of entry i added over the workgroups in order (f64); coef = the three means BN_g / BN_x's backward takes
__global__ void __launch_bounds__(256) ag_psi_bwd_finalize_kernel(const float* __restrict__ part, int nb, int C, double count, int training,
                                                                  float* __restrict__ sums, float* __restrict__ coef) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > 4 * C) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += (double)part[(size_t)b * (4 * C + 4) + i];
  sums[i] = (float)s;
  if (i < 3 * C) coef[i] = training ? (float)(s / count) : 0.f;
}

template <typename T, bool HEAVY>
__global__ void __launch_bounds__(256) ag_psi_bwd_apply_kernel(const T* __restrict__ g1, int gpitch, const T* __restrict__ x1, int xpitch,
                                                               const float* __restrict__ q, const float* __restrict__ dqn,
                                                               const float* __restrict__ ssg, const float* __restrict__ ssx,
                                                               const float* __restrict__ mrg, const float* __restrict__ mrx,
                                                               const float* __restrict__ wpsi, const float* __restrict__ st1,
                                                               const float* __restrict__ bw1, const float* __restrict__ coef,
                                                               T* __restrict__ dg1, int dgpitch, T* __restrict__ dx1, int dxpitch, int act,
                                                               float slope, size_t M, int C) {
  constexpr int VW = 16 / sizeof(T);
  const int cv = C / VW, vl = 256 / cv;
  const int mycv = threadIdx.x % cv, myvl = threadIdx.x / cv, c0 = mycv * VW;
  if (myvl >= vl) return;
  AgTables<VW> tb;
  tb.load(ssg, ssx, mrg, mrx, wpsi, st1, bw1, c0);
  float k1[VW], kg[VW], kx[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    k1[j] = coef[c0 + j];
    kg[j] = coef[C + c0 + j];
    kx[j] = coef[2 * C + c0 + j];
  }
  const size_t stride = (size_t)gridDim.x * vl;
  for (size_t vox = (size_t)blockIdx.x * vl + myvl; vox < M; vox += stride) {
    float a[VW], b[VW];
    Vec<T, VW>::load(g1 + vox * gpitch + c0, a);
    Vec<T, VW>::load(x1 + vox * xpitch + c0, b);
    const float dq = tb.dq(q[vox], dqn[vox]);
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const float s = a[j] * tb.scg[j] + b[j] * tb.scx[j] + tb.sh[j];
      const float ds = tb.w[j] * dq * act_grad<HEAVY>(s, act, slope);
      a[j] = tb.scg[j] * (ds - k1[j] - (a[j] - tb.mg[j]) * tb.rg[j] * kg[j]);
      b[j] = tb.scx[j] * (ds - k1[j] - (b[j] - tb.mx[j]) * tb.rx[j] * kx[j]);
    }
    Vec<T, VW>::store(dg1 + vox * dgpitch + c0, a);
    Vec<T, VW>::store(dx1 + vox * dxpitch + c0, b);
  }
}

// ---- argument checks shared by the entry points: 0, or the error code with `name` in the message
int ag_check(const char* name, bool null, int dtype, int N, int voxels, int C, const int* pitches, int npitch) {
  if (null) BRATS_FAIL(BRATS_E_ARG, "%s: null pointer", name);
  if (dtype != BRATS_F32 && dtype != BRATS_BF16) BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: dtype %d (f32, bf16 or fp16 storage)", name, dtype);
  const int vw = vec_width(dtype);
  if (N <= 0 || voxels <= 0 || C <= 0 || C % vw) BRATS_FAIL(BRATS_E_ARG, "%s: N, voxels > 0 and C a multiple of %d (got %d, %d, %d)", name, vw, N, voxels, C);
  for (int i = 0; i < npitch; ++i)
    if (pitches[i] % vw || pitches[i] < C) BRATS_FAIL(BRATS_E_ARG, "%s: every pitch must be a multiple of %d and at least C = %d (got %d)", name, vw, C, pitches[i]);
  if (C / vw > 256) BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: C = %d is beyond %d channels", name, C, 256 * vw);
  return 0;
}
int ag_check_act(const char* name, int act) {
  if (act < BRATS_ACT_NONE || act > BRATS_ACT_MISH) BRATS_FAIL(BRATS_E_ARG, "%s: unknown activation %d", name, act);
  return 0;
}

}  // namespace

extern "C" int BRATS_API(brats_attgate_blocks)(int dtype, int C, int N, int voxels) {
  if (int rc = ag_check("attgate_blocks", false, dtype, N, voxels, C, nullptr, 0)) return rc;
  return ag_blocks(vec_width(dtype), C, (size_t)N * voxels);
}

extern "C" int BRATS_API(brats_attgate_psi_fwd)(const void* g1raw, int gpitch, const void* x1raw, int xpitch, const float* ss_g,
                                                const float* ss_x, const float* w_psi, float* q, double* part, int dtype, int act,
                                                float slope, int N, int voxels, int C, brats_stream_t s) {
  const int pitches[2] = {gpitch, xpitch};
  if (int rc = ag_check("attgate_psi_fwd", !g1raw || !x1raw || !ss_g || !ss_x || !w_psi || !q, dtype, N, voxels, C, pitches, 2)) return rc;
  if (int rc = ag_check_act("attgate_psi_fwd", act)) return rc;
  const size_t M = (size_t)N * voxels;
  const int nb = ag_blocks(vec_width(dtype), C, M);
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    with_flag(act > BRATS_ACT_LEAKY, [&](auto heavy) {
      hipLaunchKernelGGL((ag_psi_fwd_kernel<T, decltype(heavy)::value>), dim3(nb), dim3(256), 0, (hipStream_t)s, (const T*)g1raw, gpitch,
                         (const T*)x1raw, xpitch, ss_g, ss_x, w_psi, q, part, act, slope, M, C);
    });
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int BRATS_API(brats_attgate_bn1)(const double* part, int nb, double count, const float* gamma, const float* beta,
                                            const float* b_psi, const float* running_mean, const float* running_var, float eps,
                                            float* st1, brats_stream_t s) {
  const bool eval = running_mean != nullptr;
  if (!gamma || !beta || !b_psi || !st1 || (eval != (running_var != nullptr)) || (!eval && !part))
    BRATS_FAIL(BRATS_E_ARG, "attgate_bn1: null pointer (running_mean and running_var come together; part is needed without them)");
  if ((!eval && (nb <= 0 || nb > AG_MAX_BLOCKS)) || !(count >= 1.0)) BRATS_FAIL(BRATS_E_ARG, "attgate_bn1: nb = %d, count = %g", nb, count);
  hipLaunchKernelGGL(ag_bn1_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, part, nb, count, gamma, beta, b_psi, running_mean, running_var,
                     eps, st1);
  BRATS_CHECK_LAUNCH();
  return 0;
}

static int ag_apply_launch(const char* name, const void* x, int xpitch, const void* add, int addpitch, const float* q, const float* st1,
                           void* out, int opitch, int dtype, int N, int voxels, int C, hipStream_t st) {
  const size_t M = (size_t)N * voxels;
  const int vw = vec_width(dtype), vl = 256 / (C / vw);
  const int grid = stream_grid(M, vl * 8, 4096);
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    with_flag(add != nullptr, [&](auto ad) {
      hipLaunchKernelGGL((ag_apply_kernel<T, decltype(ad)::value>), dim3(grid), dim3(256), 0, st, (const T*)x, xpitch, (const T*)add,
                         addpitch, q, st1, (T*)out, opitch, M, C);
    });
  });
  (void)name;
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int BRATS_API(brats_attgate_apply_fwd)(const void* x, int xpitch, const float* q, const float* st1, void* out, int opitch,
                                                  int dtype, int N, int voxels, int C, brats_stream_t s) {
  const int pitches[2] = {xpitch, opitch};
  if (int rc = ag_check("attgate_apply_fwd", !x || !q || !st1 || !out, dtype, N, voxels, C, pitches, 2)) return rc;
  return ag_apply_launch("attgate_apply_fwd", x, xpitch, nullptr, 0, q, st1, out, opitch, dtype, N, voxels, C, (hipStream_t)s);
}

extern "C" int BRATS_API(brats_attgate_dx)(const void* dout, int dopitch, const void* t, int tpitch, const float* q, const float* st1,
                                           void* dx, int dxpitch, int dtype, int N, int voxels, int C, brats_stream_t s) {
  const int pitches[3] = {dopitch, tpitch, dxpitch};
  if (int rc = ag_check("attgate_dx", !dout || !t || !q || !st1 || !dx, dtype, N, voxels, C, pitches, 3)) return rc;
  return ag_apply_launch("attgate_dx", dout, dopitch, t, tpitch, q, st1, dx, dxpitch, dtype, N, voxels, C, (hipStream_t)s);
}

extern "C" int BRATS_API(brats_attgate_dx_unpool)(const void* dout, int dopitch, const void* t, int tpitch, const float* q,
                                                  const float* st1, const unsigned char* argmax, const void* d_pooled, int dppitch,
                                                  void* out, int opitch, int dtype, int N, int C, int D, int H, int W,
                                                  brats_stream_t s) {
  const char* name = "attgate_dx_unpool";
  if (D <= 0 || H <= 0 || W <= 0 || ((D | H | W) & 1) || (size_t)D * H * W > (size_t)0x7fffffff)
    BRATS_FAIL(BRATS_E_ARG, "%s: D, H, W must be positive and even, D * H * W below 2^31 (got %d, %d, %d)", name, D, H, W);
  if (N > 65535) BRATS_FAIL(BRATS_E_ARG, "%s: N = %d is beyond 65535 samples", name, N);
  const int pitches[4] = {dopitch, tpitch, dppitch, opitch};
  if (int rc = ag_check(name, !dout || !t || !q || !st1 || !argmax || !d_pooled || !out, dtype, N, D * H * W, C, pitches, 4)) return rc;
  const int vw = vec_width(dtype);
  int xb = 256 / (C / vw);
  if (xb > W) xb = W;
  const size_t items = (size_t)(D / 2) * (H / 2) * ((W + xb - 1) / xb);
  dim3 grid(stream_grid(items, 1, 8192), N);
  with_storage(dtype, [&](auto st) {
    using T = typename decltype(st)::type;
    hipLaunchKernelGGL(ag_dx_unpool_kernel<T>, grid, dim3(256), 0, (hipStream_t)s, (const T*)dout, dopitch, (const T*)t, tpitch, q, st1,
                       argmax, (const T*)d_pooled, dppitch, (T*)out, opitch, C, D, H, W);
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int BRATS_API(brats_attgate_apply_bwd)(const void* dout, int dopitch, const void* x, int xpitch, const float* q,
                                                  const float* st1, float* dqn, double* part, int dtype, int N, int voxels, int C,
                                                  brats_stream_t s) {
  const int pitches[2] = {dopitch, xpitch};
  if (int rc = ag_check("attgate_apply_bwd", !dout || !x || !q || !st1 || !dqn || !part, dtype, N, voxels, C, pitches, 2)) return rc;
  const size_t M = (size_t)N * voxels;
  const int nb = ag_blocks(vec_width(dtype), C, M);
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((ag_apply_bwd_kernel<T>), dim3(nb), dim3(256), 0, (hipStream_t)s, (const T*)dout, dopitch, (const T*)x, xpitch, q, st1,
                       dqn, part, M, C);
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int BRATS_API(brats_attgate_bn1_bwd)(const double* part, int nb, double count, int training, float* bw1, brats_stream_t s) {
  if (!part || !bw1) BRATS_FAIL(BRATS_E_ARG, "attgate_bn1_bwd: null pointer");
  if (nb <= 0 || nb > AG_MAX_BLOCKS || !(count >= 1.0)) BRATS_FAIL(BRATS_E_ARG, "attgate_bn1_bwd: nb = %d, count = %g", nb, count);
  hipLaunchKernelGGL(ag_bn1_bwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, part, nb, count, training, bw1);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int BRATS_API(brats_attgate_psi_bwd_stats)(const void* g1raw, int gpitch, const void* x1raw, int xpitch, const float* q,
                                                      const float* dqn, const float* ss_g, const float* ss_x, const float* mr_g,
                                                      const float* mr_x, const float* w_psi, const float* st1, const float* bw1,
                                                      float* part, int dtype, int act, float slope, int N, int voxels, int C,
                                                      brats_stream_t s) {
  const int pitches[2] = {gpitch, xpitch};
  if (int rc = ag_check("attgate_psi_bwd_stats", !g1raw || !x1raw || !q || !dqn || !ss_g || !ss_x || !mr_g || !mr_x || !w_psi || !st1 ||
                        !bw1 || !part, dtype, N, voxels, C, pitches, 2)) return rc;
  if (int rc = ag_check_act("attgate_psi_bwd_stats", act)) return rc;
  const size_t M = (size_t)N * voxels;
  const int nb = ag_blocks(vec_width(dtype), C, M);
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    with_flag(act > BRATS_ACT_LEAKY, [&](auto heavy) {
      hipLaunchKernelGGL((ag_psi_bwd_stats_kernel<T, decltype(heavy)::value>), dim3(nb), dim3(256), 0, (hipStream_t)s, (const T*)g1raw, gpitch,
                         (const T*)x1raw, xpitch, q, dqn, ss_g, ss_x, mr_g, mr_x, w_psi, st1, bw1, part, act, slope, M, C);
    });
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int BRATS_API(brats_attgate_psi_bwd_finalize)(const float* part, int nb, int C, double count, int training, float* sums,
                                                         float* coef, brats_stream_t s) {
  if (!part || !sums || !coef) BRATS_FAIL(BRATS_E_ARG, "attgate_psi_bwd_finalize: null pointer");
  if (nb <= 0 || nb > AG_MAX_BLOCKS || C <= 0 || C > 2048 || !(count >= 1.0))
    BRATS_FAIL(BRATS_E_ARG, "attgate_psi_bwd_finalize: nb = %d, C = %d, count = %g", nb, C, count);
  hipLaunchKernelGGL(ag_psi_bwd_finalize_kernel, dim3(ceil_div(4 * C + 1, 256)), dim3(256), 0, (hipStream_t)s, part, nb, C, count, training,
                     sums, coef);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int BRATS_API(brats_attgate_psi_bwd_apply)(const void* g1raw, int gpitch, const void* x1raw, int xpitch, const float* q,
                                                      const float* dqn, const float* ss_g, const float* ss_x, const float* mr_g,
                                                      const float* mr_x, const float* w_psi, const float* st1, const float* bw1,
                                                      const float* coef, void* dg1raw, int dgpitch, void* dx1raw, int dxpitch, int dtype,
                                                      int act, float slope, int N, int voxels, int C, brats_stream_t s) {
  const int pitches[4] = {gpitch, xpitch, dgpitch, dxpitch};
  if (int rc = ag_check("attgate_psi_bwd_apply", !g1raw || !x1raw || !q || !dqn || !ss_g || !ss_x || !mr_g || !mr_x || !w_psi || !st1 ||
                        !bw1 || !coef || !dg1raw || !dx1raw, dtype, N, voxels, C, pitches, 4)) return rc;
  if (int rc = ag_check_act("attgate_psi_bwd_apply", act)) return rc;
  const size_t M = (size_t)N * voxels;
  const int vw = vec_width(dtype), vl = 256 / (C / vw);
  const int grid = stream_grid(M, vl * 8, 4096);
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    with_flag(act > BRATS_ACT_LEAKY, [&](auto heavy) {
      hipLaunchKernelGGL((ag_psi_bwd_apply_kernel<T, decltype(heavy)::value>), dim3(grid), dim3(256), 0, (hipStream_t)s, (const T*)g1raw, gpitch,
                         (const T*)x1raw, xpitch, q, dqn, ss_g, ss_x, mr_g, mr_x, w_psi, st1, bw1, coef, (T*)dg1raw, dgpitch, (T*)dx1raw,
                         dxpitch, act, slope, M, C);
    });
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}
#include "twin_end.hpp"
