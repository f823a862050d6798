// CBAM attention block of AttEquiUnet (networks/equiunet2020.py:147-235 of the reference: ChannelGate + SpatialGate with
// InstanceNorm3d(1)) on NDHWC tensors of f32 or bf16 storage.  Element arithmetic is f32; the small MLP kernels, the
// forward stencil and the backward sums that feed cancelling combinations accumulate in f64 (mlp_hidden, stencil7, lanes_to_partial).
//   s[n][c]  = sigmoid(mlp(mean_v x) + mlp(max_v x)),  mlp(u) = W2 relu(W1 u + b1) + b2
//   comp     = [max_c x s | mean_c x s]                 (two f32 planes per sample)
//   z        = conv7x7x7(comp), zero padding, no bias   (one f32 plane)
//   g        = sigmoid(relu(gamma (z - mu_n) rstd_n + beta))
//   out      = x s g
// Passes over the x-sized tensors: forward pool (read x), compress (read x), apply (read x, write out); backward reduce (read
// dout, x), chan (read x), apply (read dout, write dx).  x s and g are never stored at x size.
// In front of a 2x2x2 max pool (the pooled encoder levels of AttEquiUnet) three passes take the pooling in: apply_pool also writes
// maxpool2(out) and its window-index bytes; bwd_reduce_pool / bwd_apply_pool compose dout = d_skip + maxpool2_bwd(d_pooled) on load
// and never store it -- bit-identical to the composition with brats_maxpool2_fwd / brats_maxpool2_bwd_idx (pool_up.hip).
// Every reduction that crosses a workgroup goes through per-workgroup partials that are added in a fixed order (or, for the
// arg-max, combined under a total order): no floating-point atomics, the same bits at every run.  Ties: the gradient of the
// per-channel maximum over voxels goes to the lowest voxel index, that of the per-voxel maximum over channels to the lowest
// channel (torch's max_pool3d / torch.max on the CPU).
#include "common.hpp"
#include <limits.h>
#include <math.h>

namespace {

constexpr int CBAM_MAX_BLOCKS = 1024;  // workgroups per sample of the streaming reductions
// the 7x7x7 stencil: a 4 x 8 x 32 output tile per workgroup, staged with its 3-voxel halo
constexpr int TD = 4, TH = 8, TW = 32, HD = TD + 6, HH = TH + 6, HW = TW + 6;
constexpr int HPLANE = HH * HW, HTILE = HD * HPLANE, TTILE = TD * TH * TW, TAPS = 343;

// How a streaming pass walks one sample: the voxel walk of common.hpp (256 threads = cv 16-byte channel vectors x vl voxel lanes,
// threads beyond cv * vl idle) on nb workgroups, workgroup b owning the voxels [b * chunk, (b + 1) * chunk): the partials of the
// reductions are per workgroup, so each owns one contiguous run
struct Split {
  int cv, vl, nb, chunk;
};
Split cbam_split(int dtype, int C, int V) {
  const Walk w = voxel_walk(vec_width(dtype), V, C);
  const int nb = (int)w.grid(CBAM_MAX_BLOCKS);
  return Split{w.cv, w.vl, nb, (V + nb - 1) / nb};
}
int cbam_tiles(int D, int H, int W) { return ceil_div(D, TD) * ceil_div(H, TH) * ceil_div(W, TW); }

DEVI float sigm(float a) { return 1.f / (1.f + expf(-a)); }

// The MLP of the channel gate, one thread per output, accumulated in f64: the backward multiplies the rounding error of s by
// |ds| (hundreds at the network's volumes) on its way into the MLP gradients, so s is formed as exactly as f32 can hold it -- and
// the backward (cbam_bwd_gate_kernel) recomputes it in f64 from the pooled vectors instead of reading the rounded one.
// h[k][j] = relu(b1[j] + W1[j] . pooled[k]) for this workgroup's sample, into LDS
DEVI void mlp_hidden(const float* pn, const float* w1, const float* b1, double (*h)[512], int C, int Ch) {
  for (int j = threadIdx.x; j < Ch; j += 256) {
    for (int k = 0; k < 2; ++k) {
      double a = b1[j];
      for (int c = 0; c < C; ++c) a += (double)w1[(size_t)j * C + c] * (double)pn[k * C + c];
      h[k][j] = a > 0.0 ? a : 0.0;
    }
  }
  __syncthreads();
}
// s[c] = sigmoid(mlp(avg)[c] + mlp(max)[c]) from the hidden vectors
DEVI double mlp_scale(const double (*h)[512], const float* w2, const float* b2, int c, int Ch) {
  double a0 = b2[c], a1 = b2[c];
  for (int j = 0; j < Ch; ++j) {
    a0 += (double)w2[(size_t)c * Ch + j] * h[0][j];
    a1 += (double)w2[(size_t)c * Ch + j] * h[1][j];
  }
  return 1.0 / (1.0 + exp(-(a0 + a1)));
}

// the spatial gate of one voxel from its convolution output; zhat = the normalised value, zn = the affine one
struct Norm1 {
  float mu, rstd, gamma, beta;
};
DEVI Norm1 load_norm(const float* stats, const float* gamma, const float* beta, int n) {
  return Norm1{stats[2 * n], stats[2 * n + 1], gamma[0], beta[0]};
}
DEVI float spatial_gate(float z, const Norm1& p, float& zhat, float& zn) {
  zhat = (z - p.mu) * p.rstd;
  zn = zhat * p.gamma + p.beta;
  return sigm(fmaxf(zn, 0.f));
}

// sum over the 256 threads in a fixed tree; red: 256 doubles of LDS
DEVI double block_sum(double v, double* red) {
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

// The sums of the backward pass that feed cancelling combinations (ds -> the MLP backward, dgamma, dbeta) are accumulated in
// f64 and stored as f32: the bar of tests/test_cbam_gpu.py is a few f32 roundings of the RESULT, which a chain of f32 partial
// sums does not keep.  The vector f64 rate of the chip is far above what these memory-bound passes ask for.
// per-channel sums of a workgroup: the voxel lanes are added in lane order; lds: 256 * VW doubles
template <int VW> DEVI void lanes_to_partial(const double (&a)[VW], double* lds, float* dst, int C, int vl, int cvi, int vlane) {
  if (vlane < vl) {
#pragma unroll
    for (int j = 0; j < VW; ++j) lds[vlane * C + cvi * VW + j] = a[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    double s = 0.0;
    for (int l = 0; l < vl; ++l) s += lds[l * C + c];
    dst[c] = (float)s;
  }
  __syncthreads();
}

// out[i] = sum over nb partial vectors in a fixed order (8 entries x 32 slices per workgroup, as ordered_sum_kernel of dice.hip),
// accumulated in f64
__global__ void __launch_bounds__(256) cbam_sum_partials_kernel(const float* __restrict__ part, float* __restrict__ out, int nb, int total) {
  const int e = threadIdx.x & 7, g = threadIdx.x >> 3, i = blockIdx.x * 8 + e;
  double s = 0.0;
  if (i < total)
    for (int b = g; b < nb; b += 32) s += (double)part[(size_t)b * total + i];
  __shared__ double sm[32][8];
  sm[g][e] = s;
  __syncthreads();
  if (g == 0 && i < total) {
    for (int k = 1; k < 32; ++k) s += sm[k][e];
    out[i] = (float)s;
  }
}
void cbam_sum_partials(const float* part, float* out, int nb, int total, hipStream_t st) {
  hipLaunchKernelGGL(cbam_sum_partials_kernel, dim3((total + 7) / 8), dim3(256), 0, st, part, out, nb, total);
}

// ---- forward: global pooling -------------------------------------------------------------------------------------------------
// partials [nb][N * C]: sum, maximum and the lowest voxel index that holds it
template <typename T>
__global__ void __launch_bounds__(256) cbam_pool_kernel(const T* __restrict__ x, int pitch, float* __restrict__ psum, float* __restrict__ pmax,
                                                        int* __restrict__ pidx, int V, int C, int cv, int vl, int chunk) {
  constexpr int VW = 16 / sizeof(T);
  __shared__ float ls[256 * VW], lm[256 * VW];
  __shared__ int li[256 * VW];
  const int n = blockIdx.y, N = gridDim.y, cvi = threadIdx.x % cv, vlane = threadIdx.x / cv;
  const int v0 = min(V, (int)blockIdx.x * chunk), v1 = min(V, v0 + chunk);
  const T* xn = x + (size_t)n * V * pitch + cvi * VW;
  float sum[VW], mx[VW];
  int ix[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) { sum[j] = 0.f; mx[j] = -INFINITY; ix[j] = INT_MAX; }
  if (vlane < vl) {
    for (int v = v0 + vlane; v < v1; v += vl) {  // increasing v and a strict comparison: the lowest index of equal maxima stays
      float f[VW];
      Vec<T, VW>::load(xn + (size_t)v * pitch, f);
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        sum[j] += f[j];
        if (f[j] > mx[j]) { mx[j] = f[j]; ix[j] = v; }
      }
    }
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const int o = vlane * C + cvi * VW + j;
      ls[o] = sum[j]; lm[o] = mx[j]; li[o] = ix[j];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f, m = -INFINITY;
    int i = INT_MAX;
    for (int l = 0; l < vl; ++l) {
      s += ls[l * C + c];
      const float mv = lm[l * C + c];
      const int iv = li[l * C + c];
      if (mv > m || (mv == m && iv < i)) { m = mv; i = iv; }
    }
    const size_t o = ((size_t)blockIdx.x * N + n) * C + c;
    psum[o] = s; pmax[o] = m; pidx[o] = i;
  }
}

// 8 entries x 32 slices per workgroup (as ordered_sum_kernel, dice.hip): sums in slice order, (maximum, index) pairs under their
// total order
__global__ void __launch_bounds__(256) cbam_pool_finalize_kernel(const float* __restrict__ psum, const float* __restrict__ pmax,
                                                                 const int* __restrict__ pidx, float* __restrict__ pooled /*[N][2][C]*/,
                                                                 int* __restrict__ argvox /*[N][C]*/, int nb, int total, int C, float V) {
  const int e = threadIdx.x & 7, g = threadIdx.x >> 3, i = blockIdx.x * 8 + e;
  float s = 0.f, m = -INFINITY;
  int ix = INT_MAX;
  if (i < total) {
    for (int b = g; b < nb; b += 32) {
      const size_t o = (size_t)b * total + i;
      s += psum[o];
      const float mv = pmax[o];
      const int iv = pidx[o];
      if (mv > m || (mv == m && iv < ix)) { m = mv; ix = iv; }
    }
  }
  __shared__ float ss[32][8], sm[32][8];
  __shared__ int si[32][8];
  ss[g][e] = s; sm[g][e] = m; si[g][e] = ix;
  __syncthreads();
  if (g == 0 && i < total) {
    for (int k = 1; k < 32; ++k) {
      s += ss[k][e];
      if (sm[k][e] > m || (sm[k][e] == m && si[k][e] < ix)) { m = sm[k][e]; ix = si[k][e]; }
    }
    const int n = i / C, c = i % C;
    pooled[((size_t)n * 2 + 0) * C + c] = s / V;
    pooled[((size_t)n * 2 + 1) * C + c] = m;
    argvox[i] = ix;
  }
}

// ---- forward: the shared MLP, one workgroup per sample ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cbam_gate_kernel(const float* __restrict__ pooled, const float* __restrict__ w1, const float* __restrict__ b1,
                                                        const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ hidden /*[N][2][Ch]*/,
                                                        float* __restrict__ scale /*[N][C]*/, int C, int Ch) {
  __shared__ double h[2][512];
  const int n = blockIdx.x;
  mlp_hidden(pooled + (size_t)n * 2 * C, w1, b1, h, C, Ch);
  for (int j = threadIdx.x; j < Ch; j += 256)
    for (int k = 0; k < 2; ++k) hidden[((size_t)n * 2 + k) * Ch + j] = (float)h[k][j];
  for (int c = threadIdx.x; c < C; c += 256) scale[(size_t)n * C + c] = (float)mlp_scale(h, w2, b2, c, Ch);
}

// ---- forward: per-voxel channel maximum and mean of x s ----------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) cbam_compress_kernel(const T* __restrict__ x, int pitch, const float* __restrict__ scale, float* __restrict__ comp,
                                                            uint16_t* __restrict__ cidx, int V, int C, int cv, int vl, int chunk) {
  constexpr int VW = 16 / sizeof(T);
  __shared__ float lm[256], ls[256];
  __shared__ int li[256];
  const int n = blockIdx.y, tid = threadIdx.x, cvi = tid % cv, vlane = tid / cv;
  const bool lane_on = vlane < vl;
  const int v0 = min(V, (int)blockIdx.x * chunk), v1 = min(V, v0 + chunk), iters = (v1 - v0 + vl - 1) / vl;
  const T* xn = x + (size_t)n * V * pitch + cvi * VW;
  float sc[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) sc[j] = lane_on ? scale[(size_t)n * C + cvi * VW + j] : 0.f;
  int p2 = 1;
  while (p2 < cv) p2 <<= 1;
  for (int it = 0; it < iters; ++it) {
    const int v = v0 + it * vl + vlane;
    const bool ok = lane_on && v < v1;
    float m = -INFINITY, s = 0.f;
    int ix = INT_MAX;
    if (ok) {
      float f[VW];
      Vec<T, VW>::load(xn + (size_t)v * pitch, f);
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        const float t = f[j] * sc[j];
        s += t;
        if (t > m) { m = t; ix = cvi * VW + j; }
      }
    }
    lm[tid] = m; ls[tid] = s; li[tid] = ix;
    __syncthreads();
    // the cv partials of a voxel in a fixed tree; equal maxima: the lower channel
    for (int h = p2 >> 1; h > 0; h >>= 1) {
      if (lane_on && cvi < h && cvi + h < cv) {
        const float m2 = lm[tid + h];
        const int i2 = li[tid + h];
        s += ls[tid + h];
        if (m2 > m || (m2 == m && i2 < ix)) { m = m2; ix = i2; }
        lm[tid] = m; ls[tid] = s; li[tid] = ix;
      }
      __syncthreads();
    }
    if (ok && cvi == 0) {
      comp[((size_t)n * 2 + 0) * V + v] = m;
      comp[((size_t)n * 2 + 1) * V + v] = s / (float)C;
      if (cidx) cidx[(size_t)n * V + v] = (uint16_t)ix;
    }
  }
}

// ---- the 7x7x7 stencil on f32 planes -------------------------------------------------------------------------------------------------
struct Tile {
  int d0, h0, w0;
};
DEVI Tile tile_origin(int tile, int H, int W) {
  const int ntw = (W + TW - 1) / TW, nth = (H + TH - 1) / TH;
  return Tile{(tile / (ntw * nth)) * TD, ((tile / ntw) % nth) * TH, (tile % ntw) * TW};
}
// thread (th, tw) owns the TD outputs of its column: acc[po][j] += sum_taps wl[po][pi][tap] * tile[pi][j + kz][th + ky][tw + kx];
// the 49 taps of a (plane, ky) slab are summed on their own first (two short sums instead of one of 686 terms).  A = the
// accumulator type: f64 in the forward pass (z decides every ReLU and carries its rounding into dgamma / dbeta through rstd;
// measured cost at 2 x 128^3: 0.25 -> 0.33 ms), f32 in the backward pass
template <int PI, int PO, typename A> DEVI void stencil7(const float* tile, const A* wl, int th, int tw, A (&total)[PO][TD]) {
  for (int pi = 0; pi < PI; ++pi) {
#pragma unroll 1
    for (int ky = 0; ky < 7; ++ky) {
      A acc[PO][TD] = {};
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const float* col = tile + pi * HTILE + (th + ky) * HW + tw + kx;
        A in[HD];
#pragma unroll
        for (int i = 0; i < HD; ++i) in[i] = (A)col[i * HPLANE];
#pragma unroll
        for (int po = 0; po < PO; ++po) {
#pragma unroll
          for (int kz = 0; kz < 7; ++kz) {
            const A w = wl[(po * PI + pi) * TAPS + kz * 49 + ky * 7 + kx];
#pragma unroll
            for (int j = 0; j < TD; ++j) acc[po][j] += w * in[j + kz];
          }
        }
      }
#pragma unroll
      for (int po = 0; po < PO; ++po)
#pragma unroll
        for (int j = 0; j < TD; ++j) total[po][j] += acc[po][j];
    }
  }
}

// z = conv(comp, wc); per-tile (count, mean, M2) of z for the instance norm
__global__ void __launch_bounds__(256) cbam_spatial_fwd_kernel(const float* __restrict__ comp, const float* __restrict__ wc, float* __restrict__ z,
                                                               float* __restrict__ part /*[N][tiles][3]*/, int D, int H, int W) {
  __shared__ float tile[2 * HTILE];
  __shared__ double wl[2 * TAPS], red[256];
  const int n = blockIdx.y, tid = threadIdx.x;
  const size_t V = (size_t)D * H * W;
  const Tile t = tile_origin(blockIdx.x, H, W);
  for (int i = tid; i < 2 * HTILE; i += 256) {
    const int p = i / HTILE, r = i % HTILE;
    const int gd = t.d0 - 3 + r / HPLANE, gh = t.h0 - 3 + (r / HW) % HH, gw = t.w0 - 3 + r % HW;
    const bool in = gd >= 0 && gd < D && gh >= 0 && gh < H && gw >= 0 && gw < W;
    tile[i] = in ? comp[((size_t)n * 2 + p) * V + ((size_t)gd * H + gh) * W + gw] : 0.f;
  }
  for (int i = tid; i < 2 * TAPS; i += 256) wl[i] = (double)wc[i];
  __syncthreads();
  const int tw = tid % TW, th = tid / TW;
  double acc[1][TD] = {};
  stencil7<2, 1, double>(tile, wl, th, tw, acc);
  const int gh = t.h0 + th, gw = t.w0 + tw;
  // the tile's moments are taken of the STORED (f32) values: what the later passes normalise
  float zs[TD];
  double cnt = 0.0, sum = 0.0;
#pragma unroll
  for (int j = 0; j < TD; ++j) {
    zs[j] = (float)acc[0][j];
    if (t.d0 + j < D && gh < H && gw < W) {
      z[(size_t)n * V + ((size_t)(t.d0 + j) * H + gh) * W + gw] = zs[j];
      cnt += 1.0;
      sum += (double)zs[j];
    }
  }
  const double bc = block_sum(cnt, red), mean = block_sum(sum, red) / bc;  // (every tile holds at least one voxel)
  double m2 = 0.0;
#pragma unroll
  for (int j = 0; j < TD; ++j)
    if (t.d0 + j < D && gh < H && gw < W) m2 += ((double)zs[j] - mean) * ((double)zs[j] - mean);
  m2 = block_sum(m2, red);
  if (tid == 0) {
    float* o = part + ((size_t)n * gridDim.x + blockIdx.x) * 3;
    o[0] = (float)bc; o[1] = (float)mean; o[2] = (float)m2;
  }
}

// (count, mean, M2) merged pairwise (Chan et al.): each thread a run of tiles in order, then a fixed tree
struct Moments {
  double n, mean, m2;
};
DEVI Moments merge(const Moments& a, const Moments& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  const double n = a.n + b.n, d = b.mean - a.mean;
  return Moments{n, a.mean + d * (b.n / n), a.m2 + b.m2 + d * d * (a.n * (b.n / n))};
}
__global__ void __launch_bounds__(256) cbam_norm_finalize_kernel(const float* __restrict__ part, float* __restrict__ stats /*[N][2]*/, int tiles, float eps) {
  __shared__ Moments sm[256];
  const int n = blockIdx.x, tid = threadIdx.x, per = (tiles + 255) / 256;
  Moments a{0.0, 0.0, 0.0};
  for (int i = tid * per; i < min(tiles, (tid + 1) * per); ++i) {
    const float* p = part + ((size_t)n * tiles + i) * 3;
    a = merge(a, Moments{(double)p[0], (double)p[1], (double)p[2]});
  }
  sm[tid] = a;
  __syncthreads();
  // (neighbours first: thread t holds the tiles before thread t + 1's)
  for (int m = 1; m < 256; m <<= 1) {
    if (tid % (2 * m) == 0) sm[tid] = merge(sm[tid], sm[tid + m]);
    __syncthreads();
  }
  if (tid == 0) {
    stats[2 * n] = (float)sm[0].mean;
    stats[2 * n + 1] = (float)(1.0 / sqrt(sm[0].m2 / sm[0].n + (double)eps));  // biased variance
  }
}

// ---- forward: out = x s g ----------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) cbam_apply_kernel(const T* __restrict__ x, int pitch, const float* __restrict__ scale, const float* __restrict__ z,
                                                         const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         T* __restrict__ out, int opitch, int V, int C, int cv, int vl, int chunk) {
  constexpr int VW = 16 / sizeof(T);
  const int n = blockIdx.y, cvi = threadIdx.x % cv, vlane = threadIdx.x / cv;
  if (vlane >= vl) return;
  const int v0 = min(V, (int)blockIdx.x * chunk), v1 = min(V, v0 + chunk);
  const Norm1 nm = load_norm(stats, gamma, beta, n);
  float sc[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) sc[j] = scale[(size_t)n * C + cvi * VW + j];
  const T* xn = x + (size_t)n * V * pitch + cvi * VW;
  T* on = out + (size_t)n * V * opitch + cvi * VW;
  const float* zn_ = z + (size_t)n * V;
#pragma unroll 4
  for (int v = v0 + vlane; v < v1; v += vl) {
    float f[VW], zhat, zn;
    Vec<T, VW>::load(xn + (size_t)v * pitch, f);
    const float g = spatial_gate(zn_[v], nm, zhat, zn);
#pragma unroll
    for (int j = 0; j < VW; ++j) f[j] = f[j] * sc[j] * g;
    Vec<T, VW>::store(on + (size_t)v * opitch, f);
  }
}

// ---- the gate in front of a 2x2x2 max pool (the encoder levels of AttEquiUnet) ------------------------------------------------------
// a value as the storage type holds it
template <typename T, int VW> DEVI void round_to_storage(float (&f)[VW]) {
  if constexpr (std::is_same<T, bf16_t>::value) {
#pragma unroll
    for (int j = 0; j < VW; j += 2) unpack2(pack2(f[j], f[j + 1]), f[j], f[j + 1]);
  }
}

// forward: the apply pass that also writes maxpool2(out).  A thread owns one x position of one channel vector and the 2 x 2 (z, y)
// voxels above it, as in maxpool2_bwd_idx_kernel (pool_up.hip): its four loads and four stores are contiguous runs of a row across
// the lanes.  It gates and stores them and keeps the maximum of the STORED values with its window index; the two threads of an x
// pair then merge through LDS, and the even one writes the pooled vector and the index bytes.  The result is the sequential scan
// of maxpool2_fwd_kernel over the window in (d, h, w) order with `a > max || a != a`: the first of equal maxima, the last NaN.
// Work item q = xb consecutive positions of the flattened (z pair, y pair, x) index, xb even
DEVI void pool_merge(float& m, int& k, float m2, int k2) {
  const bool n1 = m != m, n2 = m2 != m2;
  const bool take = (n1 || n2) ? (n2 && (!n1 || k2 > k)) : (m2 > m || (m2 == m && k2 < k));
  if (take) { m = m2; k = k2; }
}
template <typename T>
__global__ void __launch_bounds__(256) cbam_apply_pool_kernel(const T* __restrict__ x, int pitch, const float* __restrict__ scale, const float* __restrict__ z,
                                                              const float* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              T* __restrict__ out, int opitch, T* __restrict__ pooled, int ppitch, uint8_t* __restrict__ idx,
                                                              int D, int H, int W, int C, int cv, int xb) {
  constexpr int VW = 16 / sizeof(T);
  __shared__ float lmx[VW][256];
  __shared__ int lam[VW][256];
  const int n = blockIdx.y, tid = threadIdx.x, cvi = tid % cv, xl = tid / cv;
  const bool lane_on = xl < xb;
  const int Ho = H / 2, Wo = W / 2, V = D * H * W, Vp = V / 8, Q = (D / 2) * Ho * W, items = (Q + xb - 1) / xb;
  const Norm1 nm = load_norm(stats, gamma, beta, n);
  float sc[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) sc[j] = lane_on ? scale[(size_t)n * C + cvi * VW + j] : 0.f;
  const T* xn = x + (size_t)n * V * pitch + cvi * VW;
  T* on = out + (size_t)n * V * opitch + cvi * VW;
  T* pn = pooled + (size_t)n * Vp * ppitch + cvi * VW;
  uint8_t* in = idx ? idx + (size_t)n * Vp * C + cvi * VW : nullptr;
  const float* zn_ = z + (size_t)n * V;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int q = item * xb + xl;
    const bool ok = lane_on && q < Q;
    const int xx = q % W, r = q / W, yo = r % Ho, zo = r / Ho;
    float mx[VW];
    int am[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) { mx[j] = -INFINITY; am[j] = xx & 1; }
    if (ok) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int v = ((2 * zo + (k >> 1)) * H + 2 * yo + (k & 1)) * W + xx, kk = 2 * k + (xx & 1);  // kk: the voxel's index in its window
        float f[VW], zhat, zn;
        Vec<T, VW>::load(xn + (size_t)v * pitch, f);
        const float g = spatial_gate(zn_[v], nm, zhat, zn);
#pragma unroll
        for (int j = 0; j < VW; ++j) f[j] = f[j] * sc[j] * g;
        Vec<T, VW>::store(on + (size_t)v * opitch, f);
        round_to_storage<T, VW>(f);
#pragma unroll
        for (int j = 0; j < VW; ++j)
          if (f[j] > mx[j] || f[j] != f[j]) { mx[j] = f[j]; am[j] = kk; }
      }
      if (xx & 1) {
#pragma unroll
        for (int j = 0; j < VW; ++j) { lmx[j][tid] = mx[j]; lam[j][tid] = am[j]; }
      }
    }
    __syncthreads();
    if (ok && !(xx & 1)) {  // (W and xb even: the odd neighbour is thread tid + cv of this item)
#pragma unroll
      for (int j = 0; j < VW; ++j) pool_merge(mx[j], am[j], lmx[j][tid + cv], lam[j][tid + cv]);
      const size_t pv = ((size_t)zo * Ho + yo) * Wo + (xx >> 1);
      Vec<T, VW>::store(pn + pv * ppitch, mx);
      if (in) {
        uint32_t* ap = (uint32_t*)(in + pv * C);
#pragma unroll
        for (int qq = 0; qq < VW / 4; ++qq) ap[qq] = am[4 * qq] | (am[4 * qq + 1] << 8) | (am[4 * qq + 2] << 16) | (am[4 * qq + 3] << 24);
      }
    }
    __syncthreads();
  }
}

// backward: the gradient that arrives at the gate's output when a max pool reads it beside the skip connection, composed on load
// and never stored: dout[v][c] = round_to_storage(d_skip[v][c] + (idx[parent(v)][c] == pos(v) ? d_pooled[parent(v)][c] : 0)) in
// the arithmetic of maxpool2_bwd_idx_kernel (pool_up.hip), so the two passes below see the bits its output tensor would hold.
// Pointers are the sample's, at the thread's channel vector (dskip may be null: no skip term)
template <typename T> struct PoolGrad {
  const T* dskip;
  const T* dpool;      // [D/2][H/2][W/2], pitch ppitch
  const uint8_t* idx;  // [D/2][H/2][W/2][C] window-index bytes (d, h, w order)
  int spitch, ppitch, C, H, W;
  DEVI PoolGrad at(int n, int D, int c0) const {
    PoolGrad p = *this;
    const size_t V = (size_t)D * H * W;
    p.dskip = dskip ? dskip + n * V * spitch + c0 : nullptr;
    p.dpool = dpool + n * (V / 8) * ppitch + c0;
    p.idx = idx + n * (V / 8) * C + c0;
    return p;
  }
  template <int VW> DEVI void load(int v, float (&d)[VW]) const {
    const int xx = v % W, r = v / W, yy = r % H, zz = r / H;
    const size_t pv = ((size_t)(zz >> 1) * (H >> 1) + (yy >> 1)) * (W >> 1) + (xx >> 1);
    const int kk = ((zz & 1) << 2) | ((yy & 1) << 1) | (xx & 1);
    uint32_t aw[VW / 4];
#pragma unroll
    for (int q = 0; q < VW / 4; ++q) aw[q] = ((const uint32_t*)(idx + pv * C))[q];
    float g[VW];
    Vec<T, VW>::load(dpool + pv * ppitch, g);
#pragma unroll
    for (int j = 0; j < VW; ++j) d[j] = 0.f + ((int)((aw[j >> 2] >> (8 * (j & 3))) & 0xff) == kk ? g[j] : 0.f);
    if (dskip) {
      float sk[VW];
      Vec<T, VW>::load(dskip + (size_t)v * spitch, sk);
#pragma unroll
      for (int j = 0; j < VW; ++j) d[j] += sk[j];
    }
    round_to_storage<T, VW>(d);
  }
};

// ---- backward pass 1: reads dout and x ----------------------------------------------------------------------------------------
// dg[v] = sum_c dout x s  ->  dzn[v] = dg g (1 - g) [zn > 0]  (the gradient at the instance norm's output, written);
// partials of A[n][c] = sum_v dout x g and of S1 = sum_v dzn, S2 = sum_v dzn zhat.  POOL: dout is composed on load (PoolGrad)
template <typename T, bool POOL>
__global__ void __launch_bounds__(256) cbam_bwd_reduce_kernel(const T* __restrict__ dout, int dpitch, PoolGrad<T> pool, int D, const T* __restrict__ x, int pitch,
                                                              const float* __restrict__ scale, const float* __restrict__ z, const float* __restrict__ stats,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ dzn,
                                                              float* __restrict__ parta /*[nb][N*C]*/, float* __restrict__ parts /*[nb][N*2]*/, int V,
                                                              int C, int cv, int vl, int chunk) {
  constexpr int VW = 16 / sizeof(T);
  __shared__ double lds[256 * VW];
  const int n = blockIdx.y, N = gridDim.y, tid = threadIdx.x, cvi = tid % cv, vlane = tid / cv;
  const bool lane_on = vlane < vl;
  const int v0 = min(V, (int)blockIdx.x * chunk), v1 = min(V, v0 + chunk), iters = (v1 - v0 + vl - 1) / vl;
  const Norm1 nm = load_norm(stats, gamma, beta, n);
  const T* xn = x + (size_t)n * V * pitch + cvi * VW;
  const T* dn = POOL ? nullptr : dout + (size_t)n * V * dpitch + cvi * VW;
  const PoolGrad<T> pg = POOL ? pool.at(n, D, cvi * VW) : pool;
  float sc[VW];
  double a[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) { sc[j] = lane_on ? scale[(size_t)n * C + cvi * VW + j] : 0.f; a[j] = 0.0; }
  double s1 = 0.0, s2 = 0.0;
  int p2 = 1;
  while (p2 < cv) p2 <<= 1;
  for (int it = 0; it < iters; ++it) {
    const int v = v0 + it * vl + vlane;
    const bool ok = lane_on && v < v1;
    double dg = 0.0;
    float zv = 0.f;
    if (ok) {
      float f[VW], d[VW], zhat, zn;
      Vec<T, VW>::load(xn + (size_t)v * pitch, f);
      if constexpr (POOL) pg.load(v, d);
      else Vec<T, VW>::load(dn + (size_t)v * dpitch, d);
      zv = z[(size_t)n * V + v];
      const double g = (double)spatial_gate(zv, nm, zhat, zn);  // (the gate the forward pass applied)
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        const double t = (double)d[j] * (double)f[j];
        dg += t * (double)sc[j];
        a[j] += t * g;
      }
    }
    lds[tid] = dg;
    __syncthreads();
    for (int h = p2 >> 1; h > 0; h >>= 1) {
      if (lane_on && cvi < h && cvi + h < cv) { dg += lds[tid + h]; lds[tid] = dg; }
      __syncthreads();
    }
    if (ok && cvi == 0) {  // sigmoid'(relu(zn)) = g (1 - g) cancels for a wide-open gate: taken in f64 from the stored z and statistics
      const double zhat = ((double)zv - (double)nm.mu) * (double)nm.rstd, zn = zhat * (double)nm.gamma + (double)nm.beta;
      const double g = 1.0 / (1.0 + exp(-zn)), dz = zn > 0.0 ? dg * g * (1.0 - g) : 0.0;
      dzn[(size_t)n * V + v] = (float)dz;
      s1 += dz;
      s2 += dz * zhat;
    }
  }
  lanes_to_partial<VW>(a, lds, parta + ((size_t)blockIdx.x * N + n) * C, C, vl, cvi, vlane);
  s1 = block_sum(s1, lds);
  s2 = block_sum(s2, lds);
  if (tid == 0) {
    float* o = parts + ((size_t)blockIdx.x * N + n) * 2;
    o[0] = (float)s1; o[1] = (float)s2;
  }
}

// ---- backward of norm + convolution on the planes ---------------------------------------------------------------------------------
// dz = gamma rstd (dzn - S1 / V - zhat S2 / V) is formed while the halo tile is staged; dcomp[p] = conv^T(dz) (the stencil with
// flipped taps); per-tile partials of dwc[p][tap] = sum_u comp[p][u] dz[u - off(tap)], u over the tile, dz out of the halo
__global__ void __launch_bounds__(256) cbam_spatial_bwd_kernel(const float* __restrict__ dzn, const float* __restrict__ z, const float* __restrict__ stats,
                                                               const float* __restrict__ s12, const float* __restrict__ gamma, const float* __restrict__ comp,
                                                               const float* __restrict__ wc, float* __restrict__ dcomp, float* __restrict__ partw /*[N*tiles][686]*/,
                                                               int D, int H, int W) {
  __shared__ float dzh[HTILE], ct[2 * TTILE], wl[2 * TAPS], wp[2][2 * TAPS];
  const int n = blockIdx.y, tid = threadIdx.x;
  const size_t V = (size_t)D * H * W;
  const Tile t = tile_origin(blockIdx.x, H, W);
  const float mu = stats[2 * n], rstd = stats[2 * n + 1], k = gamma[0] * rstd, m1 = s12[2 * n] / (float)V, m2 = s12[2 * n + 1] / (float)V;
  for (int i = tid; i < HTILE; i += 256) {
    const int gd = t.d0 - 3 + i / HPLANE, gh = t.h0 - 3 + (i / HW) % HH, gw = t.w0 - 3 + i % HW;
    float v = 0.f;
    if (gd >= 0 && gd < D && gh >= 0 && gh < H && gw >= 0 && gw < W) {
      const size_t o = (size_t)n * V + ((size_t)gd * H + gh) * W + gw;
      v = k * (dzn[o] - m1 - (z[o] - mu) * rstd * m2);
    }
    dzh[i] = v;
  }
  for (int i = tid; i < 2 * TTILE; i += 256) {
    const int p = i / TTILE, r = i % TTILE;
    const int gd = t.d0 + r / (TH * TW), gh = t.h0 + (r / TW) % TH, gw = t.w0 + r % TW;
    ct[i] = (gd < D && gh < H && gw < W) ? comp[((size_t)n * 2 + p) * V + ((size_t)gd * H + gh) * W + gw] : 0.f;
  }
  for (int i = tid; i < 2 * TAPS; i += 256) wl[i] = wc[(i / TAPS) * TAPS + (TAPS - 1 - i % TAPS)];
  __syncthreads();
  {
    const int tw = tid % TW, th = tid / TW, gh = t.h0 + th, gw = t.w0 + tw;
    float acc[2][TD] = {};
    stencil7<1, 2, float>(dzh, wl, th, tw, acc);
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int j = 0; j < TD; ++j)
        if (t.d0 + j < D && gh < H && gw < W) dcomp[((size_t)n * 2 + p) * V + ((size_t)(t.d0 + j) * H + gh) * W + gw] = acc[p][j];
  }
  // weight gradient: thread = (half of the tile's planes, plane p, kz, ky), its seven kx taps in registers, rows walked in order
  if (tid < 196) {
    const int half = tid / 98, r = tid % 98, p = r / 49, kz = (r % 49) / 7, ky = r % 7;
    float acc[7] = {};
    for (int ld = half * (TD / 2); ld < (half + 1) * (TD / 2); ++ld) {
#pragma unroll 1
      for (int lh = 0; lh < TH; ++lh) {
        const float* crow = ct + p * TTILE + (ld * TH + lh) * TW;
        const float* drow = dzh + (ld + 6 - kz) * HPLANE + (lh + 6 - ky) * HW;
        float d[HW], row[7] = {};  // (a row's 32 products first, then into the running sums)
#pragma unroll
        for (int i = 0; i < HW; ++i) d[i] = drow[i];
#pragma unroll
        for (int lw = 0; lw < TW; ++lw) {
          const float c = crow[lw];
#pragma unroll
          for (int kx = 0; kx < 7; ++kx) row[kx] += c * d[lw + 6 - kx];
        }
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) acc[kx] += row[kx];
      }
    }
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) wp[half][p * TAPS + kz * 49 + ky * 7 + kx] = acc[kx];
  }
  __syncthreads();
  float* o = partw + ((size_t)n * gridDim.x + blockIdx.x) * (2 * TAPS);
  for (int i = tid; i < 2 * TAPS; i += 256) o[i] = wp[0][i] + wp[1][i];
}

// ---- backward pass 2: reads x ---------------------------------------------------------------------------------------------------
// partials of R[n][c] = sum_v x (dcomp0 [c == arg-max channel of v] + dcomp1 / C): the part of ds that comes through the planes
template <typename T>
__global__ void __launch_bounds__(256) cbam_bwd_chan_kernel(const T* __restrict__ x, int pitch, const float* __restrict__ dcomp, const uint16_t* __restrict__ cidx,
                                                            float* __restrict__ partr /*[nb][N*C]*/, int V, int C, int cv, int vl, int chunk) {
  constexpr int VW = 16 / sizeof(T);
  __shared__ double lds[256 * VW];
  const int n = blockIdx.y, N = gridDim.y, cvi = threadIdx.x % cv, vlane = threadIdx.x / cv;
  const int v0 = min(V, (int)blockIdx.x * chunk), v1 = min(V, v0 + chunk);
  const T* xn = x + (size_t)n * V * pitch + cvi * VW;
  const float* d0 = dcomp + (size_t)n * 2 * V;
  const float* d1 = d0 + V;
  const uint16_t* cn = cidx + (size_t)n * V;
  double a[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) a[j] = 0.0;
  if (vlane < vl) {
#pragma unroll 4
    for (int v = v0 + vlane; v < v1; v += vl) {
      float f[VW];
      Vec<T, VW>::load(xn + (size_t)v * pitch, f);
      const double ga = (double)d1[v] / (double)C, gb = (double)d0[v] + ga;
      const int cm = (int)cn[v] - cvi * VW;
#pragma unroll
      for (int j = 0; j < VW; ++j) a[j] += (double)f[j] * (j == cm ? gb : ga);
    }
  }
  lanes_to_partial<VW>(a, lds, partr + ((size_t)blockIdx.x * N + n) * C, C, vl, cvi, vlane);
}

// ---- backward of the MLP --------------------------------------------------------------------------------------------------------
// one workgroup per sample: da = (A + R) s (1 - s), dh = W2^T da [h > 0] for both pooled vectors, dpool = W1^T dh
__global__ void __launch_bounds__(256) cbam_bwd_gate_kernel(const float* __restrict__ asum, const float* __restrict__ rsum, const float* __restrict__ pooled,
                                                            const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                            const float* __restrict__ b2,
                                                            float* __restrict__ da_g /*[N][C]*/, float* __restrict__ dh_g /*[N][2][Ch]*/,
                                                            float* __restrict__ dpool /*[N][2][C]*/, int C, int Ch) {
  __shared__ double da[512], dh[2][512], h[2][512];
  const int n = blockIdx.x;
  mlp_hidden(pooled + (size_t)n * 2 * C, w1, b1, h, C, Ch);
  for (int c = threadIdx.x; c < C; c += 256) {
    const double s = mlp_scale(h, w2, b2, c, Ch), v = ((double)asum[(size_t)n * C + c] + (double)rsum[(size_t)n * C + c]) * s * (1.0 - s);
    da[c] = v;
    da_g[(size_t)n * C + c] = (float)v;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < Ch; j += 256) {
    double acc = 0.0;
    for (int c = 0; c < C; ++c) acc += (double)w2[(size_t)c * Ch + j] * da[c];
    for (int k = 0; k < 2; ++k) {
      const double v = h[k][j] > 0.0 ? acc : 0.0;
      dh[k][j] = v;
      dh_g[((size_t)n * 2 + k) * Ch + j] = (float)v;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    for (int k = 0; k < 2; ++k) {
      double acc = 0.0;
      for (int j = 0; j < Ch; ++j) acc += (double)w1[(size_t)j * C + c] * dh[k][j];
      dpool[((size_t)n * 2 + k) * C + c] = (float)acc;
    }
  }
}
// parameter gradients: one thread per element, the samples added in order
__global__ void __launch_bounds__(256) cbam_bwd_params_kernel(const float* __restrict__ da, const float* __restrict__ dh, const float* __restrict__ pooled,
                                                              const float* __restrict__ hidden, const float* __restrict__ s12, float* __restrict__ dw1,
                                                              float* __restrict__ db1, float* __restrict__ dw2, float* __restrict__ db2,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta, int N, int C, int Ch) {
  const int nw = C * Ch, total = 2 * nw + Ch + C + 2;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    double acc = 0.0;
    if (i < nw) {  // dW1 [Ch][C]
      const int j = i / C, c = i % C;
      for (int n = 0; n < N; ++n)
        acc += (double)dh[((size_t)n * 2 + 0) * Ch + j] * pooled[((size_t)n * 2 + 0) * C + c] +
               (double)dh[((size_t)n * 2 + 1) * Ch + j] * pooled[((size_t)n * 2 + 1) * C + c];
      dw1[i] = (float)acc;
    } else if (i < 2 * nw) {  // dW2 [C][Ch]
      const int c = (i - nw) / Ch, j = (i - nw) % Ch;
      for (int n = 0; n < N; ++n) acc += (double)da[(size_t)n * C + c] * ((double)hidden[((size_t)n * 2 + 0) * Ch + j] + (double)hidden[((size_t)n * 2 + 1) * Ch + j]);
      dw2[i - nw] = (float)acc;
    } else if (i < 2 * nw + Ch) {
      const int j = i - 2 * nw;
      for (int n = 0; n < N; ++n) acc += (double)dh[((size_t)n * 2 + 0) * Ch + j] + (double)dh[((size_t)n * 2 + 1) * Ch + j];
      db1[j] = (float)acc;
    } else if (i < 2 * nw + Ch + C) {  // (b2 enters the sum of the two MLP outputs twice)
      const int c = i - 2 * nw - Ch;
      for (int n = 0; n < N; ++n) acc += 2.0 * (double)da[(size_t)n * C + c];
      db2[c] = (float)acc;
    } else {  // dbeta = sum dzn, dgamma = sum dzn zhat
      const int k = i - (2 * nw + Ch + C);
      for (int n = 0; n < N; ++n) acc += (double)s12[2 * n + k];
      (k == 0 ? dbeta : dgamma)[0] = (float)acc;
    }
  }
}

// ---- backward pass 3: reads dout, writes dx (x itself is not needed) ------------------------------------------------------------------------------
// dx = (dout g + dcomp0 [c == arg-max channel] + dcomp1 / C) s + davg / V + dmax [v == arg-max voxel of c].  POOL: dout is
// composed on load (PoolGrad)
template <typename T, bool POOL>
__global__ void __launch_bounds__(256) cbam_bwd_apply_kernel(const T* __restrict__ dout, int dpitch, PoolGrad<T> pool, int D, const float* __restrict__ scale,
                                                             const float* __restrict__ z, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ dcomp, const uint16_t* __restrict__ cidx,
                                                             const float* __restrict__ dpool, const int* __restrict__ argvox, T* __restrict__ dx, int xdpitch,
                                                             int V, int C, int cv, int vl, int chunk) {
  constexpr int VW = 16 / sizeof(T);
  const int n = blockIdx.y, cvi = threadIdx.x % cv, vlane = threadIdx.x / cv;
  if (vlane >= vl) return;
  const int v0 = min(V, (int)blockIdx.x * chunk), v1 = min(V, v0 + chunk);
  const Norm1 nm = load_norm(stats, gamma, beta, n);
  float sc[VW], davg[VW], dmx[VW];
  int av[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    const int c = cvi * VW + j;
    sc[j] = scale[(size_t)n * C + c];
    davg[j] = dpool[((size_t)n * 2 + 0) * C + c] / (float)V;
    dmx[j] = dpool[((size_t)n * 2 + 1) * C + c];
    av[j] = argvox[(size_t)n * C + c];
  }
  const T* dn = POOL ? nullptr : dout + (size_t)n * V * dpitch + cvi * VW;
  const PoolGrad<T> pg = POOL ? pool.at(n, D, cvi * VW) : pool;
  T* on = dx + (size_t)n * V * xdpitch + cvi * VW;
  const float* zp = z + (size_t)n * V;
  const float* d0 = dcomp + (size_t)n * 2 * V;
  const float* d1 = d0 + V;
  const uint16_t* cn = cidx + (size_t)n * V;
#pragma unroll 4
  for (int v = v0 + vlane; v < v1; v += vl) {
    float d[VW], zhat, zn;
    if constexpr (POOL) pg.load(v, d);
    else Vec<T, VW>::load(dn + (size_t)v * dpitch, d);
    const float g = spatial_gate(zp[v], nm, zhat, zn);
    const float gm = d0[v], ga = d1[v] / (float)C;
    const int cm = (int)cn[v] - cvi * VW;
#pragma unroll
    for (int j = 0; j < VW; ++j) d[j] = (d[j] * g + (j == cm ? gm + ga : ga)) * sc[j] + davg[j] + (v == av[j] ? dmx[j] : 0.f);
    Vec<T, VW>::store(on + (size_t)v * xdpitch, d);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
bool aligned16(const void* p, int pitch, int dtype) { return ((size_t)p & 15) == 0 && pitch % vec_width(dtype) == 0; }

// the limits the entry points share; 0 = fine (message set otherwise).  The plane passes have a shape only
int cbam_check_shape(const char* what, int N, int D, int H, int W) {
  if (N < 1 || N > 65535 || D < 1 || H < 1 || W < 1) BRATS_FAIL(BRATS_E_ARG, "%s: bad shape N=%d D=%d H=%d W=%d", what, N, D, H, W);
  if ((size_t)D * H * W > ((size_t)1 << 30)) BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: more than 2^30 voxels per sample", what);
  return 0;
}
int cbam_check(const char* what, int dtype, int N, int C, int D, int H, int W) {
  if (dtype == BRATS_F16) BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: fp16 storage is not built for the CBAM block (use BRATS_F32 or BRATS_BF16)", what);
  if (dtype != BRATS_F32 && dtype != BRATS_BF16) BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: dtype %d (BRATS_F32 or BRATS_BF16 only)", what, dtype);
  if (C < 8 || C > 512 || C % 8) BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: C = %d (a multiple of 8, at most 512)", what, C);
  return cbam_check_shape(what, N, D, H, W);
}
int cbam_check_act(const char* what, const void* p, int pitch, int dtype, int C) {
  if (!p || pitch < C || !aligned16(p, pitch, dtype)) BRATS_FAIL(BRATS_E_ARG, "%s: activation pointer NULL / not 16-byte aligned, or pitch %d < C or not a whole vector", what, pitch);
  return 0;
}

}  // namespace

#define CBAM_CHECKED(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

extern "C" int brats_cbam_blocks(int dtype, int C, int D, int H, int W) {
  if (cbam_check("cbam_blocks", dtype, 1, C, D, H, W)) return 0;
  return cbam_split(dtype, C, D * H * W).nb;
}
extern "C" int brats_cbam_tiles(int D, int H, int W) { return (D < 1 || H < 1 || W < 1) ? 0 : cbam_tiles(D, H, W); }

extern "C" int brats_cbam_pool(const void* x, int xpitch, float* part, float* pooled, int* argvox, int dtype, int N, int C, int D, int H, int W,
                               brats_stream_t s) {
  CBAM_CHECKED(cbam_check("cbam_pool", dtype, N, C, D, H, W));
  CBAM_CHECKED(cbam_check_act("cbam_pool", x, xpitch, dtype, C));
  if (!part || !pooled || !argvox) BRATS_FAIL(BRATS_E_ARG, "cbam_pool: null pointer");
  const int V = D * H * W, total = N * C;
  const Split sp = cbam_split(dtype, C, V);
  float* psum = part;
  float* pmax = part + (size_t)sp.nb * total;
  int* pidx = (int*)(part + (size_t)2 * sp.nb * total);
  hipStream_t st = (hipStream_t)s;
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(cbam_pool_kernel<T>, dim3(sp.nb, N), dim3(256), 0, st, (const T*)x, xpitch, psum, pmax, pidx, V, C, sp.cv, sp.vl, sp.chunk);
  });
  hipLaunchKernelGGL(cbam_pool_finalize_kernel, dim3((total + 7) / 8), dim3(256), 0, st, psum, pmax, pidx, pooled, argvox, sp.nb, total, C, (float)V);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_cbam_gate(const float* pooled, const float* w1, const float* b1, const float* w2, const float* b2, float* hidden, float* scale,
                               int N, int C, int Ch, brats_stream_t s) {
  if (!pooled || !w1 || !b1 || !w2 || !b2 || !hidden || !scale) BRATS_FAIL(BRATS_E_ARG, "cbam_gate: null pointer");
  if (N < 1 || C < 1 || C > 512 || Ch < 1 || Ch > 512) BRATS_FAIL(BRATS_E_UNSUPPORTED, "cbam_gate: N=%d C=%d hidden=%d (C and hidden width 1 .. 512)", N, C, Ch);
  hipLaunchKernelGGL(cbam_gate_kernel, dim3(N), dim3(256), 0, (hipStream_t)s, pooled, w1, b1, w2, b2, hidden, scale, C, Ch);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_cbam_compress(const void* x, int xpitch, const float* scale, float* comp, uint16_t* cidx, int dtype, int N, int C, int D, int H,
                                   int W, brats_stream_t s) {
  CBAM_CHECKED(cbam_check("cbam_compress", dtype, N, C, D, H, W));
  CBAM_CHECKED(cbam_check_act("cbam_compress", x, xpitch, dtype, C));
  if (!scale || !comp) BRATS_FAIL(BRATS_E_ARG, "cbam_compress: null pointer");
  const int V = D * H * W;
  const Split sp = cbam_split(dtype, C, V);
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(cbam_compress_kernel<T>, dim3(sp.nb, N), dim3(256), 0, (hipStream_t)s, (const T*)x, xpitch, scale, comp, cidx, V, C, sp.cv, sp.vl,
                       sp.chunk);
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_cbam_spatial(const float* comp, const float* wc, float* z, float* part, float* stats, float eps, int N, int D, int H, int W,
                                  brats_stream_t s) {
  CBAM_CHECKED(cbam_check_shape("cbam_spatial", N, D, H, W));
  if (!comp || !wc || !z || !part || !stats) BRATS_FAIL(BRATS_E_ARG, "cbam_spatial: null pointer");
  const int tiles = cbam_tiles(D, H, W);
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(cbam_spatial_fwd_kernel, dim3(tiles, N), dim3(256), 0, st, comp, wc, z, part, D, H, W);
  hipLaunchKernelGGL(cbam_norm_finalize_kernel, dim3(N), dim3(256), 0, st, part, stats, tiles, eps);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_cbam_apply(const void* x, int xpitch, const float* scale, const float* z, const float* stats, const float* gamma,
                                const float* beta, void* out, int opitch, int dtype, int N, int C, int D, int H, int W, brats_stream_t s) {
  CBAM_CHECKED(cbam_check("cbam_apply", dtype, N, C, D, H, W));
  CBAM_CHECKED(cbam_check_act("cbam_apply", x, xpitch, dtype, C));
  CBAM_CHECKED(cbam_check_act("cbam_apply", out, opitch, dtype, C));
  if (!scale || !z || !stats || !gamma || !beta) BRATS_FAIL(BRATS_E_ARG, "cbam_apply: null pointer");
  const int V = D * H * W;
  const Split sp = cbam_split(dtype, C, V);
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(cbam_apply_kernel<T>, dim3(sp.nb, N), dim3(256), 0, (hipStream_t)s, (const T*)x, xpitch, scale, z, stats, gamma, beta, (T*)out,
                       opitch, V, C, sp.cv, sp.vl, sp.chunk);
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

namespace {

// Where the output gradient of the two dout-reading backward passes comes from: one stored tensor, or (pooled: the _pool entry
// points) the skip gradient, the pooled gradient and the window-index bytes it is composed from on load
struct DoutSrc {
  const void* dout;  // the stored gradient; pooled: the skip gradient, may be NULL
  int dopitch;
  const void* dpooled;
  int dppitch;
  const unsigned char* idx;
  bool pooled;
};
int cbam_check_dout(const char* what, const DoutSrc& g, int dtype, int C, int D, int H, int W) {
  if (!g.pooled) return cbam_check_act(what, g.dout, g.dopitch, dtype, C);
  if ((D | H | W) & 1) BRATS_FAIL(BRATS_E_ARG, "%s: D, H, W = %d, %d, %d must be even (2x2x2 pooling)", what, D, H, W);
  if (g.dout) CBAM_CHECKED(cbam_check_act(what, g.dout, g.dopitch, dtype, C));
  CBAM_CHECKED(cbam_check_act(what, g.dpooled, g.dppitch, dtype, C));
  if (!g.idx || ((size_t)g.idx & 3)) BRATS_FAIL(BRATS_E_ARG, "%s: window-index pointer NULL or not 4-byte aligned", what);
  return 0;
}
template <typename T> PoolGrad<T> pool_grad(const DoutSrc& g, int C, int H, int W) {
  return PoolGrad<T>{(const T*)g.dout, (const T*)g.dpooled, g.idx, g.dopitch, g.dppitch, C, H, W};
}

int cbam_bwd_reduce_run(const char* what, const DoutSrc& g, const void* x, int xpitch, const float* scale, const float* z, const float* stats,
                        const float* gamma, const float* beta, float* dzn, float* part, float* asum, float* s12, int dtype, int N, int C,
                        int D, int H, int W, brats_stream_t s) {
  CBAM_CHECKED(cbam_check(what, dtype, N, C, D, H, W));
  CBAM_CHECKED(cbam_check_act(what, x, xpitch, dtype, C));
  CBAM_CHECKED(cbam_check_dout(what, g, dtype, C, D, H, W));
  if (!scale || !z || !stats || !gamma || !beta || !dzn || !part || !asum || !s12) BRATS_FAIL(BRATS_E_ARG, "%s: null pointer", what);
  const int V = D * H * W;
  const Split sp = cbam_split(dtype, C, V);
  float* parta = part;
  float* parts = part + (size_t)sp.nb * N * C;
  hipStream_t st = (hipStream_t)s;
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    with_flag(g.pooled, [&](auto p) {
      hipLaunchKernelGGL((cbam_bwd_reduce_kernel<T, decltype(p)::value>), dim3(sp.nb, N), dim3(256), 0, st, (const T*)g.dout, g.dopitch,
                         pool_grad<T>(g, C, H, W), D, (const T*)x, xpitch, scale, z, stats, gamma, beta, dzn, parta, parts, V, C, sp.cv, sp.vl, sp.chunk);
    });
  });
  cbam_sum_partials(parta, asum, sp.nb, N * C, st);
  cbam_sum_partials(parts, s12, sp.nb, N * 2, st);
  BRATS_CHECK_LAUNCH();
  return 0;
}

int cbam_bwd_apply_run(const char* what, const DoutSrc& g, const float* scale, const float* z, const float* stats, const float* gamma,
                       const float* beta, const float* dcomp, const uint16_t* cidx, const float* dpool, const int* argvox, void* dx, int dxpitch,
                       int dtype, int N, int C, int D, int H, int W, brats_stream_t s) {
  CBAM_CHECKED(cbam_check(what, dtype, N, C, D, H, W));
  CBAM_CHECKED(cbam_check_dout(what, g, dtype, C, D, H, W));
  CBAM_CHECKED(cbam_check_act(what, dx, dxpitch, dtype, C));
  if (!scale || !z || !stats || !gamma || !beta || !dcomp || !cidx || !dpool || !argvox) BRATS_FAIL(BRATS_E_ARG, "%s: null pointer", what);
  const int V = D * H * W;
  const Split sp = cbam_split(dtype, C, V);
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    with_flag(g.pooled, [&](auto p) {
      hipLaunchKernelGGL((cbam_bwd_apply_kernel<T, decltype(p)::value>), dim3(sp.nb, N), dim3(256), 0, (hipStream_t)s, (const T*)g.dout, g.dopitch,
                         pool_grad<T>(g, C, H, W), D, scale, z, stats, gamma, beta, dcomp, cidx, dpool, argvox, (T*)dx, dxpitch, V, C, sp.cv, sp.vl,
                         sp.chunk);
    });
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int brats_cbam_apply_pool(const void* x, int xpitch, const float* scale, const float* z, const float* stats, const float* gamma,
                                     const float* beta, void* out, int opitch, void* pooled, int ppitch, unsigned char* idx, int dtype, int N,
                                     int C, int D, int H, int W, brats_stream_t s) {
  CBAM_CHECKED(cbam_check("cbam_apply_pool", dtype, N, C, D, H, W));
  if ((D | H | W) & 1) BRATS_FAIL(BRATS_E_ARG, "cbam_apply_pool: D, H, W = %d, %d, %d must be even (2x2x2 pooling)", D, H, W);
  CBAM_CHECKED(cbam_check_act("cbam_apply_pool", x, xpitch, dtype, C));
  CBAM_CHECKED(cbam_check_act("cbam_apply_pool", out, opitch, dtype, C));
  CBAM_CHECKED(cbam_check_act("cbam_apply_pool", pooled, ppitch, dtype, C));
  if (!scale || !z || !stats || !gamma || !beta) BRATS_FAIL(BRATS_E_ARG, "cbam_apply_pool: null pointer");
  if ((size_t)idx & 3) BRATS_FAIL(BRATS_E_ARG, "cbam_apply_pool: window-index pointer not 4-byte aligned");
  const int cv = C / vec_width(dtype);
  int xb = (256 / cv) & ~1;  // x positions per work item: even, so that both voxels of an x pair are in one workgroup
  if (xb > W) xb = W;
  const size_t items = ((size_t)(D / 2) * (H / 2) * W + xb - 1) / xb;
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(cbam_apply_pool_kernel<T>, dim3(stream_grid(items, 1, 8 * CBAM_MAX_BLOCKS), N), dim3(256), 0, (hipStream_t)s, (const T*)x, xpitch,
                       scale, z, stats, gamma, beta, (T*)out, opitch, (T*)pooled, ppitch, idx, D, H, W, C, cv, xb);
  });
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_cbam_bwd_reduce(const void* dout, int dopitch, const void* x, int xpitch, const float* scale, const float* z,
                                     const float* stats, const float* gamma, const float* beta, float* dzn, float* part, float* asum,
                                     float* s12, int dtype, int N, int C, int D, int H, int W, brats_stream_t s) {
  return cbam_bwd_reduce_run("cbam_bwd_reduce", DoutSrc{dout, dopitch, nullptr, 0, nullptr, false}, x, xpitch, scale, z, stats, gamma, beta, dzn, part,
                             asum, s12, dtype, N, C, D, H, W, s);
}
extern "C" int brats_cbam_bwd_reduce_pool(const void* dskip, int dspitch, const void* dpooled, int dppitch, const unsigned char* idx, const void* x,
                                          int xpitch, const float* scale, const float* z, const float* stats, const float* gamma,
                                          const float* beta, float* dzn, float* part, float* asum, float* s12, int dtype, int N, int C, int D,
                                          int H, int W, brats_stream_t s) {
  return cbam_bwd_reduce_run("cbam_bwd_reduce_pool", DoutSrc{dskip, dspitch, dpooled, dppitch, idx, true}, x, xpitch, scale, z, stats, gamma, beta, dzn,
                             part, asum, s12, dtype, N, C, D, H, W, s);
}

extern "C" int brats_cbam_bwd_spatial(const float* dzn, const float* z, const float* stats, const float* s12, const float* gamma,
                                      const float* comp, const float* wc, float* dcomp, float* part, float* dwc, int N, int D, int H, int W,
                                      brats_stream_t s) {
  CBAM_CHECKED(cbam_check_shape("cbam_bwd_spatial", N, D, H, W));
  if (!dzn || !z || !stats || !s12 || !gamma || !comp || !wc || !dcomp || !part || !dwc) BRATS_FAIL(BRATS_E_ARG, "cbam_bwd_spatial: null pointer");
  const int tiles = cbam_tiles(D, H, W);
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(cbam_spatial_bwd_kernel, dim3(tiles, N), dim3(256), 0, st, dzn, z, stats, s12, gamma, comp, wc, dcomp, part, D, H, W);
  cbam_sum_partials(part, dwc, N * tiles, 2 * TAPS, st);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_cbam_bwd_chan(const void* x, int xpitch, const float* dcomp, const uint16_t* cidx, float* part, float* rsum, int dtype, int N,
                                   int C, int D, int H, int W, brats_stream_t s) {
  CBAM_CHECKED(cbam_check("cbam_bwd_chan", dtype, N, C, D, H, W));
  CBAM_CHECKED(cbam_check_act("cbam_bwd_chan", x, xpitch, dtype, C));
  if (!dcomp || !cidx || !part || !rsum) BRATS_FAIL(BRATS_E_ARG, "cbam_bwd_chan: null pointer");
  const int V = D * H * W;
  const Split sp = cbam_split(dtype, C, V);
  hipStream_t st = (hipStream_t)s;
  with_storage(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL(cbam_bwd_chan_kernel<T>, dim3(sp.nb, N), dim3(256), 0, st, (const T*)x, xpitch, dcomp, cidx, part, V, C, sp.cv, sp.vl, sp.chunk);
  });
  cbam_sum_partials(part, rsum, sp.nb, N * C, st);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_cbam_bwd_gate(const float* asum, const float* rsum, const float* pooled, const float* hidden, const float* w1,
                                   const float* b1, const float* w2, const float* b2, const float* s12, float* tmp, float* dpool, float* dw1,
                                   float* db1, float* dw2, float* db2, float* dgamma, float* dbeta, int N, int C, int Ch, brats_stream_t s) {
  if (!asum || !rsum || !pooled || !hidden || !w1 || !b1 || !w2 || !b2 || !s12 || !tmp || !dpool || !dw1 || !db1 || !dw2 || !db2 || !dgamma || !dbeta)
    BRATS_FAIL(BRATS_E_ARG, "cbam_bwd_gate: null pointer");
  if (N < 1 || C < 1 || C > 512 || Ch < 1 || Ch > 512) BRATS_FAIL(BRATS_E_UNSUPPORTED, "cbam_bwd_gate: N=%d C=%d hidden=%d (C and hidden width 1 .. 512)", N, C, Ch);
  float* da = tmp;
  float* dh = tmp + (size_t)N * C;
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(cbam_bwd_gate_kernel, dim3(N), dim3(256), 0, st, asum, rsum, pooled, w1, b1, w2, b2, da, dh, dpool, C, Ch);
  const int total = 2 * C * Ch + Ch + C + 2;
  hipLaunchKernelGGL(cbam_bwd_params_kernel, dim3(stream_grid(total, 256, 1024)), dim3(256), 0, st, da, dh, pooled, hidden, s12, dw1, db1, dw2, db2, dgamma,
                     dbeta, N, C, Ch);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_cbam_bwd_apply(const void* dout, int dopitch, const float* scale, const float* z,
                                    const float* stats, const float* gamma, const float* beta, const float* dcomp, const uint16_t* cidx,
                                    const float* dpool, const int* argvox, void* dx, int dxpitch, int dtype, int N, int C, int D, int H, int W,
                                    brats_stream_t s) {
  return cbam_bwd_apply_run("cbam_bwd_apply", DoutSrc{dout, dopitch, nullptr, 0, nullptr, false}, scale, z, stats, gamma, beta, dcomp, cidx, dpool, argvox,
                            dx, dxpitch, dtype, N, C, D, H, W, s);
}
extern "C" int brats_cbam_bwd_apply_pool(const void* dskip, int dspitch, const void* dpooled, int dppitch, const unsigned char* idx,
                                         const float* scale, const float* z, const float* stats, const float* gamma, const float* beta,
                                         const float* dcomp, const uint16_t* cidx, const float* dpool, const int* argvox, void* dx, int dxpitch,
                                         int dtype, int N, int C, int D, int H, int W, brats_stream_t s) {
  return cbam_bwd_apply_run("cbam_bwd_apply_pool", DoutSrc{dskip, dspitch, dpooled, dppitch, idx, true}, scale, z, stats, gamma, beta, dcomp, cidx, dpool,
                            argvox, dx, dxpitch, dtype, N, C, D, H, W, s);
}
