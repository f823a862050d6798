// STAPLE fusion of an ensemble's binary segmentations (Warfield et al.; ITK's STAPLEImageFilter::GenerateData as restated in
// DESIGN.md section 6): the reference's --perform_staple / --staple_threshold (learning/engine.py:244-247 ->
// perform_staple_on_brats_multi_channel, utils/transforms.py:650-687, SimpleITK on the host, one thread, three channels in turn).
// A rater's decision on a voxel is one bit: bits[problem][word][voxel] (uint32, word = rater / 32) holds up to 256 raters; a
// problem is one (sample, channel).  The f32 maps of the raters are never kept.
//   staple_pack    : OR rater r's 0/1 map into the planes, count_r += its foreground voxels (integer atomics)
//   staple_zeros   : n0 = voxels that no rater marks (they all share one weight W0)
//   staple_state   : g = (sum of all votes, exact integer) / (R V); p = q = 0, last_p = last_q = -10, iteration counter, done flag
//   staple_sums    : pass (a) of an iteration: the E-step of the previous one (W from the voxel's pattern and p, q; votes / R in
//                    iteration 0) fused with the sums of the M-step: per workgroup, sum of W over the marked voxels and sum of
//                    W D[j] per rater.  Tiles that no rater marks cost one load and one compare per voxel.
//   staple_update  : pass (b), one workgroup per problem: adds the workgroups' rows in a fixed order, p[j], q[j] from
//                    q_num[j] = (V - sum W) - (count_j - p_num[j]), ITK's convergence rule, the done flag
//   staple_apply   : W(pattern) > threshold -> f32 / uint8 0/1 (NaN: 0), optionally W itself (f64)
// All floating-point arithmetic is f64 in a fixed order, no floating-point atomics: two runs give the same bits.  The
// data-dependent loop is the host's: every launch returns at once for a problem whose done flag is set, no kernel waits for
// another workgroup.
#include "common.hpp"

static constexpr int STAPLE_TILE = 256;       // voxels per tile = threads per workgroup
static constexpr int STAPLE_MAX_BLOCKS = 512;  // rows of partial sums per problem
static constexpr int STAPLE_MAX_R = 256;
static constexpr int STAPLE_PACK_PER_THREAD = 4;
enum { FL_ITER = 0, FL_DONE = 1, FL_ITERATIONS = 2, FL_N0 = 3 };  // flags[problem][4]
// state[problem][2 + 4 R] (f64): g, sum W of the last M-step, p[R], q[R], last_p[R], last_q[R]
static inline __host__ __device__ size_t staple_state_stride(int R) { return 2 + 4 * (size_t)R; }

static int staple_blocks(size_t V) {
  const size_t tiles = (V + STAPLE_TILE - 1) / STAPLE_TILE;
  const size_t per = (tiles + STAPLE_MAX_BLOCKS - 1) / STAPLE_MAX_BLOCKS;
  return (int)((tiles + per - 1) / (per ? per : 1));
}

// the lanes of a workgroup as (rater, part): raters 0 .. RP-1 (RP = 64, 128 or 256 >= R), 256 / RP parts that split a range
__device__ __forceinline__ int staple_rp(int R) { return R <= 64 ? 64 : (R <= 128 ? 128 : 256); }

template <typename T>
__global__ void __launch_bounds__(256) staple_pack_kernel(const T* __restrict__ mask, uint32_t* __restrict__ bits,
                                                          uint32_t* __restrict__ counts, int words, size_t V, int rater,
                                                          int count_stride) {
  const int nc = blockIdx.y;
  const T* __restrict__ m = mask + (size_t)nc * V;
  uint32_t* __restrict__ plane = bits + ((size_t)nc * words + (rater >> 5)) * V;
  int n = 0;
#pragma unroll
  for (int i = 0; i < STAPLE_PACK_PER_THREAD; ++i) {  // independent voxels per thread: the loads of all of them are in flight together
    const size_t v = ((size_t)blockIdx.x * STAPLE_PACK_PER_THREAD + i) * 256 + threadIdx.x;
    const bool on = v < V && m[v] == (T)1;  // ITK's foreground value
    if (on) plane[v] |= 1u << (rater & 31);
    n += __popcll(__ballot(on));
  }
  __shared__ int wave_n[4];
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    if (total) atomicAdd(&counts[(size_t)nc * count_stride + rater], (uint32_t)total);
  }
}

__global__ void __launch_bounds__(64) staple_reset_kernel(int* __restrict__ flags, int total) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < total) flags[i] = 0;
}

__global__ void __launch_bounds__(256) staple_zeros_kernel(const uint32_t* __restrict__ bits, int* __restrict__ flags, int words,
                                                           size_t V) {
  const int nc = blockIdx.y;
  int n = 0;
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < V; v += (size_t)gridDim.x * 256) {
    uint32_t any = 0;
    for (int k = 0; k < words; ++k) any |= bits[((size_t)nc * words + k) * V + v];
    n += any == 0;
  }
  __shared__ int red[256];
  red[threadIdx.x] = n;
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x == 0 && red[0]) atomicAdd(&flags[nc * 4 + FL_N0], red[0]);
}

__global__ void __launch_bounds__(256) staple_state_kernel(const uint32_t* __restrict__ counts, int count_stride,
                                                           double* __restrict__ state, int R, size_t V) {
  const int nc = blockIdx.x, t = threadIdx.x;
  double* __restrict__ st = state + (size_t)nc * staple_state_stride(R);
  __shared__ unsigned long long red[256];
  red[t] = t < R ? counts[(size_t)nc * count_stride + t] : 0ull;
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if (t < m) red[t] += red[t + m];
    __syncthreads();
  }
  if (t == 0) {
    st[0] = (double)red[0] / (double)((unsigned long long)R * (unsigned long long)V);  // both integers < 2^53: one rounding
    st[1] = 0.0;
  }
  if (t < R) {
    st[2 + t] = 0.0;
    st[2 + R + t] = 0.0;
    st[2 + 2 * R + t] = -10.0;
    st[2 + 3 * R + t] = -10.0;
  }
}

// W of one voxel from its pattern: plain products in rater order, as ITK's E-step
template <int WORDS>
__device__ __forceinline__ double staple_weight(const uint32_t (&w)[WORDS], const double* __restrict__ sp,
                                                const double* __restrict__ sq, int R, double g) {
  double a = 1.0, b = 1.0;
#pragma unroll
  for (int k = 0; k < WORDS; ++k) {
    const int n = R - k * 32 < 32 ? R - k * 32 : 32;
    for (int i = 0; i < n; ++i) {
      const bool d = (w[k] >> i) & 1u;
      const double pj = sp[k * 32 + i], qj = sq[k * 32 + i];
      a *= d ? pj : 1.0 - pj;
      b *= d ? 1.0 - qj : qj;
    }
  }
  return g * a / (g * a + (1.0 - g) * b);
}

__device__ __forceinline__ double staple_weight0(const double* __restrict__ sp, const double* __restrict__ sq, int R, double g) {
  double a = 1.0, b = 1.0;
  for (int j = 0; j < R; ++j) {
    a *= 1.0 - sp[j];
    b *= sq[j];
  }
  return g * a / (g * a + (1.0 - g) * b);
}

template <int WORDS>
__global__ void __launch_bounds__(256) staple_sums_kernel(const uint32_t* __restrict__ bits, const double* __restrict__ state,
                                                          const int* __restrict__ flags, double* __restrict__ partial, int R,
                                                          size_t V, int tiles_per_block) {
  const int nc = blockIdx.y, t = threadIdx.x;
  if (flags[nc * 4 + FL_DONE]) return;
  const int it = flags[nc * 4 + FL_ITER];
  const double* __restrict__ st = state + (size_t)nc * staple_state_stride(R);
  __shared__ double sp[STAPLE_MAX_R], sq[STAPLE_MAX_R], sW[STAPLE_TILE];
  __shared__ uint32_t sbits[WORDS][STAPLE_TILE];
  const double g = st[0];
  if (t < R) {
    sp[t] = st[2 + t];
    sq[t] = st[2 + R + t];
  }
  __syncthreads();
  const int RP = staple_rp(R), j = t & (RP - 1), part = t / RP;  // lane (j, part) walks voxels [part RP, part RP + RP) of a tile
  const int jw = j >> 5, jb = j & 31;
  const double rd = (double)R;
  double accw = 0.0, accj = 0.0;
  const size_t ntiles = (V + STAPLE_TILE - 1) / STAPLE_TILE;
  const size_t tile0 = (size_t)blockIdx.x * tiles_per_block;
  const size_t tile1 = tile0 + tiles_per_block < ntiles ? tile0 + tiles_per_block : ntiles;
  const uint32_t* __restrict__ plane = bits + (size_t)nc * WORDS * V;
  for (size_t tile = tile0; tile < tile1; ++tile) {
    const size_t v = tile * STAPLE_TILE + t;
    uint32_t w[WORDS];
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < WORDS; ++k) {
      w[k] = v < V ? plane[(size_t)k * V + v] : 0u;
      any |= w[k];
    }
    if (!__syncthreads_or(any != 0)) continue;  // a tile no rater marks: its voxels are counted in n0
    double W = 0.0;
    if (any) {
      if (it == 0) {
        int pc = 0;
#pragma unroll
        for (int k = 0; k < WORDS; ++k) pc += __popc(w[k]);
        W = (double)pc / rd;
      } else {
        W = staple_weight<WORDS>(w, sp, sq, R, g);
      }
      accw += W;
    }
    sW[t] = W;
#pragma unroll
    for (int k = 0; k < WORDS; ++k) sbits[k][t] = w[k];
    __syncthreads();
    if (j < R) {
      const uint32_t* __restrict__ row = sbits[jw];
      for (int u = part * RP; u < part * RP + RP; ++u)
        if ((row[u] >> jb) & 1u) accj += sW[u];
    }
    __syncthreads();
  }
  // rater sums: the parts in order; sum of W: the fixed tree
  __shared__ double red[256];
  red[t] = accj;
  __syncthreads();
  double* __restrict__ out = partial + ((size_t)nc * gridDim.x + blockIdx.x) * (R + 1);
  if (t < R) {  // (t < R <= RP: part 0)
    double s = red[t];
    for (int q = 1; q < 256 / RP; ++q) s += red[q * RP + t];
    out[t] = s;
  }
  __syncthreads();
  red[t] = accw;
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if (t < m) red[t] += red[t + m];
    __syncthreads();
  }
  if (t == 0) out[R] = red[0];
}

__global__ void __launch_bounds__(256) staple_update_kernel(const double* __restrict__ partial, const uint32_t* __restrict__ counts,
                                                            int count_stride, double* __restrict__ state, int* __restrict__ flags,
                                                            int R, size_t V, int nblocks, int max_iterations) {
  const int nc = blockIdx.x, t = threadIdx.x;
  if (flags[nc * 4 + FL_DONE]) return;
  const int it = flags[nc * 4 + FL_ITER];
  double* __restrict__ st = state + (size_t)nc * staple_state_stride(R);
  const double* __restrict__ rows = partial + (size_t)nc * nblocks * (R + 1);
  __shared__ double sp[STAPLE_MAX_R], sq[STAPLE_MAX_R], red[256];
  if (t < R) {
    sp[t] = st[2 + t];
    sq[t] = st[2 + R + t];
  }
  __syncthreads();
  // sum of W over the marked voxels: thread t adds rows t, t + 256, ..., then the fixed tree
  double s = 0.0;
  for (int b = t; b < nblocks; b += 256) s += rows[(size_t)b * (R + 1) + R];
  red[t] = s;
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if (t < m) red[t] += red[t + m];
    __syncthreads();
  }
  double sum_w = red[0];
  const int n0 = flags[nc * 4 + FL_N0];
  if (n0 > 0 && it > 0) sum_w += (double)n0 * staple_weight0(sp, sq, R, st[0]);  // (iteration 0: W0 = 0 / R)
  __syncthreads();
  // p_num[j]: lane (j, part) adds its share of the rows in order, then the parts in order
  const int RP = staple_rp(R), j = t & (RP - 1), part = t / RP, parts = 256 / RP;
  const int per = (nblocks + parts - 1) / parts;
  const int b0 = part * per, b1 = b0 + per < nblocks ? b0 + per : nblocks;
  double acc = 0.0;
  if (j < R) {
    int b = b0;
    for (; b + 8 <= b1; b += 8) {  // eight loads in flight, added in row order
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = rows[(size_t)(b + k) * (R + 1) + j];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += v[k];
    }
    for (; b < b1; ++b) acc += rows[(size_t)b * (R + 1) + j];
  }
  red[t] = acc;
  __syncthreads();
  bool moved = false;
  if (t < R) {
    double pn = red[t];
    for (int q = 1; q < parts; ++q) pn += red[q * RP + t];
    const double rest = (double)V - sum_w;
    const double p = pn / sum_w;
    const double q = (rest - ((double)counts[(size_t)nc * count_stride + t] - pn)) / rest;
    const double dp = p - st[2 + 2 * R + t], dq = q - st[2 + 3 * R + t];
    moved = dp * dp > 1e-14 || dq * dq > 1e-14;  // (written so that a NaN counts as converged, as in ITK)
    st[2 + t] = p;
    st[2 + R + t] = q;
    st[2 + 2 * R + t] = p;
    st[2 + 3 * R + t] = q;
  }
  const int any_moved = __syncthreads_or(moved);
  if (t == 0) {
    st[1] = sum_w;
    flags[nc * 4 + FL_ITER] = it + 1;
    if (!any_moved) {
      flags[nc * 4 + FL_DONE] = 1;
      flags[nc * 4 + FL_ITERATIONS] = it;  // ITK's m_ElapsedIterations: the index of the iteration that converged
    } else if (it + 1 >= max_iterations) {
      flags[nc * 4 + FL_DONE] = 1;
      flags[nc * 4 + FL_ITERATIONS] = max_iterations;
    }
  }
}

template <int WORDS, typename T>
__global__ void __launch_bounds__(256) staple_apply_kernel(const uint32_t* __restrict__ bits, const double* __restrict__ state,
                                                           int R, size_t V, double threshold, T* __restrict__ seg,
                                                           double* __restrict__ prob) {
  const int nc = blockIdx.y, t = threadIdx.x;
  const double* __restrict__ st = state + (size_t)nc * staple_state_stride(R);
  __shared__ double sp[STAPLE_MAX_R], sq[STAPLE_MAX_R];
  if (t < R) {
    sp[t] = st[2 + t];
    sq[t] = st[2 + R + t];
  }
  __syncthreads();
  const double g = st[0];
  const double W0 = staple_weight0(sp, sq, R, g);
  const uint32_t* __restrict__ plane = bits + (size_t)nc * WORDS * V;
  for (size_t v = (size_t)blockIdx.x * 256 + t; v < V; v += (size_t)gridDim.x * 256) {
    uint32_t w[WORDS];
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < WORDS; ++k) {
      w[k] = plane[(size_t)k * V + v];
      any |= w[k];
    }
    const double W = any ? staple_weight<WORDS>(w, sp, sq, R, g) : W0;
    if (seg) seg[(size_t)nc * V + v] = W > threshold ? (T)1 : (T)0;  // (a NaN is background)
    if (prob) prob[(size_t)nc * V + v] = W;
  }
}

static int staple_check(const char* what, int NC, int R, size_t V) {
  if (NC < 1 || NC > 65535) BRATS_FAIL(BRATS_E_ARG, "%s: %d problems (1 .. 65535 supported)", what, NC);
  if (R < 1 || R > STAPLE_MAX_R) BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: %d raters (1 .. %d supported)", what, R, STAPLE_MAX_R);
  if (V < 1 || V >= ((size_t)1 << 31)) BRATS_FAIL(BRATS_E_UNSUPPORTED, "%s: %zu voxels per sample (1 .. 2^31 - 1 supported)", what, V);
  return 0;
}

extern "C" int brats_staple_blocks(size_t V) { return V >= 1 && V < ((size_t)1 << 31) ? staple_blocks(V) : 0; }

extern "C" int brats_staple_pack(const void* mask, int mask_kind, uint32_t* bits, uint32_t* counts, int count_stride, int NC,
                                 int words, size_t V, int rater, brats_stream_t s) {
  if (!mask || !bits || !counts) BRATS_FAIL(BRATS_E_ARG, "staple_pack: null mask / bits / counts");
  if (mask_kind != BRATS_MASK_F32 && mask_kind != BRATS_MASK_U8) BRATS_FAIL(BRATS_E_ARG, "staple_pack: unknown mask kind %d", mask_kind);
  if (words < 1 || words > STAPLE_MAX_R / 32) BRATS_FAIL(BRATS_E_UNSUPPORTED, "staple_pack: %d words (1 .. 8: at most 256 raters)", words);
  if (rater < 0 || rater >= words * 32 || rater >= count_stride)
    BRATS_FAIL(BRATS_E_ARG, "staple_pack: rater %d outside the %d words / %d counts", rater, words, count_stride);
  if (int rc = staple_check("staple_pack", NC, 1, V)) return rc;
  hipStream_t st = (hipStream_t)s;
  const dim3 grid((unsigned)((V + 256 * STAPLE_PACK_PER_THREAD - 1) / (256 * STAPLE_PACK_PER_THREAD)), NC);
  if (mask_kind == BRATS_MASK_F32)
    hipLaunchKernelGGL(staple_pack_kernel<float>, grid, dim3(256), 0, st, (const float*)mask, bits, counts, words, V, rater, count_stride);
  else
    hipLaunchKernelGGL(staple_pack_kernel<uint8_t>, grid, dim3(256), 0, st, (const uint8_t*)mask, bits, counts, words, V, rater, count_stride);
  BRATS_CHECK_LAUNCH();
  return 0;
}

extern "C" int brats_staple_init(const uint32_t* bits, const uint32_t* counts, int count_stride, double* state, int* flags, int NC,
                                 int R, size_t V, brats_stream_t s) {
  if (!bits || !counts || !state || !flags) BRATS_FAIL(BRATS_E_ARG, "staple_init: null bits / counts / state / flags");
  if (int rc = staple_check("staple_init", NC, R, V)) return rc;
  if (count_stride < R) BRATS_FAIL(BRATS_E_ARG, "staple_init: %d counts per problem for %d raters", count_stride, R);
  hipStream_t st = (hipStream_t)s;
  const int words = (R + 31) / 32;
  hipLaunchKernelGGL(staple_reset_kernel, dim3((NC * 4 + 63) / 64), dim3(64), 0, st, flags, NC * 4);
  BRATS_CHECK_LAUNCH();
  hipLaunchKernelGGL(staple_zeros_kernel, dim3(staple_blocks(V), NC), dim3(256), 0, st, bits, flags, words, V);
  BRATS_CHECK_LAUNCH();
  hipLaunchKernelGGL(staple_state_kernel, dim3(NC), dim3(256), 0, st, counts, count_stride, state, R, V);
  BRATS_CHECK_LAUNCH();
  return 0;
}

template <int WORDS>
static void staple_launch_sums(dim3 grid, hipStream_t st, const uint32_t* bits, const double* state, const int* flags, double* partial,
                               int R, size_t V, int tpb) {
  hipLaunchKernelGGL(staple_sums_kernel<WORDS>, grid, dim3(256), 0, st, bits, state, flags, partial, R, V, tpb);
}

extern "C" int brats_staple_iterate(const uint32_t* bits, const uint32_t* counts, int count_stride, double* state, int* flags,
                                    double* partial, int NC, int R, size_t V, int max_iterations, int iterations, brats_stream_t s) {
  if (!bits || !counts || !state || !flags || !partial) BRATS_FAIL(BRATS_E_ARG, "staple_iterate: null bits / counts / state / flags / partial");
  if (int rc = staple_check("staple_iterate", NC, R, V)) return rc;
  if (count_stride < R) BRATS_FAIL(BRATS_E_ARG, "staple_iterate: %d counts per problem for %d raters", count_stride, R);
  if (max_iterations < 1 || iterations < 0) BRATS_FAIL(BRATS_E_ARG, "staple_iterate: max_iterations %d < 1 or %d iterations", max_iterations, iterations);
  hipStream_t st = (hipStream_t)s;
  const int nblocks = staple_blocks(V);
  const size_t tiles = (V + STAPLE_TILE - 1) / STAPLE_TILE;
  const int tpb = (int)((tiles + nblocks - 1) / nblocks);
  const dim3 grid(nblocks, NC);
  for (int i = 0; i < iterations; ++i) {
    switch ((R + 31) / 32) {
      case 1: staple_launch_sums<1>(grid, st, bits, state, flags, partial, R, V, tpb); break;
      case 2: staple_launch_sums<2>(grid, st, bits, state, flags, partial, R, V, tpb); break;
      case 3: staple_launch_sums<3>(grid, st, bits, state, flags, partial, R, V, tpb); break;
      case 4: staple_launch_sums<4>(grid, st, bits, state, flags, partial, R, V, tpb); break;
      case 5: staple_launch_sums<5>(grid, st, bits, state, flags, partial, R, V, tpb); break;
      case 6: staple_launch_sums<6>(grid, st, bits, state, flags, partial, R, V, tpb); break;
      case 7: staple_launch_sums<7>(grid, st, bits, state, flags, partial, R, V, tpb); break;
      default: staple_launch_sums<8>(grid, st, bits, state, flags, partial, R, V, tpb); break;
    }
    BRATS_CHECK_LAUNCH();
    hipLaunchKernelGGL(staple_update_kernel, dim3(NC), dim3(256), 0, st, (const double*)partial, counts, count_stride, state, flags, R,
                       V, nblocks, max_iterations);
    BRATS_CHECK_LAUNCH();
  }
  return 0;
}

template <int WORDS>
static void staple_launch_apply(dim3 grid, hipStream_t st, const uint32_t* bits, const double* state, int R, size_t V, double thr,
                                void* seg, int seg_kind, double* prob) {
  if (seg_kind == BRATS_MASK_U8)
    hipLaunchKernelGGL((staple_apply_kernel<WORDS, uint8_t>), grid, dim3(256), 0, st, bits, state, R, V, thr, (uint8_t*)seg, prob);
  else
    hipLaunchKernelGGL((staple_apply_kernel<WORDS, float>), grid, dim3(256), 0, st, bits, state, R, V, thr, (float*)seg, prob);
}

extern "C" int brats_staple_apply(const uint32_t* bits, const double* state, int NC, int R, size_t V, double threshold, void* seg,
                                  int seg_kind, double* prob, brats_stream_t s) {
  if (!bits || !state || (!seg && !prob)) BRATS_FAIL(BRATS_E_ARG, "staple_apply: null bits / state, or neither seg nor prob");
  if (seg_kind != BRATS_MASK_F32 && seg_kind != BRATS_MASK_U8) BRATS_FAIL(BRATS_E_ARG, "staple_apply: unknown seg kind %d", seg_kind);
  if (!(threshold >= 0.0 && threshold <= 1.0)) BRATS_FAIL(BRATS_E_ARG, "staple_apply: threshold %g outside [0, 1]", threshold);
  if (int rc = staple_check("staple_apply", NC, R, V)) return rc;
  hipStream_t st = (hipStream_t)s;
  const dim3 grid((unsigned)(((V + 255) / 256 + 3) / 4), NC);
  switch ((R + 31) / 32) {
    case 1: staple_launch_apply<1>(grid, st, bits, state, R, V, threshold, seg, seg_kind, prob); break;
    case 2: staple_launch_apply<2>(grid, st, bits, state, R, V, threshold, seg, seg_kind, prob); break;
    case 3: staple_launch_apply<3>(grid, st, bits, state, R, V, threshold, seg, seg_kind, prob); break;
    case 4: staple_launch_apply<4>(grid, st, bits, state, R, V, threshold, seg, seg_kind, prob); break;
    case 5: staple_launch_apply<5>(grid, st, bits, state, R, V, threshold, seg, seg_kind, prob); break;
    case 6: staple_launch_apply<6>(grid, st, bits, state, R, V, threshold, seg, seg_kind, prob); break;
    case 7: staple_launch_apply<7>(grid, st, bits, state, R, V, threshold, seg, seg_kind, prob); break;
    default: staple_launch_apply<8>(grid, st, bits, state, R, V, threshold, seg, seg_kind, prob); break;
  }
  BRATS_CHECK_LAUNCH();
  return 0;
}
