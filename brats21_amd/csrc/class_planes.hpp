// Shared by the streaming passes over [N][K][V] f32 class planes (softmax_loss.hip, sigmoid_loss.hip): the grid of a pass, W
// voxels of every plane to and from registers, and per-thread sums -> one row of partials per workgroup in a fixed order.
#pragma once
#include "common.hpp"

constexpr int SM_MAX_K = 16;
constexpr int SM_MAX_BLOCKS = 2048;  // per sample: rows of per-workgroup partials in the workspace
constexpr int SM_BLOCK = 256;

static inline bool aligned_to(const void* p, size_t a) { return ((size_t)p & (a - 1)) == 0; }

// grid.x of a pass over `voxels` voxels of each of N samples, W per thread: about 2048 workgroups in all, SM_MAX_BLOCKS per sample at most
static inline unsigned sm_grid(size_t voxels, int W, int N) {
  const size_t need = (voxels / W + SM_BLOCK - 1) / SM_BLOCK;
  size_t cap = 2048 / (size_t)N;
  cap = cap < 1 ? 1 : (cap > SM_MAX_BLOCKS ? SM_MAX_BLOCKS : cap);
  return (unsigned)(need < 1 ? 1 : (need > cap ? cap : need));
}

// W voxels of the K planes starting at voxel group i -> registers
template <int K, int W> DEVI void load_planes(const float* __restrict__ xp, size_t V, size_t i, float (&x)[K][W]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if constexpr (W == 4) {
      const f32x4 v = ((const f32x4*)(xp + (size_t)k * V))[i];
      x[k][0] = v[0]; x[k][1] = v[1]; x[k][2] = v[2]; x[k][3] = v[3];
    } else if constexpr (W == 2) {
      const f32x2 v = ((const f32x2*)(xp + (size_t)k * V))[i];
      x[k][0] = v[0]; x[k][1] = v[1];
    } else {
      x[k][0] = xp[(size_t)k * V + i];
    }
  }
}
template <int K, int W> DEVI void store_planes(float* __restrict__ op, size_t V, size_t i, const float (&o)[K][W]) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if constexpr (W == 4) {
      const f32x4 v = {o[k][0], o[k][1], o[k][2], o[k][3]};
      ((f32x4*)(op + (size_t)k * V))[i] = v;
    } else if constexpr (W == 2) {
      const f32x2 v = {o[k][0], o[k][1]};
      ((f32x2*)(op + (size_t)k * V))[i] = v;
    } else {
      op[(size_t)k * V + i] = o[k][0];
    }
  }
}
// the W labels of voxel group i, one per byte
template <int W> DEVI uint32_t load_labels(const uint8_t* __restrict__ yp, size_t i) {
  if constexpr (W == 4) return ((const uint32_t*)yp)[i];
  else if constexpr (W == 2) return ((const uint16_t*)yp)[i];
  else return yp[i];
}

// v + the value of another lane chosen by a DPP control word, in the rows of row_mask (elsewhere: v + 0)
template <int CTRL, int ROW_MASK> DEVI float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
// the sum over the 64 lanes of a wave, valid in lane 63: six VALU instructions with DPP operands, a fixed order of additions
// (a shuffle per step goes through the LDS crossbar: with 3K + 1 sums per thread that was the larger part of a workgroup's time)
DEVI float wave_sum_lane63(float v) {
  v = dpp_add<0xb1, 0xf>(v);   // quad_perm:[1,0,3,2]
  v = dpp_add<0x4e, 0xf>(v);   // quad_perm:[2,3,0,1]
  v = dpp_add<0x124, 0xf>(v);  // row_ror:4
  v = dpp_add<0x128, 0xf>(v);  // row_ror:8 -- every lane holds the sum of its row of 16
  v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 -- rows 1 and 3 add the row before them
  v = dpp_add<0x143, 0xc>(v);  // row_bcast:31 -- rows 2 and 3 add rows 0 + 1
  return v;
}

// T per-thread sums -> one row of T per workgroup: the lanes of a wave by DPP, the four waves through LDS in wave order
template <int T> DEVI void block_sums(const float (&acc)[T], float* __restrict__ row) {
  __shared__ float sm[SM_BLOCK / 64][T];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const float v = wave_sum_lane63(acc[t]);
    if (lane == 63) sm[wave][t] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < T) {
    float s = sm[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < SM_BLOCK / 64; ++w) s += sm[w][threadIdx.x];
    row[threadIdx.x] = s;
  }
}
