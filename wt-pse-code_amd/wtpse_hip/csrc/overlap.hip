// Soft Dice / Tversky / focal Tversky overlap loss per image (plane) and its gradient added into the region loss's.
// Specification: wtpse_hip/overlap.py (overlap_planes_host / overlap_loss_host / overlap_grad_host).
//
// Per plane b of hw elements, z = x m, s = sigmoid(z):  TP = sum m s t, FP = sum m s - TP, FN = sum m t - TP,
// TI = (TP + eps) / (TP + a FP + b FN + eps), L_b = (1 - TI)^g; the loss is the mean of L_b over the planes.
//   ov_sums_k   grid (blocks per plane, B): a workgroup owns one contiguous chunk of one plane and writes the fp64 partials of
//               sum m s t, sum m s, sum m t to partial[b][block][3].
//   ov_apply_k  same grid: every workgroup folds its plane's partials in block order (all workgroups of a plane hold identical
//               bits), derives TI, L_b and the two coefficients of the gradient — which is affine in t_i:
//                   d(w L)/dx_i = (A0 + A1 t_i) m_i^2 s_i (1 - s_i),
//                   A0 = -K a N / D^2,  A1 = K (D - N (1 - a - b)) / D^2,  K = (w / B) (-g (1 - TI)^(g - 1))
//               and adds it into its chunk of dx: fp64 arithmetic, rounded once on the add.  Workgroup 0 stores L_b.
// Both passes walk a chunk in groups of four consecutive elements, group k of a round on thread k, and add a group's elements in
// index order: a plane whose four bases are 16-byte aligned loads a group with one 16-byte load, any other plane (33 x 65 floats:
// every odd plane) and the ragged last group with four guarded 4-byte loads — the SAME order of additions either way, so a plane's
// bits do not depend on where in the batch it lies.  s and s (1 - s) come from e = exp(-|z|) in fp64 as in bd_loss_k.
// The wave is folded by shuffles, the workgroup's four waves in wave order.  No atomics anywhere in this file.
#include "common.h"

#define OV_CHUNK 4096        // elements of a plane per workgroup, at least
#define OV_MAXBLK 32         // workgroups per plane, at most

// workgroups per plane: a function of hw alone, never of B (a plane's partials and their order must not depend on the batch)
static int ov_blocks(int hw) {
  const int nb = ceil_div(hw, OV_CHUNK);
  return nb < 1 ? 1 : nb > OV_MAXBLK ? OV_MAXBLK : nb;
}
// (hw <= 2^30: the kernels' int element indices run up to hw + one round of the workgroup)
static bool ov_dims_ok(int B, int hw) { return B > 0 && B < 65536 && hw > 0 && hw <= (1 << 30) && (long long)B * hw <= 0x7fffffffLL; }
// elements per chunk: a multiple of four, so that every chunk of an aligned plane starts aligned
static int ov_chunk(int hw) { return ceil_div(ceil_div(hw, ov_blocks(hw)), 4) * 4; }

__device__ __forceinline__ bool ov_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// four consecutive elements at p[i .. i + 3]; those at or behind `end` read as `fill`
__device__ __forceinline__ void ov_load4(const float* __restrict__ p, int i, int end, bool vec, float fill, float v[4]) {
  if (vec && i + 4 <= end) {
    const float4 q = *reinterpret_cast<const float4*>(p + i);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = i + u < end ? p[i + u] : fill;
  }
}

__global__ __launch_bounds__(256) void ov_sums_k(const float* __restrict__ x, const float* __restrict__ m, const float* __restrict__ t,
                                                 int hw, int chunk, double* __restrict__ partial) {
  __shared__ double sh[4][3];
  const size_t base = (size_t)blockIdx.y * hw;
  const float* xp = x + base;
  const float* tp = t + base;
  const float* mp = m ? m + base : nullptr;
  const bool vec = ov_aligned(xp) && ov_aligned(tp) && (!mp || ov_aligned(mp));
  const int c0 = blockIdx.x * chunk, c1 = min(hw, c0 + chunk);
  double a_st = 0.0, a_s = 0.0, a_t = 0.0;
  for (int i = c0 + 4 * (int)threadIdx.x; i < c1; i += 1024) {
    float xv[4], tv[4], mv[4] = {1.f, 1.f, 1.f, 1.f};
    ov_load4(xp, i, c1, vec, 0.f, xv);
    ov_load4(tp, i, c1, vec, 0.f, tv);
    if (mp) ov_load4(mp, i, c1, vec, 0.f, mv);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i + u < c1) {
        const double mi = (double)mv[u], ti = (double)tv[u], z = (double)xv[u] * mi;
        const double e = exp(-fabs(z)), r = 1.0 / (1.0 + e);
        const double ms = mi * (z >= 0.0 ? r : e * r);
        a_st += ms * ti;
        a_s += ms;
        a_t += mi * ti;
      }
    }
  }
  for (int k = 1; k <= 32; k <<= 1) {
    a_st += __shfl_xor(a_st, k, 64);
    a_s += __shfl_xor(a_s, k, 64);
    a_t += __shfl_xor(a_t, k, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6][0] = a_st;
    sh[threadIdx.x >> 6][1] = a_s;
    sh[threadIdx.x >> 6][2] = a_t;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int j = threadIdx.x;
    partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + j] = ((sh[0][j] + sh[1][j]) + sh[2][j]) + sh[3][j];
  }
}

__global__ __launch_bounds__(256) void ov_apply_k(const float* __restrict__ x, const float* __restrict__ m, const float* __restrict__ t,
                                                  const float* __restrict__ w_dev, int B, int hw, int chunk, double a, double b,
                                                  double g, double eps, const double* __restrict__ partial,
                                                  float* __restrict__ plane_loss, float* __restrict__ dx) {
  // the plane's three sums: every thread of every workgroup of the plane adds the same numbers in the same (block) order
  const double* P = partial + (size_t)blockIdx.y * gridDim.x * 3;
  double p_st = 0.0, p_s = 0.0, p_t = 0.0;
  for (unsigned k = 0; k < gridDim.x; ++k) {
    p_st += P[3 * k];
    p_s += P[3 * k + 1];
    p_t += P[3 * k + 2];
  }
  const double N = p_st + eps, D = p_st + a * (p_s - p_st) + b * (p_t - p_st) + eps;
  const double u = 1.0 - N / D;
  const bool zero = u <= 0.0;                        // decided before any power is taken (a NaN is not <= 0 and goes through)
  if (blockIdx.x == 0 && threadIdx.x == 0) plane_loss[blockIdx.y] = zero ? 0.f : (float)(g == 1.0 ? u : pow(u, g));
  if (!dx || zero) return;
  const double K = ((double)*w_dev / (double)B) * (-g * (g == 1.0 ? 1.0 : pow(u, g - 1.0)));
  const double A0 = -K * a * N / (D * D), A1 = K * (D - N * (1.0 - a - b)) / (D * D);

  const size_t base = (size_t)blockIdx.y * hw;
  const float* xp = x + base;
  const float* tp = t + base;
  const float* mp = m ? m + base : nullptr;
  float* dp = dx + base;
  const bool vec = ov_aligned(xp) && ov_aligned(tp) && (!mp || ov_aligned(mp)) && ov_aligned(dp);
  const int c0 = blockIdx.x * chunk, c1 = min(hw, c0 + chunk);
  for (int i = c0 + 4 * (int)threadIdx.x; i < c1; i += 1024) {
    float xv[4], tv[4], dv[4], mv[4] = {1.f, 1.f, 1.f, 1.f};
    ov_load4(xp, i, c1, vec, 0.f, xv);
    ov_load4(tp, i, c1, vec, 0.f, tv);
    if (mp) ov_load4(mp, i, c1, vec, 0.f, mv);
    ov_load4(dp, i, c1, vec, 0.f, dv);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double mi = (double)mv[q], z = (double)xv[q] * mi;
      const double e = exp(-fabs(z)), r = 1.0 / (1.0 + e);
      const double inc = (A0 + A1 * (double)tv[q]) * (mi * mi) * (e * r * r);
      // an increment of zero (weight 0, mask 0) leaves the stored bits alone, a -0.0 included
      if (inc != 0.0) dv[q] = (float)((double)dv[q] + inc);
    }
    if (vec && i + 4 <= c1) {
      *reinterpret_cast<float4*>(dp + i) = make_float4(dv[0], dv[1], dv[2], dv[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (i + q < c1) dp[i + q] = dv[q];
    }
  }
}

// ================================================================================================ C ABI
extern "C" int wtpse_overlap_loss_ws(int B, int hw) {
  if (!ov_dims_ok(B, hw)) return -1;
  const long long bytes = (long long)B * ov_blocks(hw) * 3 * 8 + (long long)B * 4;      // fp64 partials, then B fp32 plane losses
  return bytes > 0x7fffffffLL ? -1 : (int)bytes;
}

extern "C" int wtpse_overlap_loss(const float* x, const float* mask, const float* t, const float* w_dev, int B, int hw, float fp,
                                  float fn, float focal, float smooth, void* ws, float* plane_loss, float* loss, float* dx,
                                  void* stream) {
  WTPSE_REQUIRE(x && t && ws && loss && wtpse_overlap_loss_ws(B, hw) > 0 && (!dx || w_dev));
  WTPSE_REQUIRE(fp >= 0.f && fn >= 0.f && fp + fn > 0.f && focal > 0.f && smooth > 0.f);
  WTPSE_REQUIRE(fp + fn < INFINITY && focal < INFINITY && smooth < INFINITY);
  WTPSE_REQUIRE((((uintptr_t)ws) & 7) == 0);
  const int nb = ov_blocks(hw), chunk = ov_chunk(hw);
  double* partial = (double*)ws;
  if (!plane_loss) plane_loss = (float*)(partial + (size_t)B * nb * 3);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)nb, (unsigned)B);
  hipLaunchKernelGGL(ov_sums_k, grid, dim3(256), 0, st, x, mask, t, hw, chunk, partial);
  hipLaunchKernelGGL(ov_apply_k, grid, dim3(256), 0, st, x, mask, t, w_dev, B, hw, chunk, (double)fp, (double)fn, (double)focal,
                     (double)smooth, (const double*)partial, plane_loss, dx);
  return wtpse_reduce_rows(plane_loss, B, 1, loss, 0, 1.f / (float)B, stream);
}
