// Prediction entropy per image (plane) and its gradient: the objective of test-time entropy minimisation (TENT / EATA's filter).
// Specification: wtpse_hip/tent.py (entropy_planes_host / tent_loss_host / tent_grad_host).
//
// Per plane b of hw elements, z = x m, e = exp(-|z|):  h(z) = log1p(e) + |z| e / (1 + e),  h'(z) = -z e / (1 + e)^2,
// M_b = sum m, H_b = (sum m h) / M_b (0 where M_b = 0), c_b = [M_b > 0 and H_b < margin], w_b = exp(margin - H_b) or 1;
// the loss is (1 / B) sum_b c_b w_b H_b and dL/dx_i = (c_b w_b / (B M_b)) m_i^2 h'(z_i).
//   ent_sums_k   grid (blocks per plane, B): a workgroup owns one contiguous chunk of one plane and writes the fp64 partials of
//                sum m h, sum m to partial[b][block][2].
//   ent_apply_k  same grid: every workgroup folds its plane's partials in block order (all workgroups of a plane hold identical
//                bits), derives H_b, c_b, w_b and WRITES its chunk of dx: fp64 arithmetic, rounded once; every element is written,
//                an unselected plane gets +0.0.  Workgroup 0 stores H_b, c_b and the plane's term c_b w_b H_b.
//   ent_fold_k   one thread: the terms added in plane order in fp64, times 1 / B, rounded once.
// Both passes walk a chunk in groups of four consecutive elements exactly as csrc/overlap.hip does, group k of a round on thread k,
// a group's elements added in index order: one 16-byte load where the plane's bases are 16-byte aligned, four guarded 4-byte loads
// otherwise and in the ragged last group — the SAME order of additions either way, so a plane's bits do not depend on where in the
// batch it lies.  The wave is folded by shuffles, the workgroup's four waves in wave order.  No atomics anywhere in this file.
#include "common.h"

#define ENT_CHUNK 4096        // elements of a plane per workgroup, at least
#define ENT_MAXBLK 32         // workgroups per plane, at most

// workgroups per plane: a function of hw alone, never of B (a plane's partials and their order must not depend on the batch)
static int ent_blocks(int hw) {
  const int nb = ceil_div(hw, ENT_CHUNK);
  return nb < 1 ? 1 : nb > ENT_MAXBLK ? ENT_MAXBLK : nb;
}
// (hw <= 2^30: the kernels' int element indices run up to hw + one round of the workgroup)
static bool ent_dims_ok(int B, int hw) { return B > 0 && B < 65536 && hw > 0 && hw <= (1 << 30) && (long long)B * hw <= 0x7fffffffLL; }
// elements per chunk: a multiple of four, so that every chunk of an aligned plane starts aligned
static int ent_chunk(int hw) { return ceil_div(ceil_div(hw, ent_blocks(hw)), 4) * 4; }

__device__ __forceinline__ bool ent_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// four consecutive elements at p[i .. i + 3]; those at or behind `end` read as `fill`
__device__ __forceinline__ void ent_load4(const float* __restrict__ p, int i, int end, bool vec, float fill, float v[4]) {
  if (vec && i + 4 <= end) {
    const float4 q = *reinterpret_cast<const float4*>(p + i);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = i + u < end ? p[i + u] : fill;
  }
}

__global__ __launch_bounds__(256) void ent_sums_k(const float* __restrict__ x, const float* __restrict__ m, int hw, int chunk,
                                                  double* __restrict__ partial) {
  __shared__ double sh[4][2];
  const size_t base = (size_t)blockIdx.y * hw;
  const float* xp = x + base;
  const float* mp = m ? m + base : nullptr;
  const bool vec = ent_aligned(xp) && (!mp || ent_aligned(mp));
  const int c0 = blockIdx.x * chunk, c1 = min(hw, c0 + chunk);
  double a_h = 0.0, a_m = 0.0;
  for (int i = c0 + 4 * (int)threadIdx.x; i < c1; i += 1024) {
    float xv[4], mv[4] = {1.f, 1.f, 1.f, 1.f};
    ent_load4(xp, i, c1, vec, 0.f, xv);
    if (mp) ent_load4(mp, i, c1, vec, 0.f, mv);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i + u < c1) {
        const double mi = (double)mv[u], z = (double)xv[u] * mi, az = fabs(z);
        const double e = exp(-az), r = 1.0 / (1.0 + e);
        a_h += mi * (log1p(e) + az * e * r);
        a_m += mi;
      }
    }
  }
  for (int k = 1; k <= 32; k <<= 1) {
    a_h += __shfl_xor(a_h, k, 64);
    a_m += __shfl_xor(a_m, k, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6][0] = a_h;
    sh[threadIdx.x >> 6][1] = a_m;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int j = threadIdx.x;
    partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 + j] = ((sh[0][j] + sh[1][j]) + sh[2][j]) + sh[3][j];
  }
}

__global__ __launch_bounds__(256) void ent_apply_k(const float* __restrict__ x, const float* __restrict__ m, int B, int hw, int chunk,
                                                   double margin, int reweight, const double* __restrict__ partial,
                                                   double* __restrict__ term, float* __restrict__ planes, int* __restrict__ selected,
                                                   float* __restrict__ dx) {
  // the plane's two sums: every thread of every workgroup of the plane adds the same numbers in the same (block) order
  const double* P = partial + (size_t)blockIdx.y * gridDim.x * 2;
  double p_h = 0.0, p_m = 0.0;
  for (unsigned k = 0; k < gridDim.x; ++k) {
    p_h += P[2 * k];
    p_m += P[2 * k + 1];
  }
  const bool some = p_m > 0.0;
  const double H = some ? p_h / p_m : 0.0;
  const bool sel = some && H < margin;                 // (a NaN or +inf plane fails `<`)
  const double w = (reweight && margin < INFINITY) ? exp(margin - H) : 1.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    planes[blockIdx.y] = (float)H;
    selected[blockIdx.y] = sel ? 1 : 0;
    term[blockIdx.y] = sel ? w * H : 0.0;
  }
  if (!dx) return;
  const double K = sel ? w / ((double)B * p_m) : 0.0;

  const size_t base = (size_t)blockIdx.y * hw;
  const float* xp = x + base;
  const float* mp = m ? m + base : nullptr;
  float* dp = dx + base;
  const bool vec = ent_aligned(xp) && (!mp || ent_aligned(mp)) && ent_aligned(dp);
  const int c0 = blockIdx.x * chunk, c1 = min(hw, c0 + chunk);
  for (int i = c0 + 4 * (int)threadIdx.x; i < c1; i += 1024) {
    float dv[4] = {0.f, 0.f, 0.f, 0.f};
    if (sel) {
      float xv[4], mv[4] = {1.f, 1.f, 1.f, 1.f};
      ent_load4(xp, i, c1, vec, 0.f, xv);
      if (mp) ent_load4(mp, i, c1, vec, 0.f, mv);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double mi = (double)mv[q], z = (double)xv[q] * mi;
        const double e = exp(-fabs(z)), r = 1.0 / (1.0 + e);
        dv[q] = (float)(K * (mi * mi) * (-z * (e * r * r)));
      }
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

__global__ void ent_fold_k(const double* __restrict__ term, int B, float* __restrict__ loss) {
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += term[b];
  *loss = (float)(s / (double)B);
}

// ================================================================================================ C ABI
// workspace: fp64 partials [B][blocks][2], fp64 terms [B], then B fp32 plane entropies and B int32 selections (used when the
// caller does not want them)
extern "C" int wtpse_entropy_loss_ws(int B, int hw) {
  if (!ent_dims_ok(B, hw)) return -1;
  const long long bytes = (long long)B * ent_blocks(hw) * 2 * 8 + (long long)B * 8 + (long long)B * 8;
  return bytes > 0x7fffffffLL ? -1 : (int)bytes;
}

extern "C" int wtpse_entropy_loss(const float* x, const float* mask, int B, int hw, double margin, int reweight, void* ws,
                                  float* planes, int* selected, float* loss, float* dx, void* stream) {
  WTPSE_REQUIRE(x && ws && loss && wtpse_entropy_loss_ws(B, hw) > 0);
  WTPSE_REQUIRE(margin == margin && margin > 0.0);          // a number, positive; +inf: every plane with M_b > 0 is selected
  WTPSE_REQUIRE((((uintptr_t)ws) & 7) == 0);
  const int nb = ent_blocks(hw), chunk = ent_chunk(hw);
  double* partial = (double*)ws;
  double* term = partial + (size_t)B * nb * 2;
  if (!planes) planes = (float*)(term + B);
  if (!selected) selected = (int*)(term + B) + B;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)nb, (unsigned)B);
  hipLaunchKernelGGL(ent_sums_k, grid, dim3(256), 0, st, x, mask, hw, chunk, partial);
  hipLaunchKernelGGL(ent_apply_k, grid, dim3(256), 0, st, x, mask, B, hw, chunk, margin, reweight ? 1 : 0, (const double*)partial, term,
                     planes, selected, dx);
  hipLaunchKernelGGL(ent_fold_k, dim3(1), dim3(1), 0, st, (const double*)term, B, loss);
  return wtpse_status();
}
