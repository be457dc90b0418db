// Boundary loss (Kervadec et al., MIDL 2019) on the device: the signed distance map phi of a batch of label planes — an exact
// Euclidean distance transform of the foreground AND of the background from one read of the label — and the loss
// mean(sigmoid(logit) * phi) with its gradient added into the region loss's.  Specification: wtpse_hip/boundary.py
// (signed_distance_host / boundary_loss_host / boundary_grad_host).
//
// The transform is separable and exact in integers (the two-pass scheme of postprocess.hip's met_col_k / met_row_k, here for
// every pixel instead of the surface pixels only):
//   bd_col_k   one thread per column, two sweeps: G = g_out | g_in << 16, the vertical distance to the nearest member /
//              non-member of the column (BD_NONE: the column has none).  Lanes run along a row, so every access coalesces; the
//              loads of eight rows are issued together (a sweep is a chain of h dependent steps otherwise), and 64-thread
//              workgroups spread the few columns of a training batch (64 planes x 256) over all CUs.  The upward sweep reads G
//              alone: g == 0 already says which set the pixel belongs to.
//   bd_row_k   one workgroup per (row, plane): the row's G staged in LDS (consecutive lanes read consecutive words: no bank
//              conflict), then per pixel min over q of (x - q)^2 + g(q)^2 by an outward scan that stops once (x - q)^2 >= best —
//              exact, and on wave64 far cheaper than a serial lower-envelope pass: the lanes of a wave are neighbours, their
//              scans have almost the same length.  A pixel needs ONE scan: a member's distance to the members is 0, a
//              non-member's to the non-members is 0.
// A plane without a contour (empty or full: phi = 0 by definition) is recognised in the row pass itself: a column whose g_out is
// BD_NONE has no member in ANY row, so "some column of this row has a member above or below" is the same answer in every row of
// the plane — one workgroup-wide OR over the staged row, no counter, no atomic, no host read.
// sqrt runs in fp64 on the exact integer (correctly rounded, and float(sqrt_fp64) of an integer below 2^26 IS the correctly rounded
// fp32 root: 53 >= 2 * 24 + 2), so phi equals float32(float64 specification) bit for bit.  No atomics anywhere in this file.
#include "common.h"

#define BD_MAXDIM 4096
#define BD_NONE 0xFFFFu

static bool bd_dims_ok(int B, int h, int w) {
  return B > 0 && B < 65536 && h > 0 && w > 0 && h <= BD_MAXDIM && w <= BD_MAXDIM && (long long)B * h * w <= 0x7fffffffLL;
}

__global__ __launch_bounds__(64) void bd_col_k(const float* __restrict__ t, unsigned* __restrict__ G, int h, int w) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= w) return;
  const size_t base = (size_t)blockIdx.y * h * w + x;
  int lp = -1, ln = -1;                                            // last member / non-member row above
  for (int y0 = 0; y0 < h; y0 += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = t[base + (size_t)min(y0 + u, h - 1) * w];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int y = y0 + u;
      if (y < h) {
        if (v[u] != 0.f) lp = y; else ln = y;
        G[base + (size_t)y * w] = (lp < 0 ? BD_NONE : (unsigned)(y - lp)) | ((ln < 0 ? BD_NONE : (unsigned)(y - ln)) << 16);
      }
    }
  }
  lp = ln = -1;                                                    // next member / non-member row below
  for (int y1 = h - 1; y1 >= 0; y1 -= 8) {
    unsigned g[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) g[u] = G[base + (size_t)max(y1 - u, 0) * w];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int y = y1 - u;
      if (y >= 0) {
        unsigned go = g[u] & 0xFFFFu, gi = g[u] >> 16;
        if (go == 0) lp = y; else ln = y;                          // (exactly one of the two is 0: the pixel's own set)
        if (lp >= 0 && (unsigned)(lp - y) < go) go = (unsigned)(lp - y);
        if (ln >= 0 && (unsigned)(ln - y) < gi) gi = (unsigned)(ln - y);
        G[base + (size_t)y * w] = go | (gi << 16);
      }
    }
  }
}

// min over q of (x - q)^2 + g(q)^2 on one row (g = the 16-bit half `sh` of G); the caller knows that some column has a finite g.
__device__ __forceinline__ int bd_row_min(const unsigned* G, int x, int w, int sh) {
  int best = 0x7fffffff;
  for (int r = 0;; ++r) {
    const int r2 = r * r;
    if (r2 >= best) break;
    const bool lo = x - r >= 0, hi = r > 0 && x + r < w;
    if (!lo && !hi) break;
    if (lo) {
      const unsigned g = (G[x - r] >> sh) & 0xFFFFu;
      if (g != BD_NONE) best = min(best, r2 + (int)(g * g));
    }
    if (hi) {
      const unsigned g = (G[x + r] >> sh) & 0xFFFFu;
      if (g != BD_NONE) best = min(best, r2 + (int)(g * g));
    }
  }
  return best;
}

__global__ __launch_bounds__(256) void bd_row_k(const unsigned* __restrict__ Gg, float* __restrict__ phi, int* __restrict__ d2_out,
                                                int* __restrict__ d2_in, int h, int w) {
  __shared__ unsigned G[BD_MAXDIM];
  const size_t row = ((size_t)blockIdx.y * h + blockIdx.x) * w;
  int has_out = 0, has_in = 0;
  for (int x = threadIdx.x; x < w; x += 256) {
    const unsigned g = Gg[row + x];
    G[x] = g;
    has_out |= (g & 0xFFFFu) != BD_NONE;
    has_in |= (g >> 16) != BD_NONE;
  }
  has_out = __syncthreads_or(has_out);                             // (a barrier: G is staged behind it)
  has_in = __syncthreads_or(has_in);
  const bool contour = has_out && has_in;
  for (int x = threadIdx.x; x < w; x += 256) {
    const bool pos = (G[x] & 0xFFFFu) == 0;
    // a member's distance to the members is 0, a non-member's to the non-members; the other one is the scan, or -1 for "no such pixel"
    const int d = contour ? bd_row_min(G, x, w, pos ? 16 : 0) : -1;
    float f = 0.f;
    if (contour) f = pos ? (float)(1.0 - sqrt((double)d)) : (float)sqrt((double)d);
    phi[row + x] = f;
    if (d2_out) d2_out[row + x] = pos ? 0 : d;
    if (d2_in) d2_in[row + x] = pos ? d : 0;
  }
}

// sum over the workgroup's elements of sigmoid(x m) phi into partial[block] (fp64 inside the workgroup, folded in a fixed order) and,
// with dx, dx += alpha / n * phi * s (1 - s) * m.  s and s (1 - s) come from e = exp(-|z|) in fp64: 1 - s in fp32 loses every digit
// the increment has where the network is confident (|z| ~ 10), which is where phi is large.
__global__ __launch_bounds__(256) void bd_loss_k(const float* __restrict__ x, const float* __restrict__ m, const float* __restrict__ phi,
                                                 const float* __restrict__ alpha_dev, long long n, float* __restrict__ partial,
                                                 float* __restrict__ dx) {
  __shared__ double sh[4];
  const double a = dx ? (double)*alpha_dev / (double)n : 0.0;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double mi = m ? (double)m[i] : 1.0;
    const double z = (double)x[i] * mi, p = (double)phi[i];
    const double e = exp(-fabs(z)), r = 1.0 / (1.0 + e);
    const double s = z >= 0.0 ? r : e * r;
    acc += s * p;
    if (dx) dx[i] += (float)(a * p * (e * r * r) * mi);
  }
  for (int k = 1; k <= 32; k <<= 1) acc += __shfl_xor(acc, k, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (float)(((sh[0] + sh[1]) + sh[2]) + sh[3]);
}

// ================================================================================================ C ABI
extern "C" int wtpse_signed_distance_ws(int B, int h, int w) {
  if (!bd_dims_ok(B, h, w)) return -1;
  return (int)((long long)B * h * w);
}

extern "C" int wtpse_signed_distance(const float* t, float* phi, int* d2_out, int* d2_in, void* ws, int B, int h, int w, void* stream) {
  WTPSE_REQUIRE(t && phi && ws && wtpse_signed_distance_ws(B, h, w) > 0);
  unsigned* G = (unsigned*)ws;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bd_col_k, dim3((unsigned)ceil_div(w, 64), (unsigned)B), dim3(64), 0, st, t, G, h, w);
  hipLaunchKernelGGL(bd_row_k, dim3((unsigned)h, (unsigned)B), dim3(256), 0, st, G, phi, d2_out, d2_in, h, w);
  return wtpse_status();
}

extern "C" int wtpse_boundary_loss(const float* x, const float* mask, const float* phi, const float* alpha_dev, long long n,
                                   float* partial, float* loss, float* dx, void* stream) {
  WTPSE_REQUIRE(x && phi && partial && loss && n > 0 && (!dx || alpha_dev));
  const int nb = wtpse_reduce_blocks(n);
  hipLaunchKernelGGL(bd_loss_k, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, mask, phi, alpha_dev, n, partial, dx);
  return wtpse_reduce_rows(partial, nb, 1, loss, 0, 1.f / (float)n, stream);
}
