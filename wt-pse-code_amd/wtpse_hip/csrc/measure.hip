// Ground-truth-free segmentation outputs (wtpse_hip/segment.py): what is taken from a pair of post-processed masks when there is no
// label to score them against.
//
//   label_map_k : the dataset's grey-level encoding of a (disc, cup) pair — 0 where cup, else 128 where disc, else 255 — the inverse of
//                 label_thresholds_k (csrc/overlay.hip): read back, oc = (cup != 0) and od = ((disc | cup) != 0).  A byte stream.
//   geom_k      : per mask the pixel count, the bounding box and the row / column index sums of the nonzero pixels (the vertical and
//                 horizontal cup-to-disc ratios and the centroids follow on the host, segment.measure).  Integer only: every lane folds
//                 16 pixels, a wave folds its lanes with lane-xor butterflies, a workgroup its four waves through LDS, and one lane
//                 sends the workgroup's seven numbers with 64-bit vector atomics (add, min, max) to the record geom_init_k has set to
//                 the empty mask's values.  Sums, minima and maxima of integers do not depend on the order: the record is exact and
//                 the same on every run; no host synchronisation, so the pair of launches captures in a graph.
//                 Row / column sums pass 2^32 from about 2100 x 2100 pixels: they are 64-bit from the wave fold on (a lane's own
//                 16 pixels stay below 2^17).
#include "common.h"

#define GEO_MAXDIM 4096
#define GEO_ITERS 4                              // dwords per lane
#define GEO_PER_BLOCK (256 * 4 * GEO_ITERS)      // pixels per workgroup

static bool ms_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static unsigned ms_stream_blocks(long long items) {                // a memory-bound pass: at most 2048 workgroups, grid-stride the rest
  const long long nb = (items + 255) / 256;
  return (unsigned)(nb < 1 ? 1 : nb > 2048 ? 2048 : nb);
}

template <int VEC>
__global__ __launch_bounds__(256) void label_map_k(const unsigned char* __restrict__ disc, const unsigned char* __restrict__ cup,
                                                   unsigned char* __restrict__ out, long long n) {
  const long long step = (long long)gridDim.x * 256;
  if (VEC) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n / 4; i += step) {
      const unsigned d = reinterpret_cast<const unsigned*>(disc)[i], c = reinterpret_cast<const unsigned*>(cup)[i];
      unsigned v = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) v |= (((c >> (8 * k)) & 255u) ? 0u : ((d >> (8 * k)) & 255u) ? 128u : 255u) << (8 * k);
      reinterpret_cast<unsigned*>(out)[i] = v;
    }
  } else {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step)
      out[i] = cup[i] ? (unsigned char)0 : disc[i] ? (unsigned char)128 : (unsigned char)255;
  }
}

// rec [B][8] int64 = {area, top, bottom, left, right, sum_r, sum_c, 0}: the empty mask's record
__global__ __launch_bounds__(256) void geom_init_k(long long* __restrict__ rec, int B, int h, int w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * 8) return;
  const int f = i & 7;
  rec[i] = f == 1 ? (long long)h : f == 3 ? (long long)w : (f == 2 || f == 4) ? -1ll : 0ll;
}

__device__ __forceinline__ int wave_min_i(int v) {
  for (int m = 1; m < 64; m <<= 1) v = min(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
  for (int m = 1; m < 64; m <<= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// mask [B][h][w]; grid (ceil(h * w / GEO_PER_BLOCK), B).  VEC: h * w % 4 == 0 and mask 4-byte aligned (every image then is).
template <int VEC>
__global__ __launch_bounds__(256) void geom_k(const unsigned char* __restrict__ mask, long long* __restrict__ rec, int h, int w) {
  __shared__ unsigned long long S[4][3];
  __shared__ int Q[4][4];
  const int n = h * w;                                             // <= 2^24
  const unsigned char* m = mask + (size_t)blockIdx.y * n;
  const int base = blockIdx.x * GEO_PER_BLOCK;
  unsigned area = 0u, sr = 0u, sc = 0u;
  int top = h, bottom = -1, left = w, right = -1;
#pragma unroll
  for (int k = 0; k < GEO_ITERS; ++k) {
    const int i = base + (k * 256 + (int)threadIdx.x) * 4;
    if (i >= n) break;
    unsigned v = 0u;
    if (VEC) {
      v = *reinterpret_cast<const unsigned*>(m + i);               // n % 4 == 0: i + 3 < n
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j < n) v |= (unsigned)m[i + j] << (8 * j);
    }
    if (!v) continue;
    int y = i / w, x = i - y * w;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if ((v >> (8 * j)) & 255u) {
        ++area;
        top = min(top, y); bottom = max(bottom, y);
        left = min(left, x); right = max(right, x);
        sr += (unsigned)y; sc += (unsigned)x;
      }
      if (++x == w) { x = 0; ++y; }
    }
  }
  const unsigned long long a64 = wave_sum_u64(area), r64 = wave_sum_u64(sr), c64 = wave_sum_u64(sc);
  top = wave_min_i(top); left = wave_min_i(left);
  bottom = wave_max_i(bottom); right = wave_max_i(right);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    S[wv][0] = a64; S[wv][1] = r64; S[wv][2] = c64;
    Q[wv][0] = top; Q[wv][1] = bottom; Q[wv][2] = left; Q[wv][3] = right;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long a = 0ull, r = 0ull, c = 0ull;
    int t = h, b = -1, l = w, g = -1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a += S[k][0]; r += S[k][1]; c += S[k][2];
      t = min(t, Q[k][0]); b = max(b, Q[k][1]); l = min(l, Q[k][2]); g = max(g, Q[k][3]);
    }
    if (a) {
      long long* o = rec + (size_t)blockIdx.y * 8;
      (void)__hip_atomic_fetch_add(o + 0, (long long)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_min(o + 1, (long long)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_max(o + 2, (long long)b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_min(o + 3, (long long)l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_max(o + 4, (long long)g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_add(o + 5, (long long)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      (void)__hip_atomic_fetch_add(o + 6, (long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---- entry points (see include/wtpse_hip.h) ------------------------------------------------------------------------------
extern "C" int wtpse_label_map(const unsigned char* disc, const unsigned char* cup, unsigned char* out, long long n, void* stream) {
  WTPSE_REQUIRE(disc && cup && out && n > 0);
  const hipStream_t st = (hipStream_t)stream;
  if ((n & 3) == 0 && ms_aligned(disc, 4) && ms_aligned(cup, 4) && ms_aligned(out, 4))
    hipLaunchKernelGGL(label_map_k<1>, dim3(ms_stream_blocks(n / 4)), dim3(256), 0, st, disc, cup, out, n);
  else
    hipLaunchKernelGGL(label_map_k<0>, dim3(ms_stream_blocks(n)), dim3(256), 0, st, disc, cup, out, n);
  return wtpse_status();
}

extern "C" int wtpse_mask_geometry(const unsigned char* mask, long long* rec, int B, int h, int w, void* stream) {
  WTPSE_REQUIRE(mask && rec && B > 0 && B < 8192 && h >= 1 && w >= 1 && h <= GEO_MAXDIM && w <= GEO_MAXDIM && ms_aligned(rec, 8));
  const hipStream_t st = (hipStream_t)stream;
  const int n = h * w;
  hipLaunchKernelGGL(geom_init_k, dim3((unsigned)ceil_div(B * 8, 256)), dim3(256), 0, st, rec, B, h, w);
  const dim3 grid((unsigned)ceil_div(n, GEO_PER_BLOCK), (unsigned)B);
  if ((n & 3) == 0 && ms_aligned(mask, 4))
    hipLaunchKernelGGL(geom_k<1>, grid, dim3(256), 0, st, mask, rec, h, w);
  else
    hipLaunchKernelGGL(geom_k<0>, grid, dim3(256), 0, st, mask, rec, h, w);
  return wtpse_status();
}
