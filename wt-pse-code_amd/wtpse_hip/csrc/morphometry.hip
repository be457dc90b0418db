// Optic-disc morphometry (wtpse_hip/morphometry.py): one more exact integer pass over a (disc, cup) pair of post-processed masks, behind
// wtpse_mask_geometry's record of the disc.
//
//   onh_k : per image the angular profile around the disc's centroid — per sector the largest squared distance and the pixel count of
//           the disc and of the cup — and the second-order sums (y^2, x^2, x y) of both masks, from which the host fits the ellipses.
//           The centre is the disc record's centroid in half-pixel units, so every pixel vector p = (2 x - c2x, c2y - 2 y) is an
//           integer.  A pixel's sector is found without an angle: the signs of p give the quadrant, a binary search over the quadrant's
//           entries of the host's table T (unit vectors scaled by 2^20, rounded; morphometry.sector_table) the sector s with
//           cross(T[s], p) >= 0 > cross(T[s + 1], p), in 64-bit products.  Each wave keeps its own [N][4] record in LDS (a filled disc
//           sends the 64 neighbouring lanes of a wave to a handful of sectors) and updates it with LDS integer atomics: a lane folds
//           the four pixels of its dword in registers while they share a sector; at the end of each dword step the wave groups its
//           lanes by sector, folds a group with lane-xor butterflies and lets one lane send the group's atomics (64 lanes on one LDS
//           address would be served one after the other), for up to four sectors per step; lanes beyond that send their own.  The
//           nonzero entries go out as 32-bit global atomic max / add.
//           The moments fold as geom_k's sums do: 32-bit per lane (16 pixels of at most 2^24 each), lane-xor butterflies in 64 bits,
//           the four waves through LDS, 64-bit atomics.  Maxima and sums of integers: exact and the same on every run.
//           Background costs what it costs geom_k: a dword pair that is zero is skipped, a wave without an object pixel folds nothing.
#include "common.h"

#define ONH_MAXDIM 4096
#define ONH_MAXN 360
#define ONH_ITERS 4                              // dwords per lane and mask
#define ONH_PER_BLOCK (256 * 4 * ONH_ITERS)      // pixels per workgroup

static bool onh_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

__device__ __forceinline__ unsigned long long onh_wave_sum(unsigned long long v) {
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__device__ __forceinline__ long long onh_cross(int2 a, int px, int py) { return (long long)a.x * py - (long long)a.y * px; }

// One wave's record of one sector: {disc_r2 max, cup_r2 max, disc_n, cup_n}.
__device__ __forceinline__ void onh_flush(unsigned* __restrict__ P, int s, unsigned dr2, unsigned cr2, unsigned dn, unsigned cn) {
  unsigned* e = P + 4 * s;
  if (dn) {
    (void)__hip_atomic_fetch_max(e + 0, dr2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    (void)__hip_atomic_fetch_add(e + 2, dn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  if (cn) {
    (void)__hip_atomic_fetch_max(e + 1, cr2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    (void)__hip_atomic_fetch_add(e + 3, cn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// The end of a dword step, reached by every lane of the wave: the lanes' pending records go to the wave's LDS record.  The lanes that
// name the first pending lane's sector are folded with lane-xor butterflies and that lane sends the atomics; this is repeated for up to
// ONH_FOLDS sectors (256 consecutive pixels hold two to four sectors of 24 on average, more near the centre), whoever is left sends its
// own.  Maxima and sums: neither the grouping nor the order matters.
#define ONH_FOLDS 4
__device__ __forceinline__ void onh_wave_flush(unsigned* __restrict__ P, int lane, int& cur, unsigned& dr2, unsigned& cr2, unsigned& dn,
                                               unsigned& cn) {
  bool pend = cur >= 0;
#pragma unroll 1
  for (int it = 0; it < ONH_FOLDS; ++it) {
    const unsigned long long pm = __ballot(pend);
    if (!pm) break;                                                  // uniform over the wave
    const int lead = __ffsll(pm) - 1;
    const int s0 = __shfl(cur, lead, 64);
    const bool mine = pend && cur == s0;
    unsigned a = mine ? dr2 : 0u, b = mine ? cr2 : 0u, c = mine ? dn : 0u, d = mine ? cn : 0u;
    if (__popcll(__ballot(mine)) > 1) {                              // uniform
      for (int m = 1; m < 64; m <<= 1) {
        a = max(a, (unsigned)__shfl_xor(a, m, 64));
        b = max(b, (unsigned)__shfl_xor(b, m, 64));
        c += (unsigned)__shfl_xor(c, m, 64);
        d += (unsigned)__shfl_xor(d, m, 64);
      }
    }
    if (lane == lead) onh_flush(P, s0, a, b, c, d);
    pend = pend && !mine;
  }
  if (pend) onh_flush(P, cur, dr2, cr2, dn, cn);
  cur = -1;
  dr2 = cr2 = dn = cn = 0u;
}

// disc, cup [B][h][w]; geom [B][8] the disc's record; table [N + 1][2]; profile [B][N][4] and moments [B][2][4] zeroed.
// grid (ceil(h * w / ONH_PER_BLOCK), B); dynamic LDS: 4 * N * 4 unsigneds (the waves' records) + (N + 1) int2 (the table).
// VEC: h * w % 4 == 0 and both masks 4-byte aligned (every image then is).
template <int VEC>
__global__ __launch_bounds__(256) void onh_k(const unsigned char* __restrict__ disc, const unsigned char* __restrict__ cup,
                                             const long long* __restrict__ geom, const int* __restrict__ table,
                                             unsigned* __restrict__ profile, long long* __restrict__ moments, int N, int h, int w) {
  extern __shared__ __align__(16) unsigned onh_lds[];
  __shared__ unsigned long long S[4][6];
  __shared__ int C[2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  unsigned* P = onh_lds + wv * N * 4;                                // this wave's record
  const int2* T = reinterpret_cast<const int2*>(onh_lds + 16 * N);   // 64 N bytes in: 8-byte aligned
  const long long* g = geom + (size_t)blockIdx.y * 8;
  const long long area = g[0];
  const bool centred = area > 0;                                     // uniform over the workgroup
  if (centred) {
    for (int e = tid; e < 16 * N; e += 256) onh_lds[e] = 0u;
    for (int e = tid; e < 2 * (N + 1); e += 256) onh_lds[16 * N + e] = (unsigned)table[e];
    if (tid == 0) {
      C[0] = (int)((4 * g[5] + area) / (2 * area));                  // 2 * centroid, rounded half up: at most 2 * 4095
      C[1] = (int)((4 * g[6] + area) / (2 * area));
    }
  }
  __syncthreads();
  const int c2y = centred ? C[0] : 0, c2x = centred ? C[1] : 0;
  const int n = h * w;                                               // <= 2^24
  const unsigned char* md = disc + (size_t)blockIdx.y * n;
  const unsigned char* mc = cup + (size_t)blockIdx.y * n;
  const int base = blockIdx.x * ONH_PER_BLOCK;
  const int nq = N >> 2;
  unsigned m[6] = {0u, 0u, 0u, 0u, 0u, 0u};                          // disc (yy, xx, xy), cup (yy, xx, xy)
  int cur = -1;                                                      // the sector being folded in registers
  unsigned dr2 = 0u, cr2 = 0u, dn = 0u, cn = 0u;
  bool any = false;
#pragma unroll
  for (int k = 0; k < ONH_ITERS; ++k) {
    const int i = base + (k * 256 + tid) * 4;
    unsigned vd = 0u, vc = 0u;
    if (i < n) {
      if (VEC) {
        vd = *reinterpret_cast<const unsigned*>(md + i);             // n % 4 == 0: i + 3 < n
        vc = *reinterpret_cast<const unsigned*>(mc + i);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (i + j < n) {
            vd |= (unsigned)md[i + j] << (8 * j);
            vc |= (unsigned)mc[i + j] << (8 * j);
          }
      }
    }
    if (vd | vc) {                                                   // most of a fundus crop is background
      any = true;
      int y = i / w, x = i - y * w;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool d = (vd >> (8 * j)) & 255u, c = (vc >> (8 * j)) & 255u;
        if (d | c) {
          const unsigned yy = (unsigned)(y * y), xx = (unsigned)(x * x), xy = (unsigned)(x * y);
          if (d) { m[0] += yy; m[1] += xx; m[2] += xy; }
          if (c) { m[3] += yy; m[4] += xx; m[5] += xy; }
          if (centred) {
            const int px = 2 * x - c2x, py = c2y - 2 * y;
            const unsigned r2 = (unsigned)(px * px + py * py);         // < 2^28
            int s = 0;
            if (px | py) {
              const int q = (px > 0 && py >= 0) ? 0 : (px <= 0 && py > 0) ? 1 : (px < 0 && py <= 0) ? 2 : 3;
              int lo = q * nq, hi = lo + nq;                           // cross(T[lo], p) >= 0 > cross(T[hi], p)
              while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (onh_cross(T[mid], px, py) >= 0) lo = mid; else hi = mid;
              }
              s = lo;
            }
            if (s != cur) {
              if (cur >= 0) onh_flush(P, cur, dr2, cr2, dn, cn);
              cur = s; dr2 = cr2 = dn = cn = 0u;
            }
            if (d) { dr2 = max(dr2, r2); ++dn; }
            if (c) { cr2 = max(cr2, r2); ++cn; }
          }
        }
        if (++x == w) { x = 0; ++y; }
      }
    }
    if (centred) onh_wave_flush(P, lane, cur, dr2, cr2, dn, cn);      // every lane of the wave is here
  }
  const bool wave_any = __ballot(any) != 0ull;                       // uniform over the wave
  unsigned long long f[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  if (wave_any) {
#pragma unroll
    for (int k = 0; k < 6; ++k) f[k] = onh_wave_sum(m[k]);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) S[wv][k] = f[k];
  }
  __syncthreads();                                                   // the waves' LDS atomics and S are complete
  if (centred && wave_any) {
    unsigned* o = profile + (size_t)blockIdx.y * N * 4;
    for (int e = lane; e < 4 * N; e += 64) {
      const unsigned v = P[e];
      if (!v) continue;
      if (e & 2) (void)__hip_atomic_fetch_add(o + e, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else (void)__hip_atomic_fetch_max(o + e, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (tid < 6) {
    const unsigned long long v = S[0][tid] + S[1][tid] + S[2][tid] + S[3][tid];
    const int slot = tid < 3 ? tid : tid + 1;                        // the cup's row starts at 4
    if (v) (void)__hip_atomic_fetch_add(moments + (size_t)blockIdx.y * 8 + slot, (long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (centred && blockIdx.x == 0 && tid == 0) {                      // the centre the kernel used: nobody else writes these two
    moments[(size_t)blockIdx.y * 8 + 3] = c2y;
    moments[(size_t)blockIdx.y * 8 + 7] = c2x;
  }
}

// ---- entry point (see include/wtpse_hip.h) -----------------------------------------------------------------------------------
extern "C" int wtpse_onh_profile(const unsigned char* disc, const unsigned char* cup, const long long* geom, const int* table,
                                 unsigned* profile, long long* moments, int N, int B, int h, int w, void* stream) {
  WTPSE_REQUIRE(disc && cup && geom && table && profile && moments);
  WTPSE_REQUIRE(B > 0 && B < 8192 && h >= 1 && w >= 1 && h <= ONH_MAXDIM && w <= ONH_MAXDIM);
  WTPSE_REQUIRE(N >= 8 && N <= ONH_MAXN && (N & 7) == 0);
  WTPSE_REQUIRE(onh_aligned(geom, 8) && onh_aligned(moments, 8) && onh_aligned(table, 4) && onh_aligned(profile, 4));
  const hipStream_t st = (hipStream_t)stream;
  const int n = h * w;
  if (hipMemsetAsync(profile, 0, (size_t)B * N * 4 * sizeof(unsigned), st) != hipSuccess) return wtpse_status();
  if (hipMemsetAsync(moments, 0, (size_t)B * 8 * sizeof(long long), st) != hipSuccess) return wtpse_status();
  const dim3 grid((unsigned)ceil_div(n, ONH_PER_BLOCK), (unsigned)B);
  const size_t lds = (size_t)16 * N * sizeof(unsigned) + (size_t)(N + 1) * 2 * sizeof(int);   // at most 25928 bytes
  if ((n & 3) == 0 && onh_aligned(disc, 4) && onh_aligned(cup, 4))
    hipLaunchKernelGGL(onh_k<1>, grid, dim3(256), lds, st, disc, cup, geom, table, profile, moments, N, h, w);
  else
    hipLaunchKernelGGL(onh_k<0>, grid, dim3(256), lds, st, disc, cup, geom, table, profile, moments, N, h, w);
  return wtpse_status();
}
