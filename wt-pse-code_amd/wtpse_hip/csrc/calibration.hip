// Calibration against labels (wtpse_hip/calibration.py): one exact integer pass over a probability map, a spread map and a label that
// leaves, per image, the sufficient statistic of every calibration number the host forms in float64.
//
//   cal_hist_k : per image the record of include/wtpse_hip.h — hist_p[q][y], the labels per quantised probability; hist_s[u][e], right and
//           wrong pixels per quantised spread; tail[4], the pixels that were not scored and the number that were.  A lane owns one pixel
//           per step (no alignment or width premise: native label sizes are odd), CAL_ITERS steps per workgroup.  The workgroup keeps ONE
//           record in LDS (16 416 bytes, static) and updates it with LDS integer atomics.  The input is their worst case: most of a
//           fundus crop is background with q = 0 and u = 0, whole waves share one key, and 64 lanes on one LDS address are served one
//           after the other.  So the wave folds before it adds: the lanes that name the first pending lane's key are counted with a
//           ballot and that lane sends ONE atomic with the popcount (a wave-uniform key — the first lane's key, then the ballot — is
//           the first round of this and ends it); this is repeated for up to CAL_FOLDS keys (a row through a disc's edge holds 0, the
//           ramp's few values and 1), whoever is left sends its own.  The tail's four counts never touch LDS per pixel: they are
//           ballot popcounts kept in a wave-uniform register.  At the end the workgroup sends its nonzero slots as 32-bit global
//           atomic adds.  Sums of integers: neither the grouping nor the order matters — exact and the same on every run.
#include "common.h"

#define CAL_MAXDIM 4096
#define CAL_BINS WTPSE_CAL_BINS
#define CAL_REC WTPSE_CAL_REC
#define CAL_HS (2 * (CAL_BINS + 1))              // where hist_s starts in a record
#define CAL_TAIL (4 * (CAL_BINS + 1))            // where tail starts
#define CAL_ITERS 32                             // pixels per lane
#define CAL_UNROLL 4                             // of which this many have their loads in flight together
#define CAL_PER_BLOCK (256 * CAL_ITERS)          // pixels per workgroup
#define CAL_FOLDS 6

static_assert(CAL_REC == CAL_TAIL + 4, "hist_p[BINS + 1][2], hist_s[BINS + 1][2], tail[4]");
static_assert(CAL_ITERS % CAL_UNROLL == 0, "whole groups of steps");

// Every lane of the wave calls; key: this lane's slot of the record R (0 <= key < CAL_TAIL), or -1 for a lane without a pixel to add.
__device__ __forceinline__ void cal_wave_add(unsigned* __restrict__ R, int lane, int key) {
  bool pend = key >= 0;
#pragma unroll 1
  for (int it = 0; it < CAL_FOLDS; ++it) {
    const unsigned long long pm = __ballot(pend);
    if (!pm) return;                                                 // uniform over the wave
    const int lead = __ffsll(pm) - 1;
    const int k0 = __shfl(key, lead, 64);
    const bool mine = pend && key == k0;
    const unsigned cnt = (unsigned)__popcll(__ballot(mine));
    if (lane == lead) (void)__hip_atomic_fetch_add(R + k0, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    pend = pend && !mine;
  }
  if (pend) (void)__hip_atomic_fetch_add(R + key, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// prob, spread (or null), label [B][h * w] fp32; region (or null) [B][h * w] uint8; rec [B][CAL_REC] zeroed.
// grid (ceil(h * w / CAL_PER_BLOCK), B).
__global__ __launch_bounds__(256) void cal_hist_k(const float* __restrict__ prob, const float* __restrict__ spread,
                                                  const float* __restrict__ label, const unsigned char* __restrict__ region,
                                                  float threshold, unsigned* __restrict__ rec, int n) {
  __shared__ unsigned R[CAL_REC];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int e = tid; e < CAL_REC; e += 256) R[e] = 0u;
  __syncthreads();
  const size_t img = (size_t)blockIdx.y * (size_t)n;                 // B n may pass 2^31
  const float* pp = prob + img;
  const float* ps = spread ? spread + img : nullptr;
  const float* pl = label + img;
  const unsigned char* pr = region ? region + img : nullptr;
  const int base = blockIdx.x * CAL_PER_BLOCK;                       // < n <= 2^24
  unsigned t0 = 0u, t1 = 0u, t2 = 0u, t3 = 0u;                       // the tail, wave-uniform
#pragma unroll 1
  for (int k0 = 0; k0 < CAL_ITERS; k0 += CAL_UNROLL) {
    if (base + k0 * 256 >= n) break;                                 // uniform over the workgroup
    float vp[CAL_UNROLL], vs[CAL_UNROLL], vl[CAL_UNROLL];
    unsigned vr[CAL_UNROLL];
#pragma unroll
    for (int j = 0; j < CAL_UNROLL; ++j) {
      const int i = base + (k0 + j) * 256 + tid;
      const bool in = i < n;
      vp[j] = in ? pp[i] : 0.f;
      vl[j] = in ? pl[i] : 0.f;
      vs[j] = (in && ps) ? ps[i] : 0.f;
      vr[j] = (in && pr) ? (unsigned)pr[i] : 1u;
    }
#pragma unroll
    for (int j = 0; j < CAL_UNROLL; ++j) {
      const bool in = base + (k0 + j) * 256 + tid < n;
      const float p = vp[j], s = vs[j];
      const int y = vl[j] != 0.f ? 1 : 0;                            // (a NaN label is nonzero)
      const bool excl = in && vr[j] == 0u;
      const bool bad = in && !excl && (p != p || s != s);
      const bool ok = in && !excl && !bad;
      t0 += (unsigned)__popcll(__ballot(excl && !y));
      t1 += (unsigned)__popcll(__ballot(excl && y));
      t2 += (unsigned)__popcll(__ballot(bad));
      t3 += (unsigned)__popcll(__ballot(ok));
      const float pc = p < 0.f ? 0.f : p > 1.f ? 1.f : p;
      const float sc = s < 0.f ? 0.f : s > 0.5f ? 0.5f : s;
      const int q = (int)rintf(pc * 1024.f), u = (int)rintf(sc * 2048.f);     // exact products, round half even; 0 .. 1024 (NaN: not ok)
      const int e = ((p > threshold) ? 1 : 0) != y;
      cal_wave_add(R, lane, ok ? 2 * q + y : -1);
      cal_wave_add(R, lane, ok ? CAL_HS + 2 * u + e : -1);
    }
  }
  if (lane == 0) {
    if (t0) (void)__hip_atomic_fetch_add(R + CAL_TAIL + 0, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (t1) (void)__hip_atomic_fetch_add(R + CAL_TAIL + 1, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (t2) (void)__hip_atomic_fetch_add(R + CAL_TAIL + 2, t2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (t3) (void)__hip_atomic_fetch_add(R + CAL_TAIL + 3, t3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();                                                   // the waves' LDS atomics are complete
  unsigned* o = rec + (size_t)blockIdx.y * CAL_REC;
  for (int e = tid; e < CAL_REC; e += 256) {
    const unsigned v = R[e];
    if (v) (void)__hip_atomic_fetch_add(o + e, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- entry point (see include/wtpse_hip.h) -----------------------------------------------------------------------------------
extern "C" int wtpse_calibration_hist(const float* prob, const float* spread, const float* label, const unsigned char* region,
                                      float threshold, unsigned* rec, int B, int h, int w, void* stream) {
  WTPSE_REQUIRE(prob && label && rec);
  WTPSE_REQUIRE(B > 0 && B < 8192 && h >= 1 && w >= 1 && h <= CAL_MAXDIM && w <= CAL_MAXDIM);
  WTPSE_REQUIRE(((uintptr_t)prob & 3) == 0 && ((uintptr_t)label & 3) == 0 && ((uintptr_t)spread & 3) == 0 && ((uintptr_t)rec & 3) == 0);
  const hipStream_t st = (hipStream_t)stream;
  const int n = h * w;                                               // <= 2^24
  if (hipMemsetAsync(rec, 0, (size_t)B * CAL_REC * sizeof(unsigned), st) != hipSuccess) return wtpse_status();
  const dim3 grid((unsigned)ceil_div(n, CAL_PER_BLOCK), (unsigned)B);
  hipLaunchKernelGGL(cal_hist_k, grid, dim3(256), 0, st, prob, spread, label, region, threshold, rec, n);
  return wtpse_status();
}
