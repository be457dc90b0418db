// Dense weight averaging (SWAD): running means of the flat parameter buffers, on the device (include/wtpse_hip.h, "weight
// averaging"; specification: wtpse_hip/averaging.py, avg_step_spec / avg_merge_spec — the results are the same bits).
#include "common.h"

// Every product and sum below is rounded on its own: hipcc contracts a * b + c into one fused multiply-add by default, and the
// specification rounds twice.  Plain operators under this pragma, NOT __fmul_rn / __fadd_rn: those are inline functions of the HIP
// headers, compiled under the headers' own (contracting) setting, and came out as v_pk_fma_f32 here.
#pragma clang fp contract(off)

#define ST ((hipStream_t)stream)

constexpr int AVG_SEGS = 4;
constexpr int AVG_TILE = 256 * 4;          // floats of one workgroup pass: one 16-byte access per lane
constexpr unsigned AVG_MAX_GRID = 2048;    // 256 CUs x 8 workgroups; the tiles beyond are grid-strided

// Up to four (mean, iterate, length) segments of one launch.  end[s]: tiles of the segments 0..s (a running total), so that a
// tile index finds its segment with at most three compares.
struct AvgSegs {
  float* a[AVG_SEGS];
  const float* p[AVG_SEGS];
  long long n[AVG_SEGS];
  long long end[AVG_SEGS];
};

// a <- a + (p - a) / k with k = *count + 1 (k == 1: a <- p).  Subtraction, division and addition are each rounded to nearest
// (nothing here can be contracted: there is no multiply; the division is the correctly rounded one).  count / gate / hold are
// read by one thread per workgroup; the count is bumped by avg_bump_k BEHIND this launch, so every workgroup sees the same k.
__global__ __launch_bounds__(256) void avg_step_k(AvgSegs sg, const int* __restrict__ count, const int* __restrict__ gate,
                                                  const int* __restrict__ hold) {
  __shared__ int k_s;
  if (threadIdx.x == 0) {
    const bool off = (gate && *gate == 0) || (hold && *hold != 0);
    k_s = off ? 0 : *count + 1;
  }
  __syncthreads();
  const int k = k_s;
  if (k <= 0) return;
  const float kf = (float)k;
  const long long ntiles = sg.end[AVG_SEGS - 1];
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int s = (t >= sg.end[0]) + (t >= sg.end[1]) + (t >= sg.end[2]);
    const long long t0 = s ? sg.end[s - 1] : 0;
    float* __restrict__ a = sg.a[s];
    const float* __restrict__ p = sg.p[s];
    const long long n = sg.n[s];
    const long long i = (t - t0) * AVG_TILE + (long long)threadIdx.x * 4;
    if (i + 4 <= n) {
      const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
      if (k == 1) {
        *reinterpret_cast<f32x4*>(a + i) = pv;
      } else {
        f32x4 av = *reinterpret_cast<const f32x4*>(a + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) av[j] = av[j] + (pv[j] - av[j]) / kf;
        *reinterpret_cast<f32x4*>(a + i) = av;
      }
    } else {
      for (long long j = i; j < n; ++j) {        // the segment's scalar tail: at most three elements, in one lane
        const float pj = p[j];
        a[j] = k == 1 ? pj : a[j] + (pj - a[j]) / kf;
      }
    }
  }
}

__global__ __launch_bounds__(64) void avg_bump_k(int* __restrict__ count, const int* __restrict__ gate, const int* __restrict__ hold) {
  if (threadIdx.x != 0) return;
  if ((gate && *gate == 0) || (hold && *hold != 0)) return;
  *count = *count + 1;
}

extern "C" int wtpse_avg_step(float* a0, const float* p0, long long n0, float* a1, const float* p1, long long n1, float* a2,
                              const float* p2, long long n2, float* a3, const float* p3, long long n3, int* count, const int* gate,
                              const int* hold, void* stream) {
  WTPSE_REQUIRE(count);
  AvgSegs sg;
  float* a[AVG_SEGS] = {a0, a1, a2, a3};
  const float* p[AVG_SEGS] = {p0, p1, p2, p3};
  const long long n[AVG_SEGS] = {n0, n1, n2, n3};
  long long tiles = 0;
  for (int s = 0; s < AVG_SEGS; ++s) {
    WTPSE_REQUIRE(n[s] >= 0);
    if (n[s] > 0) {
      WTPSE_REQUIRE(a[s] && p[s] && a[s] != p[s]);
      WTPSE_REQUIRE((((uintptr_t)a[s] | (uintptr_t)p[s]) & 15) == 0);
      tiles += (n[s] + AVG_TILE - 1) / AVG_TILE;
    }
    sg.a[s] = a[s]; sg.p[s] = p[s]; sg.n[s] = n[s]; sg.end[s] = tiles;
  }
  if (tiles > 0)
    hipLaunchKernelGGL(avg_step_k, dim3((unsigned)(tiles < AVG_MAX_GRID ? tiles : AVG_MAX_GRID)), dim3(256), 0, ST, sg,
                       (const int*)count, gate, hold);
  hipLaunchKernelGGL(avg_bump_k, dim3(1), dim3(64), 0, ST, count, gate, hold);
  return wtpse_status();
}

// acc <- acc + (seg - acc) * w, multiply and add rounded separately (contraction is off in this file); copy: acc <- seg.
__global__ __launch_bounds__(256) void avg_merge_k(float* __restrict__ acc, const float* __restrict__ seg, long long n, float w, int copy) {
  const long long ntiles = (n + AVG_TILE - 1) / AVG_TILE;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long i = t * AVG_TILE + (long long)threadIdx.x * 4;
    if (i + 4 <= n) {
      const f32x4 sv = *reinterpret_cast<const f32x4*>(seg + i);
      if (copy) {
        *reinterpret_cast<f32x4*>(acc + i) = sv;
      } else {
        f32x4 av = *reinterpret_cast<const f32x4*>(acc + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) av[j] = av[j] + (sv[j] - av[j]) * w;
        *reinterpret_cast<f32x4*>(acc + i) = av;
      }
    } else {
      for (long long j = i; j < n; ++j) {
        const float sj = seg[j];
        acc[j] = copy ? sj : acc[j] + (sj - acc[j]) * w;
      }
    }
  }
}

extern "C" int wtpse_avg_merge(float* acc, const float* seg, long long n, long long n_acc, long long n_seg, void* stream) {
  WTPSE_REQUIRE(acc && seg && acc != seg && n > 0 && n_acc >= 0 && n_seg >= 1);
  WTPSE_REQUIRE((((uintptr_t)acc | (uintptr_t)seg) & 15) == 0);
  const float w = (float)((double)n_seg / (double)(n_acc + n_seg));
  const long long tiles = (n + AVG_TILE - 1) / AVG_TILE;
  hipLaunchKernelGGL(avg_merge_k, dim3((unsigned)(tiles < AVG_MAX_GRID ? tiles : AVG_MAX_GRID)), dim3(256), 0, ST, acc, seg, n, w,
                     (int)(n_acc == 0));
  return wtpse_status();
}
