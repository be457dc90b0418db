// Validation back half on the device: the reference post-processes and scores every validation image on
// the host (utils.py:267-329 with skimage / scipy; Dice, metrics.py:68-97; medpy's asd / hd95, Trainer.py:218-239).
//
// Post-processing, [B][h][w] fp32 logits -> uint8 masks, bit for bit validate.postprocess:
//   threshold  sigmoidf_(x) > threshold (the function roi_k decides od_pred with);
//   largest 8-connected component: union-find with union by minimum index (every root is the smallest raster index of its
//              component; linking is an atomic min on a root, so the forest a launch ends with does not depend on how the
//              threads race).  cc_local_k labels a 32 x 16 tile in LDS, cc_merge_k unions the pairs that cross tile edges in
//              global memory (agent-scope atomic loads of the parents: a plain load may return a line another XCD has since
//              changed), cc_flatten_k points every pixel at its root and adds the tile-local areas to the roots' (integer
//              atomics).  cc_select_k keeps one 64-bit key per image, (area << 32) | ~root: the maximum is the largest
//              component and, on a tie, the one met first in raster order (skimage's labels + np.argmax);
//   hole fill  the same labelling of the background (everything but the kept component) with 4-connectivity; the roots of
//              components that touch the image border are flagged, every other background pixel is filled
//              (scipy.ndimage.binary_fill_holes with its default cross).
// No propagation sweep count: a union either links two roots or finds them already joined, so a spiral is as good as a disc.
//
// Metrics, per image: post-processed mask A + label B (fp32, nonzero = object) -> one record of 8 int64 (header):
//   met_surf_k   |A & B|, |A|, |B|; surfaces = object XOR its erosion by the 4-neighbour cross, pixels beyond the image count as
//                background (scipy's border_value 0); their sizes;
//   met_col_k    column pass of the exact squared EDT to each surface: vertical distance to the nearest surface pixel in the
//                column (two 16-bit halves of one word, 0xFFFF = none);
//   met_row_k    row pass: for a surface pixel at x the squared distance to the other surface is min_q (x - q)^2 + g(q)^2 over
//                its row, scanned outward from x and stopped once (x - q)^2 reaches the best found (an exact integer minimum:
//                the value a lower-envelope pass would give); ASD = sum of sqrt(d2) result -> reference in fp64, folded per
//                row in a fixed tree and per image in row order (no float atomics); the pooled d2 of both directions go into a
//                4096-bin histogram of their high bits;
//   met_sel1_k   numpy's linear-method positions of the 95th percentile ((n - 1) * q, _get_indexes) -> the histogram bins
//                holding the two order statistics;
//   met_hist2_k / met_sel2_k   the low bits inside those bins -> the two order statistics d2_lo, d2_hi.
// The host finishes a record in float64 as validate.dice / asd / hd95 do (wtpse_hip/validate.py).
#include "common.h"

#define PP_TW 32
#define PP_TH 16
#define PP_TP (PP_TW * PP_TH)
#define PP_MAXDIM 4096
#define MET_L1 4096                    // first-level histogram bins
#define G_NONE 0xFFFFu                 // no surface pixel in the column

// ---- union-find, union by minimum index -------------------------------------------------------------------------------
// LDS: one workgroup.  Members hold an index >= 0, non-members -1.
__device__ __forceinline__ int l_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int l_find(int* L, int i) {
  int p = l_load(L + i);
  while (p != i) {
    i = p;
    p = l_load(L + i);
  }
  return i;
}
__device__ __forceinline__ void l_union(int* L, int a, int b) {
  for (;;) {
    a = l_find(L, a);
    b = l_find(L, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(L + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == b) return;              // b was still a root: linked
    b = old;                           // b had been linked meanwhile (old < b): join a with where it went
  }
}
// Global memory, across workgroups and XCDs: every parent read is an agent-scope atomic load.
__device__ __forceinline__ int g_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(const int* L, int i) {
  int p = g_load(L + i);
  while (p != i) {
    i = p;
    p = g_load(L + i);
  }
  return i;
}
__device__ __forceinline__ void g_union(int* L, int a, int b) {
  for (;;) {
    a = g_find(L, a);
    b = g_find(L, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(L + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == b) return;
    b = old;
  }
}

// The root of the kept component from the image's key, or -1 (no foreground: key 0).
__device__ __forceinline__ int kept_root(unsigned long long key) {
  return key ? (int)~(unsigned)(key & 0xffffffffull) : -1;
}

// FG = 1: members = sigmoid(logit) > thr, 8-connected; zeroes `area` and the image's key.
// FG = 0: members = background of the kept component, 4-connected; writes out = kept, zeroes `area` (the border flags next).
// lab [B][h*w]: index of the pixel's tile-local root in the image (-1: not a member); cnt (FG only): the tile-local component's
// area at its root pixel, 0 elsewhere.
template <int FG>
__global__ __launch_bounds__(256) void cc_local_k(const float* __restrict__ logit, float thr, unsigned char* __restrict__ out,
                                                  int* lab, int* __restrict__ cnt, int* __restrict__ area,
                                                  unsigned long long* best, int h, int w, int tiles_x) {
  __shared__ int L[PP_TP];
  __shared__ int C[PP_TP];
  const int b = blockIdx.y;
  const int tx0 = (blockIdx.x % tiles_x) * PP_TW, ty0 = (blockIdx.x / tiles_x) * PP_TH;
  const size_t base = (size_t)b * h * w;
  const int keep = FG ? -1 : kept_root(best[b]);
  for (int k = threadIdx.x; k < PP_TP; k += 256) {
    const int y = ty0 + k / PP_TW, x = tx0 + k % PP_TW;
    bool in = false;
    if (y < h && x < w) {
      const size_t g = base + (size_t)y * w + x;
      if (FG) {
        in = sigmoidf_(logit[g]) > thr;
      } else {
        const bool kept = keep >= 0 && lab[g] == keep;
        out[g] = kept ? 1 : 0;
        in = !kept;
      }
      area[g] = 0;
    }
    L[k] = in ? k : -1;
    C[k] = 0;
  }
  if (FG && blockIdx.x == 0 && threadIdx.x == 0) best[b] = 0ull;
  __syncthreads();
  for (int k = threadIdx.x; k < PP_TP; k += 256) {
    if (l_load(L + k) < 0) continue;
    const int lx = k % PP_TW, ly = k / PP_TW;
    if (lx > 0 && l_load(L + k - 1) >= 0) l_union(L, k, k - 1);
    if (ly > 0) {
      if (l_load(L + k - PP_TW) >= 0) l_union(L, k, k - PP_TW);
      if (FG && lx > 0 && l_load(L + k - PP_TW - 1) >= 0) l_union(L, k, k - PP_TW - 1);
      if (FG && lx < PP_TW - 1 && l_load(L + k - PP_TW + 1) >= 0) l_union(L, k, k - PP_TW + 1);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < PP_TP; k += 256) {
    if (l_load(L + k) < 0) continue;
    const int r = l_find(L, k);
    __hip_atomic_store(L + k, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (FG) atomicAdd(C + r, 1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < PP_TP; k += 256) {
    const int y = ty0 + k / PP_TW, x = tx0 + k % PP_TW;
    if (y >= h || x >= w) continue;
    const size_t g = base + (size_t)y * w + x;
    const int r = L[k];
    lab[g] = r < 0 ? -1 : (ty0 + r / PP_TW) * w + tx0 + r % PP_TW;   // raster order is kept: the tile root is the smallest index
    if (FG) cnt[g] = C[k];
  }
}

// Unions of the member pairs that cross a tile edge (W, N and, for 8-connectivity, NW, NE).
template <int FG>
__global__ __launch_bounds__(256) void cc_merge_k(int* lab, int h, int w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= h * w) return;
  const int y = i / w, x = i - y * w;
  const int cx = x % PP_TW, cy = y % PP_TH;
  if (cx != 0 && cy != 0 && !(FG && cx == PP_TW - 1)) return;
  int* L = lab + (size_t)blockIdx.y * h * w;
  if (g_load(L + i) < 0) return;
  if (x > 0 && cx == 0 && g_load(L + i - 1) >= 0) g_union(L, i, i - 1);
  if (y > 0) {
    if (cy == 0 && g_load(L + i - w) >= 0) g_union(L, i, i - w);
    if (FG && x > 0 && (cx == 0 || cy == 0) && g_load(L + i - w - 1) >= 0) g_union(L, i, i - w - 1);
    if (FG && x + 1 < w && (cx == PP_TW - 1 || cy == 0) && g_load(L + i - w + 1) >= 0) g_union(L, i, i - w + 1);
  }
}

// Every member -> its root.  FG: the tile-local areas are added to the roots'; background: roots of components that touch the
// image border are flagged in `area`.
template <int FG>
__global__ __launch_bounds__(256) void cc_flatten_k(int* lab, const int* __restrict__ cnt, int* area, int h, int w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= h * w) return;
  const size_t base = (size_t)blockIdx.y * h * w;
  int* L = lab + base;
  if (g_load(L + i) < 0) return;
  const int r = g_find(L, i);
  __hip_atomic_store(L + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (FG) {
    const int c = cnt[base + i];
    if (c) __hip_atomic_fetch_add(area + base + r, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    const int y = i / w, x = i - y * w;
    if (y == 0 || x == 0 || y == h - 1 || x == w - 1) __hip_atomic_store(area + base + r, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void cc_select_k(const int* __restrict__ lab, const int* __restrict__ area,
                                                   unsigned long long* best, int h, int w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= h * w) return;
  const size_t base = (size_t)blockIdx.y * h * w;
  if (lab[base + i] != i) return;                                  // roots only
  const unsigned long long key = ((unsigned long long)(unsigned)area[base + i] << 32) | (unsigned)~(unsigned)i;
  (void)__hip_atomic_fetch_max(best + blockIdx.y, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Background pixels in a component that does not touch the border are holes: filled.
__global__ __launch_bounds__(256) void cc_fill_k(const int* __restrict__ lab, const int* __restrict__ flag,
                                                 unsigned char* __restrict__ out, int h, int w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= h * w) return;
  const size_t base = (size_t)blockIdx.y * h * w;
  const int r = lab[base + i];
  if (r >= 0) out[base + i] = flag[base + r] ? 0 : 1;
}

// ---- metrics ------------------------------------------------------------------------------------------------------------
// rec [B][8] int64: 0 |A & B|, 1 |A|, 2 |B|, 3 surface pixels of A, 4 of B, 5 d2_lo, 6 d2_hi, 7 ASD sum (fp64 bits).
__global__ __launch_bounds__(256) void met_zero_k(unsigned long long* __restrict__ rec, int nrec, int* __restrict__ hist, int nhist) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nrec) rec[i] = 0ull;
  if (i < nhist) hist[i] = 0;
}

// bit 0: surface of A, bit 1: surface of B
__global__ __launch_bounds__(256) void met_surf_k(const unsigned char* __restrict__ mask, const float* __restrict__ label,
                                                  unsigned char* __restrict__ sbits, unsigned long long* rec, int h, int w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const size_t base = (size_t)blockIdx.y * h * w;
  bool a = false, l = false, sa = false, sb = false;
  if (i < h * w) {
    const int y = i / w, x = i - y * w;
    const unsigned char* m = mask + base;
    const float* t = label + base;
    a = m[i] != 0;
    l = t[i] != 0.f;
    if (a) sa = y == 0 || x == 0 || y == h - 1 || x == w - 1 || !m[i - w] || !m[i + w] || !m[i - 1] || !m[i + 1];
    if (l) sb = y == 0 || x == 0 || y == h - 1 || x == w - 1 || t[i - w] == 0.f || t[i + w] == 0.f || t[i - 1] == 0.f || t[i + 1] == 0.f;
    sbits[base + i] = (sa ? 1 : 0) | (sb ? 2 : 0);
  }
  // one atomic per wave and counter (integer: the sums do not depend on the order)
  const unsigned long long c[5] = {(unsigned long long)__popcll(__ballot(a && l)), (unsigned long long)__popcll(__ballot(a)),
                                   (unsigned long long)__popcll(__ballot(l)), (unsigned long long)__popcll(__ballot(sa)),
                                   (unsigned long long)__popcll(__ballot(sb))};
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* r = rec + (size_t)blockIdx.y * 8;
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (c[k]) (void)__hip_atomic_fetch_add(r + k, c[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One thread per column: G = gA | gB << 16, the vertical distance to the nearest surface pixel of A / B in the column.
__global__ __launch_bounds__(256) void met_col_k(const unsigned char* __restrict__ sbits, unsigned* __restrict__ G, int h, int w) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= w) return;
  const size_t base = (size_t)blockIdx.y * h * w + x;
  int la = -1, lb = -1;                                            // last surface row above
  for (int y = 0; y < h; ++y) {
    const unsigned s = sbits[base + (size_t)y * w];
    if (s & 1) la = y;
    if (s & 2) lb = y;
    G[base + (size_t)y * w] = (la < 0 ? G_NONE : (unsigned)(y - la)) | ((lb < 0 ? G_NONE : (unsigned)(y - lb)) << 16);
  }
  la = lb = -1;                                                    // next surface row below
  for (int y = h - 1; y >= 0; --y) {
    const size_t g = base + (size_t)y * w;
    const unsigned s = sbits[g];
    if (s & 1) la = y;
    if (s & 2) lb = y;
    unsigned v = G[g], ga = v & 0xFFFFu, gb = v >> 16;
    if (la >= 0 && (unsigned)(la - y) < ga) ga = (unsigned)(la - y);
    if (lb >= 0 && (unsigned)(lb - y) < gb) gb = (unsigned)(lb - y);
    G[g] = ga | (gb << 16);
  }
}

// min over q of (x - q)^2 + g(q)^2 on one row (g = the 16-bit half `sh` of G), -1 if no column has a surface pixel.
__device__ __forceinline__ int row_min(const unsigned* G, int x, int w, int sh) {
  int best = 0x7fffffff;
  for (int r = 0;; ++r) {
    const int r2 = r * r;
    if (r2 >= best) break;
    const bool lo = x - r >= 0, hi = r > 0 && x + r < w;
    if (!lo && !hi && r > 0) break;
    if (lo) {
      const unsigned g = (G[x - r] >> sh) & 0xFFFFu;
      if (g != G_NONE) best = min(best, r2 + (int)(g * g));
    }
    if (hi) {
      const unsigned g = (G[x + r] >> sh) & 0xFFFFu;
      if (g != G_NONE) best = min(best, r2 + (int)(g * g));
    }
  }
  return best == 0x7fffffff ? -1 : best;
}

// One workgroup per (row, image).  dA / dB: d2 of the surface pixels of A (to B's surface) / of B (to A's), -1 elsewhere.
__global__ __launch_bounds__(256) void met_row_k(const unsigned char* __restrict__ sbits, const unsigned* __restrict__ Gg,
                                                 int* __restrict__ dA, int* __restrict__ dB, double* __restrict__ partial,
                                                 int* __restrict__ hist1, int shift, int h, int w) {
  __shared__ unsigned G[PP_MAXDIM];
  __shared__ double red[256];
  const int y = blockIdx.x, b = blockIdx.y;
  const size_t row = (size_t)b * h * w + (size_t)y * w;
  for (int x = threadIdx.x; x < w; x += 256) G[x] = Gg[row + x];
  __syncthreads();
  int* hist = hist1 + (size_t)b * MET_L1;
  double acc = 0.0;
  for (int x = threadIdx.x; x < w; x += 256) {
    const unsigned s = sbits[row + x];
    int da = -1, db = -1;
    if (s & 1) {
      da = row_min(G, x, w, 16);
      if (da >= 0) {
        acc += sqrt((double)da);
        atomicAdd(hist + (da >> shift), 1);
      }
    }
    if (s & 2) {
      db = row_min(G, x, w, 0);
      if (db >= 0) atomicAdd(hist + (db >> shift), 1);
    }
    dA[row + x] = da;
    dB[row + x] = db;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[(size_t)b * h + y] = red[0];
}

// 256 threads: the bin of hist[0:nb] that holds the element of rank k (0-based) and k's rank inside it.
__device__ void block_select(const int* hist, int nb, long long k, int* sh_sum, int* out_bin, long long* out_rank) {
  const int per = (nb + 255) / 256;
  const int b0 = min(nb, (int)threadIdx.x * per), b1 = min(nb, b0 + per);
  int s = 0;
  for (int j = b0; j < b1; ++j) s += hist[j];
  __syncthreads();
  sh_sum[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {                                         // exclusive prefix over 256 chunk sums
    long long run = 0;
    *out_bin = 0;
    *out_rank = 0;
    for (int t = 0; t < 256; ++t) {
      const int v = sh_sum[t];
      if (k >= run && k < run + v) {
        long long r = k - run;
        int j = min(nb, t * per);
        const int jend = min(nb, j + per);
        while (j < jend - 1 && r >= hist[j]) r -= hist[j++];
        *out_bin = j;
        *out_rank = r;
        break;
      }
      run += v;
    }
  }
  __syncthreads();
}

// numpy.percentile(a, 95) on n pooled float64 values: the ranks of the two order statistics, as _get_indexes takes them from the
// linear method's virtual index (n - 1) * q, q = 95 / 100.0 (numpy's _QuantileMethods["linear"]; one rounding, kept uncontracted).
__device__ __forceinline__ void percentile_ranks(long long n, long long* lo, long long* hi) {
  const double q = __ddiv_rn(95.0, 100.0);
  const double vi = __dmul_rn((double)(n - 1), q);
  if (vi >= (double)(n - 1)) {
    *lo = *hi = n - 1;
  } else if (vi < 0.0) {
    *lo = *hi = 0;
  } else {
    *lo = (long long)floor(vi);
    *hi = *lo + 1;
  }
}

// One workgroup per image: the ASD sum (row partials in row order) and the first-level bins of the two order statistics.
__global__ __launch_bounds__(256) void met_sel1_k(unsigned long long* rec, const double* __restrict__ partial,
                                                  const int* __restrict__ hist1, int* __restrict__ sel, int h) {
  __shared__ double red[256];
  __shared__ int sh_sum[256];
  __shared__ int bin[2];
  __shared__ long long rank[2];
  const int b = blockIdx.x;
  unsigned long long* r = rec + (size_t)b * 8;
  double acc = 0.0;
  for (int y = threadIdx.x; y < h; y += 256) acc += partial[(size_t)b * h + y];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) r[7] = (unsigned long long)__double_as_longlong(red[0]);
  const long long na = (long long)r[3], nb = (long long)r[4];
  if (na == 0 || nb == 0) {                                       // an empty mask: the host scores the image without d2
    if (threadIdx.x == 0) sel[4 * b] = sel[4 * b + 2] = -1;
    return;
  }
  long long lo, hi;
  percentile_ranks(na + nb, &lo, &hi);
  block_select(hist1 + (size_t)b * MET_L1, MET_L1, lo, sh_sum, &bin[0], &rank[0]);
  block_select(hist1 + (size_t)b * MET_L1, MET_L1, hi, sh_sum, &bin[1], &rank[1]);
  if (threadIdx.x == 0) {
    sel[4 * b] = bin[0];
    sel[4 * b + 1] = (int)rank[0];
    sel[4 * b + 2] = bin[1];
    sel[4 * b + 3] = (int)rank[1];
  }
}

// Second level: the low `shift` bits of the d2 inside the two selected bins.
__global__ __launch_bounds__(256) void met_hist2_k(const unsigned char* __restrict__ sbits, const int* __restrict__ dA,
                                                   const int* __restrict__ dB, const int* __restrict__ sel, int* __restrict__ hist2,
                                                   int shift, int h, int w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= h * w) return;
  const int b_lo = sel[4 * b], b_hi = sel[4 * b + 2];
  if (b_lo < 0) return;
  const size_t g = (size_t)b * h * w + i;
  const unsigned s = sbits[g];
  if (!s) return;
  const int m = (1 << shift) - 1;
  int* h2 = hist2 + (size_t)b * 2 * (m + 1);
  for (int k = 0; k < 2; ++k) {
    if (!(s & (1u << k))) continue;
    const int d2 = k ? dB[g] : dA[g];
    if (d2 < 0) continue;
    if ((d2 >> shift) == b_lo) atomicAdd(h2 + (d2 & m), 1);
    if ((d2 >> shift) == b_hi) atomicAdd(h2 + (m + 1) + (d2 & m), 1);
  }
}

__global__ __launch_bounds__(256) void met_sel2_k(unsigned long long* rec, const int* __restrict__ sel, const int* __restrict__ hist2,
                                                  int shift) {
  __shared__ int sh_sum[256];
  __shared__ int bin[2];
  __shared__ long long rank[2];
  const int b = blockIdx.x;
  if (sel[4 * b] < 0) return;
  const int nb = 1 << shift;
  const int* h2 = hist2 + (size_t)b * 2 * nb;
  block_select(h2, nb, sel[4 * b + 1], sh_sum, &bin[0], &rank[0]);
  block_select(h2 + nb, nb, sel[4 * b + 3], sh_sum, &bin[1], &rank[1]);
  if (threadIdx.x == 0) {
    rec[(size_t)b * 8 + 5] = ((unsigned long long)sel[4 * b] << shift) | (unsigned)bin[0];
    rec[(size_t)b * 8 + 6] = ((unsigned long long)sel[4 * b + 2] << shift) | (unsigned)bin[1];
  }
}

// ---- entry points (see include/wtpse_hip.h) ------------------------------------------------------------------------------
static bool pp_dims_ok(int B, int h, int w) {
  return B > 0 && B < 65536 && h > 0 && w > 0 && h <= PP_MAXDIM && w <= PP_MAXDIM;
}

extern "C" int wtpse_postprocess_ws(int B, int h, int w) {
  if (!pp_dims_ok(B, h, w)) return -1;
  const long long words = 2LL * B + 3LL * B * h * w;              // keys (u64), lab, cnt, area
  return words > 0x7fffffffLL ? -1 : (int)words;
}

extern "C" int wtpse_postprocess(const float* logit, unsigned char* out, void* ws, float threshold, int B, int h, int w,
                                 void* stream) {
  WTPSE_REQUIRE(logit && out && ws && wtpse_postprocess_ws(B, h, w) > 0);
  const size_t n = (size_t)B * h * w;
  unsigned long long* best = (unsigned long long*)ws;
  int* lab = (int*)(best + B);
  int* cnt = lab + n;
  int* area = cnt + n;
  const hipStream_t st = (hipStream_t)stream;
  const int tiles_x = ceil_div(w, PP_TW);
  const dim3 gt((unsigned)(tiles_x * ceil_div(h, PP_TH)), (unsigned)B), gp((unsigned)ceil_div(h * w, 256), (unsigned)B);
  hipLaunchKernelGGL(cc_local_k<1>, gt, dim3(256), 0, st, logit, threshold, out, lab, cnt, area, best, h, w, tiles_x);
  hipLaunchKernelGGL(cc_merge_k<1>, gp, dim3(256), 0, st, lab, h, w);
  hipLaunchKernelGGL(cc_flatten_k<1>, gp, dim3(256), 0, st, lab, cnt, area, h, w);
  hipLaunchKernelGGL(cc_select_k, gp, dim3(256), 0, st, lab, area, best, h, w);
  hipLaunchKernelGGL(cc_local_k<0>, gt, dim3(256), 0, st, logit, threshold, out, lab, cnt, area, best, h, w, tiles_x);
  hipLaunchKernelGGL(cc_merge_k<0>, gp, dim3(256), 0, st, lab, h, w);
  hipLaunchKernelGGL(cc_flatten_k<0>, gp, dim3(256), 0, st, lab, cnt, area, h, w);
  hipLaunchKernelGGL(cc_fill_k, gp, dim3(256), 0, st, lab, area, out, h, w);
  return wtpse_status();
}

// log2 of the second-level histogram size: d2 <= (h-1)^2 + (w-1)^2 splits into 12 high bits and `shift` low bits.
static int met_shift(int h, int w) {
  const long long m = (long long)(h - 1) * (h - 1) + (long long)(w - 1) * (w - 1);
  int bits = 0;
  while ((m >> bits) != 0) ++bits;
  return bits > 12 ? bits - 12 : 0;
}

extern "C" int wtpse_seg_metrics_ws(int B, int h, int w) {
  if (!pp_dims_ok(B, h, w)) return -1;
  const long long n = (long long)B * h * w;
  const long long words = 2LL * B * h + (long long)B * MET_L1 + 2LL * B * (1LL << met_shift(h, w)) + 4LL * B + 3 * n + (n + 3) / 4;
  return words > 0x7fffffffLL ? -1 : (int)words;
}

extern "C" int wtpse_seg_metrics(const unsigned char* mask, const float* label, long long* rec, void* ws, int B, int h, int w,
                                 void* stream) {
  WTPSE_REQUIRE(mask && label && rec && ws && wtpse_seg_metrics_ws(B, h, w) > 0);
  const size_t n = (size_t)B * h * w;
  const int shift = met_shift(h, w);
  double* partial = (double*)ws;
  int* hist1 = (int*)(partial + (size_t)B * h);
  int* hist2 = hist1 + (size_t)B * MET_L1;
  int* sel = hist2 + (size_t)B * 2 * (1 << shift);
  unsigned* G = (unsigned*)(sel + 4 * (size_t)B);
  int* dA = (int*)(G + n);
  int* dB = dA + n;
  unsigned char* sbits = (unsigned char*)(dB + n);
  unsigned long long* r = (unsigned long long*)rec;
  const hipStream_t st = (hipStream_t)stream;
  const int nhist = B * MET_L1 + B * 2 * (1 << shift);
  const dim3 gp((unsigned)ceil_div(h * w, 256), (unsigned)B);
  hipLaunchKernelGGL(met_zero_k, dim3((unsigned)ceil_div(max(nhist, 8 * B), 256)), dim3(256), 0, st, r, 8 * B, hist1, nhist);
  hipLaunchKernelGGL(met_surf_k, gp, dim3(256), 0, st, mask, label, sbits, r, h, w);
  hipLaunchKernelGGL(met_col_k, dim3((unsigned)ceil_div(w, 256), (unsigned)B), dim3(256), 0, st, sbits, G, h, w);
  hipLaunchKernelGGL(met_row_k, dim3((unsigned)h, (unsigned)B), dim3(256), 0, st, sbits, G, dA, dB, partial, hist1, shift, h, w);
  hipLaunchKernelGGL(met_sel1_k, dim3((unsigned)B), dim3(256), 0, st, r, partial, hist1, sel, h);
  hipLaunchKernelGGL(met_hist2_k, gp, dim3(256), 0, st, sbits, dA, dB, sel, hist2, shift, h, w);
  hipLaunchKernelGGL(met_sel2_k, dim3((unsigned)B), dim3(256), 0, st, r, sel, hist2, shift);
  return wtpse_status();
}
