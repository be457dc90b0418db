// CLAHE preprocessing: contrast-limited adaptive histogram equalisation of the uint8 batch [N][H][W][3] in front of the
// normalisation (Pizer et al. 1987, Zuiderveld 1994).  The definition is integers throughout (include/wtpse_hip.h has the
// formulas; input_pipeline.clahe_host is the same text in numpy int64), so the device equals the specification byte for byte.
//   clahe_hist_k  : one workgroup = up to CL_CHUNK pixels of one tile of one picture.  A lane counts into one of several copies of the
//                   256 bins in LDS (adjacent lanes see adjacent pixels, which on a fundus picture mostly share a bin: on one array the
//                   LDS atomics of a wave would serialise on that bin), the copies are summed per bin and added to the tile's
//                   histogram in global memory with one integer atomic per non-empty bin.  A tile larger than CL_CHUNK pixels is
//                   split over workgroups, which meet in those atomics: integer adds, so the result is the same in any order.
//   clahe_lut_k   : one wave = one (picture, plane, tile).  A lane owns four bins: clip, redistribute, a wave scan, the division.
//   clahe_apply_k : one workgroup = up to CL_APPLY_GROUPS groups of 4 pixels of the rows that blend the same two tile rows, whose
//                   LUTs it stages in LDS; a thread works on 4 pixels = 12 consecutive bytes of a row at a time; the axis tables
//                   come from the host.
// Rows are 3 W bytes, so with an odd W most rows start off a dword: dword accesses where the address is 4-byte aligned and the 12
// bytes lie inside the row, byte accesses where not.  Nothing here shifts a value to the right before packing it into a byte
// (profiles/quality.md records what v_ashr_pk_u8_i32 did to that form): every byte is clipped or bounded as it stands.
#include "common.h"

#define CL_CHUNK 4096                            // pixels of a tile per workgroup of the histogram pass
#define CL_STRIDE 257                            // words between two copies of the bins: the same bin of two copies in two banks

typedef unsigned int cl_u32x4 __attribute__((ext_vector_type(4)));
typedef int cl_i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned cl_byte(const unsigned* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }
__device__ __forceinline__ unsigned cl_luma(unsigned r, unsigned g, unsigned b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// `nvalid` (0 .. 12) bytes at p -> three dwords, little endian; the bytes beyond nvalid are not read (0)
__device__ __forceinline__ void cl_load12(const unsigned char* __restrict__ p, int nvalid, unsigned v[3]) {
  if (nvalid == 12 && ((uintptr_t)p & 3) == 0) {
    const unsigned* q = reinterpret_cast<const unsigned*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
  } else {
    v[0] = v[1] = v[2] = 0u;
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (i < nvalid) v[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
  }
}
__device__ __forceinline__ void cl_store12(unsigned char* __restrict__ p, int nvalid, const unsigned v[3]) {
  if (nvalid == 12 && ((uintptr_t)p & 3) == 0) {
    unsigned* q = reinterpret_cast<unsigned*>(p);
    q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (i < nvalid) p[i] = (unsigned char)cl_byte(v, i);
  }
}

// ------------------------------------------------------------------------------------------------ tile histograms
// grid (chunks of the largest tile, ty * tx, N); hist [N][P][ty * tx][256] is zero on entry
template <int P>
__global__ __launch_bounds__(256) void clahe_hist_k(const unsigned char* __restrict__ img, unsigned* __restrict__ hist, int H, int W,
                                                    int ty, int tx, unsigned floor) {
  constexpr int COPIES = P == 1 ? 16 : 8;
  __shared__ unsigned bins[P * COPIES * CL_STRIDE];
  const int tid = threadIdx.x, tile = blockIdx.y, n = blockIdx.z;
  const int i = tile / tx, j = tile - i * tx;
  const int y0 = (i * H) / ty, y1 = ((i + 1) * H) / ty, x0 = (j * W) / tx, x1 = ((j + 1) * W) / tx;
  const unsigned tw = (unsigned)(x1 - x0), npix = (unsigned)(y1 - y0) * tw;
  const unsigned lo = blockIdx.x * CL_CHUNK;
  if (lo >= npix) return;                                             // a smaller tile than the largest: uniform over the workgroup
  const unsigned hi = min(npix, lo + CL_CHUNK);
  for (int e = tid; e < P * COPIES * CL_STRIDE; e += 256) bins[e] = 0u;
  __syncthreads();
  unsigned* __restrict__ mine = bins + (tid & (COPIES - 1)) * CL_STRIDE;
  const unsigned char* __restrict__ src = img + ((size_t)n * H + y0) * W * 3 + (size_t)x0 * 3;
  for (unsigned e = lo + tid; e < hi; e += 256) {
    const unsigned r = e / tw, c = e - r * tw;
    const unsigned char* __restrict__ p = src + ((size_t)r * W + c) * 3;
    const unsigned R = p[0], G = p[1], B = p[2];
    if (max(max(R, G), B) < floor) continue;                          // outside the field of view: not counted
    if constexpr (P == 1) {
      atomicAdd(mine + cl_luma(R, G, B), 1u);
    } else {
      atomicAdd(mine + R, 1u);
      atomicAdd(mine + COPIES * CL_STRIDE + G, 1u);
      atomicAdd(mine + 2 * COPIES * CL_STRIDE + B, 1u);
    }
  }
  __syncthreads();
  const int ntiles = ty * tx;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    unsigned s = 0u;
#pragma unroll
    for (int c = 0; c < COPIES; ++c) s += bins[(p * COPIES + c) * CL_STRIDE + tid];
    if (s) atomicAdd(hist + (((size_t)n * P + p) * ntiles + tile) * 256 + tid, s);
  }
}

// ------------------------------------------------------------------------------------------------ LUT per (picture, plane, tile)
__device__ __forceinline__ unsigned cl_wave_sum(unsigned v) {
  for (int m = 1; m < 64; m <<= 1) v += (unsigned)__shfl_xor((int)v, m, 64);
  return v;
}

__global__ __launch_bounds__(256) void clahe_lut_k(const unsigned* __restrict__ hist, unsigned char* __restrict__ lut, int count,
                                                   unsigned clip_q8) {
  const int item = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (item >= count) return;                                          // uniform over the wave; no barrier below
  const cl_u32x4 hv = reinterpret_cast<const cl_u32x4*>(hist + (size_t)item * 256)[lane];
  unsigned h[4] = {hv[0], hv[1], hv[2], hv[3]};
  const unsigned n = cl_wave_sum(h[0] + h[1] + h[2] + h[3]);          // <= 2^24 pixels of a tile
  unsigned packed = 0u;
  if (n == 0u) {                                                      // an empty tile: the identity
#pragma unroll
    for (int k = 0; k < 4; ++k) packed |= (unsigned)(4 * lane + k) << (8 * k);
  } else {
    const unsigned limit = max(1u, (unsigned)(((unsigned long long)clip_q8 * n) >> 16));
    unsigned over = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) over += h[k] > limit ? h[k] - limit : 0u;
    const unsigned excess = cl_wave_sum(over);
    const unsigned add = excess >> 8, r = excess & 255u, step = r ? 256u / r : 1u;
    unsigned run = 0u, cum[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned b = 4u * lane + k, q = b / step;
      unsigned v = min(h[k], limit) + add;
      if (r && q * step == b && q < r) v += 1u;                       // bins 0, step, 2 step, ..: the first r of them
      run += v;
      cum[k] = run;
    }
    unsigned before = run;                                            // inclusive scan of the lanes' totals ..
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = (unsigned)__shfl_up((int)before, d, 64);
      if (lane >= d) before += up;
    }
    before -= run;                                                    // .. made exclusive
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned v = min(((before + cum[k]) * 255u + (n >> 1)) / n, 255u);       // <= 2^24 * 255 + 2^23 < 2^32
      packed |= v << (8 * k);
    }
  }
  reinterpret_cast<unsigned*>(lut + (size_t)item * 256)[lane] = packed;
}

// ------------------------------------------------------------------------------------------------ apply
// One bilinear blend of four LUT values: ((256 - wy) ((256 - wx) a + wx b) + wy ((256 - wx) c + wx d) + 32768) >> 16 <= 255
__device__ __forceinline__ unsigned cl_blend(const unsigned char* __restrict__ l00, const unsigned char* __restrict__ l01,
                                             const unsigned char* __restrict__ l10, const unsigned char* __restrict__ l11, unsigned v,
                                             unsigned wy, unsigned wx) {
  const unsigned a = l00[v], b = l01[v], c = l10[v], d = l11[v];
  return ((256u - wy) * ((256u - wx) * a + wx * b) + wy * ((256u - wx) * c + wx * d) + 32768u) >> 16;
}

// Rows that share their lower tile row k0y form a band (k0y does not decrease with y); a workgroup works on up to CL_APPLY_GROUPS
// 4-pixel groups of one band of one picture, so every pixel of it blends tile rows k0y and min(k0y + 1, ty - 1): those two rows of
// LUTs (2 * P * tx * 256 bytes, at most 24 KiB) are staged once and read from LDS.  (Read through the cache instead — one thread per
// group, four byte gathers from global memory per pixel and plane — the launch took as long in "luma" and 1.6 times as long in
// "rgb": profiles/clahe.md.)
// grid (chunks of the longest band, ty, N); rows [H], cols [W rounded up to 4]: k0 | w << 8; bands [ty + 1]: the first row of band
// k, bands[ty] = H
#define CL_APPLY_GROUPS 2048
template <int P>
__global__ __launch_bounds__(256) void clahe_apply_k(const unsigned char* __restrict__ img, const unsigned char* __restrict__ lut,
                                                         const int* __restrict__ rows, const int* __restrict__ cols,
                                                         const int* __restrict__ bands, unsigned char* __restrict__ out, int H, int W,
                                                         int ty, int tx, unsigned floor) {
  __shared__ unsigned staged[2 * P * 1024];                           // [upper?][plane][16 tiles][256] bytes
  const int tid = threadIdx.x, k = blockIdx.y, n = blockIdx.z, G = (W + 3) >> 2;
  const int yb = bands[k], total = (bands[k + 1] - yb) * G;
  const int lo = (int)blockIdx.x * CL_APPLY_GROUPS;
  if (lo >= total) return;                                            // a shorter band than the longest: uniform over the workgroup
  const int hi = min(total, lo + CL_APPLY_GROUPS);
  const int k1 = min(k + 1, ty - 1), row_dwords = tx * 64;
#pragma unroll
  for (int rp = 0; rp < 2 * P; ++rp) {
    const int p = rp % P, ky = rp < P ? k : k1;
    const unsigned* __restrict__ src = reinterpret_cast<const unsigned*>(lut + (((size_t)n * P + p) * ty + ky) * tx * 256);
    for (int e = tid; e < row_dwords; e += 256) staged[rp * 1024 + e] = src[e];
  }
  __syncthreads();
  const unsigned char* __restrict__ sl = reinterpret_cast<const unsigned char*>(staged);
  for (int e = lo + tid; e < hi; e += 256) {
    const int yrel = e / G, x = (e - yrel * G) * 4, y = yb + yrel;
    const int nvalid = min(12, (W - x) * 3);
    const size_t at = (((size_t)n * H + y) * W + x) * 3;
    unsigned v[3];
    cl_load12(img + at, nvalid, v);
    const unsigned wy = (unsigned)rows[y] >> 8;
    const cl_i32x4 cx = *reinterpret_cast<const cl_i32x4*>(cols + x);
    unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {                                  // (a pixel beyond the row is zeros through in-range tables)
      const int kx0 = cx[pp] & 255, kx1 = min(kx0 + 1, tx - 1);
      const unsigned wx = (unsigned)cx[pp] >> 8;
      const unsigned ch[3] = {cl_byte(v, 3 * pp), cl_byte(v, 3 * pp + 1), cl_byte(v, 3 * pp + 2)};
      unsigned res[3] = {ch[0], ch[1], ch[2]};
      if (max(max(ch[0], ch[1]), ch[2]) >= floor) {
        if constexpr (P == 1) {
          const unsigned Y = cl_luma(ch[0], ch[1], ch[2]);
          const int delta = (int)cl_blend(sl + (kx0 << 8), sl + (kx1 << 8), sl + 4096 + (kx0 << 8), sl + 4096 + (kx1 << 8), Y, wy, wx) - (int)Y;
#pragma unroll
          for (int c = 0; c < 3; ++c) res[c] = (unsigned)min(max((int)ch[c] + delta, 0), 255);
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const unsigned char* __restrict__ l0 = sl + c * 4096;
            const unsigned char* __restrict__ l1 = sl + (P + c) * 4096;
            res[c] = cl_blend(l0 + (kx0 << 8), l0 + (kx1 << 8), l1 + (kx0 << 8), l1 + (kx1 << 8), ch[c], wy, wx);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int i = 3 * pp + c;
        o[i >> 2] |= res[c] << (8 * (i & 3));
      }
    }
    cl_store12(out + at, nvalid, o);
  }
}

// ================================================================================================ C ABI (include/wtpse_hip.h)
#define ST ((hipStream_t)stream)

static inline bool clahe_geometry_ok(int N, int H, int W, int ty, int tx, int floor, int planes) {
  return N > 0 && N < 65536 && H > 0 && H <= 4096 && W > 0 && W <= 4096 && ty > 0 && ty <= 16 && tx > 0 && tx <= 16 && ty <= H &&
         tx <= W && floor >= 0 && floor <= 255 && (planes == 1 || planes == 3);
}

extern "C" int wtpse_clahe_hist(const unsigned char* img, unsigned* hist, int N, int H, int W, int ty, int tx, int floor, int planes,
                                void* stream) {
  WTPSE_REQUIRE(img && hist && clahe_geometry_ok(N, H, W, ty, tx, floor, planes));
  const hipError_t e = hipMemsetAsync(hist, 0, (size_t)N * planes * ty * tx * 256 * sizeof(unsigned), ST);
  if (e != hipSuccess) return (int)e;
  const int largest = ((H + ty - 1) / ty) * ((W + tx - 1) / tx);    // (k L) // t steps by at most ceil(L / t)
  const dim3 grid((unsigned)((largest + CL_CHUNK - 1) / CL_CHUNK), (unsigned)(ty * tx), (unsigned)N);
  if (planes == 1)
    hipLaunchKernelGGL(clahe_hist_k<1>, grid, dim3(256), 0, ST, img, hist, H, W, ty, tx, (unsigned)floor);
  else
    hipLaunchKernelGGL(clahe_hist_k<3>, grid, dim3(256), 0, ST, img, hist, H, W, ty, tx, (unsigned)floor);
  return wtpse_status();
}

extern "C" int wtpse_clahe_lut(const unsigned* hist, unsigned char* lut, int count, int clip_q8, void* stream) {
  WTPSE_REQUIRE(hist && lut && count > 0 && count <= 65535 * 3 * 256 && clip_q8 >= 256 && clip_q8 <= 65536);
  hipLaunchKernelGGL(clahe_lut_k, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, ST, hist, lut, count, (unsigned)clip_q8);
  return wtpse_status();
}

extern "C" int wtpse_clahe_apply(const unsigned char* img, const unsigned char* lut, const int* rows, const int* cols,
                                 const int* bands, unsigned char* out, int N, int H, int W, int ty, int tx, int floor, int planes,
                                 void* stream) {
  WTPSE_REQUIRE(img && lut && rows && cols && bands && out && img != out && clahe_geometry_ok(N, H, W, ty, tx, floor, planes));
  WTPSE_REQUIRE(((uintptr_t)cols & 15) == 0 && ((uintptr_t)lut & 3) == 0);
  // a band reaches from one tile centre to the next (the first one also from the picture's edge): at most 1.5 tiles and a row
  const int longest = min(H, (3 * ((H + ty - 1) / ty)) / 2 + 2) * ((W + 3) / 4);
  const dim3 grid((unsigned)((longest + CL_APPLY_GROUPS - 1) / CL_APPLY_GROUPS), (unsigned)ty, (unsigned)N);
  if (planes == 1)
    hipLaunchKernelGGL(clahe_apply_k<1>, grid, dim3(256), 0, ST, img, lut, rows, cols, bands, out, H, W, ty, tx, (unsigned)floor);
  else
    hipLaunchKernelGGL(clahe_apply_k<3>, grid, dim3(256), 0, ST, img, lut, rows, cols, bands, out, H, W, ty, tx, (unsigned)floor);
  return wtpse_status();
}
