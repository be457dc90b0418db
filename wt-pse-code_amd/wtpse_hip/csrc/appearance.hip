// Random appearance networks (GIN + IPA): the optional stage of the input pipeline between amplitude mixing (spectrum.hip)
// and the image-quality stage (quality.hip).  A selected sample of the uint8 batch [N][S][S][3] is centred on its own mean, pushed
// through one or two shallow convolutional networks whose weights the host drew for this sample (input_pipeline.draw_appearance),
// mixed with the original, scaled back to the input's energy and — with two networks — blended through a smooth random field.  Every
// operation is fixed point (include/wtpse_hip.h has the formulas; input_pipeline.appearance_host is the same text in numpy int64), so
// the device equals the specification byte for byte.  The definition is this project's own: it is not byte-equal to anyone's float
// code.  The only floating-point instructions of this file are the three fp64 operations per net and sample that form the gain R_j
// (a division, a square root, a multiplication by 4096: each correctly rounded, on integers below 2^53), in appearance_finish_k.
//   appearance_nets_k   : one workgroup = one tile of A_TH rows x A_TW pixels of one sample.  The centred signal of the tile plus its
//                         4-pixel halo is staged in LDS as 32-bit values; the four layers of a net run through LDS planes, ping-pong,
//                         never written out between layers.  Layer l computes the positions that lie l + 1 rings inside the staged
//                         region (the valid region shrinks by one ring per layer, whatever its kernel size), and a position outside
//                         the picture is stored as 0 behind EVERY layer: zero padding at every layer, although the bias would make
//                         the value computed there non-zero.  The last layer's three channels stay in registers: z_j goes to the
//                         workspace, the tile's sums of squares into the sample's 64-bit integer energies (one atomic per workgroup
//                         and sum; integer adds in any order).  Net 1 reuses the LDS.
//   appearance_finish_k : the same tiles.  Thread 0 forms the gains R_j; the blend field of the tile comes from the control grid through
//                         the axis table, separably (rows of the grid along x into LDS, then along y per pixel); then per value the
//                         scaling, the blend, the mean, the clip and the byte store.
// The weights, biases, kernel sizes and flags of a sample are read at a workgroup-uniform address (scalar registers); a 1x1 layer
// skips the eight dead taps by a uniform branch; a sample that is not selected leaves pass 1 at once and is copied by pass 2.
// The 64-bit sums: a product reaches 2^33 and a layer adds 27 of them, so every multiply-add is 32 x 32 + 64 -> 64 bits.
#include "common.h"

#define A_TW 64                                  // pixels of a tile along x
#define A_TH 32                                  // rows of a tile
#define A_HALO 4                                 // one ring per layer
#define A_LAYERS 4
#define A_NET_COLS 193                           // k[4], weights [180], biases [9]
#define A_COLS (3 + 2 * A_NET_COLS)              // flags, alpha_0, alpha_1, net 0, net 1
#define A_CL 524287                              // 2^19 - 1
#define A_PROWS 12                               // control rows a tile can touch: 32 / 4 + 4
#define A_PCOLS 20                               // control columns: 64 / 4 + 4
constexpr int A_W = A_TW + 2 * A_HALO;           // 72
constexpr int A_H = A_TH + 2 * A_HALO;           // 40
constexpr int A_PLANE = A_W * A_H;               // 2880 values of one channel
constexpr int A_GROUPS = A_TW / 4;               // 12-byte groups per tile row (pass 2)

typedef int a_i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned a_byte(const unsigned* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }

// `nvalid` (0 .. 12) bytes at p -> three dwords, little endian; the bytes beyond nvalid are not read (0)
__device__ __forceinline__ void a_load12(const unsigned char* __restrict__ p, int nvalid, unsigned v[3]) {
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
__device__ __forceinline__ void a_store12(unsigned char* __restrict__ p, int nvalid, const unsigned v[3]) {
  if (nvalid == 12 && ((uintptr_t)p & 3) == 0) {
    unsigned* q = reinterpret_cast<unsigned*>(p);
    q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (i < nvalid) p[i] = (unsigned char)a_byte(v, i);
  }
}
// 12 ints at p (4-byte aligned) -> z[12]; those beyond nvalid are not read (0)
__device__ __forceinline__ void a_load12i(const int* __restrict__ p, int nvalid, int z[12]) {
  if (nvalid == 12 && ((uintptr_t)p & 15) == 0) {
    const a_i32x4* q = reinterpret_cast<const a_i32x4*>(p);
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const a_i32x4 t = q[v];
#pragma unroll
      for (int i = 0; i < 4; ++i) z[4 * v + i] = t[i];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i) z[i] = i < nvalid ? p[i] : 0;
  }
}

// m8 = (256 SUM + cnt / 2) / cnt <= 65280 by shift and subtract, as quality_apply_k forms the same pivot: the compiler's division
// starts from a floating-point reciprocal
__device__ __forceinline__ int a_mean_q8(unsigned sum, int S) {
  const unsigned long long cnt = 3ull * (unsigned)S * (unsigned)S;
  unsigned long long rem = 256ull * sum + (cnt >> 1);
  unsigned m = 0u;
#pragma unroll
  for (int bit = 15; bit >= 0; --bit) {
    const unsigned long long d = cnt << bit;
    if (d <= rem) {
      rem -= d;
      m |= 1u << bit;
    }
  }
  return (int)m;
}

// One output position of one layer: `in` = the CIN input planes in LDS, idx = the position within a plane, w = W[COUT][CIN][3][3]
// (Q12), bias[COUT] (Q8), both at uniform addresses -> v[COUT] behind the shift, the bias, the leak and the clip.
template <int CIN, int COUT, bool LEAK>
__device__ __forceinline__ void a_point(const int* in, int idx, const int* __restrict__ w, const int* __restrict__ bias, bool k3,
                                        int v[COUT]) {
  long long acc[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) acc[co] = 0;
  if (k3) {
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci)
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int h = in[ci * A_PLANE + idx + (dy - 1) * A_W + (dx - 1)];
#pragma unroll
          for (int co = 0; co < COUT; ++co) acc[co] += (long long)w[((co * CIN + ci) * 3 + dy) * 3 + dx] * (long long)h;
        }
  } else {
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) {
      const int h = in[ci * A_PLANE + idx];
#pragma unroll
      for (int co = 0; co < COUT; ++co) acc[co] += (long long)w[(co * CIN + ci) * 9 + 4] * (long long)h;
    }
  }
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    int t = (int)((acc[co] + 2048) >> 12) + bias[co];
    if (LEAK && t < 0) t = (3 * t + 128) >> 8;
    v[co] = min(max(t, -A_CL), A_CL);
  }
}

// A hidden layer over the positions M rings inside the staged region: `in` -> `out` (LDS planes that do not overlap).  (gy0, gx0):
// the picture coordinates of the region's first position.  Outside the picture the output is 0.
template <int CIN, int COUT, int M>
__device__ __forceinline__ void a_layer(const int* in, int* out, const int* __restrict__ w, const int* __restrict__ bias, bool k3,
                                        int gy0, int gx0, int S, int tid) {
  constexpr int RW = A_W - 2 * M, RH = A_H - 2 * M;
  for (int e = tid; e < RW * RH; e += 256) {
    const int ry = e / RW + M, rx = e % RW + M;
    const int idx = ry * A_W + rx;
    const bool inside = (unsigned)(gy0 + ry) < (unsigned)S && (unsigned)(gx0 + rx) < (unsigned)S;
    int v[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) v[co] = 0;
    if (inside) a_point<CIN, COUT, true>(in, idx, w, bias, k3, v);
#pragma unroll
    for (int co = 0; co < COUT; ++co) out[co * A_PLANE + idx] = v[co];
  }
}

__device__ __forceinline__ unsigned long long a_wave_sum(unsigned long long v) {
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), m, 64);
    v += ((unsigned long long)hi << 32) | lo;
  }
  return v;
}

// energy [N][3] = (E_in, E_0, E_1), zero on entry; z [N][2][S][S][3]
__global__ __launch_bounds__(256) void appearance_nets_k(const unsigned char* __restrict__ img, const int* __restrict__ params,
                                                         const unsigned* __restrict__ sums, unsigned long long* __restrict__ energy,
                                                         int* __restrict__ z, int S) {
  __shared__ int plane[5 * A_PLANE];             // A = planes 0, 1; B = planes 2, 3; the centred input = planes 2, 3, 4
  __shared__ unsigned long long part[4][3];
  const int n = blockIdx.z, tid = threadIdx.x;
  const int* __restrict__ prm = params + (size_t)n * A_COLS;
  const int flags = prm[0];
  if (!(flags & 1)) return;                                         // not selected: pass 2 copies the sample
  const int x0 = (int)blockIdx.x * A_TW, y0 = (int)blockIdx.y * A_TH;
  const int gx0 = x0 - A_HALO, gy0 = y0 - A_HALO;
  const int m8 = a_mean_q8(sums[n], S);
  const unsigned char* __restrict__ src = img + (size_t)n * S * S * 3;
  int* pa = plane;
  int* pb = plane + 2 * A_PLANE;
  const int nnets = (flags & 2) ? 2 : 1;
  unsigned long long e_in = 0ull, e_net[2] = {0ull, 0ull};

  for (int j = 0; j < nnets; ++j) {
    const int* __restrict__ net = prm + 3 + j * A_NET_COLS;
    const int alpha = prm[1 + j];
    // ---- stage the centred input: rows y0 - 4 .. y0 + 35, pixels x0 - 4 .. x0 + 67; 0 outside the picture
    // (all of a thread's byte loads are issued before the first is used: one round trip per net instead of twelve)
    {
      constexpr int TRIPS = (A_PLANE + 255) / 256;
      int c[TRIPS][3];
#pragma unroll
      for (int t = 0; t < TRIPS; ++t) {
        const int e = tid + 256 * t;
        const int ry = e / A_W, rx = e - ry * A_W;
        const int gy = gy0 + ry, gx = gx0 + rx;
        const bool inside = e < A_PLANE && (unsigned)gy < (unsigned)S && (unsigned)gx < (unsigned)S;
        const unsigned char* __restrict__ p = src + (inside ? ((size_t)gy * S + gx) * 3 : 0);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int v = p[ch];                                      // unconditional, at an address that is always valid
          c[t][ch] = inside ? (v << 8) - m8 : 0;
        }
      }
#pragma unroll
      for (int t = 0; t < TRIPS; ++t) {
        const int e = tid + 256 * t;
        if (e < A_PLANE) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) pb[ch * A_PLANE + e] = c[t][ch];
        }
      }
    }
    __syncthreads();
    a_layer<3, 2, 1>(pb, pa, net + 4, net + 184, net[0] == 3, gy0, gx0, S, tid);
    __syncthreads();
    a_layer<2, 2, 2>(pa, pb, net + 4 + 54, net + 184 + 2, net[1] == 3, gy0, gx0, S, tid);
    __syncthreads();
    a_layer<2, 2, 3>(pb, pa, net + 4 + 90, net + 184 + 4, net[2] == 3, gy0, gx0, S, tid);
    __syncthreads();
    // ---- the last layer on the tile itself, the mix with the original, the store and the energies
    int* __restrict__ zj = z + ((size_t)n * 2 + j) * S * S * 3;
    const bool k3 = net[3] == 3;
    constexpr int OUT_TRIPS = A_TW * A_TH / 256;
    int xin[OUT_TRIPS][3];                                          // the tile's own bytes, all loads in flight at once
#pragma unroll
    for (int t = 0; t < OUT_TRIPS; ++t) {
      const int e = tid + 256 * t;
      const int gy = min(y0 + e / A_TW, S - 1), gx = min(x0 + e % A_TW, S - 1);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) xin[t][ch] = src[((size_t)gy * S + gx) * 3 + ch];
    }
#pragma unroll
    for (int t = 0; t < OUT_TRIPS; ++t) {
      const int e = tid + 256 * t;
      const int ry = e / A_TW, rx = e % A_TW;
      const int gy = y0 + ry, gx = x0 + rx;
      if (gy >= S || gx >= S) continue;
      int y[3];
      a_point<2, 3, false>(pa, (ry + A_HALO) * A_W + rx + A_HALO, net + 4 + 126, net + 184 + 6, k3, y);
      const size_t o = ((size_t)gy * S + gx) * 3;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int c0 = (xin[t][ch] << 8) - m8;
        const int zz = (alpha * c0 + (256 - alpha) * y[ch] + 128) >> 8;
        zj[o + ch] = zz;
        const int q = (zz + 8) >> 4;
        e_net[j] += (unsigned)(q * q);
        if (j == 0) {
          const int q0 = (c0 + 8) >> 4;
          e_in += (unsigned)(q0 * q0);
        }
      }
    }
    __syncthreads();                                                // net 1 stages over what this loop read
  }
  e_in = a_wave_sum(e_in);
  e_net[0] = a_wave_sum(e_net[0]);
  e_net[1] = a_wave_sum(e_net[1]);
  if ((tid & 63) == 0) {
    part[tid >> 6][0] = e_in;
    part[tid >> 6][1] = e_net[0];
    part[tid >> 6][2] = e_net[1];
  }
  __syncthreads();
  if (tid < 3) {
    const unsigned long long t = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
    if (t) atomicAdd(energy + (size_t)n * 3 + tid, t);
  }
}

// R_j = min(rint(sqrt(E_in / E_j) * 4096), 2^20): the three fp64 operations of the stage, each correctly rounded, on exact integers
__device__ __forceinline__ int a_gain(unsigned long long e_in, unsigned long long e_j) {
  if (e_j == 0ull) return 4096;
  const double r = rint(sqrt((double)e_in / (double)e_j) * 4096.0);
  return r > 1048576.0 ? 1048576 : (int)r;
}

__global__ __launch_bounds__(256) void appearance_finish_k(const unsigned char* __restrict__ img, const int* __restrict__ params,
                                                           const int* __restrict__ field, const int* __restrict__ axis,
                                                           const unsigned* __restrict__ sums,
                                                           const unsigned long long* __restrict__ energy, const int* __restrict__ z,
                                                           unsigned char* __restrict__ out, int S, int G) {
  __shared__ int ctl[A_PROWS * A_PCOLS];         // the control values the tile touches
  __shared__ int hx[A_PROWS * A_TW];             // their rows interpolated along x, Q8 of 0 .. 256
  __shared__ int gain[4];                        // R_0, R_1, E_0 == 0, E_1 == 0
  const int n = blockIdx.z, tid = threadIdx.x;
  const int x0 = (int)blockIdx.x * A_TW, y0 = (int)blockIdx.y * A_TH;
  const int rows_out = min(A_TH, S - y0), row_bytes = 3 * S;
  const int* __restrict__ prm = params + (size_t)n * A_COLS;
  const int flags = prm[0];
  const unsigned char* __restrict__ src = img + (size_t)n * S * row_bytes;
  unsigned char* __restrict__ dst = out + (size_t)n * S * row_bytes;

  if (!(flags & 1)) {                                               // not selected: a copy
    for (int e = tid; e < rows_out * A_GROUPS; e += 256) {
      const int y = y0 + e / A_GROUPS, x = x0 + (e % A_GROUPS) * 4;
      const int nvalid = min(12, (S - x) * 3);
      if (nvalid <= 0) continue;
      unsigned v[3];
      a_load12(src + (size_t)y * row_bytes + x * 3, nvalid, v);
      a_store12(dst + (size_t)y * row_bytes + x * 3, nvalid, v);
    }
    return;
  }
  const bool blend = (flags & 2) != 0;
  const int m8 = a_mean_q8(sums[n], S);
  if (tid == 0) {
    const unsigned long long e_in = energy[(size_t)n * 3], e0 = energy[(size_t)n * 3 + 1], e1 = energy[(size_t)n * 3 + 2];
    gain[0] = a_gain(e_in, e0);
    gain[1] = blend ? a_gain(e_in, e1) : 4096;
    gain[2] = e0 == 0ull;
    gain[3] = blend && e1 == 0ull;
  }
  int iy0 = 0, ix0 = 0;
  if (blend) {
    // the tile's rows and columns of the control grid; every index is clamped into the grid and into the LDS arrays, so a table
    // that does not belong to (S, G) gives wrong values and nothing else
    iy0 = min(max(axis[y0 * 5], 0), G - 4);
    ix0 = min(max(axis[x0 * 5], 0), G - 4);
    const int iy1 = min(max(axis[(y0 + rows_out - 1) * 5], iy0), G - 4), ix1 = min(max(axis[min(x0 + A_TW, S) * 5 - 5], ix0), G - 4);
    const int nr = min(iy1 - iy0 + 4, A_PROWS), nc = min(ix1 - ix0 + 4, A_PCOLS);
    const int* __restrict__ P = field + (size_t)n * G * G;
    for (int e = tid; e < nr * nc; e += 256) {
      const int r = e / nc, c = e - r * nc;
      ctl[r * A_PCOLS + c] = P[(iy0 + r) * G + ix0 + c];
    }
    __syncthreads();
    for (int e = tid; e < nr * A_TW; e += 256) {
      const int r = e / A_TW, xl = e % A_TW;
      const int gx = min(x0 + xl, S - 1);
      const int* __restrict__ t = axis + gx * 5;
      const int c = min(max(t[0] - ix0, 0), A_PCOLS - 4);
      const int* row = ctl + r * A_PCOLS + c;
      hx[e] = (t[1] * row[0] + t[2] * row[1] + t[3] * row[2] + t[4] * row[3] + 8) >> 4;
    }
  }
  __syncthreads();
  const int R0 = gain[0], R1 = gain[1];
  const bool keep0 = gain[2] != 0, keep1 = gain[3] != 0;
  const int* __restrict__ z0 = z + (size_t)n * 2 * S * S * 3;
  const int* __restrict__ z1 = z0 + (size_t)S * S * 3;

  for (int e = tid; e < rows_out * A_GROUPS; e += 256) {
    const int r = e / A_GROUPS, g = e % A_GROUPS;
    const int y = y0 + r, x = x0 + 4 * g;
    const int nvalid = min(12, (S - x) * 3);
    if (nvalid <= 0) continue;
    const size_t o = (size_t)y * row_bytes + x * 3;
    unsigned v[3];
    a_load12(src + o, nvalid, v);
    int b[4] = {256, 256, 256, 256};
    int za[12], zb[12];
    a_load12i(z0 + o, nvalid, za);
    if (blend) {
      a_load12i(z1 + o, nvalid, zb);
      const int* __restrict__ t = axis + y * 5;
      const int rl = min(max(t[0] - iy0, 0), A_PROWS - 4);
      const int* col = hx + rl * A_TW + 4 * g;
#pragma unroll
      for (int pp = 0; pp < 4; ++pp)
        b[pp] = (t[1] * col[pp] + t[2] * col[A_TW + pp] + t[3] * col[2 * A_TW + pp] + t[4] * col[3 * A_TW + pp] + (1 << 19)) >> 20;
    }
    unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int c0 = (int)(a_byte(v, i) << 8) - m8;
      const long long s0 = (long long)R0 * (long long)(keep0 ? c0 : za[i]);
      const int g0 = (int)min(max((s0 + 2048) >> 12, (long long)-A_CL), (long long)A_CL);
      int t = 256 * g0;
      if (blend) {
        const long long s1 = (long long)R1 * (long long)(keep1 ? c0 : zb[i]);
        const int g1 = (int)min(max((s1 + 2048) >> 12, (long long)-A_CL), (long long)A_CL);
        t = b[i / 3] * g0 + (256 - b[i / 3]) * g1;
      }
      t = m8 + ((t + 128) >> 8);
      // the clip in front of the shift: quality.hip has the reason (the packed shift-and-clip instruction)
      const unsigned u = (unsigned)min(max(t + 128, 0), 65535) >> 8;
      w[i >> 2] |= u << (8 * (i & 3));
    }
    a_store12(dst + o, nvalid, w);
  }
}

// ================================================================================================ C ABI (include/wtpse_hip.h)
#define ST ((hipStream_t)stream)

// 4-byte words: energies [N][3] of 64 bits, byte sums [N], padding to 16 bytes, z [N][2][S][S][3]
static inline long long a_z_offset(int N) { return ((long long)7 * N + 3) & ~3ll; }

extern "C" int wtpse_appearance_workspace(int N, int S) {
  if (N <= 0 || N >= 65536 || S <= 0 || S > 512) return -1;
  const long long words = a_z_offset(N) + 6ll * N * S * S;
  return words > 2147483647ll ? -1 : (int)words;
}

extern "C" int wtpse_appearance_nets(const unsigned char* img, const int* params, void* work, int N, int S, void* stream) {
  WTPSE_REQUIRE(img && params && work && ((uintptr_t)work & 15) == 0 && wtpse_appearance_workspace(N, S) > 0);
  unsigned* words = static_cast<unsigned*>(work);
  const hipError_t e = hipMemsetAsync(words, 0, (size_t)N * 3 * sizeof(unsigned long long), ST);
  if (e != hipSuccess) return (int)e;
  const int rc = wtpse_quality_sums(img, words + 6 * (size_t)N, N, S, stream);
  if (rc != WTPSE_OK) return rc;
  const dim3 grid((unsigned)((S + A_TW - 1) / A_TW), (unsigned)((S + A_TH - 1) / A_TH), (unsigned)N);
  hipLaunchKernelGGL(appearance_nets_k, grid, dim3(256), 0, ST, img, params, words + 6 * (size_t)N,
                     reinterpret_cast<unsigned long long*>(words), reinterpret_cast<int*>(words + a_z_offset(N)), S);
  return wtpse_status();
}

extern "C" int wtpse_appearance_finish(const unsigned char* img, const int* params, const int* field, const int* axis,
                                       const void* work, unsigned char* out, int N, int S, int G, void* stream) {
  WTPSE_REQUIRE(img && params && field && axis && work && out && img != out && ((uintptr_t)work & 15) == 0);
  WTPSE_REQUIRE(wtpse_appearance_workspace(N, S) > 0 && G >= 4 && G <= 131);
  const unsigned* words = static_cast<const unsigned*>(work);
  const dim3 grid((unsigned)((S + A_TW - 1) / A_TW), (unsigned)((S + A_TH - 1) / A_TH), (unsigned)N);
  hipLaunchKernelGGL(appearance_finish_k, grid, dim3(256), 0, ST, img, params, field, axis, words + 6 * (size_t)N,
                     reinterpret_cast<const unsigned long long*>(words), reinterpret_cast<const int*>(words + a_z_offset(N)), out, S, G);
  return wtpse_status();
}
