// JPEG compression augmentation: the optional stage of the input pipeline between the image-quality stage (quality.hip) and CLAHE
// (clahe.hip).  Baseline JPEG's round trip of the pixels on the uint8 batch [N][S][S][3], S a multiple of 16 — colour conversion,
// 2 x 2 chroma downsampling, libjpeg's "islow" forward DCT, quantisation, dequantisation, the "islow" inverse DCT, "fancy" chroma
// upsampling and the colour conversion back — without the entropy coder, which is lossless.  The draws stay on the host
// (input_pipeline.draw_jpeg) and the pixels on the GPU.  Every operation is libjpeg's 32-bit integer arithmetic
// (include/wtpse_hip.h has the formulas; input_pipeline.jpeg_host is the same text in numpy int64, pinned byte for byte to Pillow's
// save and open), so the device equals the specification byte for byte and no floating-point instruction occurs in this file:
// the quantiser divides by a multiply-high with a host-computed reciprocal, and no index is divided by a run-time value.
//   jpeg_chroma_k : 4:2:0 samples only.  One workgroup = J_CT x J_CT pixels of one sample -> its 32 x 32 decoded chroma samples
//                   of both planes, written to the workspace [N][2][S/2][S/2] (a pixel's chroma needs the decoded samples one
//                   step away in each direction, which belong to neighbouring MCUs: they meet in the second launch)
//   jpeg_apply_k  : one workgroup = J_TW x J_TH pixels of one sample.  Luma always, chroma too in 4:4:4; in 4:2:0 the chroma
//                   comes out of the workspace (a halo of one sample, indices clamped: libjpeg's edge cases are exactly the clamp),
//                   is upsampled, and the decoded tile is written once.  A mode-0 sample is copied without touching LDS.
// The mode and the tables of a sample depend on blockIdx.z alone: every mode branch is uniform over the workgroup.
// The 8 x 8 transforms run one lane per row, then one lane per column, then one lane per row, through LDS: the column task runs
// the forward DCT's second pass, the quantiser and the inverse DCT's first pass on the eight values it holds.  A block sits in LDS as
// 8 rows of 9 ints (J_BS = 72 per block): 4-byte LDS accesses are served per 32-lane half with bank = dword address mod 32, and a
// half — 4 blocks x 8 rows or columns — then hits 32 different banks in the row passes (8 (b + r) + r + i) and in the column pass
// (8 (b + j) + j + c) alike.
#include "common.h"

#define J_TW 64                                  // pixels of jpeg_apply_k's tile along x
#define J_TH 32                                  // its rows
#define J_CT 64                                  // jpeg_chroma_k's tile: J_CT x J_CT pixels
constexpr int J_BS = 72;                         // ints per 8 x 8 block in LDS: 8 rows, 9 apart
constexpr int J_BPR = J_TW / 8;                  // blocks per tile row of jpeg_apply_k
constexpr int J_NB = J_BPR * (J_TH / 8);         // blocks per plane of its tile
constexpr int J_CBPR = J_CT / 16;                // chroma blocks per tile row of jpeg_chroma_k
constexpr int J_CNB = J_CBPR * J_CBPR;
constexpr int J_VPR = J_TW * 3 / 16;             // 16-byte vectors per staged row (both kernels: J_CT == J_TW)
constexpr int J_HW = J_TW / 2 + 2;               // the chroma halo of jpeg_apply_k's tile: samples per row ...
constexpr int J_HH = J_TH / 2 + 2;               // ... and rows
constexpr int J_HP = 40;                         // bytes per halo row in LDS: sample (row, col) at byte row * J_HP + col + 3
static_assert(J_HP % 4 == 0 && J_HW + 3 <= J_HP && ((J_TW / 2 - 2 + 3) & ~3) + 8 <= J_HP, "two aligned dwords cover any four halo samples");
static_assert(J_CT == J_TW && J_TW % 16 == 0 && J_TH % 16 == 0 && J_CT % 16 == 0, "whole MCUs; one staging width");

typedef unsigned int j_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int j_at(int b, int r, int c) { return b * J_BS + r * 9 + c; }
__device__ __forceinline__ int j_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int j_clamp(int v) { return min(max(v, 0), 255); }
__device__ __forceinline__ int j_byte(const unsigned* w, int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }

__device__ __forceinline__ int j_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int j_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16; }
__device__ __forceinline__ int j_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16; }

// libjpeg's jfdctint.c on eight values: the row pass (outputs 0 and 4 times 4, the others DESCALE 11) or the column pass (outputs 0
// and 4 DESCALE 2, the others DESCALE 15)
template <bool ROWS>
__device__ __forceinline__ void j_fdct8(int d[8]) {
  constexpr int n = ROWS ? 11 : 15;
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = ROWS ? (t10 + t11) * 4 : j_descale(t10 + t11, 2);
  d[4] = ROWS ? (t10 - t11) * 4 : j_descale(t10 - t11, 2);
  int z1 = (t12 + t13) * 4433;
  d[2] = j_descale(z1 + t13 * 6270, n);
  d[6] = j_descale(z1 - t12 * 15137, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7] = j_descale(a4 + z1 + z3, n);
  d[5] = j_descale(a5 + z2 + z4, n);
  d[3] = j_descale(a6 + z2 + z3, n);
  d[1] = j_descale(a7 + z1 + z4, n);
}

// libjpeg's jidctint.c on eight values: N = 11 the column pass, N = 18 the row pass
template <int N>
__device__ __forceinline__ void j_idct8(int d[8]) {
  int z2 = d[2], z3 = d[6];
  int z1 = (z2 + z3) * 4433;
  const int t2 = z1 - z3 * 15137, t3 = z1 + z2 * 6270;
  const int t0 = (d[0] + d[4]) * 8192, t1 = (d[0] - d[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int o0 = d[7], o1 = d[5], o2 = d[3], o3 = d[1];
  z1 = o0 + o3;
  z2 = o1 + o2;
  z3 = o0 + o2;
  int z4 = o1 + o3;
  const int z5 = (z3 + z4) * 9633;
  o0 *= 2446;
  o1 *= 16819;
  o2 *= 25172;
  o3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  o0 += z1 + z3;
  o1 += z2 + z4;
  o2 += z2 + z3;
  o3 += z1 + z4;
  d[0] = j_descale(t10 + o3, N);
  d[7] = j_descale(t10 - o3, N);
  d[1] = j_descale(t11 + o2, N);
  d[6] = j_descale(t11 - o2, N);
  d[2] = j_descale(t12 + o1, N);
  d[5] = j_descale(t12 - o1, N);
  d[3] = j_descale(t13 + o0, N);
  d[4] = j_descale(t13 - o0, N);
}

// Sample's tables -> LDS: q[0 .. 127] the two tables, q[128 .. 255] their reciprocals.  256 threads.
__device__ __forceinline__ void j_load_tables(const int* __restrict__ tables, const int* __restrict__ recips, int n, int tid, int* q) {
  q[tid] = tid < 128 ? tables[(size_t)n * 128 + tid] : recips[(size_t)n * 128 + tid - 128];
}

// The codec on `nplanes` planes of level-shifted samples in LDS (block slot b = by * BPR + bx of plane p at planes + (p * NB + b) *
// J_BS; only the slots with bx < bw and by < bh hold data): in place -> the decoded samples 0 .. 255.  Plane p quantises with table
// min(p + tab0, 1).  Every thread of the workgroup calls; the planes are written and `q` is loaded before, behind a barrier that
// this function starts with.
template <int BPR, int NB>
__device__ __forceinline__ void j_codec(int* planes, int nplanes, int tab0, int bw, int bh, const int* q, int tid) {
  const int ntask = nplanes * NB * 8;
  __syncthreads();
  for (int t = tid; t < ntask; t += 256) {                           // forward DCT, rows
    const int slot = t >> 3, r = t & 7, b = slot % NB;
    if (b % BPR >= bw || b / BPR >= bh) continue;
    int* p = planes + j_at(slot, r, 0);
    int d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = p[i];
    j_fdct8<true>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = d[i];
  }
  __syncthreads();
  for (int t = tid; t < ntask; t += 256) {                           // forward DCT, columns; quantiser; inverse DCT, columns
    const int slot = t >> 3, c = t & 7, b = slot % NB;
    if (b % BPR >= bw || b / BPR >= bh) continue;
    const int* qt = q + 64 * min(slot / NB + tab0, 1) + c;
    int* p = planes + j_at(slot, 0, c);
    int d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = p[9 * j];
    j_fdct8<false>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int Q = qt[8 * j], k = __mulhi(abs(d[j]) + ((8 * Q) >> 1), qt[128 + 8 * j]);
      d[j] = (d[j] < 0 ? -k : k) * Q;
    }
    j_idct8<11>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) p[9 * j] = d[j];
  }
  __syncthreads();
  for (int t = tid; t < ntask; t += 256) {                           // inverse DCT, rows; level shift and clamp
    const int slot = t >> 3, r = t & 7, b = slot % NB;
    if (b % BPR >= bw || b / BPR >= bh) continue;
    int* p = planes + j_at(slot, r, 0);
    int d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = p[i];
    j_idct8<18>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = j_clamp(d[i] + 128);
  }
  __syncthreads();
}

// rows y0 .. y0 + th - 1, pixels x0 .. x0 + tw - 1 of a sample -> stage, J_VPR 16-byte vectors per row (tw a multiple of 16: whole
// vectors; 3 S and 3 x0 are multiples of 16 bytes)
__device__ __forceinline__ void j_stage(const unsigned char* __restrict__ src, int S, int x0, int y0, int tw, int th, int tid, j_u32x4* stage) {
  const int vpr = tw * 3 / 16;
  for (int e = tid; e < th * J_VPR; e += 256) {
    const int r = e / J_VPR, v = e % J_VPR;
    if (v < vpr) stage[e] = *reinterpret_cast<const j_u32x4*>(src + ((size_t)(y0 + r) * S + x0) * 3 + 16 * v);
  }
}

__global__ __launch_bounds__(256) void jpeg_chroma_k(const unsigned char* __restrict__ img, const int* __restrict__ mode,
                                                     const int* __restrict__ tables, const int* __restrict__ recips,
                                                     unsigned char* __restrict__ chroma, int S) {
  const int n = blockIdx.z, tid = threadIdx.x;
  if (mode[n] != 2) return;
  __shared__ j_u32x4 stage[J_CT * J_VPR];        // the tile's bytes
  __shared__ int planes[2 * J_CNB * J_BS];       // Cb and Cr at half resolution
  __shared__ int q[256];
  const int x0 = (int)blockIdx.x * J_CT, y0 = (int)blockIdx.y * J_CT;
  const int tw = min(J_CT, S - x0), th = min(J_CT, S - y0), H = S >> 1;
  j_load_tables(tables, recips, n, tid, q);
  j_stage(img + (size_t)n * S * S * 3, S, x0, y0, tw, th, tid, stage);
  __syncthreads();
  // ---- colour conversion and 2 x 2 downsampling: a task = two chroma samples side by side = 4 pixels (12 bytes) of two rows
  const unsigned* sw = reinterpret_cast<const unsigned*>(stage);
  for (int e = tid; e < (J_CT / 2) * (J_CT / 4); e += 256) {
    const int cy = e / (J_CT / 4), g = e % (J_CT / 4);               // chroma row, group of 4 pixels
    if (4 * g >= tw || 2 * cy >= th) continue;
    int cb[2] = {1, 2}, cr[2] = {1, 2};                              // the bias: 1 in even output columns, 2 in odd ones (x0 / 2 is even)
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      unsigned w[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) w[i] = sw[(2 * cy + rr) * (J_VPR * 4) + 3 * g + i];
#pragma unroll
      for (int pp = 0; pp < 4; ++pp) {
        const int R = j_byte(w, 3 * pp), G = j_byte(w, 3 * pp + 1), B = j_byte(w, 3 * pp + 2);
        cb[pp >> 1] += j_cb(R, G, B);
        cr[pp >> 1] += j_cr(R, G, B);
      }
    }
    const int cx = 2 * g, b = (cy >> 3) * J_CBPR + (cx >> 3);
    int* p = planes + j_at(b, cy & 7, cx & 7);
    p[0] = (cb[0] >> 2) - 128;
    p[1] = (cb[1] >> 2) - 128;
    p[J_CNB * J_BS] = (cr[0] >> 2) - 128;
    p[J_CNB * J_BS + 1] = (cr[1] >> 2) - 128;
  }
  j_codec<J_CBPR, J_CNB>(planes, 2, 1, tw >> 4, th >> 4, q, tid);
  // ---- the decoded samples to the workspace, 4 bytes at a time
  for (int e = tid; e < 2 * (J_CT / 2) * (J_CT / 8); e += 256) {
    const int g = e % (J_CT / 8), cy = (e / (J_CT / 8)) % (J_CT / 2), pl = e / ((J_CT / 8) * (J_CT / 2));
    if (8 * g >= tw || 2 * cy >= th) continue;
    const int cx = 4 * g, b = (cy >> 3) * J_CBPR + (cx >> 3);
    const int* p = planes + pl * J_CNB * J_BS + j_at(b, cy & 7, cx & 7);
    const unsigned v = (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16 | (unsigned)p[3] << 24;
    *reinterpret_cast<unsigned*>(chroma + ((size_t)(2 * n + pl) * H + (y0 >> 1) + cy) * H + (x0 >> 1) + cx) = v;
  }
}

__global__ __launch_bounds__(256) void jpeg_apply_k(const unsigned char* __restrict__ img, const int* __restrict__ mode,
                                                    const int* __restrict__ tables, const int* __restrict__ recips,
                                                    const unsigned char* __restrict__ chroma, unsigned char* __restrict__ out, int S) {
  const int n = blockIdx.z, tid = threadIdx.x, m = mode[n];
  const int x0 = (int)blockIdx.x * J_TW, y0 = (int)blockIdx.y * J_TH;
  const int tw = min(J_TW, S - x0), th = min(J_TH, S - y0);
  const unsigned char* __restrict__ src = img + (size_t)n * S * S * 3;
  unsigned char* __restrict__ dst = out + (size_t)n * S * S * 3;
  if (m == 0) {                                                       // neutral: a copy, no LDS
    const int vpr = tw * 3 / 16;
    for (int e = tid; e < th * J_VPR; e += 256) {
      const int r = e / J_VPR, v = e % J_VPR;
      const size_t off = ((size_t)(y0 + r) * S + x0) * 3 + 16 * v;
      if (v < vpr) *reinterpret_cast<j_u32x4*>(dst + off) = *reinterpret_cast<const j_u32x4*>(src + off);
    }
    return;
  }
  __shared__ j_u32x4 stage[J_TH * J_VPR];        // the tile's bytes, in and out
  __shared__ int planes[3 * J_NB * J_BS];        // Y, and in 4:4:4 Cb and Cr
  __shared__ int q[256];
  __shared__ unsigned halo[2 * J_HH * J_HP / 4];   // 4:2:0: the decoded chroma under the tile and one sample around it, bytes
  const int nplanes = m == 1 ? 3 : 1;
  j_load_tables(tables, recips, n, tid, q);
  j_stage(src, S, x0, y0, tw, th, tid, stage);
  if (m == 2) {
    const int H = S >> 1, cx0 = (x0 >> 1) - 1, cy0 = (y0 >> 1) - 1;
    for (int e = tid; e < 2 * J_HH * J_HW; e += 256) {
      const int hx = e % J_HW, hy = (e / J_HW) % J_HH, pl = e / (J_HW * J_HH);
      const int gx = min(max(cx0 + hx, 0), H - 1), gy = min(max(cy0 + hy, 0), H - 1);
      reinterpret_cast<unsigned char*>(halo)[(pl * J_HH + hy) * J_HP + hx + 3] = chroma[((size_t)(2 * n + pl) * H + gy) * H + gx];
    }
  }
  __syncthreads();
  // ---- colour conversion forward: a task = 4 pixels = 12 bytes of a row, all in one block
  unsigned* sw = reinterpret_cast<unsigned*>(stage);
  for (int e = tid; e < J_TH * (J_TW / 4); e += 256) {
    const int r = e / (J_TW / 4), g = e % (J_TW / 4);
    if (4 * g >= tw || r >= th) continue;
    unsigned w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = sw[r * (J_VPR * 4) + 3 * g + i];
    int* p = planes + j_at((r >> 3) * J_BPR + (g >> 1), r & 7, (4 * g) & 7);
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
      const int R = j_byte(w, 3 * pp), G = j_byte(w, 3 * pp + 1), B = j_byte(w, 3 * pp + 2);
      p[pp] = j_y(R, G, B) - 128;
      if (m == 1) {
        p[J_NB * J_BS + pp] = j_cb(R, G, B) - 128;
        p[2 * J_NB * J_BS + pp] = j_cr(R, G, B) - 128;
      }
    }
  }
  j_codec<J_BPR, J_NB>(planes, nplanes, 0, tw >> 3, th >> 3, q, tid);
  // ---- chroma (4:2:0: fancy upsampling out of the halo) and the colour conversion back, into the staging buffer
  for (int e = tid; e < J_TH * (J_TW / 4); e += 256) {
    const int r = e / (J_TW / 4), g = e % (J_TW / 4);
    if (4 * g >= tw || r >= th) continue;
    const int* p = planes + j_at((r >> 3) * J_BPR + (g >> 1), r & 7, (4 * g) & 7);
    int cb[4], cr[4];
    if (m == 1) {
#pragma unroll
      for (int pp = 0; pp < 4; ++pp) {
        cb[pp] = p[J_NB * J_BS + pp];
        cr[pp] = p[2 * J_NB * J_BS + pp];
      }
    } else {
      // pixels 4 g .. 4 g + 3 lie over chroma columns 2 g, 2 g + 1 = halo columns 2 g + 1, 2 g + 2; the near row is halo row
      // (r >> 1) + 1, the far one above it for an even r and below for an odd one.  Halo columns 2 g .. 2 g + 3 are the bytes from
      // 2 g + 3 on: two aligned dwords and a byte shift instead of four byte reads
      const int hn = (r >> 1) + 1, hf = hn + ((r & 1) ? 1 : -1), o = 2 * g + 3;
#pragma unroll
      for (int pl = 0; pl < 2; ++pl) {
        const unsigned* nr = halo + ((pl * J_HH + hn) * J_HP + (o & ~3)) / 4, * fr = halo + ((pl * J_HH + hf) * J_HP + (o & ~3)) / 4;
        const unsigned n4 = __builtin_amdgcn_alignbyte(nr[1], nr[0], (unsigned)(o & 3));
        const unsigned f4 = __builtin_amdgcn_alignbyte(fr[1], fr[0], (unsigned)(o & 3));
        int cs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) cs[i] = 3 * j_byte(&n4, i) + j_byte(&f4, i);
        int* c = pl ? cr : cb;
        c[0] = (3 * cs[1] + cs[0] + 8) >> 4;
        c[1] = (3 * cs[1] + cs[2] + 7) >> 4;
        c[2] = (3 * cs[2] + cs[1] + 8) >> 4;
        c[3] = (3 * cs[2] + cs[3] + 7) >> 4;
      }
    }
    unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int pp = 0; pp < 4; ++pp) {
      const int Y = p[pp], b = cb[pp] - 128, c = cr[pp] - 128;
      const int v[3] = {j_clamp(Y + ((91881 * c + 32768) >> 16)), j_clamp(Y + ((-22554 * b - 46802 * c + 32768) >> 16)),
                        j_clamp(Y + ((116130 * b + 32768) >> 16))};
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) o[(3 * pp + ch) >> 2] |= (unsigned)v[ch] << (8 * ((3 * pp + ch) & 3));
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) sw[r * (J_VPR * 4) + 3 * g + i] = o[i];
  }
  __syncthreads();
  {
    const int vpr = tw * 3 / 16;
    for (int e = tid; e < th * J_VPR; e += 256) {
      const int r = e / J_VPR, v = e % J_VPR;
      if (v < vpr) *reinterpret_cast<j_u32x4*>(dst + ((size_t)(y0 + r) * S + x0) * 3 + 16 * v) = stage[e];
    }
  }
}

// ================================================================================================ C ABI (include/wtpse_hip.h)
#define ST ((hipStream_t)stream)

extern "C" int wtpse_jpeg_roundtrip(const unsigned char* img, const int* mode, const int* tables, const int* recips,
                                    unsigned char* chroma, unsigned char* out, int N, int S, void* stream) {
  WTPSE_REQUIRE(img && mode && tables && recips && out && img != out && N > 0 && N < 65536 && S >= 16 && S <= 4096 && S % 16 == 0);
  WTPSE_REQUIRE(((uintptr_t)img & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)chroma & 3) == 0);
  if (chroma) {
    const dim3 grid((unsigned)((S + J_CT - 1) / J_CT), (unsigned)((S + J_CT - 1) / J_CT), (unsigned)N);
    hipLaunchKernelGGL(jpeg_chroma_k, grid, dim3(256), 0, ST, img, mode, tables, recips, chroma, S);
  }
  const dim3 grid((unsigned)((S + J_TW - 1) / J_TW), (unsigned)((S + J_TH - 1) / J_TH), (unsigned)N);
  hipLaunchKernelGGL(jpeg_apply_k, grid, dim3(256), 0, ST, img, mode, tables, recips, chroma, out, S);
  return wtpse_status();
}
