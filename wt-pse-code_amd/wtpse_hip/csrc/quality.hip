// Image-quality augmentation: the optional stage of the input pipeline between amplitude mixing (spectrum.hip) and input_finish_k
// (pipeline.hip).  Focus (Gaussian blur / unsharp masking), contrast about the sample's mean, brightness and dense sensor noise on
// the uint8 batch [N][S][S][3] — the "image quality" transforms of the stacked-transformation recipe (BigAug).  The
// random draws stay on the host (input_pipeline.draw_quality) and the pixels on the GPU.  Every operation is fixed point
// (include/wtpse_hip.h has the formulas; input_pipeline.quality_host is the same text in numpy int64), so the device equals the
// specification byte for byte and no floating-point instruction occurs in this file.
//   quality_sums_k  : the byte sum of every sample (the contrast pivot), one integer atomic per workgroup
//   quality_apply_k : one workgroup = one tile of Q_TH rows x Q_TW pixels of one sample.  A sample with a focus amount stages the
//                     tile plus its 8-pixel halo in LDS as bytes (edge replicated: clamped indices), runs the horizontal pass into an
//                     LDS array of 32-bit Q12 values and the vertical pass out of it; then the pointwise chain, one Philox block per
//                     pixel for the noise, and the store to a second buffer.  A sample without focus skips LDS altogether, a
//                     neutral one is copied: both branches are uniform over the workgroup (they depend on blockIdx.z alone).
// A thread works on 4 pixels = 12 consecutive bytes of a row.  Rows are 3 S bytes, so with an odd S most rows start off a dword:
// dword accesses where the address is 4-byte aligned and the 12 bytes (the 4 of a staged dword) lie inside the row, byte accesses
// where not.  The taps and the other parameters of the sample are read at a workgroup-uniform address (scalar registers).
#include "common.h"

#define Q_R 8                                    // the largest blur radius
#define Q_TW 64                                  // pixels of a tile along x
#define Q_TH 32                                  // rows of a tile
#define Q_COLS 13                                // ints per sample: a, c, beta, k, w[0..8]
constexpr int Q_GROUPS = Q_TW / 4;               // 12-byte groups per tile row
constexpr int Q_LW = (Q_TW + 2 * Q_R) * 3 / 4;   // dwords per staged row: 240 bytes
constexpr int Q_HB = Q_TW * 3;                   // Q12 values per row of the horizontal pass
constexpr int Q_ROWS = Q_TH + 2 * Q_R;
static_assert(Q_TW % 4 == 0 && (Q_R * 3) % 4 == 0, "a staged row and a group start on a dword");

typedef unsigned int q_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned q_byte(const unsigned* w, int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }
__device__ __forceinline__ unsigned q_bytesum(unsigned w, unsigned acc) { return __builtin_amdgcn_sad_u8(w, 0u, acc); }

// `nvalid` (0 .. 12) bytes at p -> three dwords, little endian; the bytes beyond nvalid are not read (0)
__device__ __forceinline__ void q_load12(const unsigned char* __restrict__ p, int nvalid, unsigned v[3]) {
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
__device__ __forceinline__ void q_store12(unsigned char* __restrict__ p, int nvalid, const unsigned v[3]) {
  if (nvalid == 12 && ((uintptr_t)p & 3) == 0) {
    unsigned* q = reinterpret_cast<unsigned*>(p);
    q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
  } else {
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (i < nvalid) p[i] = (unsigned char)q_byte(v, i);
  }
}

// Words 0, 1, 2 of the Philox4x32-10 block with counter (ctr lo, ctr hi, 0, 1) and key (seed lo, seed hi): the noise of the three
// channels of one pixel.  The 1 in the last counter word: uniform_f64_k (augment.hip) and philox_normal4 (common.h) have 0 there.
__device__ __forceinline__ void q_philox3(unsigned long long ctr, unsigned long long seed, uint32_t word[3]) {
  uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0, c3 = 1;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  word[0] = c0; word[1] = c1; word[2] = c2;
}

struct QPoint {
  int c, beta, k, m8;
  unsigned long long seed, pos;      // pos: the sample's base position in the noise stream
};

// s[12]: the focus stage's Q8 values of 4 pixels x 3 channels starting at pixel (y, x) -> contrast, brightness, noise, rounding;
// stores the `nvalid` bytes that lie inside the row
__device__ __forceinline__ void q_finish(const int s[12], const QPoint& q, int y, int x, int S, unsigned char* __restrict__ dst, int nvalid) {
  unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
  for (int pp = 0; pp < 4; ++pp) {
    uint32_t word[3] = {0u, 0u, 0u};
    if (q.k > 0) q_philox3(q.pos + (unsigned long long)((long long)y * S + x + pp), q.seed, word);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int i = pp * 3 + ch;
      int t = q.m8 + ((q.c * (s[i] - q.m8) + 128) >> 8) + q.beta;
      if (q.k > 0) t += (q.k * ((int)q_bytesum(word[ch], 0u) - 510) + 2048) >> 12;
      // clip((t + 128) >> 8, 0, 255) with the clip in front of the shift.  Written as shift, then clip, the compiler packs pairs of
      // bytes with v_ashr_pk_u8_i32 and ORs its register into the dword whole; on the MI355X bytes 2 and 3 of those dwords then
      // came out with foreign bits set (a superset of the right bits; tests/test_quality_gpu.py caught it).  Presumably the
      // instruction leaves the upper half of its destination as it was.  This form does not select it, and the bytes are right.
      const unsigned v = (unsigned)min(max(t + 128, 0), 65535) >> 8;
      o[i >> 2] |= v << (8 * (i & 3));
    }
  }
  q_store12(dst, nvalid, o);
}

__global__ __launch_bounds__(256) void quality_apply_k(const unsigned char* __restrict__ img, const int* __restrict__ params,
                                                       const unsigned* __restrict__ sums, const unsigned long long* __restrict__ pos,
                                                       unsigned long long seed, unsigned char* __restrict__ out, int S) {
  __shared__ unsigned tile[Q_ROWS * Q_LW];       // the tile and its halo, bytes
  __shared__ unsigned hbuf[Q_ROWS * Q_HB];       // the horizontal pass, Q12
  const int n = blockIdx.z, tid = threadIdx.x;
  const int x0 = (int)blockIdx.x * Q_TW, y0 = (int)blockIdx.y * Q_TH;
  const int rows_out = min(Q_TH, S - y0), row_bytes = 3 * S;
  const int* __restrict__ prm = params + (size_t)n * Q_COLS;
  const int a = prm[0];
  QPoint q;
  q.c = prm[1]; q.beta = prm[2]; q.k = prm[3];
  const unsigned char* __restrict__ src = img + (size_t)n * S * row_bytes;
  unsigned char* __restrict__ dst = out + (size_t)n * S * row_bytes;

  if (a == 0 && q.c == 256 && q.beta == 0 && q.k == 0) {          // neutral: a copy
    for (int e = tid; e < rows_out * Q_GROUPS; e += 256) {
      const int y = y0 + e / Q_GROUPS, x = x0 + (e % Q_GROUPS) * 4;
      const int nvalid = min(12, (S - x) * 3);
      if (nvalid <= 0) continue;
      unsigned v[3];
      q_load12(src + (size_t)y * row_bytes + x * 3, nvalid, v);
      q_store12(dst + (size_t)y * row_bytes + x * 3, nvalid, v);
    }
    return;
  }
  {
    // m8 = (256 SUM + cnt / 2) / cnt <= 65280 by shift and subtract: the compiler's division starts from a floating-point
    // reciprocal, and this kernel is integers only
    const unsigned long long cnt = 3ull * (unsigned)S * (unsigned)S;
    unsigned long long rem = 256ull * sums[n] + (cnt >> 1);
    unsigned m = 0u;
#pragma unroll
    for (int bit = 15; bit >= 0; --bit) {
      const unsigned long long d = cnt << bit;
      if (d <= rem) {
        rem -= d;
        m |= 1u << bit;
      }
    }
    q.m8 = (int)m;
  }
  q.seed = seed;
  q.pos = pos[n];

  if (a == 0) {                                                     // no focus: pointwise from global memory
    for (int e = tid; e < rows_out * Q_GROUPS; e += 256) {
      const int y = y0 + e / Q_GROUPS, x = x0 + (e % Q_GROUPS) * 4;
      const int nvalid = min(12, (S - x) * 3);
      if (nvalid <= 0) continue;
      unsigned v[3];
      q_load12(src + (size_t)y * row_bytes + x * 3, nvalid, v);
      int s[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) s[i] = (int)(q_byte(v, i) << 8);
      q_finish(s, q, y, x, S, dst + (size_t)y * row_bytes + x * 3, nvalid);
    }
    return;
  }

  unsigned w[Q_R + 1];
#pragma unroll
  for (int j = 0; j <= Q_R; ++j) w[j] = (unsigned)prm[4 + j];
  // ---- stage rows y0 - 8 .. y0 + rows_out + 7, pixels x0 - 8 .. x0 + Q_TW + 7, every index clamped into the picture
  const int hrows = rows_out + 2 * Q_R;
  for (int e = tid; e < hrows * Q_LW; e += 256) {
    const int r = e / Q_LW, wq = e - r * Q_LW;
    const int gy = min(max(y0 - Q_R + r, 0), S - 1);
    const unsigned char* __restrict__ rowp = src + (size_t)gy * row_bytes;
    const int b0 = (x0 - Q_R) * 3 + 4 * wq;                        // the dword's first byte within the row; may lie outside
    unsigned v;
    if (b0 >= 0 && b0 + 3 < row_bytes && ((uintptr_t)(rowp + b0) & 3) == 0) {
      v = *reinterpret_cast<const unsigned*>(rowp + b0);
    } else {
      v = 0u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int lb = 4 * wq + i;                                  // byte of the staged row: pixel lb / 3 of it, channel lb % 3
        const int px = min(max(x0 - Q_R + lb / 3, 0), S - 1);
        v |= (unsigned)rowp[px * 3 + lb % 3] << (8 * i);
      }
    }
    tile[e] = v;
  }
  __syncthreads();
  // ---- horizontal pass: value i of a group needs bytes i + 3 m, m = 0 .. 16, of the 60-byte window that starts at the group
  for (int e = tid; e < hrows * Q_GROUPS; e += 256) {
    const int r = e / Q_GROUPS, g = e % Q_GROUPS;
    unsigned win[15];
#pragma unroll
    for (int i = 0; i < 15; ++i) win[i] = tile[r * Q_LW + 3 * g + i];
    unsigned h[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) h[i] = w[0] * q_byte(win, i + 3 * Q_R);
#pragma unroll
    for (int j = 1; j <= Q_R; ++j) {
      if (w[j] == 0u) continue;                                     // a scalar branch: a sigma of 1 has 4 taps a side, not 8
#pragma unroll
      for (int i = 0; i < 12; ++i) h[i] += w[j] * (q_byte(win, i + 3 * (Q_R - j)) + q_byte(win, i + 3 * (Q_R + j)));
    }
    q_u32x4* hp = reinterpret_cast<q_u32x4*>(hbuf + r * Q_HB + 12 * g);
    hp[0] = q_u32x4{h[0], h[1], h[2], h[3]};
    hp[1] = q_u32x4{h[4], h[5], h[6], h[7]};
    hp[2] = q_u32x4{h[8], h[9], h[10], h[11]};
  }
  __syncthreads();
  // ---- vertical pass (unsigned: up to 255 * 2^24), focus, and the pointwise chain
  for (int e = tid; e < rows_out * Q_GROUPS; e += 256) {
    const int r = e / Q_GROUPS, g = e % Q_GROUPS;
    const int y = y0 + r, x = x0 + 4 * g;
    const int nvalid = min(12, (S - x) * 3);
    if (nvalid <= 0) continue;
    unsigned B[12];
    {
      const q_u32x4* hp = reinterpret_cast<const q_u32x4*>(hbuf + (r + Q_R) * Q_HB + 12 * g);
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const q_u32x4 hv = hp[v];
#pragma unroll
        for (int i = 0; i < 4; ++i) B[4 * v + i] = w[0] * hv[i];
      }
    }
#pragma unroll
    for (int j = 1; j <= Q_R; ++j) {
      if (w[j] == 0u) continue;
      const q_u32x4* up = reinterpret_cast<const q_u32x4*>(hbuf + (r + Q_R - j) * Q_HB + 12 * g);
      const q_u32x4* dn = reinterpret_cast<const q_u32x4*>(hbuf + (r + Q_R + j) * Q_HB + 12 * g);
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const q_u32x4 hu = up[v], hd = dn[v];
#pragma unroll
        for (int i = 0; i < 4; ++i) B[4 * v + i] += w[j] * (hu[i] + hd[i]);
      }
    }
    unsigned xin[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) xin[i] = tile[(r + Q_R) * Q_LW + (Q_R * 3) / 4 + 3 * g + i];
    int s[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int x8 = (int)(q_byte(xin, i) << 8), b8 = (int)((B[i] + 32768u) >> 16);
      s[i] = x8 + ((a * (x8 - b8) + 128) >> 8);
    }
    q_finish(s, q, y, x, S, dst + (size_t)y * row_bytes + x * 3, nvalid);
  }
}

// ------------------------------------------------------------------------------------------------ byte sums
#define QS_CHUNK 16384                           // bytes of a sample per workgroup

__global__ __launch_bounds__(256) void quality_sums_k(const unsigned char* __restrict__ img, unsigned* __restrict__ sums, unsigned len) {
  __shared__ unsigned part[4];
  const int n = blockIdx.y, tid = threadIdx.x;
  const unsigned lo = blockIdx.x * QS_CHUNK, hi = min(len, lo + QS_CHUNK);
  const unsigned char* __restrict__ p = img + (size_t)n * len + lo;
  const unsigned bytes = hi - lo;
  // bytes up to the first 16-byte boundary, 16-byte vectors, bytes behind the last whole vector
  const unsigned head = min(bytes, (unsigned)((0 - (uintptr_t)p) & 15));
  const unsigned nvec = (bytes - head) >> 4, tail = bytes - head - (nvec << 4);
  unsigned acc = 0u;
  if ((unsigned)tid < head) acc += p[tid];
  if ((unsigned)tid < tail) acc += p[head + (nvec << 4) + tid];
  const q_u32x4* __restrict__ pv = reinterpret_cast<const q_u32x4*>(p + head);
  for (unsigned i = tid; i < nvec; i += 256) {
    const q_u32x4 v = pv[i];
    acc = q_bytesum(v[0], acc);
    acc = q_bytesum(v[1], acc);
    acc = q_bytesum(v[2], acc);
    acc = q_bytesum(v[3], acc);
  }
  for (int m = 1; m < 64; m <<= 1) acc += (unsigned)__shfl_xor((int)acc, m, 64);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) atomicAdd(sums + n, part[0] + part[1] + part[2] + part[3]);
}

// ================================================================================================ C ABI (include/wtpse_hip.h)
#define ST ((hipStream_t)stream)

extern "C" int wtpse_quality_sums(const unsigned char* img, unsigned* sums, int N, int S, void* stream) {
  WTPSE_REQUIRE(img && sums && N > 0 && N < 65536 && S > 0 && S <= 512);      // 3 * 512^2 * 255 < 2^32
  const unsigned len = 3u * (unsigned)S * (unsigned)S;
  const hipError_t e = hipMemsetAsync(sums, 0, (size_t)N * sizeof(unsigned), ST);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(quality_sums_k, dim3((len + QS_CHUNK - 1) / QS_CHUNK, (unsigned)N), dim3(256), 0, ST, img, sums, len);
  return wtpse_status();
}

extern "C" int wtpse_quality_apply(const unsigned char* img, const int* params, const unsigned* sums, const unsigned long long* pos,
                                   unsigned long long seed, unsigned char* out, int N, int S, void* stream) {
  WTPSE_REQUIRE(img && params && sums && pos && out && img != out && N > 0 && N < 65536 && S > 0 && S <= 512);
  const dim3 grid((unsigned)((S + Q_TW - 1) / Q_TW), (unsigned)((S + Q_TH - 1) / Q_TH), (unsigned)N);
  hipLaunchKernelGGL(quality_apply_k, grid, dim3(256), 0, ST, img, params, sums, pos, seed, out, S);
  return wtpse_status();
}
