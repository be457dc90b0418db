// Whole fundus photographs (wtpse_hip/locate.py): the one pass over the full-size picture, and the two pure copies around the crop.
//
//   cells_k  : per c x c cell of an interleaved-RGB uint8 picture the count n of its field-of-view pixels (max(R,G,B) >= t) and the sum
//              s of 77 R + 150 G + 29 B over them.  A workgroup owns one cell row (c picture rows) times a span of whole cells at most
//              LC_SPAN pixels wide and nothing else touches those cells: the sums meet in an LDS table with integer LDS atomics (n 32-bit,
//              s 64-bit: exact whatever the order), and the table is STORED to the output — no global atomic, nothing to zero first, the
//              same on every run.  A pixel is 3 bytes, so a row starts at any byte phase: a wave reads a row's span as 64 x 48 bytes from
//              the 16-byte boundary below the span's first byte (three dwordx4 loads per lane, the 13th dword from the next lane's first
//              by a shuffle, lane 63 fetches its own), v_alignbyte moves the row's phase (0..2 bytes, wave-uniform) out, and every lane
//              holds 16 whole pixels at fixed byte positions.  A lane folds its 16 pixels into runs of one cell each (one division per
//              lane, none per pixel) and sends a run with one pair of LDS atomics: at c >= 16 that is one or two pairs per 16 pixels.
//              A 16-byte block is only loaded when it holds a byte of the span, so nothing outside the 16-byte hull of the tensor is
//              read whatever H, W, c and the base address.
//   crop_k   : M boxes of one side out of one picture, zero beyond its borders; paste_k: a patch into a canvas, clipped.  Byte streams in
//              groups of four along a row: one dword each way when both sides are 4-byte aligned, bytes otherwise.
#include "common.h"

#define LC_SPAN 2048                             // pixels of a cell row per workgroup (whole cells: max(1, LC_SPAN / c) of them)
#define LC_MAXCELLS (LC_SPAN / 2)                // c >= 2
#define LC_WAVE_PX 1024                          // 64 lanes x 16 pixels
#define LC_MAXDIM 65536

static inline int lc_cells_per_block(int c) { return LC_SPAN / c > 1 ? LC_SPAN / c : 1; }

// img [N][H][W][3]; out [N][CH][CW][2] int64; grid (ceil(CW / cpb), CH, N), 256 threads
__global__ __launch_bounds__(256) void cells_k(const unsigned char* __restrict__ img, long long* __restrict__ out, int H, int W, int c, int t,
                                               int CH, int CW, int cpb) {
  __shared__ unsigned long long Ls[LC_MAXCELLS];
  __shared__ unsigned Ln[LC_MAXCELLS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int cx0 = blockIdx.x * cpb, ci = blockIdx.y;
  const int ncell = min(cpb, CW - cx0);                            // cells of this workgroup (>= 1)
  const int x0 = cx0 * c, spanw = min(W - x0, ncell * c);          // its pixels of a row: [x0, x0 + spanw), spanw >= 1
  const int y0 = ci * c, nrows = min(c, H - y0);
  for (int i = tid; i < ncell; i += 256) { Ls[i] = 0ull; Ln[i] = 0u; }
  __syncthreads();
  const int nchunk = (3 * spanw + 15 + 3071) / 3072;               // 3072-byte wave chunks a row's span can reach into (<= 3)
  const unsigned char* plane = img + (size_t)blockIdx.z * H * W * 3;
  for (int it = wv; it < nrows * nchunk; it += 4) {
    const int r = it / nchunk, q = it - r * nchunk;                // wave-uniform
    const unsigned char* sp = plane + ((size_t)(y0 + r) * W + x0) * 3;       // the span's first byte in this row
    const unsigned char* se = sp + (size_t)3 * spanw;
    const int a = (int)((uintptr_t)sp & 15);
    const int o = a % 3;                                           // byte phase of the pixels against the 16-byte grid
    const unsigned char* cb = sp - a + (size_t)q * 3072 + lane * 48;         // this lane's 48 bytes, 16-byte aligned
    if (sp - a + (size_t)q * 3072 >= se) continue;                 // the whole chunk lies behind the span (uniform)
    unsigned d[13];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const unsigned char* b = cb + 16 * j;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (b < se && b + 16 > sp) v = *reinterpret_cast<const u32x4*>(b);     // holds a byte of the span: inside the tensor's 16-byte hull
      d[4 * j] = v[0]; d[4 * j + 1] = v[1]; d[4 * j + 2] = v[2]; d[4 * j + 3] = v[3];
    }
    d[12] = (unsigned)__shfl_down((int)d[0], 1, 64);               // the next lane's first dword = this lane's bytes 48..51
    if (lane == 63) {
      const unsigned char* b = cb + 48;
      d[12] = (b < se) ? *reinterpret_cast<const unsigned*>(b) : 0u;          // (b + 4 > sp always: b > cb >= sp - 15 - ... + 48)
    }
    unsigned e[12];                                                // the 48 bytes from byte o on: 16 whole pixels
#pragma unroll
    for (int j = 0; j < 12; ++j) e[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], (unsigned)o);
    const int p0 = q * LC_WAVE_PX + lane * 16 - (a - o) / 3;       // span-relative index of the lane's first pixel (>= -5)
    if (p0 >= spanw) continue;
    const int pf = max(p0, 0);
    int lc = pf / c, left = (lc + 1) * c - pf;                     // the run's cell and the pixels left in it
    unsigned an = 0u, as = 0u;                                     // a run: <= 16 pixels, as <= 16 * 65280
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int pp = p0 + p;
      if (pp < 0) continue;
      if (pp >= spanw) break;
      const int bi = 3 * p, w0 = bi >> 2, sh = (bi & 3) * 8;
      const unsigned v = sh == 0 ? e[w0] : sh == 8 ? (e[w0] >> 8) : (unsigned)((((unsigned long long)e[w0 + (w0 < 11 ? 1 : 0)] << 32) | e[w0]) >> sh);
      const unsigned R = v & 255u, G = (v >> 8) & 255u, B = (v >> 16) & 255u;
      if ((int)max(R, max(G, B)) >= t) { ++an; as += 77u * R + 150u * G + 29u * B; }
      if (--left == 0) {
        if (an) { atomicAdd(&Ln[lc], an); atomicAdd(&Ls[lc], (unsigned long long)as); }
        an = as = 0u; ++lc; left = c;
      }
    }
    if (an) { atomicAdd(&Ln[lc], an); atomicAdd(&Ls[lc], (unsigned long long)as); }
  }
  __syncthreads();
  long long* o2 = out + (((size_t)blockIdx.z * CH + ci) * CW + cx0) * 2;
  for (int i = tid; i < 2 * ncell; i += 256) o2[i] = (i & 1) ? (long long)Ls[i >> 1] : (long long)Ln[i >> 1];
}

// One row segment of `nb` bytes as groups of four: byte k of the segment is src[k] where vb0 <= k < vb1 (src may be dereferenced only
// there), else 0 (FILL) or left alone (!FILL: then vb0 = 0, vb1 = nb).  g: the group.
template <int FILL>
__device__ __forceinline__ void copy_group(const unsigned char* src, unsigned char* dst, int nb, int vb0, int vb1, int g) {
  const int k0 = 4 * g, k1 = min(k0 + 4, nb);
  const bool full = k1 - k0 == 4, inside = k0 >= vb0 && k1 <= vb1;
  if (full && inside && (((uintptr_t)(src + k0) | (uintptr_t)(dst + k0)) & 3) == 0) {
    *reinterpret_cast<unsigned*>(dst + k0) = *reinterpret_cast<const unsigned*>(src + k0);
    return;
  }
  unsigned v = 0u;
  for (int k = k0; k < k1; ++k)
    if (k >= vb0 && k < vb1) v |= (unsigned)src[k] << (8 * (k - k0));
  if (full && ((uintptr_t)(dst + k0) & 3) == 0) {
    *reinterpret_cast<unsigned*>(dst + k0) = v;
  } else {
    for (int k = k0; k < k1; ++k) dst[k] = (unsigned char)(v >> (8 * (k - k0)));
  }
}

// img [H][W][C]; boxes [M][2] = (top, left); out [M][s][s][C]
__global__ __launch_bounds__(256) void crop_k(const unsigned char* __restrict__ img, const int* __restrict__ boxes, unsigned char* __restrict__ out,
                                              int H, int W, int C, int M, int s) {
  const int nb = s * C, gpr = (nb + 3) >> 2;                       // bytes and groups of an output row
  const long long total = (long long)M * s * gpr, step = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    const long long row = i / gpr;
    const int g = (int)(i - row * gpr), m = (int)(row / s), y = (int)(row - (long long)m * s);
    const long long top = boxes[2 * m], left = boxes[2 * m + 1];
    const long long ys = top + y;
    int vb0 = 0, vb1 = 0;                                          // the row's bytes that lie inside the picture
    if (ys >= 0 && ys < H) {
      const long long xa = left < 0 ? -left : 0, xb = (long long)W - left < s ? (long long)W - left : s;
      if (xa < xb) { vb0 = (int)xa * C; vb1 = (int)xb * C; }
    }
    const unsigned char* src = img + (ys * W + left) * C;          // only formed, never read, outside [vb0, vb1)
    copy_group<1>(src, out + (size_t)row * nb, nb, vb0, vb1, g);
  }
}

// canvas [H][W][C]; patch [h][w][C]; the clipped rectangle rows [ya, yb), columns [xa, xb) of the canvas (host: not empty)
__global__ __launch_bounds__(256) void paste_k(unsigned char* __restrict__ canvas, const unsigned char* __restrict__ patch, int W, int C, int w,
                                               int top, int left, int ya, int yb, int xa, int xb) {
  const int nb = (xb - xa) * C, gpr = (nb + 3) >> 2;
  const long long total = (long long)(yb - ya) * gpr, step = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    const int r = (int)(i / gpr), g = (int)(i - (long long)r * gpr), y = ya + r;
    copy_group<0>(patch + ((size_t)(y - top) * w + (xa - left)) * C, canvas + ((size_t)y * W + xa) * C, nb, 0, nb, g);
  }
}

static unsigned lc_stream_blocks(long long items) {                // a memory-bound pass: at most 2048 workgroups, grid-stride the rest
  const long long nb = (items + 255) / 256;
  return (unsigned)(nb < 1 ? 1 : nb > 2048 ? 2048 : nb);
}

// ---- entry points (see include/wtpse_hip.h) ------------------------------------------------------------------------------
extern "C" int wtpse_locate_cells(const unsigned char* img, long long* cells, int N, int H, int W, int c, int t, void* stream) {
  WTPSE_REQUIRE(img && cells && N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= LC_MAXDIM && W <= LC_MAXDIM && c >= 2 && c <= 256);
  WTPSE_REQUIRE(t >= 0 && t <= 255 && ((uintptr_t)cells & 7) == 0);
  const int CH = ceil_div(H, c), CW = ceil_div(W, c), cpb = lc_cells_per_block(c);
  const dim3 grid((unsigned)ceil_div(CW, cpb), (unsigned)CH, (unsigned)N);
  hipLaunchKernelGGL(cells_k, grid, dim3(256), 0, (hipStream_t)stream, img, cells, H, W, c, t, CH, CW, cpb);
  return wtpse_status();
}

extern "C" int wtpse_crop_u8(const unsigned char* img, const int* boxes, unsigned char* out, int H, int W, int C, int M, int s, void* stream) {
  WTPSE_REQUIRE(img && boxes && out && H >= 1 && W >= 1 && H <= LC_MAXDIM && W <= LC_MAXDIM && (C == 1 || C == 3));
  WTPSE_REQUIRE(M >= 1 && M <= 65535 && s >= 1 && s <= 8192 && ((uintptr_t)boxes & 3) == 0);
  const long long groups = (long long)M * s * ((s * C + 3) / 4);
  hipLaunchKernelGGL(crop_k, dim3(lc_stream_blocks(groups)), dim3(256), 0, (hipStream_t)stream, img, boxes, out, H, W, C, M, s);
  return wtpse_status();
}

extern "C" int wtpse_paste_u8(unsigned char* canvas, const unsigned char* patch, int H, int W, int C, int h, int w, int top, int left,
                              void* stream) {
  WTPSE_REQUIRE(canvas && patch && H >= 1 && W >= 1 && H <= LC_MAXDIM && W <= LC_MAXDIM && (C == 1 || C == 3));
  WTPSE_REQUIRE(h >= 1 && w >= 1 && h <= LC_MAXDIM && w <= LC_MAXDIM);
  WTPSE_REQUIRE(top >= -(1 << 24) && top <= (1 << 24) && left >= -(1 << 24) && left <= (1 << 24));
  const int ya = top > 0 ? top : 0, yb = top + h < H ? top + h : H;
  const int xa = left > 0 ? left : 0, xb = left + w < W ? left + w : W;
  if (ya >= yb || xa >= xb) return WTPSE_OK;                       // wholly outside: nothing to do
  const long long groups = (long long)(yb - ya) * (((xb - xa) * C + 3) / 4);
  hipLaunchKernelGGL(paste_k, dim3(lc_stream_blocks(groups)), dim3(256), 0, (hipStream_t)stream, canvas, patch, W, C, w, top, left, ya, yb,
                     xa, xb);
  return wtpse_status();
}
