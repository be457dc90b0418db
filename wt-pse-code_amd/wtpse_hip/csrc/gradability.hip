// Gradability check (wtpse_hip/gradability.py): the one exact-integer pass over a full-size picture that leaves, per picture, the
// record every focus, exposure and field measure is formed from on the host (include/wtpse_hip.h has the layout; gradability.record_host
// is the specification, bit for bit).
//
//   grad_init_k   : the records zeroed, the bounding box at its empty value (H, -1, W, -1).
//   grad_record_k : a workgroup walks tiles of GR_TH rows x GR_TW pixels of ONE picture (tile, tile + gridDim.x, ...) and keeps one
//              record in LDS and registers for all of them; at its end the registers are folded per wave (shuffles), the waves meet in
//              the LDS record, and its nonzero slots are added into the picture's record with 64-bit integer vector atomics (add /
//              smin / smax).  Sums, counts and extrema of integers: neither the grouping nor the order matters — exact and the same
//              on every run; nothing is allocated, nothing waits for the host.
//              Per tile, two phases around a barrier:
//              (1) the rows [y0 - 4, y0 + GR_TH + 4) x pixels [x0 - 4, x0 + GR_TW + 4), clipped to the picture, are read as cells_k
//                  (locate.hip) reads a span: from the 16-byte boundary below the span's first byte a lane takes 48 bytes as three
//                  dwordx4 loads plus the dword behind them, v_alignbyte moves the row's byte phase (0..2) out, and the lane holds 16
//                  whole pixels.  A 16-byte block (and the trailing dword) is only loaded when it holds a byte of the span: nothing
//                  outside the 16-byte hull of the tensor is read.  A span is at most 264 pixels = GR_LPR lanes, so a wave reads
//                  three rows per pass.  Every pixel goes to the LDS tile as 16 bits, G | field << 8 (positions outside the picture
//                  hold 0: not in the field); the pixels the tile OWNS (no halo) and that lie in the field are folded: luma histogram
//                  by LDS atomics, one per run of equal luma within a lane's 16 pixels; channel sums, saturation counts, area and
//                  extrema in registers.
//              (2) a thread takes 4 consecutive owned pixels of a row: three 8-byte LDS reads for the row (12 pixels: 4 to each side),
//                  two per dilation for the rows above and below, and the Laplacian / gradient energies of the pixels whose five field
//                  bits are all set go to per-thread 64-bit sums.  A wave reads one row's 64 quads: consecutive 8-byte words, no bank
//                  conflict.  The arithmetic runs on the two pixels of a dword at once: packed 16-bit adds (|L| <= 1020) and
//                  v_dot2_i32_i16 for the squares, the pixels that are not interior masked out of one factor.
//   Tile shape: the halo is 4 on every side.  Along a row it costs 8 pixels of 264 (3 %), and they share cache lines with the owned
//   ones; across rows it costs 8 rows in GR_TH + 8, which a neighbour's workgroup reads again — from L2 where it runs on the same XCD,
//   else from the Infinity Cache (a photograph is 9 - 37 MB and has just been written or read by locate_cells).  256 x 32 keeps that
//   re-read at 25 % and the tile at 21 KB of LDS (7 workgroups a CU by LDS, 6 by registers); a row of the tile is 792 contiguous bytes.  Taller tiles
//   re-read less (64 rows: 12.5 %, 38 KB) and were not measured against this one.  HBM sees every row once.
#include "common.h"

#define GR_TW 256                                // owned pixels of a tile row
#define GR_TH 32                                 // owned rows of a tile
#define GR_HALO 4                                // the largest dilation
#define GR_PW (GR_TW + 2 * GR_HALO)              // 264 pixels of an LDS row (528 bytes: 8-byte aligned rows)
#define GR_PH (GR_TH + 2 * GR_HALO)              // 40 LDS rows
#define GR_LPR 21                                // lanes per row in phase 1: 21 * 16 - 5 (phase pixels in front) >= GR_PW
#define GR_RPW 3                                 // rows per wave pass (63 lanes)
#define GR_REC WTPSE_GRAD_REC
#define GR_MAXDIM 65536
#define GR_MAX_WG 2048                           // workgroups of a launch (over all pictures) before they start to loop over tiles
#define GR_MAX_TILES 512                         // tiles one workgroup walks at most: 2^22 pixels, which bounds its 32-bit partial sums

static_assert(GR_LPR * 16 - 5 >= GR_PW && GR_LPR * GR_RPW <= 64, "a span fits the lanes of its row");
static_assert(GR_REC == 276 && (GR_PW * 2) % 8 == 0 && GR_TW == 64 * 4, "record layout; 8-byte LDS rows; one wave = one row of quads");

typedef short s16x2 __attribute__((ext_vector_type(2)));
// the green bytes of two staged pixels (G | field << 8 in each half of a dword) as two 16-bit integers
__device__ __forceinline__ s16x2 gr_green(unsigned w) { return __builtin_bit_cast(s16x2, w & 0x00FF00FFu); }
__device__ __forceinline__ s16x2 gr_keep(s16x2 v, unsigned keep) { return __builtin_bit_cast(s16x2, __builtin_bit_cast(unsigned, v) & keep); }

// the sum over the 64 lanes of a full wave, in every lane
__device__ __forceinline__ unsigned gr_wave_sum(unsigned v) {
  for (int m = 1; m < 64; m <<= 1) v += (unsigned)__shfl_xor((int)v, m, 64);
  return v;
}
__device__ __forceinline__ unsigned long long gr_wave_sum(unsigned long long v) {
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// rec [N][GR_REC]
__global__ __launch_bounds__(256) void grad_init_k(long long* __restrict__ rec, long long total, int H, int W) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int e = (int)(i % GR_REC);
  rec[i] = e == 263 ? (long long)H : e == 265 ? (long long)W : (e == 264 || e == 266) ? -1ll : 0ll;
}

// img [N][H][W][3]; rec [N][GR_REC] initialised; grid (G, 1, N), 256 threads; TX tiles per tile row, T tiles per picture
__global__ __launch_bounds__(256) void grad_record_k(const unsigned char* __restrict__ img, long long* __restrict__ rec, int H, int W, int t,
                                                     int sat, int TX, int T) {
  __shared__ __attribute__((aligned(16))) unsigned short Tl[GR_PH * GR_PW];
  __shared__ unsigned Hs[256];                                     // luma histogram (a workgroup's pixels: <= 2^22, see the launcher)
  __shared__ unsigned long long Rs[GR_REC - 256];                  // rec[256 ..) of this workgroup (the bounding box: Bx)
  __shared__ int Bx[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  Hs[tid] = 0u;
  if (tid < GR_REC - 256) Rs[tid] = 0ull;
  if (tid < 4) Bx[tid] = tid == 0 ? H : tid == 2 ? W : -1;
  const unsigned char* plane = img + (size_t)blockIdx.z * H * W * 3;
  // phase 1's registers.  A lane sees at most 4 passes x 16 pixels of a tile and a workgroup at most GR_MAX_TILES tiles (launcher):
  // sums <= 512 * 64 * 255 < 2^24, counts <= 2^15
  unsigned sR = 0u, sG = 0u, sB = 0u, cR = 0u, cG = 0u, cB = 0u, cn = 0u;
  int top = H, bottom = -1, left = W, right = -1;
  // phase 2's: counts <= 512 * 32 pixels a thread; the energies 64-bit
  unsigned nd[3] = {0u, 0u, 0u};
  unsigned long long Ed[3] = {0ull, 0ull, 0ull}, Qd[3] = {0ull, 0ull, 0ull};
  const int lrw = lane / GR_LPR, ll = lane - lrw * GR_LPR;         // phase 1: the lane's row of the pass (3: idle) and place in it
  for (int tile = blockIdx.x; tile < T; tile += gridDim.x) {
    const int ty = tile / TX, tx = tile - ty * TX;
    const int y0 = ty * GR_TH, x0 = tx * GR_TW;
    const int ys = max(y0 - GR_HALO, 0), ye = min(y0 + GR_TH + GR_HALO, H);
    const int xs = max(x0 - GR_HALO, 0), xe = min(x0 + GR_TW + GR_HALO, W);
    const int spanw = xe - xs, nrow = ye - ys;                     // >= 1
    __syncthreads();                                               // the tile before (or the set-up above) is done with
    if (ys != y0 - GR_HALO || ye != y0 + GR_TH + GR_HALO || xs != x0 - GR_HALO || xe != x0 + GR_TW + GR_HALO) {     // uniform
      uint4* z = reinterpret_cast<uint4*>(Tl);                     // part of the tile lies outside the picture: not in the field
      for (int i = tid; i < GR_PH * GR_PW * 2 / 16; i += 256) z[i] = make_uint4(0u, 0u, 0u, 0u);
      __syncthreads();
    }
    // ---- phase 1 ----
    for (int rb = wv * GR_RPW; rb < nrow; rb += 4 * GR_RPW) {
      const int r = rb + lrw;
      if (lrw >= GR_RPW || r >= nrow) continue;
      const int y = ys + r;
      const unsigned char* sp = plane + ((size_t)y * W + xs) * 3;  // the span's first byte in this row
      const unsigned char* se = sp + (size_t)3 * spanw;
      const int a = (int)((uintptr_t)sp & 15);
      const int o = a % 3;                                         // byte phase of the pixels against the 16-byte grid
      const unsigned char* cb = sp - a + ll * 48;                  // this lane's 48 bytes, 16-byte aligned
      const int p0 = ll * 16 - (a - o) / 3;                        // span-relative index of the lane's first pixel (>= -5)
      if (p0 >= spanw) continue;                                   // (then cb >= se as well: nothing to load)
      unsigned d[13];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const unsigned char* b = cb + 16 * j;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (b < se && b + 16 > sp) v = *reinterpret_cast<const u32x4*>(b);       // holds a byte of the span: inside the tensor's 16-byte hull
        d[4 * j] = v[0]; d[4 * j + 1] = v[1]; d[4 * j + 2] = v[2]; d[4 * j + 3] = v[3];
      }
      d[12] = (cb + 48 < se) ? *reinterpret_cast<const unsigned*>(cb + 48) : 0u;  // first dword of a block that holds a byte of the span
      unsigned e[12];                                              // the 48 bytes from byte o on: 16 whole pixels
#pragma unroll
      for (int j = 0; j < 12; ++j) e[j] = __builtin_amdgcn_alignbyte(d[j + 1], d[j], (unsigned)o);
      unsigned short* trow = Tl + (y - (y0 - GR_HALO)) * GR_PW + (xs - (x0 - GR_HALO));
      const bool yown = y >= y0 && y < y0 + GR_TH;
      int curY = -1;
      unsigned curN = 0u, got = 0u;                                // a run of equal luma (<= 16 pixels); owned field pixels of the lane
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        const int pp = p0 + p;
        if (pp < 0) continue;
        if (pp >= spanw) break;
        const int bi = 3 * p, w0 = bi >> 2, sh = (bi & 3) * 8;
        const unsigned v = sh == 0 ? e[w0] : sh == 8 ? (e[w0] >> 8) : (unsigned)((((unsigned long long)e[w0 + (w0 < 11 ? 1 : 0)] << 32) | e[w0]) >> sh);
        const unsigned R = v & 255u, G = (v >> 8) & 255u, B = (v >> 16) & 255u;
        const bool f = (int)max(R, max(G, B)) >= t;
        trow[pp] = (unsigned short)(G | (f ? 256u : 0u));
        const int x = xs + pp;
        if (f && yown && x >= x0 && x < x0 + GR_TW) {
          const int Y = (int)((77u * R + 150u * G + 29u * B + 128u) >> 8);
          if (Y == curY) {
            ++curN;
          } else {
            if (curN) atomicAdd(&Hs[curY], curN);
            curY = Y; curN = 1u;
          }
          sR += R; sG += G; sB += B;
          cR += (int)R >= sat; cG += (int)G >= sat; cB += (int)B >= sat;
          ++got;
          left = min(left, x); right = max(right, x);
        }
      }
      if (curN) atomicAdd(&Hs[curY], curN);
      if (got) { cn += got; top = min(top, y); bottom = max(bottom, y); }
    }
    __syncthreads();
    // ---- phase 2 ----
    const int nr = min(GR_TH, H - y0), nq = (min(GR_TW, W - x0) + 3) >> 2;
    if (lane < nq) {
      for (int r = wv; r < nr; r += 4) {
        const unsigned short* crow = Tl + (r + GR_HALO) * GR_PW + 4 * lane;      // columns x0 - 4 + 4 lane ..: 12 pixels
        unsigned C[6];                                             // two pixels a dword: C[2], C[3] are the thread's four
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const uint2 w = *reinterpret_cast<const uint2*>(crow + 4 * j);
          C[2 * j] = w.x; C[2 * j + 1] = w.y;
        }
        if (((C[2] | C[3]) & 0x01000100u) == 0u) continue;         // none of the four is in the field
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int dd = 1 << k;
          const uint2 wu = *reinterpret_cast<const uint2*>(crow - dd * GR_PW + 4);
          const uint2 wd = *reinterpret_cast<const uint2*>(crow + dd * GR_PW + 4);
          unsigned n4 = 0u;
          int e4 = 0, q4 = 0;                                      // four pixels: e4 <= 4 * 1020^2 < 2^23, q4 <= 8 * 255^2 < 2^20
#pragma unroll
          for (int p = 0; p < 2; ++p) {                            // a pair of pixels in the halves of a dword, packed 16-bit arithmetic
            const unsigned c = C[2 + p], u = p ? wu.y : wu.x, dn = p ? wd.y : wd.x;
            const unsigned l = dd == 1 ? __builtin_amdgcn_alignbit(c, C[1 + p], 16) : C[2 + p - dd / 2];
            const unsigned rr = dd == 1 ? __builtin_amdgcn_alignbit(C[3 + p], c, 16) : C[2 + p + dd / 2];
            const unsigned in = ((c & l & rr & u & dn) >> 8) & 0x00010001u;      // bit 0 / 16: the pixel is interior
            const unsigned keep = (in << 16) - in;                 // 0xFFFF in the halves of the interior pixels
            const s16x2 gc = gr_green(c), gl = gr_green(l), gr = gr_green(rr), gu = gr_green(u), gd = gr_green(dn);
            const s16x2 L = gc * (short)4 - (gu + gd) - (gl + gr), dx = gr - gl, dy = gd - gu;      // |L| <= 1020, |dx|, |dy| <= 255
            n4 += (unsigned)__popc(in);
            e4 = __builtin_amdgcn_sdot2(gr_keep(L, keep), L, e4, false);
            q4 = __builtin_amdgcn_sdot2(gr_keep(dx, keep), dx, q4, false);
            q4 = __builtin_amdgcn_sdot2(gr_keep(dy, keep), dy, q4, false);
          }
          nd[k] += n4; Ed[k] += (unsigned)e4; Qd[k] += (unsigned)q4;
        }
      }
    }
  }
  // ---- the workgroup's record ----
  // The wave folds first (every lane of every wave is here): 256 lanes on one LDS address are served one after the other, and twenty
  // such atomics per workgroup cost more than the tile did.  32-bit wave sums: 64 lanes x (< 2^24) and 64 x 2^14.
  sR = gr_wave_sum(sR); sG = gr_wave_sum(sG); sB = gr_wave_sum(sB);
  cR = gr_wave_sum(cR); cG = gr_wave_sum(cG); cB = gr_wave_sum(cB); cn = gr_wave_sum(cn);
  for (int m = 1; m < 64; m <<= 1) {
    top = min(top, __shfl_xor(top, m, 64)); bottom = max(bottom, __shfl_xor(bottom, m, 64));
    left = min(left, __shfl_xor(left, m, 64)); right = max(right, __shfl_xor(right, m, 64));
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { nd[k] = gr_wave_sum(nd[k]); Ed[k] = gr_wave_sum(Ed[k]); Qd[k] = gr_wave_sum(Qd[k]); }
  if (lane == 0) {
    if (cn) {
      atomicAdd(&Rs[0], (unsigned long long)sR); atomicAdd(&Rs[1], (unsigned long long)sG); atomicAdd(&Rs[2], (unsigned long long)sB);
      if (cR) atomicAdd(&Rs[3], (unsigned long long)cR);
      if (cG) atomicAdd(&Rs[4], (unsigned long long)cG);
      if (cB) atomicAdd(&Rs[5], (unsigned long long)cB);
      atomicAdd(&Rs[6], (unsigned long long)cn);
      atomicMin(&Bx[0], top); atomicMax(&Bx[1], bottom); atomicMin(&Bx[2], left); atomicMax(&Bx[3], right);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (nd[k]) {
        atomicAdd(&Rs[11 + 3 * k], (unsigned long long)nd[k]);
        if (Ed[k]) atomicAdd(&Rs[12 + 3 * k], Ed[k]);
        if (Qd[k]) atomicAdd(&Rs[13 + 3 * k], Qd[k]);
      }
  }
  __syncthreads();
  long long* o = rec + (size_t)blockIdx.z * GR_REC;
  for (int e = tid; e < GR_REC; e += 256) {
    if (e >= 263 && e <= 266) {
      if (Rs[6] == 0ull) continue;                                 // no field pixel here: the box stays
      const long long b = (long long)Bx[e - 263];
      if (e & 1) (void)__hip_atomic_fetch_min(o + e, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // 263 top, 265 left
      else (void)__hip_atomic_fetch_max(o + e, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);             // 264 bottom, 266 right
      continue;
    }
    const unsigned long long v = e < 256 ? (unsigned long long)Hs[e] : Rs[e - 256];
    if (v) (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(o + e), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- entry point (see include/wtpse_hip.h) -----------------------------------------------------------------------------------
extern "C" int wtpse_gradability_record(const unsigned char* img, long long* rec, int N, int H, int W, int t, int sat, void* stream) {
  WTPSE_REQUIRE(img && rec && N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= GR_MAXDIM && W <= GR_MAXDIM);
  WTPSE_REQUIRE(t >= 0 && t <= 255 && sat >= 1 && sat <= 255 && ((uintptr_t)rec & 7) == 0);
  const hipStream_t st = (hipStream_t)stream;
  const int TX = ceil_div(W, GR_TW), T = TX * ceil_div(H, GR_TH);  // <= 256 * 2048 tiles
  const int cap = GR_MAX_WG / N > 1 ? GR_MAX_WG / N : 1;           // workgroups per picture ...
  const int few = T < cap ? T : cap, need = ceil_div(T, GR_MAX_TILES);       // ... but none walks more than GR_MAX_TILES tiles
  const int G = few > need ? few : need;                           // <= max(2048, 1024)
  const long long total = (long long)N * GR_REC;
  hipLaunchKernelGGL(grad_init_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, rec, total, H, W);
  hipLaunchKernelGGL(grad_record_k, dim3((unsigned)G, 1u, (unsigned)N), dim3(256), 0, st, img, rec, H, W, t, sat, TX, T);
  return wtpse_status();
}
