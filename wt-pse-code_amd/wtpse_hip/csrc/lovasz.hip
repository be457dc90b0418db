// Lovász hinge loss per image (plane) and its gradient added into the region loss's: a segmented, stable sort on the device.
// Specification: wtpse_hip/lovasz.py (lovasz_planes_host / lovasz_loss_host / lovasz_grad_host / lovasz_ranks_host).
//
// Per plane b of hw pixels: a pixel is kept iff mask == NULL or m_i != 0; sign_i = t_i > 0 ? +1 : -1; e_i = fmaf(-x_i, sign_i, 1) in
// fp32.  The kept pixels with e > 0 are ordered by e descending, ties by ascending pixel index; with G = kept foreground pixels (all
// of them, whatever their e) and c_r = foreground among the first r of the order,
//     J_r = 1 - (G - c_r) / (G + r - c_r),  g_r = J_r - J_{r-1} (g_1 = J_1),  L_b = sum_r e_(r) g_r,
//     d(w L)/dx_i = (w / B) (-sign_i) g_rank(i)     (fp64 from exact integers; pixels with e <= 0 follow all others and add nothing)
// A plane is cut into chunks of LV_CHUNK consecutive elements, one workgroup each: the number of chunks depends on hw alone, so a
// plane's bits do not depend on the batch or on its place in it.  Inside a chunk, element (wave w, round r, lane l) is number
// 512 w + 64 r + l: a wave owns 512 consecutive elements and walks them in eight rounds of 64.
//   lv_keys_k     every pixel -> (key, payload): key = ~bits(e) for a kept pixel with e > 0 — unsigned ascending = e descending —
//                 and 0xffffffff for every other pixel (they sort behind: stable, never looked at); payload = pixel index | the
//                 foreground bit.  Counts G, the pixels with e > 0, the non-finite kept logits; the first digit's histogram.
//   LSD radix sort, four passes over 8-bit digits, keys and payloads ping-pong through the workspace:
//     lv_hist_k     a chunk's digit histogram (the first pass takes lv_keys_k's);
//     lv_scan_k     one workgroup per plane: the exclusive prefix over (digit, chunk) in place — where chunk c's keys of digit d go;
//     lv_scatter_k  a chunk's keys to their places: per wave and digit a base (the chunk's offset + the counts of the waves before
//                   it), inside a wave the rank among the lanes of the same digit from ballots, round after round.  Every place
//                   follows from counts and prefixes: stable, so ties keep ascending pixel index.  The only atomics in this file
//                   are integer adds that build a histogram in LDS; no place is ever claimed with one.
//   lv_fg_k       foreground pixels per chunk of the sorted order.
//   lv_apply_k    c_r from the chunks before, the waves before and ballots; J_r, g_r; the chunk's sum of e g in fp64 in a fixed order;
//                 dx[pixel] = (float)((double)dx[pixel] + inc) for inc != 0 (an increment of exactly 0 leaves the bits alone);
//                 ranks[pixel] = r - 1.
//   lv_plane_k    L_b = the chunks' sums in chunk order (NaN for a plane with a non-finite kept logit, which adds nothing to dx).
// The mean over the planes is wtpse_reduce_rows, as in overlap.hip.
#include "common.h"

#define LV_CHUNK 2048                // elements of a plane per workgroup: 4 waves x 8 rounds x 64 lanes
#define LV_ROUNDS 8
#define LV_WAVE_SPAN 512             // consecutive elements a wave owns
#define LV_SENTINEL 0xffffffffu      // key of a pixel that is ignored or has e <= 0
#define LV_FG 0x80000000u            // payload = pixel index (< 2^30) | foreground bit
#define LV_PIX 0x3fffffffu

// chunks per plane: a function of hw alone, never of B
static int lv_chunks(int hw) { return ceil_div(hw, LV_CHUNK); }
// the limits of overlap.hip (hw <= 2^30: int element indices run up to hw + one chunk)
static bool lv_dims_ok(int B, int hw) { return B > 0 && B < 65536 && hw > 0 && hw <= (1 << 30) && (long long)B * hw <= 0x7fffffffLL; }

struct LvWs {
  double* partial;                   // [B][chunks] the chunks' sums of e g
  unsigned *key[2], *pay[2];         // [B][hw] each
  int* hist;                         // [B][chunks][256] digit counts, then offsets
  int* cnt;                          // [B][chunks][4]  G, e > 0, non-finite kept, kept — per chunk
  int* info;                         // [B][4]          the same per plane
  int* fg;                           // [B][chunks]     foreground per chunk of the sorted order
  float* plane;                      // [B]
};
// carves the workspace (base may be NULL: sizes only) -> bytes
static long long lv_layout(int B, int hw, char* base, LvWs* w) {
  const long long nch = lv_chunks(hw), n = (long long)B * hw;
  long long off = 0;
  auto take = [&](long long bytes) { char* p = base ? base + off : nullptr; off += bytes; return p; };
  w->partial = (double*)take(8 * B * nch);
  for (int k = 0; k < 2; ++k) w->key[k] = (unsigned*)take(4 * n);
  for (int k = 0; k < 2; ++k) w->pay[k] = (unsigned*)take(4 * n);
  w->hist = (int*)take(4 * B * nch * 256);
  w->cnt = (int*)take(4 * B * nch * 4);
  w->info = (int*)take(4 * B * 4);
  w->fg = (int*)take(4 * B * nch);
  w->plane = (float*)take(4 * B);
  return off;
}

// the lanes of the wave that hold a valid element of the same digit as this lane's (meaningful in valid lanes); every lane of the
// wave calls it
__device__ __forceinline__ unsigned long long lv_match(unsigned d, bool valid) {
  unsigned long long peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long m = __ballot(valid && bit);
    peers &= bit ? m : ~m;
  }
  return peers;
}

__device__ __forceinline__ int lv_wave_sum(int v) {
  for (int k = 1; k <= 32; k <<= 1) v += __shfl_xor(v, k, 64);
  return v;
}

// a wave's valid lanes add their digits into the LDS histogram h[256]: one integer add per distinct digit
__device__ __forceinline__ void lv_count(int* h, unsigned d, bool valid, int lane) {
  const unsigned long long peers = lv_match(d, valid);
  if (valid && lane == __ffsll((long long)peers) - 1) atomicAdd(&h[d], __popcll(peers));
}

__global__ __launch_bounds__(256) void lv_keys_k(const float* __restrict__ x, const float* __restrict__ m, const float* __restrict__ t,
                                                 int hw, unsigned* __restrict__ key, unsigned* __restrict__ pay,
                                                 int* __restrict__ hist, int* __restrict__ cnt, int* __restrict__ ranks) {
  __shared__ int h[256];
  __shared__ int tot[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  h[tid] = 0;
  if (tid < 4) tot[tid] = 0;
  __syncthreads();
  const size_t base = (size_t)blockIdx.y * hw;
  const int c0 = blockIdx.x * LV_CHUNK + wave * LV_WAVE_SPAN + lane;
  int n_fg = 0, n_pos = 0, n_bad = 0, n_kept = 0;
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const int i = c0 + r * 64;
    const bool valid = i < hw;
    unsigned k = LV_SENTINEL;
    if (valid) {
      const float xv = x[base + i];
      const bool fg = t[base + i] > 0.f;
      const bool kept = !m || m[base + i] != 0.f;
      if (kept) {
        const float e = fmaf(-xv, fg ? 1.f : -1.f, 1.f);
        ++n_kept;
        n_fg += fg;
        n_bad += !isfinite(xv);
        if (e > 0.f) {
          k = ~__float_as_uint(e);
          ++n_pos;
        }
      }
      key[base + i] = k;
      pay[base + i] = (unsigned)i | (fg ? LV_FG : 0u);
      if (ranks) ranks[base + i] = -1;
    }
    lv_count(h, k & 255u, valid, lane);
  }
  n_fg = lv_wave_sum(n_fg);
  n_pos = lv_wave_sum(n_pos);
  n_bad = lv_wave_sum(n_bad);
  n_kept = lv_wave_sum(n_kept);
  if (lane == 0) {
    atomicAdd(&tot[0], n_fg);
    atomicAdd(&tot[1], n_pos);
    atomicAdd(&tot[2], n_bad);
    atomicAdd(&tot[3], n_kept);
  }
  __syncthreads();
  const size_t chunk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  hist[chunk * 256 + tid] = h[tid];
  if (tid < 4) cnt[chunk * 4 + tid] = tot[tid];
}

__global__ __launch_bounds__(256) void lv_hist_k(const unsigned* __restrict__ key, int hw, int shift, int* __restrict__ hist) {
  __shared__ int h[256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  h[tid] = 0;
  __syncthreads();
  const size_t base = (size_t)blockIdx.y * hw;
  const int c0 = blockIdx.x * LV_CHUNK + wave * LV_WAVE_SPAN + lane;
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const int i = c0 + r * 64;
    const bool valid = i < hw;
    const unsigned k = valid ? key[base + i] : LV_SENTINEL;
    lv_count(h, (k >> shift) & 255u, valid, lane);
  }
  __syncthreads();
  hist[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + tid] = h[tid];
}

// one workgroup per plane, thread d = digit d: hist[chunk][d] (counts) -> the first place of chunk's keys of digit d in the plane,
// i.e. the exclusive prefix in the order (digit, chunk).  With cnt: the chunks' four counts are added up into info[plane][4].
__global__ __launch_bounds__(256) void lv_scan_k(int* __restrict__ hist, int nch, const int* __restrict__ cnt, int* __restrict__ info) {
  __shared__ int wsum[4];
  const int d = threadIdx.x, wave = d >> 6, lane = d & 63;
  int* H = hist + (size_t)blockIdx.x * nch * 256;
  int total = 0;
#pragma unroll 8
  for (int c = 0; c < nch; ++c) total += H[(size_t)c * 256 + d];
  int incl = total;
  for (int k = 1; k <= 32; k <<= 1) {
    const int v = __shfl_up(incl, k, 64);
    if (lane >= k) incl += v;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int run = incl - total;
  for (int w = 0; w < wave; ++w) run += wsum[w];
#pragma unroll 8
  for (int c = 0; c < nch; ++c) {
    const int v = H[(size_t)c * 256 + d];
    H[(size_t)c * 256 + d] = run;
    run += v;
  }
  if (cnt && d < 4) {
    const int* C = cnt + (size_t)blockIdx.x * nch * 4;
    int s = 0;
    for (int c = 0; c < nch; ++c) s += C[(size_t)c * 4 + d];
    info[blockIdx.x * 4 + d] = s;
  }
}

__global__ __launch_bounds__(256) void lv_scatter_k(const unsigned* __restrict__ key, const unsigned* __restrict__ pay, int hw, int shift,
                                                    const int* __restrict__ offs, unsigned* __restrict__ key_out,
                                                    unsigned* __restrict__ pay_out) {
  __shared__ int wcnt[4][256];       // a wave's count of every digit, then the place of its next key of that digit
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
  __syncthreads();
  const size_t base = (size_t)blockIdx.y * hw;
  const int c0 = blockIdx.x * LV_CHUNK + wave * LV_WAVE_SPAN + lane;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned k[LV_ROUNDS], p[LV_ROUNDS];
  int rank[LV_ROUNDS], same[LV_ROUNDS];          // among the lanes of this digit: those below this lane, all of them
#pragma unroll
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const int i = c0 + r * 64;
    const bool valid = i < hw;
    k[r] = valid ? key[base + i] : LV_SENTINEL;
    p[r] = valid ? pay[base + i] : 0u;
    const unsigned d = (k[r] >> shift) & 255u;
    const unsigned long long peers = lv_match(d, valid);
    rank[r] = __popcll(peers & below);
    same[r] = __popcll(peers);
    if (valid && rank[r] == 0) atomicAdd(&wcnt[wave][d], same[r]);
  }
  __syncthreads();
  {
    int run = offs[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + tid];
    for (int w = 0; w < 4; ++w) {
      const int v = wcnt[w][tid];
      wcnt[w][tid] = run;
      run += v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const bool valid = c0 + r * 64 < hw;
    const unsigned d = (k[r] >> shift) & 255u;
    const int pos = wcnt[wave][d] + rank[r];
    __syncthreads();                 // every lane has read the place before the digit's first lane moves it on
    if (valid && rank[r] == 0) wcnt[wave][d] += same[r];
    __syncthreads();
    if (valid && pos >= 0 && pos < hw) {
      key_out[base + pos] = k[r];
      pay_out[base + pos] = p[r];
    }
  }
}

// foreground pixels among the sorted places [chunk) below n_pos
__global__ __launch_bounds__(256) void lv_fg_k(const unsigned* __restrict__ pay, int hw, const int* __restrict__ info,
                                               int* __restrict__ fgc) {
  __shared__ int tot;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid == 0) tot = 0;
  __syncthreads();
  const int n_pos = min(info[blockIdx.y * 4 + 1], hw);
  const size_t base = (size_t)blockIdx.y * hw;
  const int c0 = blockIdx.x * LV_CHUNK + wave * LV_WAVE_SPAN + lane;
  int n = 0;
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const int i = c0 + r * 64;
    if (i < n_pos) n += (pay[base + i] & LV_FG) != 0u;
  }
  n = lv_wave_sum(n);
  if (lane == 0) atomicAdd(&tot, n);
  __syncthreads();
  if (tid == 0) fgc[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void lv_apply_k(const unsigned* __restrict__ key, const unsigned* __restrict__ pay, int B, int hw,
                                                  const int* __restrict__ info, const int* __restrict__ fgc,
                                                  const float* __restrict__ w_dev, double* __restrict__ partial,
                                                  int* __restrict__ ranks, float* __restrict__ dx) {
  __shared__ int wtot[4];
  __shared__ int before;
  __shared__ double wacc[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int plane = blockIdx.y;
  const size_t chunk = (size_t)plane * gridDim.x + blockIdx.x;
  const int G = info[plane * 4], n_pos = min(info[plane * 4 + 1], hw);
  const bool bad = info[plane * 4 + 2] != 0;
  if ((int)blockIdx.x * LV_CHUNK >= n_pos) {          // (the same in every thread) nothing of the order lies in this chunk
    if (tid == 0) partial[chunk] = 0.0;
    return;
  }
  if (tid == 0) before = 0;
  __syncthreads();
  {                                              // foreground in the chunks before this one
    int s = 0;
    for (int c = tid; c < (int)blockIdx.x; c += 256) s += fgc[(size_t)plane * gridDim.x + c];
    s = lv_wave_sum(s);
    if (lane == 0) atomicAdd(&before, s);
  }
  const size_t base = (size_t)plane * hw;
  const int c0 = blockIdx.x * LV_CHUNK + wave * LV_WAVE_SPAN + lane;
  const unsigned long long upto = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
  unsigned k[LV_ROUNDS], p[LV_ROUNDS];
  int incl[LV_ROUNDS];                           // foreground among this wave's elements up to and including this one
  int run = 0;
#pragma unroll
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const int i = c0 + r * 64;
    const bool valid = i < n_pos;
    k[r] = valid ? key[base + i] : LV_SENTINEL;
    p[r] = valid ? pay[base + i] : 0u;
    const unsigned long long f = __ballot(valid && (p[r] & LV_FG) != 0u);
    incl[r] = run + __popcll(f & upto);
    run += __popcll(f);
  }
  if (lane == 0) wtot[wave] = run;
  __syncthreads();
  int cb = before;
  for (int w = 0; w < wave; ++w) cb += wtot[w];
  const double K = dx ? (double)*w_dev / (double)B : 0.0;
  const double Gd = (double)G;
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const int i = c0 + r * 64;
    if (i < n_pos) {
      const bool fg = (p[r] & LV_FG) != 0u;
      const int pix = (int)(p[r] & LV_PIX);
      const double cr = (double)(cb + incl[r]), cp = cr - (fg ? 1.0 : 0.0), rr = (double)i + 1.0;
      const double Jr = 1.0 - (Gd - cr) / (Gd + rr - cr);
      const double Jp = i == 0 ? 0.0 : 1.0 - (Gd - cp) / (Gd + (rr - 1.0) - cp);
      const double g = Jr - Jp;
      acc += (double)__uint_as_float(~k[r]) * g;
      if (pix < hw) {
        if (ranks) ranks[base + pix] = i;
        if (dx && !bad) {
          const double inc = K * (fg ? -1.0 : 1.0) * g;
          // an increment of zero (weight 0, g = 0) leaves the stored bits alone, a -0.0 included
          if (inc != 0.0) dx[base + pix] = (float)((double)dx[base + pix] + inc);
        }
      }
    }
  }
  for (int s = 1; s <= 32; s <<= 1) acc += __shfl_xor(acc, s, 64);
  if (lane == 0) wacc[wave] = acc;
  __syncthreads();
  if (tid == 0) partial[chunk] = ((wacc[0] + wacc[1]) + wacc[2]) + wacc[3];
}

__global__ __launch_bounds__(256) void lv_plane_k(const double* __restrict__ partial, const int* __restrict__ info, int B, int nch,
                                                  float* __restrict__ plane_loss) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int c = 0; c < nch; ++c) s += partial[(size_t)b * nch + c];
  plane_loss[b] = info[b * 4 + 2] != 0 ? __uint_as_float(0x7fc00000u) : (float)s;
}

// ================================================================================================ C ABI
extern "C" int wtpse_lovasz_loss_ws(int B, int hw) {
  if (!lv_dims_ok(B, hw)) return -1;
  LvWs w;
  const long long bytes = lv_layout(B, hw, nullptr, &w);
  return bytes > 0x7fffffffLL ? -1 : (int)bytes;
}

extern "C" int wtpse_lovasz_loss(const float* x, const float* mask, const float* t, const float* w_dev, int B, int hw, void* ws,
                                 float* plane_loss, int* ranks, float* loss, float* dx, void* stream) {
  WTPSE_REQUIRE(x && t && ws && loss && wtpse_lovasz_loss_ws(B, hw) > 0 && (!dx || w_dev));
  WTPSE_REQUIRE((((uintptr_t)ws) & 7) == 0);
  LvWs w;
  lv_layout(B, hw, (char*)ws, &w);
  if (!plane_loss) plane_loss = w.plane;
  const int nch = lv_chunks(hw);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)nch, (unsigned)B);
  hipLaunchKernelGGL(lv_keys_k, grid, dim3(256), 0, st, x, mask, t, hw, w.key[0], w.pay[0], w.hist, w.cnt, ranks);
  for (int pass = 0; pass < 4; ++pass) {
    const int src = pass & 1, shift = 8 * pass;
    if (pass) hipLaunchKernelGGL(lv_hist_k, grid, dim3(256), 0, st, (const unsigned*)w.key[src], hw, shift, w.hist);
    hipLaunchKernelGGL(lv_scan_k, dim3((unsigned)B), dim3(256), 0, st, w.hist, nch, pass ? (const int*)nullptr : (const int*)w.cnt, w.info);
    hipLaunchKernelGGL(lv_scatter_k, grid, dim3(256), 0, st, (const unsigned*)w.key[src], (const unsigned*)w.pay[src], hw, shift,
                       (const int*)w.hist, w.key[src ^ 1], w.pay[src ^ 1]);
  }
  // four passes: the sorted order is back in buffer 0
  hipLaunchKernelGGL(lv_fg_k, grid, dim3(256), 0, st, (const unsigned*)w.pay[0], hw, (const int*)w.info, w.fg);
  hipLaunchKernelGGL(lv_apply_k, grid, dim3(256), 0, st, (const unsigned*)w.key[0], (const unsigned*)w.pay[0], B, hw, (const int*)w.info,
                     (const int*)w.fg, w_dev, w.partial, ranks, dx);
  hipLaunchKernelGGL(lv_plane_k, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0, st, (const double*)w.partial, (const int*)w.info, B, nch,
                     plane_loss);
  return wtpse_reduce_rows(plane_loss, B, 1, loss, 0, 1.f / (float)B, stream);
}
