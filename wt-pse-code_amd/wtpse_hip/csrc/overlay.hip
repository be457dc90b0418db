// Test-run overlays on the device: the composite and contour-painting stage of the reference's test program
// (test_visulization.py:238-269 -> utils.save_per_img, utils.py:371-454; untransform, utils.py:460-463), which the reference runs per
// image on the host with skimage.  wtpse_hip/test_run.py::overlay_host is the readable restatement; this file is its gather form.
//
//   untransform  v = (img + 1) * 127.5 in fp32 (one rounded add, one rounded multiply), truncated to uint8 as numpy's astype does:
//                `original` (saved before anything is painted, utils.py:379-383) and the canvas the contours are painted on.
//   composite    channel 0 = cup mask, channel 1 = disc OR cup (test_visulization.py:243-256).  save_per_img calls channel 0
//                `disc_map` and channel 1 `cup_map` (utils.py:385-386): the names are swapped against the content and the colours
//                follow the names — the cup's contour is painted blue, the disc's green.  Kept.
//   ground truth the same composite of the labels, each channel through get_largest_fillhole (utils.py:426-427): two pseudo-logit
//                maps of +-30 through wtpse_postprocess (csrc/postprocess.hip) at threshold 0.5.  No labelling code here.
//   border       the prediction channels get their first / last row and column zeroed (utils.py:388-396), the ground truth does not.
//   contours     measure.find_contours(map, 0.5) on a 0/1 map has a vertex at the midpoint of every horizontally or vertically
//                adjacent pixel pair whose values differ (linear interpolation crosses 0.5 at one half in all 16 marching-squares
//                cases); every vertex (r, c) paints the seven pixels int(r + dr), int(c + dc), (dr, dc) = (0,0) (1,0) (1,1) (0,1)
//                (-1,0) (-1,-1) (0,-1), int = truncation towards zero (utils.py:408-448).  The painted set depends on the vertex set
//                alone, so it inverts into a gather: with EH[i][j] = map[i][j] != map[i][j+1] and EV[i][j] = map[i][j] !=
//                map[i+1][j] (0 where a pixel of the pair is outside the image), pixel (y, x) is painted iff any of
//                    EH[y][x-1] EH[y][x] EH[y][x+1]   EH[y-1][x] EH[y-1][x-1]   EH[y'][x] EH[y'][x+1]
//                    EV[y][x] EV[y][x-1] EV[y][x']    EV[y-1][x] EV[y-1][x-1]   EV[y+1][x] EV[y+1][x']
//                is set, y' = (y + 1) mod h, x' = (x + 1) mod w: an index of -1 wraps to the last row / column as numpy indexing does
//                (reached by ground truth that touches the first row / column only: the zeroed border keeps EH[0][.] and EV[.][0] of a
//                prediction empty, so one formula serves all four maps).  An index equal to h or w makes the reference raise
//                IndexError (ground truth touching the last row / column); that paint is DROPPED here — the one stated deviation —
//                which in the gather is simply a term that does not exist.
//   priority     last writer wins in the reference: prediction channel 1 green, prediction channel 0 blue, ground truth red.
//
// One kernel, HBM-bound (12 + 4 bytes read, 6 written per pixel): a 256 x 16 pixel tile per workgroup; the four masks of the tile and
// its halo (one row above, two below, one column left, two right, the wrapped row / column included) are packed into one byte per
// pixel in LDS, so one XOR compares all four maps; every lane owns four consecutive pixels of a row (16-byte image loads when w is a
// multiple of 4); the uint8 outputs are staged in LDS shifted by the row's global misalignment and leave as aligned dwords, single
// bytes only at the ragged ends of a row segment.  No atomics, no ordering between threads.
#include "common.h"

#define OV_TX 256                      // pixels of a tile row: 64 lanes x 4 pixels
#define OV_TY 16                       // rows of a tile: 4 waves x 4 rows
#define OV_MW (OV_TX + 8)              // mask tile row: columns x0 - 4 .. x0 + TX + 3 in 4-byte groups (needed: x0 - 1 .. x0 + TX + 1)
#define OV_MG (OV_MW / 4)
#define OV_MH (OV_TY + 3)              // rows y0 - 1 .. y0 + TY + 1
#define OV_SW (OV_TX * 3 + 8)          // staging row: up to 3 bytes of lead + 768 bytes, rounded to dwords
#define OV_SD (OV_SW / 4)
#define OV_MAXDIM 4096
#define OV_LOGIT 30.f                  // sigmoid(+-30) is 1 / 9e-14 in fp32: either side of any sensible threshold

// bit 0 / 1: prediction channel 0 / 1 (border zeroed), bit 2 / 3: ground-truth channel 0 / 1
__device__ __forceinline__ unsigned ov_bits(unsigned od, unsigned oc, unsigned g0, unsigned g1, bool border) {
  unsigned v = (g0 ? 4u : 0u) | (g1 ? 8u : 0u);
  if (!border) v |= (oc == 1u ? 1u : 0u) | ((od == 1u || oc == 1u) ? 2u : 0u);
  return v;
}

// gf [2][B][h][w]: the filled ground-truth channels.  vec: w % 4 == 0 and every pointer aligned for 16-byte / 4-byte vector access.
// GT = 0 (wtpse_overlay_pred): there is no ground truth — gf is not read (NULL) and bits 2 / 3 stay clear, which is what an all-zero
// ground truth packs to, so nothing is painted red and every other byte is the GT = 1 kernel's.
template <int GT>
__global__ __launch_bounds__(256) void overlay_k(const float* __restrict__ img, const unsigned char* __restrict__ pred_od,
                                                 const unsigned char* __restrict__ pred_oc, const unsigned char* __restrict__ gf,
                                                 unsigned char* __restrict__ original, unsigned char* __restrict__ overlay, int B, int h,
                                                 int w, int vec) {
  __shared__ __attribute__((aligned(16))) unsigned char M[OV_MH][OV_MW];
  __shared__ __attribute__((aligned(16))) unsigned char S0[OV_TY][OV_SW];
  __shared__ __attribute__((aligned(16))) unsigned char S1[OV_TY][OV_SW];
  const int b = blockIdx.z, x0 = blockIdx.x * OV_TX, y0 = blockIdx.y * OV_TY;
  const size_t plane = (size_t)h * w;
  const unsigned char* pd = pred_od + (size_t)b * plane;
  const unsigned char* pc = pred_oc + (size_t)b * plane;
  const unsigned char* q0 = GT ? gf + (size_t)b * plane : nullptr;
  const unsigned char* q1 = GT ? gf + ((size_t)B + b) * plane : nullptr;

  // ---- the packed mask tile: row h holds row 0 and column w holds column 0 (the -1 wrap), everything else outside is 0
  for (int idx = threadIdx.x; idx < OV_MH * OV_MG; idx += 256) {
    const int r = idx / OV_MG, g = idx - r * OV_MG;
    const int y = y0 - 1 + r, x = x0 - 4 + 4 * g;
    unsigned packed = 0u;
    if (y >= 0 && y <= h) {
      const int ys = y == h ? 0 : y;
      const bool rb = ys == 0 || ys == h - 1;
      const size_t ro = (size_t)ys * w;
      if (vec && x >= 0 && x + 3 < w) {
        const unsigned a = *reinterpret_cast<const unsigned*>(pd + ro + x), c = *reinterpret_cast<const unsigned*>(pc + ro + x);
        const unsigned e = GT ? *reinterpret_cast<const unsigned*>(q0 + ro + x) : 0u;
        const unsigned f = GT ? *reinterpret_cast<const unsigned*>(q1 + ro + x) : 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          packed |= ov_bits((a >> (8 * k)) & 255u, (c >> (8 * k)) & 255u, (e >> (8 * k)) & 255u, (f >> (8 * k)) & 255u,
                            rb || x + k == 0 || x + k == w - 1) << (8 * k);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int xx = x + k;
          if (xx < 0 || xx > w) continue;
          const int xs = xx == w ? 0 : xx;
          packed |= ov_bits(pd[ro + xs], pc[ro + xs], GT ? q0[ro + xs] : 0u, GT ? q1[ro + xs] : 0u, rb || xs == 0 || xs == w - 1) << (8 * k);
        }
      }
    }
    *reinterpret_cast<unsigned*>(&M[r][4 * g]) = packed;
  }
  __syncthreads();

  // ---- four pixels per lane, one row per wave and pass
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int x = x0 + 4 * lane;
#pragma unroll 1
  for (int it = 0; it < OV_TY / 4; ++it) {
    const int ry = wv + 4 * it, y = y0 + ry;
    if (y >= h || x >= w) continue;
    float v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* p = img + (((size_t)b * 3 + c) * h + y) * w + x;
      if (vec) {                                                   // w % 4 == 0: x + 3 < w whenever x < w
        const f32x4 t = *reinterpret_cast<const f32x4*>(p);
        v[c][0] = t[0]; v[c][1] = t[1]; v[c][2] = t[2]; v[c][3] = t[3];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[c][k] = x + k < w ? p[k] : 0.f;
      }
    }
    // m[rr][i]: rows y - 1 .. y + 2, columns x - 1 .. x + 5 (pixel k of the lane sits at i = k + 1)
    unsigned m[4][7];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const unsigned* row = reinterpret_cast<const unsigned*>(&M[ry + rr][4 * lane]);
      const unsigned d0 = row[0], d1 = row[1], d2 = row[2];
      m[rr][0] = d0 >> 24;
      m[rr][1] = d1 & 255u; m[rr][2] = (d1 >> 8) & 255u; m[rr][3] = (d1 >> 16) & 255u; m[rr][4] = d1 >> 24;
      m[rr][5] = d2 & 255u; m[rr][6] = (d2 >> 8) & 255u;
    }
    const size_t s = (((size_t)b * h + y) * w + x0) * 3;           // global byte offset of the row segment in both outputs
    const int pad = (int)(s & 3);
    const bool yu = y >= 1, yd = y <= h - 2, yd2 = y + 1 <= h - 2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int xk = x + k;
      if (xk >= w) break;
      const bool xl = xk >= 1, xr = xk <= w - 2, xr2 = xk + 1 <= w - 2;
      const int cc = k + 1;
#define T_(dr, dc) m[1 + (dr)][cc + (dc)]
#define EH_(dr, dc) (T_(dr, dc) ^ T_(dr, (dc) + 1))
#define EV_(dr, dc) (T_(dr, dc) ^ T_((dr) + 1, dc))
      unsigned pt = (xl ? EH_(0, -1) : 0u) | (xr ? EH_(0, 0) : 0u) | (xr2 ? EH_(0, 1) : 0u);
      pt |= (xr ? EH_(1, 0) : 0u) | (xr2 ? EH_(1, 1) : 0u);
      if (yu) pt |= (xr ? EH_(-1, 0) : 0u) | (xl ? EH_(-1, -1) : 0u) | EV_(-1, 0) | (xl ? EV_(-1, -1) : 0u);
      if (yd) pt |= EV_(0, 0) | (xl ? EV_(0, -1) : 0u) | EV_(0, 1);
      if (yd2) pt |= EV_(1, 0) | EV_(1, 1);
#undef T_
#undef EH_
#undef EV_
      unsigned char* o0 = &S0[ry][pad + 3 * (4 * lane + k)];
      unsigned char* o1 = &S1[ry][pad + 3 * (4 * lane + k)];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        // (img + 1) * 127.5, two roundings (utils.py:461): the intrinsics keep the compiler from contracting them into one FMA
        const unsigned u = (unsigned)(int)__fmul_rn(__fadd_rn(v[c][k], 1.0f), 127.5f) & 255u;
        unsigned col = u;
        if (pt & 12u) col = c == 0 ? 255u : 0u;                    // ground truth: red [255, 0, 0]
        else if (pt & 1u) col = c == 2 ? 255u : 0u;                // channel 0 ("disc_map": the cup): blue [0, 0, 255]
        else if (pt & 2u) col = c == 1 ? 255u : 0u;                // channel 1 ("cup_map": disc or cup): green [0, 255, 0]
        o0[c] = (unsigned char)u;
        o1[c] = (unsigned char)col;
      }
    }
  }
  __syncthreads();

  // ---- staged rows -> global memory: aligned dwords, bytes at the two ends of a row segment
  const int nb = 3 * min(OV_TX, w - x0);
  for (int idx = threadIdx.x; idx < OV_TY * OV_SD; idx += 256) {
    const int ry = idx / OV_SD, d = idx - ry * OV_SD;
    const int y = y0 + ry;
    if (y >= h) break;
    const size_t s = (((size_t)b * h + y) * w + x0) * 3;
    const int pad = (int)(s & 3);
    const int lo = 4 * d, hi = lo + 4;
    if (lo >= pad + nb) continue;
    unsigned char* g0 = original + (s - pad) + lo;
    unsigned char* g1 = overlay + (s - pad) + lo;
    if (lo >= pad && hi <= pad + nb) {
      *reinterpret_cast<unsigned*>(g0) = *reinterpret_cast<const unsigned*>(&S0[ry][lo]);
      *reinterpret_cast<unsigned*>(g1) = *reinterpret_cast<const unsigned*>(&S1[ry][lo]);
    } else {
      for (int j = max(lo, pad); j < min(hi, pad + nb); ++j) {
        g0[j - lo] = S0[ry][j];
        g1[j - lo] = S1[ry][j];
      }
    }
  }
}

// Ground-truth composite as pseudo-logits for wtpse_postprocess: logit [2][n], channel 0 = cup, channel 1 = disc OR cup
// (test_visulization.py:251-256: target[mask_od == 1] = [0, 1]; target[mask_oc == 1] = [1, 1]).
template <int VEC>
__global__ __launch_bounds__(256) void overlay_gt_logits_k(const unsigned char* __restrict__ gt_od, const unsigned char* __restrict__ gt_oc,
                                                           float* __restrict__ logit, long long n) {
  const long long step = (long long)gridDim.x * 256;
  if (VEC) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n / 4; i += step) {
      const unsigned a = reinterpret_cast<const unsigned*>(gt_od)[i], c = reinterpret_cast<const unsigned*>(gt_oc)[i];
      f32x4 l0, l1;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned od = (a >> (8 * k)) & 255u, oc = (c >> (8 * k)) & 255u;
        l0[k] = oc == 1u ? OV_LOGIT : -OV_LOGIT;
        l1[k] = (od == 1u || oc == 1u) ? OV_LOGIT : -OV_LOGIT;
      }
      reinterpret_cast<f32x4*>(logit)[i] = l0;
      reinterpret_cast<f32x4*>(logit + n)[i] = l1;
    }
  } else {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
      const unsigned od = gt_od[i], oc = gt_oc[i];
      logit[i] = oc == 1u ? OV_LOGIT : -OV_LOGIT;
      logit[n + i] = (od == 1u || oc == 1u) ? OV_LOGIT : -OV_LOGIT;
    }
  }
}

// The labels of the test feed at their original size (fundus_dataloader.py:112-134): od = (mask <= 200), oc = (mask <= 50).
template <int VEC>
__global__ __launch_bounds__(256) void label_thresholds_k(const unsigned char* __restrict__ mask, float* __restrict__ od,
                                                          float* __restrict__ oc, long long n) {
  const long long step = (long long)gridDim.x * 256;
  if (VEC) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n / 4; i += step) {
      const unsigned a = reinterpret_cast<const unsigned*>(mask)[i];
      f32x4 d, c;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned v = (a >> (8 * k)) & 255u;
        d[k] = v > 200u ? 0.f : 1.f;
        c[k] = v > 50u ? 0.f : 1.f;
      }
      reinterpret_cast<f32x4*>(od)[i] = d;
      reinterpret_cast<f32x4*>(oc)[i] = c;
    }
  } else {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
      const unsigned v = mask[i];
      od[i] = v > 200u ? 0.f : 1.f;
      oc[i] = v > 50u ? 0.f : 1.f;
    }
  }
}

// ---- entry points (see include/wtpse_hip.h) ------------------------------------------------------------------------------
static bool ov_dims_ok(int B, int h, int w) {
  return B > 0 && B < 32768 && h >= 2 && w >= 2 && h <= OV_MAXDIM && w <= OV_MAXDIM;
}
static bool ov_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static unsigned ov_stream_blocks(long long items) {                // a memory-bound pass: at most 2048 workgroups, grid-stride the rest
  const long long nb = (items + 255) / 256;
  return (unsigned)(nb < 1 ? 1 : nb > 2048 ? 2048 : nb);
}

// words: wtpse_postprocess's own workspace for 2B images (first: it wants 8-byte alignment; rounded to 16 bytes for the vector stores
// behind it), the 2B pseudo-logit maps, the 2B filled masks (bytes, rounded up to words)
extern "C" int wtpse_overlay_ws(int B, int h, int w) {
  if (!ov_dims_ok(B, h, w)) return -1;
  const int pp = wtpse_postprocess_ws(2 * B, h, w);
  if (pp <= 0) return -1;
  const long long n2 = 2LL * B * h * w;
  const long long words = ((long long)pp + 3) / 4 * 4 + n2 + (n2 + 3) / 4;
  return words > 0x7fffffffLL ? -1 : (int)words;
}

extern "C" int wtpse_overlay(const float* img, const unsigned char* pred_od, const unsigned char* pred_oc, const unsigned char* gt_od,
                             const unsigned char* gt_oc, unsigned char* original, unsigned char* overlay, void* ws, int B, int h, int w,
                             void* stream) {
  WTPSE_REQUIRE(img && pred_od && pred_oc && gt_od && gt_oc && original && overlay && ws && wtpse_overlay_ws(B, h, w) > 0);
  WTPSE_REQUIRE(ov_aligned(img, 4) && ov_aligned(original, 4) && ov_aligned(overlay, 4) && ov_aligned(ws, 8));
  const long long n = (long long)B * h * w;
  const long long pp = ((long long)wtpse_postprocess_ws(2 * B, h, w) + 3) / 4 * 4;
  float* logit = (float*)ws + pp;
  unsigned char* gf = (unsigned char*)(logit + 2 * n);
  const hipStream_t st = (hipStream_t)stream;
  const int vecn = (n & 3) == 0 && ov_aligned(gt_od, 4) && ov_aligned(gt_oc, 4) && ov_aligned(logit, 16);
  if (vecn)
    hipLaunchKernelGGL(overlay_gt_logits_k<1>, dim3(ov_stream_blocks(n / 4)), dim3(256), 0, st, gt_od, gt_oc, logit, n);
  else
    hipLaunchKernelGGL(overlay_gt_logits_k<0>, dim3(ov_stream_blocks(n)), dim3(256), 0, st, gt_od, gt_oc, logit, n);
  const int rc = wtpse_postprocess(logit, gf, ws, 0.5f, 2 * B, h, w, stream);
  if (rc) return rc;
  const int vec = (w & 3) == 0 && ov_aligned(img, 16) && ov_aligned(pred_od, 4) && ov_aligned(pred_oc, 4) && ov_aligned(gf, 4);
  hipLaunchKernelGGL(overlay_k<1>, dim3((unsigned)ceil_div(w, OV_TX), (unsigned)ceil_div(h, OV_TY), (unsigned)B), dim3(256), 0, st, img,
                     pred_od, pred_oc, gf, original, overlay, B, h, w, vec);
  return wtpse_status();
}

// No ground-truth stage, so no scratch: 0 words for a supported size, -1 otherwise (the sizes wtpse_overlay takes).
extern "C" int wtpse_overlay_pred_ws(int B, int h, int w) { return ov_dims_ok(B, h, w) ? 0 : -1; }

extern "C" int wtpse_overlay_pred(const float* img, const unsigned char* pred_od, const unsigned char* pred_oc, unsigned char* original,
                                  unsigned char* overlay, int B, int h, int w, void* stream) {
  WTPSE_REQUIRE(img && pred_od && pred_oc && original && overlay && wtpse_overlay_pred_ws(B, h, w) == 0);
  WTPSE_REQUIRE(ov_aligned(img, 4) && ov_aligned(original, 4) && ov_aligned(overlay, 4));
  const int vec = (w & 3) == 0 && ov_aligned(img, 16) && ov_aligned(pred_od, 4) && ov_aligned(pred_oc, 4);
  hipLaunchKernelGGL(overlay_k<0>, dim3((unsigned)ceil_div(w, OV_TX), (unsigned)ceil_div(h, OV_TY), (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, img, pred_od, pred_oc, (const unsigned char*)nullptr, original, overlay, B, h, w, vec);
  return wtpse_status();
}

extern "C" int wtpse_label_thresholds(const unsigned char* mask, float* od, float* oc, long long n, void* stream) {
  WTPSE_REQUIRE(mask && od && oc && n > 0);
  const hipStream_t st = (hipStream_t)stream;
  if ((n & 3) == 0 && ov_aligned(mask, 4) && ov_aligned(od, 16) && ov_aligned(oc, 16))
    hipLaunchKernelGGL(label_thresholds_k<1>, dim3(ov_stream_blocks(n / 4)), dim3(256), 0, st, mask, od, oc, n);
  else
    hipLaunchKernelGGL(label_thresholds_k<0>, dim3(ov_stream_blocks(n)), dim3(256), 0, st, mask, od, oc, n);
  return wtpse_status();
}
