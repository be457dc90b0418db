// Device-side training augmentations: the optional stage of the input pipeline between the crop and input_finish_k
// (pipeline.hip).  The reference applies them per sample on one host thread — RandomRotate, RandomFlip, elastic_transform,
// add_salt_pepper_noise, adjust_light, eraser (custom_transforms.py:310-327,204-217,87-132,22-43,45-55,58-85); its elastic
// transform alone (two gaussian_filter calls with sigma = 0.08 * S, four map_coordinates calls) costs 35-40 ms per sample.
// Here the random draws stay on the host (input_pipeline.draw_augment) and the pixels on the GPU, bit for bit:
//   uniform_f64_k     : the two uniform fields of the elastic transform, Philox4x32-10, 53 bits per number
//   blur_k            : one pass of scipy's gaussian_filter(mode="constant") in fp64 — the hot path: radius 82 at S = 256, 165
//                       taps, two passes, two fields per sample; a strip of the field plus its halo is staged in LDS
//   geometry_k        : rotation by k * 90 degrees and the two flips as one index gather, fused with the NEAREST resize + crop
//                       of the disc mask (the index tables input_finish_k would read it through)
//   warp_k            : map_coordinates(order=1) for image (mode="constant") and mask (mode="nearest")
//   photometric_k /   : gamma table and eraser rectangle per pixel, then the salt-and-pepper points of every sample
//   points_k
// Bitwise equality with scipy rests on every fp64 operation being one correctly rounded IEEE add or multiply in scipy's order:
// contraction is off for this whole file (no FMA).
#include "common.h"

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------ uniform doubles
__global__ __launch_bounds__(256) void uniform_f64_k(double* __restrict__ out, long long n, unsigned long long seed,
                                                     unsigned long long pos) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long g = pos + (unsigned long long)i, ctr = g >> 1;
  uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0, c3 = 0;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  const uint32_t a = (g & 1) ? c2 : c0, b = (g & 1) ? c3 : c1;
  // 27 + 26 bits: exact in a double, so the product with 2^-53 is exact too
  out[i] = ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// ------------------------------------------------------------------------------------------------ separable fp64 blur
#define BLUR_TA 64   // outputs along the filtered axis per workgroup
#define BLUR_TB 16   // lines (positions along the other axis) per workgroup

// One workgroup = (plane, strip): BLUR_TB lines of BLUR_TA outputs; tile[b][a] holds line b's BLUR_TA + 2 * radius sources (zeros
// outside the field, which is what mode="constant", cval=0 extends it with).  Lanes run along the filtered axis, so the LDS reads
// of one instruction are consecutive doubles; every thread keeps four lines' accumulators and shares w[j] (staged in LDS too).
template <int AXIS>
__global__ __launch_bounds__(256) void blur_k(const double* __restrict__ src, double* __restrict__ dst, const double* __restrict__ w,
                                              const int* __restrict__ src_index, int radius, int S, int pre, double post) {
  extern __shared__ double tile[];
  const int LA = BLUR_TA + 2 * radius + 1;     // odd: lines are an odd number of doubles apart, so a column of the tile spreads over the banks
  const int NA = BLUR_TA + 2 * radius;         // sources per line
  double* wl = tile + BLUR_TB * LA;            // the kernel's half, read by every lane at the same index (LDS broadcast)
  for (int j = threadIdx.x; j <= radius; j += 256) wl[j] = w[j];
  const int p = blockIdx.y;
  const int tiles_a = (S + BLUR_TA - 1) / BLUR_TA;
  const int a0 = (blockIdx.x % tiles_a) * BLUR_TA, b0 = (blockIdx.x / tiles_a) * BLUR_TB;
  const size_t plane = (size_t)S * S;
  const double* s = src + (src_index ? ((size_t)src_index[p >> 1] * 2 + (p & 1)) : (size_t)p) * plane;
  for (int e = threadIdx.x; e < BLUR_TB * NA; e += 256) {
    int a, b;
    if (AXIS == 1) { a = e % NA; b = e / NA; } else { b = e % BLUR_TB; a = e / BLUR_TB; }   // lanes along the contiguous axis
    const int ga = a0 - radius + a, gb = b0 + b;
    double v = 0.0;
    if (ga >= 0 && ga < S && gb < S) {
      v = AXIS == 1 ? s[(size_t)gb * S + ga] : s[(size_t)ga * S + gb];
      if (pre) v = v * 2.0 - 1.0;
    }
    tile[b * LA + a] = v;
  }
  __syncthreads();
  const int a = threadIdx.x % BLUR_TA, bq = threadIdx.x / BLUR_TA;     // lines bq, bq + 4, bq + 8, bq + 12
  const double* c = tile + bq * LA + radius + a;
  const int L4 = 4 * LA;
  const double w0 = wl[0];
  double acc0 = c[0] * w0, acc1 = c[L4] * w0, acc2 = c[2 * L4] * w0, acc3 = c[3 * L4] * w0;
  for (int j = radius; j >= 1; --j) {
    const double wj = wl[j];
    acc0 = acc0 + (c[-j] + c[j]) * wj;
    acc1 = acc1 + (c[L4 - j] + c[L4 + j]) * wj;
    acc2 = acc2 + (c[2 * L4 - j] + c[2 * L4 + j]) * wj;
    acc3 = acc3 + (c[3 * L4 - j] + c[3 * L4 + j]) * wj;
  }
  const double acc[4] = {acc0, acc1, acc2, acc3};
  double* d = dst + (size_t)p * plane;
  const int ga = a0 + a;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int gb = b0 + bq + 4 * q;
    if (ga < S && gb < S) d[AXIS == 1 ? (size_t)gb * S + ga : (size_t)ga * S + gb] = acc[q] * post;
  }
}

// ------------------------------------------------------------------------------------------------ rotate + flip (+ mask crop)
__global__ __launch_bounds__(256) void geometry_k(const unsigned char* __restrict__ img, const unsigned char* __restrict__ od,
                                                  const int* __restrict__ xidx, const int* __restrict__ yidx,
                                                  const int* __restrict__ code, unsigned char* __restrict__ img_out,
                                                  unsigned char* __restrict__ mask_out, int S) {
  const int n = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= S * S) return;
  int y = p / S, x = p - y * S;
  const int cd = code[n], k = cd & 3;
  if (cd & 8) y = S - 1 - y;                    // undo FLIP_TOP_BOTTOM (applied last), then FLIP_LEFT_RIGHT, then the rotation
  if (cd & 4) x = S - 1 - x;
  int sy = y, sx = x;                           // rotated[y][x] = source[sy][sx], counter-clockwise by k quarter turns
  if (k == 1) { sy = x; sx = S - 1 - y; }
  else if (k == 2) { sy = S - 1 - y; sx = S - 1 - x; }
  else if (k == 3) { sy = S - 1 - x; sx = y; }
  const size_t base = (size_t)n * S * S;
  const unsigned char* px = img + (base + (size_t)sy * S + sx) * 3;
  unsigned char* o = img_out + (base + p) * 3;
  o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
  mask_out[base + p] = od[base + (size_t)yidx[n * S + sy] * S + xidx[n * S + sx]];
}

// ------------------------------------------------------------------------------------------------ bilinear warp
__device__ __forceinline__ double blend(double tx, double ty, double g00, double g01, double g10, double g11) {
  return (1.0 - tx) * ((1.0 - ty) * g00 + ty * g01) + tx * ((1.0 - ty) * g10 + ty * g11);
}

__global__ __launch_bounds__(256) void warp_k(const unsigned char* __restrict__ img, const unsigned char* __restrict__ mask,
                                              const double* __restrict__ disp, const int* __restrict__ slot,
                                              unsigned char* __restrict__ img_out, unsigned char* __restrict__ mask_out, int S) {
  const int n = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= S * S) return;
  const size_t base = (size_t)n * S * S;
  const unsigned char* im = img + base * 3;
  const unsigned char* mk = mask + base;
  unsigned char* o = img_out + (base + p) * 3;
  const int sl = slot[n];
  if (sl < 0) {
    o[0] = im[(size_t)p * 3]; o[1] = im[(size_t)p * 3 + 1]; o[2] = im[(size_t)p * 3 + 2];
    mask_out[base + p] = mk[p];
    return;
  }
  const int r = p / S, c = p - r * S;
  const double* d = disp + (size_t)sl * 2 * S * S;
  const double last = (double)(S - 1);
  double cx = (double)r + d[p], cy = (double)c + d[(size_t)S * S + p];
  // image, mode="constant": outside the picture on either axis -> cval = 0
  if (cx < 0.0 || cx > last || cy < 0.0 || cy > last) {
    o[0] = o[1] = o[2] = 0;
  } else {
    const double fx = floor(cx), fy = floor(cy);
    const double tx = cx - fx, ty = cy - fy;
    const int x0 = (int)fx, y0 = (int)fy;
    const int x1 = x0 + 1 < S ? x0 + 1 : S - 1, y1 = y0 + 1 < S ? y0 + 1 : S - 1;     // reached with weight 0 only
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const double v = blend(tx, ty, (double)im[((size_t)x0 * S + y0) * 3 + ch], (double)im[((size_t)x0 * S + y1) * 3 + ch],
                             (double)im[((size_t)x1 * S + y0) * 3 + ch], (double)im[((size_t)x1 * S + y1) * 3 + ch]);
      o[ch] = (unsigned char)floor(v + 0.5);
    }
  }
  // mask, mode="nearest": the coordinate is clamped to the picture
  cx = cx < 0.0 ? 0.0 : (cx > last ? last : cx);
  cy = cy < 0.0 ? 0.0 : (cy > last ? last : cy);
  const double fx = floor(cx), fy = floor(cy);
  const double tx = cx - fx, ty = cy - fy;
  const int x0 = (int)fx, y0 = (int)fy;
  const int x1 = x0 + 1 < S ? x0 + 1 : S - 1, y1 = y0 + 1 < S ? y0 + 1 : S - 1;
  const double v = blend(tx, ty, (double)mk[(size_t)x0 * S + y0], (double)mk[(size_t)x0 * S + y1], (double)mk[(size_t)x1 * S + y0],
                         (double)mk[(size_t)x1 * S + y1]);
  mask_out[base + p] = (unsigned char)floor(v + 0.5);
}

// ------------------------------------------------------------------------------------------------ photometric pass
__device__ __forceinline__ bool in_rect(const int* __restrict__ rc, int y, int x) {
  return rc[2] > 0 && y >= rc[0] && y < rc[0] + rc[2] && x >= rc[1] && x < rc[1] + rc[3];
}

__global__ __launch_bounds__(256) void photometric_k(unsigned char* __restrict__ img, const unsigned char* __restrict__ lut,
                                                     const int* __restrict__ rect, int S) {
  const int n = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= S * S) return;
  const int y = p / S, x = p - y * S;
  const int* rc = rect + n * 5;
  const unsigned char* t = lut + n * 256;
  unsigned char* px = img + ((size_t)n * S * S + p) * 3;
  if (in_rect(rc, y, x)) {
    px[0] = px[1] = px[2] = (unsigned char)rc[4];
  } else {
    px[0] = t[px[0]]; px[1] = t[px[1]]; px[2] = t[px[2]];
  }
}

// after photometric_k: the noise points (written before the gamma table in the reference, so they hold lut[value]; the eraser's
// rectangle, which comes last, wins).  Several points on one pixel write the same byte.
__global__ __launch_bounds__(256) void points_k(unsigned char* __restrict__ img, const unsigned char* __restrict__ lut,
                                                const int* __restrict__ rect, const int* __restrict__ pts,
                                                const int* __restrict__ pt_off, const int* __restrict__ pt_val, int S) {
  const int n = blockIdx.y;
  const int i = pt_off[n] + blockIdx.x * 256 + threadIdx.x;
  if (i >= pt_off[n + 1]) return;
  const int p = pts[i];
  if (p < 0 || p >= S * S) return;
  const int y = p / S, x = p - y * S;
  if (in_rect(rect + n * 5, y, x)) return;
  const unsigned char v = lut[n * 256 + (pt_val[n] & 255)];
  unsigned char* px = img + ((size_t)n * S * S + p) * 3;
  px[0] = px[1] = px[2] = v;
}

// ================================================================================================ C ABI (include/wtpse_hip.h)
#define ST ((hipStream_t)stream)
#define PIXEL_GRID(S, N) dim3((unsigned)(((S) * (S) + 255) / 256), (unsigned)(N))

extern "C" int wtpse_uniform_f64(double* out, long long n, unsigned long long seed, unsigned long long pos, void* stream) {
  WTPSE_REQUIRE(out && n > 0 && n < (1LL << 39));
  hipLaunchKernelGGL(uniform_f64_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST, out, n, seed, pos);
  return wtpse_status();
}

extern "C" int wtpse_aug_blur(const double* src, double* dst, const double* w, const int* src_index, int radius, int planes, int S,
                              int axis, int pre, double post, void* stream) {
  WTPSE_REQUIRE(src && dst && src != dst && w && radius >= 0 && radius <= 216 && planes > 0 && planes < 65536 && S > 0 && S <= 16384 &&
                (axis == 0 || axis == 1) && (!src_index || planes % 2 == 0));
  const size_t lds = ((size_t)BLUR_TB * (BLUR_TA + 2 * radius + 1) + radius + 1) * sizeof(double);      // tile + weights <= 64 KiB
  const dim3 grid((unsigned)(((S + BLUR_TA - 1) / BLUR_TA) * ((S + BLUR_TB - 1) / BLUR_TB)), (unsigned)planes);
  if (axis == 0)
    hipLaunchKernelGGL(blur_k<0>, grid, dim3(256), lds, ST, src, dst, w, src_index, radius, S, pre, post);
  else
    hipLaunchKernelGGL(blur_k<1>, grid, dim3(256), lds, ST, src, dst, w, src_index, radius, S, pre, post);
  return wtpse_status();
}

extern "C" int wtpse_aug_geometry(const unsigned char* img, const unsigned char* od, const int* xidx, const int* yidx, const int* code,
                                  unsigned char* img_out, unsigned char* mask_out, int N, int S, void* stream) {
  WTPSE_REQUIRE(img && od && xidx && yidx && code && img_out && mask_out && img != img_out && N > 0 && N < 65536 && S > 0 && S <= 16384);
  hipLaunchKernelGGL(geometry_k, PIXEL_GRID(S, N), dim3(256), 0, ST, img, od, xidx, yidx, code, img_out, mask_out, S);
  return wtpse_status();
}

extern "C" int wtpse_aug_warp(const unsigned char* img, const unsigned char* mask, const double* disp, const int* slot,
                              unsigned char* img_out, unsigned char* mask_out, int N, int S, void* stream) {
  WTPSE_REQUIRE(img && mask && disp && slot && img_out && mask_out && img != img_out && mask != mask_out && N > 0 && N < 65536 &&
                S > 0 && S <= 16384);
  hipLaunchKernelGGL(warp_k, PIXEL_GRID(S, N), dim3(256), 0, ST, img, mask, disp, slot, img_out, mask_out, S);
  return wtpse_status();
}

extern "C" int wtpse_aug_photometric(unsigned char* img, const unsigned char* lut, const int* rect, const int* pts, const int* pt_off,
                                     const int* pt_val, int max_pts, int N, int S, void* stream) {
  WTPSE_REQUIRE(img && lut && rect && pt_off && pt_val && max_pts >= 0 && (pts || max_pts == 0) && N > 0 && N < 65536 && S > 0 &&
                S <= 16384);
  hipLaunchKernelGGL(photometric_k, PIXEL_GRID(S, N), dim3(256), 0, ST, img, lut, rect, S);
  if (max_pts > 0)
    hipLaunchKernelGGL(points_k, dim3((unsigned)((max_pts + 255) / 256), (unsigned)N), dim3(256), 0, ST, img, lut, rect, pts, pt_off,
                       pt_val, S);
  return wtpse_status();
}
