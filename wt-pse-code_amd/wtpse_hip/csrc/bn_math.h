// The per-channel BatchNorm arithmetic of the step, each formula ONCE: bn.hip's kernels, the tails of the convolutions (common.h:
// bnf_tail / bnb_tail), the convolution epilogues, the upsampling backward and the weight gradient's loader all call these, so two
// places that must produce the same bits do so by construction.  Nothing here chooses WHERE a caller multiplies by invstd or in which
// order it folds its partials — that stays with the caller; the expressions below fix the order of everything else (fp64 included).
//   forward : z = act(y * scale + shift), scale = gamma * invstd, shift = beta - mean * scale
//   backward: g = dz * [z > 0];  s1 = sum g;  s2 = sum g * (y - mean) * invstd;  dbeta = s1;  dgamma = s2;  dy = k1 * g + k2 * y + k3
//             k1 = gamma * invstd,  k2 = -gamma * invstd^2 * s2 / N,  k3 = -k1 * s1 / N - k2 * mean
//   frozen (running) statistics: no term through them — k2 = k3 = 0, and the conv bias in front receives k1 * s1
#pragma once
#include <hip/hip_runtime.h>

// ---- forward finish: (sum, sum of squares) of n values -> mean and the biased variance, clamped at 0
__device__ __forceinline__ void bn_moments(double s1, double s2, double n, double& mean, double& var) {
  mean = s1 / n;
  var = s2 / n - mean * mean;
  if (var < 0.0) var = 0.0;
}
// -> invstd; scale_shift[c] = the (scale, shift) pair the consumers apply on load.  (Arrays and the channel, not values: gamma and
// beta are then read, and the addresses formed, where the expressions stand — handing in values or references changed the code of
// every convolution whose tail calls this.)
__device__ __forceinline__ double bn_fwd_channel(double mean, double var, const float* gamma, const float* beta, float eps,
                                                 float* scale_shift, int c) {
  const double invstd = 1.0 / sqrt(var + (double)eps);
  scale_shift[2 * c] = (float)(gamma[c] * invstd);
  scale_shift[2 * c + 1] = (float)(beta[c] - mean * gamma[c] * invstd);
  return invstd;
}
// nn.BatchNorm2d's running statistics: momentum, and the UNBIASED variance of the batch
__device__ __forceinline__ void bn_running_update(float* rmean, float* rvar, int c, double mean, double var, double count, float momentum) {
  const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
  rmean[c] = (float)((1.0 - momentum) * rmean[c] + momentum * mean);
  rvar[c] = (float)((1.0 - momentum) * rvar[c] + momentum * unbiased);
}

// ---- backward finish: s1 = sum g, s2 = sum g (y - mean) ALREADY divided by std (the callers keep their own place for that multiply).
// dbeta[c] / dgamma[c] (+)= this rank's sums ...
__device__ __forceinline__ void bn_bwd_store(int c, double s1, double s2, int accumulate, float* dbeta, float* dgamma) {
  dbeta[c] = accumulate ? dbeta[c] + (float)s1 : (float)s1;
  dgamma[c] = accumulate ? dgamma[c] + (float)s2 : (float)s2;
}
// ... then (k1, k2, k3) -> coef[c], from the sums of all ranks where the BatchNorm is synchronised.  dbias non-null = frozen statistics:
// k2 = k3 = 0 and dbias[c] (+)= k1 s1.  (The frozen form and its store are ONE branch, as every caller had them: as a value returned
// beside the coefficients it became selects in the convolutions' tails, whose code must not move.  mean: the array, read in k3.)
__device__ __forceinline__ void bn_bwd_channel(int c, double invstd, double gamma, double s1, double s2, double count, const float* mean,
                                               int accumulate, float* dbias, float* coef) {
  const double k1 = gamma * invstd;
  double k2 = -gamma * invstd * invstd * s2 / count;
  double k3 = -k1 * s1 / count - k2 * (double)mean[c];
  if (dbias) {
    k2 = k3 = 0.0;
    dbias[c] = accumulate ? dbias[c] + (float)(k1 * s1) : (float)(k1 * s1);
  }
  coef[3 * c] = (float)k1;
  coef[3 * c + 1] = (float)k2;
  coef[3 * c + 2] = (float)k3;
}

// ---- the ReLU decision, taken exactly as the forward pass took it: z = fmaf(y, scale, shift) > 0
__device__ __forceinline__ bool bn_relu_live(float y, float sc, float sf) { return fmaf(y, sc, sf) > 0.f; }
__device__ __forceinline__ void bn_relu_mask4(float4& g, float4 y, float sc, float sf) {
  if (!bn_relu_live(y.x, sc, sf)) g.x = 0.f;
  if (!bn_relu_live(y.y, sc, sf)) g.y = 0.f;
  if (!bn_relu_live(y.z, sc, sf)) g.z = 0.f;
  if (!bn_relu_live(y.w, sc, sf)) g.w = 0.f;
}
// The same decision for the convolution epilogues, opaque to the vectoriser on purpose: with two pixels' decisions fused into one
// v_pk_fma_f32 the masks of a few lanes of the upper half-wave came out wrong in ~10 % of the launches (tools/probe/dbg_bnb.py,
// DESIGN.md); scalar v_fma_f32 has been bitwise reproducible over thousands of launches.
__device__ __forceinline__ bool bn_relu_live_opaque(float y, float sc, float sf) {
  float zz = __builtin_fmaf(y, sc, sf);
  asm volatile("" : "+v"(zz));
  return zz > 0.f;
}
// What those epilogues decide with, staged by the thread of output channel c: its entry q of three planes [scale | shift | mean] of
// CB floats; (0, 1, 0) — always live, nothing subtracted — outside the BatchNorm'd channels [bn_c0, bn_c1), (0, 1, mean) without a ReLU.
// a: the kernel's argument struct (ConvArgs / X3Args: bn_ss, bn_mean, bn_relu, bn_c0, bn_c1), read where the original text read it.
template <int CB, typename Args>
__device__ __forceinline__ void bnb_stage(float* q, int c, const Args& a) {
  const bool bn = c >= a.bn_c0 && c < a.bn_c1;
  q[0] = (bn && a.bn_relu) ? a.bn_ss[2 * (c - a.bn_c0)] : 0.f;
  q[CB] = (bn && a.bn_relu) ? a.bn_ss[2 * (c - a.bn_c0) + 1] : 1.f;
  q[2 * CB] = bn ? a.bn_mean[c - a.bn_c0] : 0.f;
}

// ---- the two sums of masked gradients, s1 += sum g, s2 += sum g * (y - mean), in this association
__device__ __forceinline__ void bn_bwd_fold(float& s1, float& s2, float g, float y, float mu) {
  s1 += g;
  s2 += g * (y - mu);
}
__device__ __forceinline__ void bn_bwd_fold4(float& s1, float& s2, float4 g, float4 y, float mu) {
  s1 += (g.x + g.y) + (g.z + g.w);
  s2 += (g.x * (y.x - mu) + g.y * (y.y - mu)) + (g.z * (y.z - mu) + g.w * (y.w - mu));
}

// ---- the apply expression
__device__ __forceinline__ float bn_dy(float k1, float k2, float k3, float g, float y) { return fmaf(k1, g, fmaf(k2, y, k3)); }
__device__ __forceinline__ float4 bn_dy4(float k1, float k2, float k3, float4 g, float4 y) {
  return make_float4(bn_dy(k1, k2, k3, g.x, y.x), bn_dy(k1, k2, k3, g.y, y.y), bn_dy(k1, k2, k3, g.z, y.z), bn_dy(k1, k2, k3, g.w, y.w));
}
