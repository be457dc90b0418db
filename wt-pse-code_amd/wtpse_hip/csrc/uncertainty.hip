// Sampled shape latents (wtpse_hip/uncertainty.py; WT_PSE.predict_samples): K draws of z ~ N(mu, exp(logvar)) per pixel and, for
// each, everything the network computes behind the latent — attention, fusion, the 1x1 output convolution, the sigmoid — folded into
// the per-pixel mean, spread and vote count of the K predictions.  All of it is pointwise, so one launch does it:
//
//   shape_samples_k : a lane owns four consecutive pixels of one image.  It reads them once — CE + 2 loads of 16 bytes (emb, mu,
//                     logvar: 40 bytes per pixel at CE = 8) — and keeps the K loop in registers: per sample one Philox4x32-10 block
//                     (philox_normal4, common.h: exactly the four normals wtpse_randn puts at these four stream positions, because
//                     HW and the offset are multiples of 4) or one 16-byte load of injected noise, then per pixel
//                         z = mu + (scale std) eps,  a = sigmoid(w z + b),  logit = (coef + a) S + bout (+ wz z),  p = sigmoid(logit)
//                     and a running Welford update of (mean, M2).  It writes two floats and a byte per pixel (16 + 16 + 4 bytes per
//                     lane), plus 16 bytes per sample when the logits are asked for.  No LDS, no atomics, plain vector stores.
//
//   samples_mask_k  : the cup's samples outside the predicted disc — what shape_samples_k would have written had the logits been
//                     multiplied by the {0,1} map od_pred first, as validate.predict_pair multiplies the deterministic ones: logit 0,
//                     probability 0.5 in every sample, so mean 0.5, spread 0, no vote.  Four pixels per lane, stores only where masked.
//
// The HOISTED form is taken: S = sum_c wout[c] emb[c] is formed once per pixel (channels in index order, fma chain) and
// logit = (coef + a) S + bout, where the composed path rounds fuse[c] = coef emb[c] + a emb[c] per channel and sums wout[c] fuse[c].
// The two differ by a few ulps of the largest term; uncertainty.shape_samples_host (fp64) is the specification of both.
//
// A quad's results depend on its own index alone: the grid (at most 2048 workgroups, grid-stride over the quads) does not enter them.
// All element indices are 64-bit; the stream position of a sample plane is offset + (b K + k) HW + p, in 64 bits as well.
#include "common.h"

#define US_MAX_K 64
#define US_MAX_CE 16

static bool us_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

__global__ __launch_bounds__(256) void shape_samples_k(const float* __restrict__ emb, int CE, const float* __restrict__ mu,
                                                       const float* __restrict__ logvar, const float* __restrict__ wb, float coef,
                                                       const float* __restrict__ wout, const float* __restrict__ bout,
                                                       const float* __restrict__ wz, float scale, int K, unsigned long long seed,
                                                       unsigned long long offset, const float* __restrict__ noise, float threshold,
                                                       float* __restrict__ mean, float* __restrict__ std_,
                                                       unsigned char* __restrict__ votes, float* __restrict__ logits, int HW,
                                                       long long nquads) {
  const long long step = (long long)gridDim.x * 256;
  const long long qpi = HW / 4;                                   // quads per image
  const float w = wb[0], bias = wb[1], b_out = bout[0], w_z = wz ? wz[0] : 0.f;
  const float inv_k = 1.f / (float)K;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nquads; q += step) {
    const long long b = q / qpi;
    const long long p = (q - b * qpi) * 4;                        // first pixel of the quad within its image
    const long long pix = b * HW + p;
    const f32x4 m4 = *reinterpret_cast<const f32x4*>(mu + pix);
    const f32x4 lv4 = *reinterpret_cast<const f32x4*>(logvar + pix);
    f32x4 S = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < CE; ++c) {
      const f32x4 e = *reinterpret_cast<const f32x4*>(emb + (b * CE + c) * HW + p);
      const float wc = wout[c];
#pragma unroll
      for (int j = 0; j < 4; ++j) S[j] = fmaf(wc, e[j], S[j]);
    }
    float sd[4], mean_[4], m2[4];
    unsigned nv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float s = expf(lv4[j] * 0.5f);
      sd[j] = isfinite(s) ? scale * s : 0.f;
      mean_[j] = 0.f;
      m2[j] = 0.f;
      nv[j] = 0u;
    }
    for (int k = 0; k < K; ++k) {
      const long long plane = (b * K + k) * HW + p;               // element of [B,K,HW]
      float eps[4];
      if (noise) {
        const f32x4 n4 = *reinterpret_cast<const f32x4*>(noise + plane);
#pragma unroll
        for (int j = 0; j < 4; ++j) eps[j] = n4[j];
      } else {
        philox_normal4((offset + (unsigned long long)plane) / 4, seed, eps);
      }
      f32x4 lg;
      const float inv_n = 1.f / (float)(k + 1);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float z = fmaf(sd[j], eps[j], m4[j]);
        const float a = sigmoidf_(fmaf(w, z, bias));
        float l = fmaf(coef + a, S[j], b_out);
        if (wz) l = fmaf(w_z, z, l);
        lg[j] = l;
        const float pr = sigmoidf_(l);
        const float d = pr - mean_[j];                            // Welford: equal samples leave d = 0 from the second on
        mean_[j] = fmaf(d, inv_n, mean_[j]);
        m2[j] = fmaf(d, pr - mean_[j], m2[j]);
        nv[j] += pr > threshold ? 1u : 0u;
      }
      if (logits) *reinterpret_cast<f32x4*>(logits + plane) = lg;
    }
    f32x4 mo, so;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mo[j] = mean_[j];
      so[j] = sqrtf(fmaxf(m2[j], 0.f) * inv_k);
    }
    *reinterpret_cast<f32x4*>(mean + pix) = mo;
    *reinterpret_cast<f32x4*>(std_ + pix) = so;
    *reinterpret_cast<unsigned*>(votes + pix) = nv[0] | (nv[1] << 8) | (nv[2] << 16) | (nv[3] << 24);
  }
}

__global__ __launch_bounds__(256) void samples_mask_k(const float* __restrict__ ref, float* __restrict__ mean, float* __restrict__ std_,
                                                     unsigned char* __restrict__ votes, float* __restrict__ logits, int K, int HW,
                                                     long long nquads) {
  const long long step = (long long)gridDim.x * 256;
  const long long qpi = HW / 4;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nquads; q += step) {
    const long long b = q / qpi;
    const long long p = (q - b * qpi) * 4;
    const long long pix = b * HW + p;
    const f32x4 r = *reinterpret_cast<const f32x4*>(ref + pix);
    const bool keep[4] = {r[0] > 0.f, r[1] > 0.f, r[2] > 0.f, r[3] > 0.f};
    if (keep[0] && keep[1] && keep[2] && keep[3]) continue;
    f32x4 m = *reinterpret_cast<const f32x4*>(mean + pix), s = *reinterpret_cast<const f32x4*>(std_ + pix);
    unsigned v = *reinterpret_cast<const unsigned*>(votes + pix);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (!keep[j]) {
        m[j] = 0.5f;
        s[j] = 0.f;
        v &= ~(255u << (8 * j));
      }
    *reinterpret_cast<f32x4*>(mean + pix) = m;
    *reinterpret_cast<f32x4*>(std_ + pix) = s;
    *reinterpret_cast<unsigned*>(votes + pix) = v;
    if (logits)
      for (int k = 0; k < K; ++k) {
        f32x4* lp = reinterpret_cast<f32x4*>(logits + (b * K + k) * HW + p);
        f32x4 l = *lp;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (!keep[j]) l[j] = 0.f;
        *lp = l;
      }
  }
}

static unsigned us_blocks(long long nquads) {                       // at most 2048 workgroups, grid-stride the rest
  const long long nb = (nquads + 255) / 256;
  return (unsigned)(nb > 2048 ? 2048 : nb);
}

extern "C" int wtpse_shape_samples_mask(const float* ref, float* mean, float* std_, unsigned char* votes, float* logits, int K, int B,
                                        int HW, void* stream) {
  WTPSE_REQUIRE(ref && mean && std_ && votes && K >= 1 && K <= US_MAX_K && B > 0 && HW > 0 && HW % 4 == 0);
  WTPSE_REQUIRE(us_aligned(ref, 16) && us_aligned(mean, 16) && us_aligned(std_, 16) && us_aligned(logits, 16) && us_aligned(votes, 4));
  const long long nquads = (long long)B * (HW / 4);
  hipLaunchKernelGGL(samples_mask_k, dim3(us_blocks(nquads)), dim3(256), 0, (hipStream_t)stream, ref, mean, std_, votes, logits, K, HW,
                     nquads);
  return wtpse_status();
}

extern "C" int wtpse_shape_samples(const float* emb, int CE, const float* mu, const float* logvar, const float* wb, float coef,
                                   const float* wout, const float* bout, const float* wz, float scale, int K,
                                   unsigned long long seed, unsigned long long offset, const float* noise, float threshold,
                                   float* mean, float* std_, unsigned char* votes, float* logits, int B, int HW, void* stream) {
  WTPSE_REQUIRE(emb && mu && logvar && wb && wout && bout && mean && std_ && votes);
  WTPSE_REQUIRE(K >= 1 && K <= US_MAX_K && CE >= 1 && CE <= US_MAX_CE && B > 0 && HW > 0);
  WTPSE_REQUIRE(HW % 4 == 0 && offset % 4 == 0);
  WTPSE_REQUIRE(scale >= 0.f);                                    // (false for a NaN as well)
  WTPSE_REQUIRE(us_aligned(emb, 16) && us_aligned(mu, 16) && us_aligned(logvar, 16) && us_aligned(noise, 16) && us_aligned(mean, 16) &&
                us_aligned(std_, 16) && us_aligned(logits, 16) && us_aligned(votes, 4));
  const long long nquads = (long long)B * (HW / 4);
  hipLaunchKernelGGL(shape_samples_k, dim3(us_blocks(nquads)), dim3(256), 0, (hipStream_t)stream, emb, CE, mu, logvar,
                     wb, coef, wout, bout, wz, scale, K, seed, offset, noise, threshold, mean, std_, votes, logits, HW, nquads);
  return wtpse_status();
}
