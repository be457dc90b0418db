// Standalone 2-D discrete wavelet transform (Haar / Daubechies-4 by lifting), analysis and synthesis, multi-level.
//
// NOT part of WT-PSE: the reference has no wavelet transform (its "WT" is the whitening transform) and
// nothing here is called from update()/predict().  BASELINE.json's wording names a "2-D DWT analysis/synthesis filter bank"
// with "wavefront shuffles for the separable Haar/Db lifting steps" and a "4-level DWT" HBM stress configuration; SURVEY.md
// §8f-4 allows it only as a standalone HBM-bandwidth micro-benchmark with a self-defined specification: oracle/dwt_cpu.py
// (periodic extension, orthonormal, Mallat layout), against which tests/test_dwt.py checks these kernels.  Parity unpinned.
//
// One launch per level (HBM-bound: reads and writes the level's h x w region once).  A lane owns one COLUMN PAIR
// (x[.., 2c], x[.., 2c+1]: one 8-byte load per row) and walks down RP row pairs, so
//   * the horizontal lifting steps take their neighbours d1[c+1], s1[c-1] from the adjacent lanes with wave shuffles — the
//     64 lanes of a wave cover 62 column pairs plus one halo lane on either side (periodic wrap = index mod), no LDS;
//   * the vertical lifting steps take their neighbours from the lane's own registers (row pairs r-1 .. r+RP, again with the
//     two halo pairs wrapped), so each lane produces the four sub-band values of its column pair for RP row pairs.
// Loads are 8 bytes per lane (512 contiguous bytes per wave and row), stores 4 bytes per lane per sub-band (forward) /
// 8 bytes per lane per row (inverse).
#include "common.h"

namespace {
constexpr float R3 = 1.7320508075688772f;
constexpr float LA = 0.4330127018922193f;     // sqrt3 / 4
constexpr float LB = -0.0669872981077807f;    // (sqrt3 - 2) / 4
constexpr float C1 = 1.9318516525781366f;     // (sqrt3 + 1) / sqrt2
constexpr float C2 = 0.5176380902050415f;     // (sqrt3 - 1) / sqrt2
constexpr float IS2 = 0.7071067811865476f;    // 1 / sqrt2
constexpr int RP = 16;                        // row pairs per wave (plus one halo pair on either side)

struct DwtArgs {
  const float* src;     // forward: the level's input region; inverse: the LL band of the level
  long long src_plane;  // plane stride (floats)
  int src_pitch;
  float* ll;            // forward: where LL goes (next level's input, or the coefficient buffer); inverse: the output region
  long long ll_plane;
  int ll_pitch;
  float* coef;          // coefficient buffer [planes][H][W] (details are written to / read from its quadrants)
  long long coef_plane;
  int coef_pitch;
  int h, w;             // size of the region this level works on (input of the forward level / output of the inverse level)
};

// 1-D forward lifting on (e, o) with neighbours: d1 of the right neighbour, and for s1[n-1] the left neighbour's values.
template <int WV>
__device__ __forceinline__ void fwd_pair_h(float e, float o, float& s, float& d) {   // horizontal: neighbours via shuffles
  if (WV == 0) {
    s = (e + o) * IS2;
    d = (o - e) * IS2;
  } else {
    const float d1 = o - R3 * e;
    const float d1n = __shfl_down(d1, 1, 64);
    const float s1 = e + LA * d1 + LB * d1n;
    const float s1p = __shfl_up(s1, 1, 64);
    s = C1 * s1;
    d = C2 * (d1 + s1p);
  }
}
}  // namespace

template <int WV>
__global__ __launch_bounds__(256) void dwt2_fwd_k(DwtArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int npairs = a.w / 2, nrp = a.h / 2;
  const int c = blockIdx.x * 62 + lane - 1;                       // column pair (lanes 0 and 63 are halo lanes)
  const int cw = ((c % npairs) + npairs) % npairs;                // periodic
  const int r0 = (blockIdx.y * 4 + wave) * RP;
  const float* src = a.src + (size_t)blockIdx.z * a.src_plane;
  // horizontal pass on rows of the pairs r0-1 .. r0+RP
  float sE[RP + 2], dE[RP + 2], sO[RP + 2], dO[RP + 2];
#pragma unroll
  for (int k = 0; k < RP + 2; ++k) {
    const int rp = (((r0 - 1 + k) % nrp) + nrp) % nrp;
    const float2 re = *reinterpret_cast<const float2*>(src + (size_t)(2 * rp) * a.src_pitch + 2 * cw);
    const float2 ro = *reinterpret_cast<const float2*>(src + (size_t)(2 * rp + 1) * a.src_pitch + 2 * cw);
    fwd_pair_h<WV>(re.x, re.y, sE[k], dE[k]);
    fwd_pair_h<WV>(ro.x, ro.y, sO[k], dO[k]);
  }
  // vertical pass (neighbours in registers) and stores
  const bool col_ok = lane >= 1 && lane <= 62 && c < npairs;
  const int h2 = a.h / 2, w2 = a.w / 2;
  float* ll = a.ll + (size_t)blockIdx.z * a.ll_plane;
  float* cf = a.coef + (size_t)blockIdx.z * a.coef_plane;
  float d1s[RP + 2], d1d[RP + 2], s1s[RP + 2], s1d[RP + 2];
  if (WV == 1) {
#pragma unroll
    for (int k = 0; k < RP + 2; ++k) {
      d1s[k] = sO[k] - R3 * sE[k];
      d1d[k] = dO[k] - R3 * dE[k];
    }
#pragma unroll
    for (int k = 0; k < RP + 1; ++k) {
      s1s[k] = sE[k] + LA * d1s[k] + LB * d1s[k + 1];
      s1d[k] = dE[k] + LA * d1d[k] + LB * d1d[k + 1];
    }
  }
#pragma unroll
  for (int k = 1; k <= RP; ++k) {
    const int rp = r0 + k - 1;
    float vll, vlh, vhl, vhh;   // (horizontal band)(vertical band): ll, l-h = low horizontal/high vertical, ...
    if (WV == 0) {
      vll = (sE[k] + sO[k]) * IS2; vlh = (sO[k] - sE[k]) * IS2;
      vhl = (dE[k] + dO[k]) * IS2; vhh = (dO[k] - dE[k]) * IS2;
    } else {
      vll = C1 * s1s[k]; vlh = C2 * (d1s[k] + s1s[k - 1]);
      vhl = C1 * s1d[k]; vhh = C2 * (d1d[k] + s1d[k - 1]);
    }
    if (col_ok && rp < nrp) {
      ll[(size_t)rp * a.ll_pitch + c] = vll;
      cf[(size_t)rp * a.coef_pitch + w2 + c] = vhl;                 // top-right: high horizontal, low vertical
      cf[(size_t)(h2 + rp) * a.coef_pitch + c] = vlh;               // bottom-left: low horizontal, high vertical
      cf[(size_t)(h2 + rp) * a.coef_pitch + w2 + c] = vhh;
    }
  }
}

template <int WV>
__global__ __launch_bounds__(256) void dwt2_inv_k(DwtArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int npairs = a.w / 2, nrp = a.h / 2;
  const int c = blockIdx.x * 62 + lane - 1;
  const int cw = ((c % npairs) + npairs) % npairs;
  const int r0 = (blockIdx.y * 4 + wave) * RP;
  const int h2 = a.h / 2, w2 = a.w / 2;
  const float* llp = a.src + (size_t)blockIdx.z * a.src_plane;
  const float* cf = a.coef + (size_t)blockIdx.z * a.coef_plane;
  float vll[RP + 2], vlh[RP + 2], vhl[RP + 2], vhh[RP + 2];
#pragma unroll
  for (int k = 0; k < RP + 2; ++k) {
    const int rp = (((r0 - 1 + k) % nrp) + nrp) % nrp;
    vll[k] = llp[(size_t)rp * a.src_pitch + cw];
    vhl[k] = cf[(size_t)rp * a.coef_pitch + w2 + cw];
    vlh[k] = cf[(size_t)(h2 + rp) * a.coef_pitch + cw];
    vhh[k] = cf[(size_t)(h2 + rp) * a.coef_pitch + w2 + cw];
  }
  float* out = a.ll + (size_t)blockIdx.z * a.ll_plane;
  const bool col_ok = lane >= 1 && lane <= 62 && c < npairs;
#pragma unroll
  for (int k = 1; k <= RP; ++k) {
    const int rp = r0 + k - 1;
    // vertical inverse: (ll, lh) -> (sE, sO) of the low horizontal band, (hl, hh) -> (dE, dO) of the high one
    float sE, sO, dE, dO;
    if (WV == 0) {
      sE = (vll[k] - vlh[k]) * IS2; sO = (vll[k] + vlh[k]) * IS2;
      dE = (vhl[k] - vhh[k]) * IS2; dO = (vhl[k] + vhh[k]) * IS2;
    } else {
      const float i1 = 1.f / C1, i2 = 1.f / C2;
      {
        const float s1 = vll[k] * i1, s1p = vll[k - 1] * i1;
        const float d1 = vlh[k] * i2 - s1p, d1n = vlh[k + 1] * i2 - s1;
        sE = s1 - LA * d1 - LB * d1n;
        sO = d1 + R3 * sE;
      }
      {
        const float s1 = vhl[k] * i1, s1p = vhl[k - 1] * i1;
        const float d1 = vhh[k] * i2 - s1p, d1n = vhh[k + 1] * i2 - s1;
        dE = s1 - LA * d1 - LB * d1n;
        dO = d1 + R3 * dE;
      }
    }
    // horizontal inverse of the two rows (neighbours: s1 of the left lane, d2 of the right lane)
    float2 re, ro;
    if (WV == 0) {
      re.x = (sE - dE) * IS2; re.y = (sE + dE) * IS2;
      ro.x = (sO - dO) * IS2; ro.y = (sO + dO) * IS2;
    } else {
      const float i1 = 1.f / C1, i2 = 1.f / C2;
      {
        const float s1 = sE * i1, d2 = dE * i2;
        const float d1 = d2 - __shfl_up(s1, 1, 64);
        const float d1n = __shfl_down(d2, 1, 64) - s1;
        re.x = s1 - LA * d1 - LB * d1n;
        re.y = d1 + R3 * re.x;
      }
      {
        const float s1 = sO * i1, d2 = dO * i2;
        const float d1 = d2 - __shfl_up(s1, 1, 64);
        const float d1n = __shfl_down(d2, 1, 64) - s1;
        ro.x = s1 - LA * d1 - LB * d1n;
        ro.y = d1 + R3 * ro.x;
      }
    }
    if (col_ok && rp < nrp) {
      *reinterpret_cast<float2*>(out + (size_t)(2 * rp) * a.ll_pitch + 2 * c) = re;
      *reinterpret_cast<float2*>(out + (size_t)(2 * rp + 1) * a.ll_pitch + 2 * c) = ro;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// Streaming / fused analysis (round 3), for square planes 256 or 512 wide.  A wave owns WHOLE rows of a plane (64 lanes x
// 2 * NPL pixels: one or two 16-byte loads per lane and row, 1-2 KB contiguous per wave), so
//   * the horizontal lifting steps get their neighbours by a lane ROTATION (ds_bpermute, (lane +- 1) & 63): the periodic
//     extension is the rotation itself — no halo lanes, every load and store a full aligned line;
//   * the vertical lifting steps run as a rolling recurrence down the rows (three registers of state per column: e[k-1],
//     d1[k-1], s1[k-2]): a row pair is read once, apart from the one pair on either side of a wave's row segment;
//   * sub-band stores are 8 / 16 bytes per lane, 512 B - 1 KB contiguous per wave.
// KEEP: the four waves of a workgroup cover one whole plane whose LL band (<= 128 x 128) stays in LDS; the remaining levels
// run there (per output pair a 6 x 6 neighbourhood straight from LDS) and only detail coefficients and the last LL go to
// memory: a 3-level transform of a 256 x 256 plane reads the plane once and writes the coefficients once.
template <int WV>
__device__ __forceinline__ void lift3(float e0, float o0, float e1, float o1, float e2, float o2, float& lo, float& hi) {
  // 1-D forward lifting at position k from the pairs k-1, k, k+1
  if (WV == 0) {
    lo = (e1 + o1) * IS2;
    hi = (o1 - e1) * IS2;
  } else {
    const float d0 = o0 - R3 * e0, d1 = o1 - R3 * e1, d2 = o2 - R3 * e2;
    const float s0 = e0 + LA * d0 + LB * d1;
    const float s1 = e1 + LA * d1 + LB * d2;
    lo = C1 * s1;
    hi = C2 * (d1 + s0);
  }
}

struct DwtFArgs {
  const float* src;      // [planes][h][w] region (pitch / plane stride below)
  long long src_plane;
  int src_pitch;
  float* ll;             // !KEEP: where this level's LL goes
  long long ll_plane;
  int ll_pitch;
  float* coef;           // [planes][H][W] Mallat buffer
  long long coef_plane;
  int coef_pitch;
  int h, w;              // the streamed level's region (w = 128 * NPL)
  int nrest;             // KEEP: levels still to do in LDS after the streamed one
};

template <int WV, int NPL, bool KEEP>
__global__ __launch_bounds__(256) void dwt2_stream_k(DwtFArgs a) {
  constexpr int NC = 2 * NPL;                              // horizontal outputs per lane and row: NPL low + NPL high
  constexpr int P = NPL >= 4 ? 2 : 4;                      // row pairs per prefetch chunk
  typedef float vecN __attribute__((ext_vector_type(NPL)));
  extern __shared__ float lds[];                           // KEEP: LL plane [h/2][w/2], then a ping-pong buffer
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nrp = a.h / 2, w2 = a.w / 2, h2 = a.h / 2;
  const int plane = blockIdx.z;
  // row segment of this wave
  const int RS = KEEP ? nrp / 4 : 32;
  const int rp0 = (KEEP ? wave : (int)blockIdx.y * 4 + wave) * RS;
  const float* src = a.src + (size_t)plane * a.src_plane + 2 * NPL * lane;
  float* cf = a.coef + (size_t)plane * a.coef_plane;
  const int up = ((lane + 1) & 63) * 4, dn = ((lane - 1) & 63) * 4;

  // horizontal lifting of one row held as NPL pairs per lane -> lo[NPL], hi[NPL]
  auto hrow = [&](const float (&x)[2 * NPL], float (&lo)[NPL], float (&hi)[NPL]) {
    if (WV == 0) {
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        lo[i] = (x[2 * i] + x[2 * i + 1]) * IS2;
        hi[i] = (x[2 * i + 1] - x[2 * i]) * IS2;
      }
    } else {
      float d1[NPL + 1], s1[NPL + 1];                      // d1[NPL] = right neighbour's first, s1[0] = left neighbour's last
#pragma unroll
      for (int i = 0; i < NPL; ++i) d1[i] = x[2 * i + 1] - R3 * x[2 * i];
      d1[NPL] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(up, __builtin_bit_cast(int, d1[0])));
#pragma unroll
      for (int i = 0; i < NPL; ++i) s1[i + 1] = x[2 * i] + LA * d1[i] + LB * d1[i + 1];
      s1[0] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(dn, __builtin_bit_cast(int, s1[NPL])));
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        lo[i] = C1 * s1[i + 1];
        hi[i] = C2 * (d1[i] + s1[i]);
      }
    }
  };

  // rolling vertical state per column (NPL low + NPL high columns)
  float Ep[NC], D1p[NC], S1pp[NC];
#pragma unroll
  for (int q = 0; q < NC; ++q) Ep[q] = D1p[q] = S1pp[q] = 0.f;

  const int k_first = WV == 0 ? rp0 : rp0 - 1;             // db2: one row pair of lead-in, one of lead-out
  const int niter = WV == 0 ? RS : RS + 2;
  const int nchunk = (niter + P - 1) / P;
  float raw[2][P][2][2 * NPL];
  auto load_chunk = [&](int c, int buf) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      int kk = k_first + c * P + j;
      kk = ((kk % nrp) + nrp) % nrp;                       // periodic (also clamps the padding iterations of the last chunk)
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const float* row = src + (size_t)(2 * kk + r) * a.src_pitch;
#pragma unroll
        for (int v = 0; v < (2 * NPL) / 4; ++v) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(row + 4 * v);
          raw[buf][j][r][4 * v] = t[0]; raw[buf][j][r][4 * v + 1] = t[1]; raw[buf][j][r][4 * v + 2] = t[2]; raw[buf][j][r][4 * v + 3] = t[3];
        }
      }
    }
  };
  auto emit = [&](int rp, const float (&L)[NC], const float (&Hh)[NC]) {
    // columns q < NPL: the low horizontal band (LL, LH); q >= NPL: the high one (HL, HH)
    vecN vll, vlh, vhl, vhh;
#pragma unroll
    for (int i = 0; i < NPL; ++i) { vll[i] = L[i]; vlh[i] = Hh[i]; vhl[i] = L[NPL + i]; vhh[i] = Hh[NPL + i]; }
    const int c = NPL * lane;
    if (KEEP) *reinterpret_cast<vecN*>(lds + (size_t)rp * w2 + c) = vll;
    else *reinterpret_cast<vecN*>(a.ll + (size_t)plane * a.ll_plane + (size_t)rp * a.ll_pitch + c) = vll;
    *reinterpret_cast<vecN*>(cf + (size_t)rp * a.coef_pitch + w2 + c) = vhl;
    *reinterpret_cast<vecN*>(cf + (size_t)(h2 + rp) * a.coef_pitch + c) = vlh;
    *reinterpret_cast<vecN*>(cf + (size_t)(h2 + rp) * a.coef_pitch + w2 + c) = vhh;
  };
  auto do_chunk = [&](int c, int buf) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int it = c * P + j;
      float eLo[NPL], eHi[NPL], oLo[NPL], oHi[NPL];
      hrow(raw[buf][j][0], eLo, eHi);
      hrow(raw[buf][j][1], oLo, oHi);
      float L[NC], Hh[NC];
#pragma unroll
      for (int q = 0; q < NC; ++q) {
        const float E = q < NPL ? eLo[q % NPL] : eHi[q % NPL], O = q < NPL ? oLo[q % NPL] : oHi[q % NPL];
        if (WV == 0) {
          L[q] = (E + O) * IS2;
          Hh[q] = (O - E) * IS2;
        } else {
          const float D1 = O - R3 * E;
          const float S1p = Ep[q] + LA * D1p[q] + LB * D1;
          L[q] = C1 * S1p;
          Hh[q] = C2 * (D1p[q] + S1pp[q]);
          Ep[q] = E; D1p[q] = D1; S1pp[q] = S1p;
        }
      }
      // haar: iteration `it` is row pair rp0 + it; db2: the recurrence delivers row pair rp0 + it - 2
      const int rp = WV == 0 ? rp0 + it : rp0 + it - 2;
      if (it < niter && rp >= rp0) emit(rp, L, Hh);
    }
  };
  load_chunk(0, 0);
  for (int c = 0; c < nchunk; c += 2) {
    if (c + 1 < nchunk) load_chunk(c + 1, 1);
    do_chunk(c, 0);
    if (c + 1 < nchunk) {
      if (c + 2 < nchunk) load_chunk(c + 2, 0);
      do_chunk(c + 1, 1);
    }
  }

  if constexpr (KEEP) {
    // ---- remaining levels in LDS: in = [hh][ww] at `cur`, LL out to `nxt`
    float* cur = lds;
    float* nxt = lds + (size_t)h2 * w2;
    int hh = h2, ww = w2;
    int coff = 0;                                        // nothing: detail quadrants are addressed from the region size
    (void)coff;
    for (int lv = 0; lv < a.nrest; ++lv) {
      __syncthreads();
      const int hp = hh / 2, wp = ww / 2;
      // (wp, hp are powers of two here: shifts and conditional wraps, no integer division in the loop)
      const int wsh = __builtin_ctz(wp);
      for (int e = threadIdx.x; e < hp * wp; e += 256) {
        const int rp = e >> wsh, cp = e & (wp - 1);
        const int c0 = (cp == 0 ? wp - 1 : cp - 1) * 2, c1 = cp * 2, c2 = (cp == wp - 1 ? 0 : cp + 1) * 2;
        // horizontal lifting of the six rows 2(rp-1) .. 2(rp+1)+1 at column pair cp, then vertical lifting of both bands
        float lo[6], hi[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          if (WV == 0 && (r < 2 || r > 3)) { lo[r] = hi[r] = 0.f; continue; }
          int row = 2 * rp - 2 + r;
          row = row < 0 ? row + hh : (row >= hh ? row - hh : row);
          const float* p = cur + (size_t)row * ww;
          lift3<WV>(p[c0], p[c0 + 1], p[c1], p[c1 + 1], p[c2], p[c2 + 1], lo[r], hi[r]);
        }
        float vll, vlh, vhl, vhh;
        lift3<WV>(lo[0], lo[1], lo[2], lo[3], lo[4], lo[5], vll, vlh);
        lift3<WV>(hi[0], hi[1], hi[2], hi[3], hi[4], hi[5], vhl, vhh);
        nxt[(size_t)rp * wp + cp] = vll;
        cf[(size_t)rp * a.coef_pitch + wp + cp] = vhl;
        cf[(size_t)(hp + rp) * a.coef_pitch + cp] = vlh;
        cf[(size_t)(hp + rp) * a.coef_pitch + wp + cp] = vhh;
      }
      float* t = cur; cur = nxt; nxt = t;
      hh = hp; ww = wp;
    }
    __syncthreads();
    const int fsh = __builtin_ctz(ww);
    for (int e = threadIdx.x; e < hh * ww; e += 256) {
      const int r = e >> fsh, c = e & (ww - 1);
      cf[(size_t)r * a.coef_pitch + c] = cur[(size_t)r * ww + c];
    }
  }
}

template <int WV>
static void dwt_stream_launch(DwtFArgs a, int planes, bool keep, hipStream_t st) {
  if (keep) {
    const size_t lds = ((size_t)(a.h / 2) * (a.w / 2) + (size_t)(a.h / 4) * (a.w / 4)) * sizeof(float);   // 80 KB at 256 x 256
    static const hipError_t once = hipFuncSetAttribute(reinterpret_cast<const void*>(&dwt2_stream_k<WV, 2, true>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    (void)once;
    hipLaunchKernelGGL((dwt2_stream_k<WV, 2, true>), dim3(1, 1, (unsigned)planes), dim3(256), lds, st, a);
  } else {
    // streaming to memory happens for the first level of a 512-wide plane only (dwt_fwd_fast): 8 pixels per lane.  A 256-wide
    // plane always keeps its LL band in LDS, so there is no <WV, 2, false> instance: nothing could reach or test it.
    dim3 grid(1, (unsigned)((a.h / 2) / 128), (unsigned)planes);
    hipLaunchKernelGGL((dwt2_stream_k<WV, 4, false>), grid, dim3(256), 0, st, a);
  }
}

// square planes of 256 or 512 pixels: the streaming / fused path
static bool dwt_fast_shape(int H, int W, int levels) { return H == W && (W == 256 || W == 512) && levels <= (W == 256 ? 7 : 8); }

template <int WV>
static void dwt_fwd_fast(const float* x, float* coef, float* tmp, int planes, int H, int W, int levels, hipStream_t st) {
  DwtFArgs a;
  a.coef = coef; a.coef_plane = (long long)H * W; a.coef_pitch = W;
  if (W == 512) {
    // level 1 streams to `tmp` (its LL plane is 256 x 256: too big for LDS), the rest as for a 256-wide input
    a.src = x; a.src_plane = (long long)H * W; a.src_pitch = W; a.h = H; a.w = W; a.nrest = 0;
    if (levels == 1) { a.ll = coef; a.ll_plane = (long long)H * W; a.ll_pitch = W; }
    else { a.ll = tmp; a.ll_plane = (long long)(H / 2) * (W / 2); a.ll_pitch = W / 2; }
    dwt_stream_launch<WV>(a, planes, false, st);
    if (levels == 1) return;
    a.src = tmp; a.src_plane = (long long)(H / 2) * (W / 2); a.src_pitch = W / 2; a.h = H / 2; a.w = W / 2; a.nrest = levels - 2;
    a.ll = nullptr; a.ll_plane = 0; a.ll_pitch = 0;
    dwt_stream_launch<WV>(a, planes, true, st);
    return;
  }
  a.src = x; a.src_plane = (long long)H * W; a.src_pitch = W; a.h = H; a.w = W; a.nrest = levels - 1;
  a.ll = nullptr; a.ll_plane = 0; a.ll_pitch = 0;
  dwt_stream_launch<WV>(a, planes, true, st);
}

static dim3 dwt_grid(int h, int w, int planes) {
  return dim3((unsigned)ceil_div(w / 2, 62), (unsigned)ceil_div(h / 2, 4 * RP), (unsigned)planes);
}

// See include/wtpse_hip.h.  tmp: 2 * planes * (H/2) * (W/2) floats.
extern "C" int wtpse_dwt2_fwd(const float* x, float* coef, float* tmp, int planes, int H, int W, int wavelet, int levels,
                              void* stream) {
  WTPSE_REQUIRE(x && coef && tmp && planes > 0 && planes <= 65535 && H > 0 && W > 0 && levels >= 1 && levels <= 12);
  WTPSE_REQUIRE((wavelet == 0 || wavelet == 1) && H % (1 << levels) == 0 && W % (1 << levels) == 0 && x != coef);
  WTPSE_REQUIRE((((uintptr_t)x | (uintptr_t)coef | (uintptr_t)tmp) & 7) == 0);   // the generic kernels load and store float2
  hipStream_t st = (hipStream_t)stream;
  if (dwt_fast_shape(H, W, levels) && (((uintptr_t)x | (uintptr_t)coef | (uintptr_t)tmp) & 15) == 0) {
    if (wavelet == 0) dwt_fwd_fast<0>(x, coef, tmp, planes, H, W, levels, st);
    else dwt_fwd_fast<1>(x, coef, tmp, planes, H, W, levels, st);
    return wtpse_status();
  }
  const long long tplane = (long long)(H / 2) * (W / 2);
  float* tbuf[2] = {tmp, tmp + (size_t)planes * tplane};
  DwtArgs a;
  a.coef = coef; a.coef_plane = (long long)H * W; a.coef_pitch = W;
  int h = H, w = W;
  for (int lv = 0; lv < levels; ++lv) {
    const bool last = lv == levels - 1;
    if (lv == 0) { a.src = x; a.src_plane = (long long)H * W; a.src_pitch = W; }
    else { a.src = tbuf[(lv - 1) & 1]; a.src_plane = tplane; a.src_pitch = w; }
    if (last) { a.ll = coef; a.ll_plane = (long long)H * W; a.ll_pitch = W; }
    else { a.ll = tbuf[lv & 1]; a.ll_plane = tplane; a.ll_pitch = w / 2; }
    a.h = h; a.w = w;
    if (wavelet == 0) hipLaunchKernelGGL(dwt2_fwd_k<0>, dwt_grid(h, w, planes), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(dwt2_fwd_k<1>, dwt_grid(h, w, planes), dim3(256), 0, st, a);
    h /= 2; w /= 2;
  }
  return wtpse_status();
}

extern "C" int wtpse_dwt2_inv(const float* coef, float* x, float* tmp, int planes, int H, int W, int wavelet, int levels,
                              void* stream) {
  WTPSE_REQUIRE(x && coef && tmp && planes > 0 && planes <= 65535 && H > 0 && W > 0 && levels >= 1 && levels <= 12);
  WTPSE_REQUIRE((wavelet == 0 || wavelet == 1) && H % (1 << levels) == 0 && W % (1 << levels) == 0 && x != coef);
  WTPSE_REQUIRE((((uintptr_t)x | (uintptr_t)coef | (uintptr_t)tmp) & 7) == 0);
  hipStream_t st = (hipStream_t)stream;
  const long long tplane = (long long)(H / 2) * (W / 2);
  float* tbuf[2] = {tmp, tmp + (size_t)planes * tplane};
  DwtArgs a;
  a.coef = const_cast<float*>(coef); a.coef_plane = (long long)H * W; a.coef_pitch = W;
  for (int lv = levels - 1; lv >= 0; --lv) {
    const int h = H >> lv, w = W >> lv;            // output region of this level
    if (lv == levels - 1) { a.src = coef; a.src_plane = (long long)H * W; a.src_pitch = W; }
    else { a.src = tbuf[(lv + 1) & 1]; a.src_plane = tplane; a.src_pitch = w / 2; }
    if (lv == 0) { a.ll = x; a.ll_plane = (long long)H * W; a.ll_pitch = W; }
    else { a.ll = tbuf[lv & 1]; a.ll_plane = tplane; a.ll_pitch = w; }
    a.h = h; a.w = w;
    if (wavelet == 0) hipLaunchKernelGGL(dwt2_inv_k<0>, dwt_grid(h, w, planes), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(dwt2_inv_k<1>, dwt_grid(h, w, planes), dim3(256), 0, st, a);
  }
  return wtpse_status();
}
