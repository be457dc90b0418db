// Amplitude mixing between source domains: the optional Fourier-space stage of the input pipeline between the augmentations (or
// the crop) and input_finish_k (pipeline.hip).  A row of the uint8 batch keeps the phase of its 2-D spectrum and moves its amplitude
// towards that of a partner row inside the low-frequency window |k_y| <= b, |k_x| <= b (input_pipeline.amplitude_mix_host is the
// float64 specification):
//     D = lam (|G| - |F|) F / |F| inside the window, 0 outside;   y = x + real(ifft2(D))
// written as a correction to x: whatever lies outside the window never goes through a transform, and lam = 0 or partner = self
// give D = 0 exactly, so the input comes back bit for bit.  Three passes, no atomics (the result is the same on every run):
//   amix_rows_k   : two real rows (y, y + 1) of one channel ride through ONE complex transform as re + i im; the half spectra
//                   of both are separated afterwards and only the columns u <= b are kept, stored [n][c][u][y] so that the
//                   next pass reads a column contiguously
//   amix_cols_k   : per (n, c, u <= b) of a row that has a partner: the column transform of own and partner, D for the rows of the
//                   window (scaled by 1 / S^2), the inverse column transform of D -> corr [n][c][y][u]
//   amix_finish_k : the inverse real row transform of the b + 1 correction columns — again two rows per complex transform,
//                   Hermitian-extended — added to the uint8 input, clipped, rounded half-even; rows without a partner are copied
// The transforms are radix-4 Stockham autosort passes in LDS (one radix-2 pass at the end for 32, 128 and 512), S / 4 threads
// per transform, 1024 / S transforms side by side in a 256-thread workgroup, ping-pong between two padded LDS arrays per
// transform.  fp32 throughout; the twiddles come from a table the host computed in float64 and rounded once.  Contraction is
// off: every multiply-add that is fused is written as fmaf, so own and partner of a row mixed with itself see the same
// operations and cancel exactly.
//
// Every phase between two barriers is a __host__ __device__ function of (workgroup, thread): a host program can run a
// workgroup phase by phase over its 256 threads.
#include "common.h"

#pragma clang fp contract(off)

#define AMIX_HD __host__ __device__ __forceinline__

template <int S>
struct AmixGeo {
  static constexpr int TG = S / 4;          // threads per transform: one radix-4 butterfly each
  static constexpr int NG = 256 / TG;       // transforms (of each of a phase's arrays) side by side in a workgroup
  static constexpr int PS = S + S / 32;     // padded length of one LDS array
};

// Complex fp32 at power-of-two strides would land on one bank: re and im live in separate float arrays, and one float of padding
// follows every 32 (a stride-4 butterfly store of 32 lanes then covers the 32 banks once).
AMIX_HD int amix_pad(int i) { return i + (i >> 5); }

struct AmixLds {
  float* re;      // [NG][KS][2][PS]
  float* im;
  float* twr;     // [S]: cos(2 pi t / S)
  float* twi;     // [S]: -sin(2 pi t / S)
};

template <int S, int KS>
AMIX_HD int amix_base(int g, int k, int p) { return ((g * KS + k) * 2 + p) * AmixGeo<S>::PS; }

AMIX_HD void amix_cmul(float& xr, float& xi, float wr, float wi) {
  const float r = fmaf(xr, wr, -(xi * wi)), i = fmaf(xr, wi, xi * wr);
  xr = r; xi = i;
}

// One radix-4 pass (sub-transform length Ns -> 4 Ns) of thread j (0 .. S/4 - 1) of group g over arrays 0 .. K - 1, from buffer p to
// buffer p ^ 1:  v[r] = in[j + r S/4] W^(r k S / (4 Ns)), k = j mod Ns;  out[(j - k) 4 + k + r Ns] = DFT4(v)[r].
template <int S, int KS, int K, bool INV>
AMIX_HD void amix_pass4(const AmixLds& L, int g, int j, int Ns, int p) {
  constexpr int Q = S / 4;
  const int k = j & (Ns - 1), m = S / (Ns * 4);
  float w1r = 1.f, w1i = 0.f, w2r = 1.f, w2i = 0.f, w3r = 1.f, w3i = 0.f;
  if (Ns > 1) {
    w1r = L.twr[k * m]; w1i = L.twi[k * m];
    w2r = L.twr[2 * k * m]; w2i = L.twi[2 * k * m];
    w3r = L.twr[3 * k * m]; w3i = L.twi[3 * k * m];
    if (INV) { w1i = -w1i; w2i = -w2i; w3i = -w3i; }
  }
  const int o = ((j - k) << 2) + k;
#pragma unroll
  for (int a = 0; a < K; ++a) {
    const int s = amix_base<S, KS>(g, a, p), d = amix_base<S, KS>(g, a, p ^ 1);
    float v0r = L.re[s + amix_pad(j)], v0i = L.im[s + amix_pad(j)];
    float v1r = L.re[s + amix_pad(j + Q)], v1i = L.im[s + amix_pad(j + Q)];
    float v2r = L.re[s + amix_pad(j + 2 * Q)], v2i = L.im[s + amix_pad(j + 2 * Q)];
    float v3r = L.re[s + amix_pad(j + 3 * Q)], v3i = L.im[s + amix_pad(j + 3 * Q)];
    if (Ns > 1) {
      amix_cmul(v1r, v1i, w1r, w1i);
      amix_cmul(v2r, v2i, w2r, w2i);
      amix_cmul(v3r, v3i, w3r, w3i);
    }
    const float t0r = v0r + v2r, t0i = v0i + v2i, t1r = v0r - v2r, t1i = v0i - v2i;
    const float t2r = v1r + v3r, t2i = v1i + v3i, t3r = v1r - v3r, t3i = v1i - v3i;
    // forward: out1 = t1 - i t3, out3 = t1 + i t3; the inverse swaps them
    const float ar = t1r + t3i, ai = t1i - t3r, br = t1r - t3i, bi = t1i + t3r;
    L.re[d + amix_pad(o)] = t0r + t2r;           L.im[d + amix_pad(o)] = t0i + t2i;
    L.re[d + amix_pad(o + Ns)] = INV ? br : ar;  L.im[d + amix_pad(o + Ns)] = INV ? bi : ai;
    L.re[d + amix_pad(o + 2 * Ns)] = t0r - t2r;  L.im[d + amix_pad(o + 2 * Ns)] = t0i - t2i;
    L.re[d + amix_pad(o + 3 * Ns)] = INV ? ar : br;  L.im[d + amix_pad(o + 3 * Ns)] = INV ? ai : bi;
  }
}

// The closing radix-2 pass (Ns = S / 2) of sizes 2 * 4^n: thread j takes the butterflies j and j + S/4.
template <int S, int KS, int K, bool INV>
AMIX_HD void amix_pass2(const AmixLds& L, int g, int j, int p) {
  constexpr int Q = S / 4, H = S / 2;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int jj = j + h * Q;
    const float wr = L.twr[jj], wi = INV ? -L.twi[jj] : L.twi[jj];
#pragma unroll
    for (int a = 0; a < K; ++a) {
      const int s = amix_base<S, KS>(g, a, p), d = amix_base<S, KS>(g, a, p ^ 1);
      const float xr = L.re[s + amix_pad(jj)], xi = L.im[s + amix_pad(jj)];
      float yr = L.re[s + amix_pad(jj + H)], yi = L.im[s + amix_pad(jj + H)];
      amix_cmul(yr, yi, wr, wi);
      L.re[d + amix_pad(jj)] = xr + yr;      L.im[d + amix_pad(jj)] = xi + yi;
      L.re[d + amix_pad(jj + H)] = xr - yr;  L.im[d + amix_pad(jj + H)] = xi - yi;
    }
  }
}

// passes of a transform of length S; the result of a transform that starts in buffer 0 lies in buffer (passes & 1)
template <int S>
struct AmixPasses {
  static constexpr int R4 = S == 32 ? 2 : (S == 64 || S == 128) ? 3 : 4;
  static constexpr bool R2 = S == 32 || S == 128 || S == 512;
  static constexpr int OUT = (R4 + (R2 ? 1 : 0)) & 1;
};

// Whole transform, on the device: a barrier in front (the caller has just filled buffer 0) and one behind every pass.
template <int S, int KS, int K, bool INV>
__device__ __forceinline__ void amix_fft(const AmixLds& L, int g, int j) {
  int p = 0, Ns = 1;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < AmixPasses<S>::R4; ++q) {
    amix_pass4<S, KS, K, INV>(L, g, j, Ns, p);
    __syncthreads();
    p ^= 1;
    Ns *= 4;
  }
  if (AmixPasses<S>::R2) {
    amix_pass2<S, KS, K, INV>(L, g, j, p);
    __syncthreads();
  }
}

// The work of a launch, shared by its phases.
struct AmixArgs {
  const unsigned char* img;     // [N][S][S][3]
  const int* partner;           // [N]: -1 = no partner
  const float* lam;             // [N]
  const float* twiddle;         // [S][2] = (cos, -sin)(2 pi t / S)
  unsigned char* out_u8;        // [N][S][S][3]
  float* out_f32;               // [N][S][S][3] or null
  float* spec;                  // [N][3][b + 1][S][2]: half spectra of the rows, columns u <= b
  float* corr;                  // [N][3][S][b + 1][2]: column-transformed corrections
  int N, b;
};

template <int S>
AMIX_HD void amix_load_twiddle(const AmixArgs& A, const AmixLds& L, int tid) {
  for (int t = tid; t < S; t += 256) {
    L.twr[t] = A.twiddle[2 * t];
    L.twi[t] = A.twiddle[2 * t + 1];
  }
}

// a row's partner, or -1 for a row that is left alone (an index outside the batch counts as none)
AMIX_HD int amix_partner(const AmixArgs& A, int n) {
  const int p = A.partner[n];
  return (p >= 0 && p < A.N) ? p : -1;
}

// ------------------------------------------------------------------------------------------------ rows pass
// item = (n, row pair): rows y, y + 1 of the three channels -> three complex arrays (re = row y, im = row y + 1)
template <int S>
AMIX_HD void amix_rows_load(const AmixArgs& A, const AmixLds& L, int item, int g, int j) {
  constexpr int TG = AmixGeo<S>::TG;
  const bool valid = item < A.N * (S / 2);
  const int n = valid ? item / (S / 2) : 0, y = valid ? 2 * (item % (S / 2)) : 0;
  const unsigned char* r0 = A.img + ((size_t)n * S + y) * S * 3;
  const unsigned char* r1 = r0 + (size_t)S * 3;
  for (int e = j; e < 3 * S; e += TG) {
    const int x = e / 3, c = e - 3 * x;
    const int at = amix_base<S, 3>(g, c, 0) + amix_pad(x);
    L.re[at] = valid ? (float)r0[e] : 0.f;
    L.im[at] = valid ? (float)r1[e] : 0.f;
  }
}

// Z = FFT(row_a + i row_b): Fa(u) = (Z(u) + conj Z(-u)) / 2, Fb(u) = (Z(u) - conj Z(-u)) / 2i, kept for u <= b.
// The store is the transpose of the layout the columns pass wants: lanes run along u, and u is the SLOW index of spec
// [n][c][u][y], so a lane's 16 bytes (rows y, y + 1) lie 8 S bytes from its neighbour's — uncoalesced; only the 1024 / S row pairs of
// a workgroup are adjacent in y (64 contiguous bytes per u at S = 256).  At (b + 1) / S of the spectrum and 14 - 24 us per launch
// (profiles/amplitude_mix.md) this is left as it is; a workgroup that took 8 or more consecutive row pairs per transform slot and
// turned them through LDS would write whole 128-byte lines.
template <int S>
AMIX_HD void amix_rows_store(const AmixArgs& A, const AmixLds& L, int item, int g, int j) {
  constexpr int TG = AmixGeo<S>::TG, P = AmixPasses<S>::OUT;
  if (item >= A.N * (S / 2)) return;
  const int n = item / (S / 2), y = 2 * (item % (S / 2));
  for (int u = j; u <= A.b; u += TG) {
    const int um = (S - u) & (S - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int s = amix_base<S, 3>(g, c, P);
      const float zr = L.re[s + amix_pad(u)], zi = L.im[s + amix_pad(u)];
      const float mr = L.re[s + amix_pad(um)], mi = L.im[s + amix_pad(um)];
      float* dst = A.spec + ((((size_t)n * 3 + c) * (A.b + 1) + u) * S + y) * 2;
      dst[0] = 0.5f * (zr + mr);
      dst[1] = 0.5f * (zi - mi);
      dst[2] = 0.5f * (zi + mi);
      dst[3] = -0.5f * (zr - mr);
    }
  }
}

// ------------------------------------------------------------------------------------------------ columns pass
// item = (n, c, u <= b): array 0 = column u of the own half spectrum, array 1 = the partner's
template <int S>
AMIX_HD void amix_cols_load(const AmixArgs& A, const AmixLds& L, int item, int g, int j) {
  constexpr int TG = AmixGeo<S>::TG;
  const int per = 3 * (A.b + 1);
  const bool valid = item < A.N * per;
  const int n = valid ? item / per : 0, cu = valid ? item % per : 0;
  const int pn = valid ? amix_partner(A, n) : -1;
  const float* f = A.spec + ((size_t)n * per + cu) * S * 2;
  const float* q = A.spec + ((size_t)(pn < 0 ? 0 : pn) * per + cu) * S * 2;
  const int s0 = amix_base<S, 2>(g, 0, 0), s1 = amix_base<S, 2>(g, 1, 0);
  for (int i = j; i < S; i += TG) {
    L.re[s0 + amix_pad(i)] = pn >= 0 ? f[2 * i] : 0.f;
    L.im[s0 + amix_pad(i)] = pn >= 0 ? f[2 * i + 1] : 0.f;
    L.re[s1 + amix_pad(i)] = pn >= 0 ? q[2 * i] : 0.f;
    L.im[s1 + amix_pad(i)] = pn >= 0 ? q[2 * i + 1] : 0.f;
  }
}

// D over array 0, in place, in the buffer the forward transform left its result in; copied to buffer 0 of array 0 for the
// inverse transform when that is another one (every thread rewrites only the elements it read)
template <int S>
AMIX_HD void amix_cols_mix(const AmixArgs& A, const AmixLds& L, int item, int g, int j) {
  constexpr int TG = AmixGeo<S>::TG, P = AmixPasses<S>::OUT;
  const int per = 3 * (A.b + 1);
  const bool valid = item < A.N * per;
  const int n = valid ? item / per : 0;
  const float lam = (valid && amix_partner(A, n) >= 0) ? A.lam[n] : 0.f;
  const float inv = 1.f / ((float)S * (float)S);
  const int sf = amix_base<S, 2>(g, 0, P), sg = amix_base<S, 2>(g, 1, P), d = amix_base<S, 2>(g, 0, 0);
  for (int v = j; v < S; v += TG) {
    float dr = 0.f, di = 0.f;
    if (v <= A.b || v >= S - A.b) {
      const float fr = L.re[sf + amix_pad(v)], fi = L.im[sf + amix_pad(v)];
      const float gr = L.re[sg + amix_pad(v)], gi = L.im[sg + amix_pad(v)];
      const float af = sqrtf(fmaf(fr, fr, fi * fi)), ag = sqrtf(fmaf(gr, gr, gi * gi));
      // the specification's operations in its order: (lam (|G| - |F|)) * (F / |F|); a picture whose sums are exact in fp32 (b = 0,
      // lam = 1) then comes out exact
      const float w = lam * (ag - af);
      const float ur = af == 0.f ? 1.f : fr / af, ui = af == 0.f ? 0.f : fi / af;
      dr = w * ur * inv;
      di = w * ui * inv;
    }
    L.re[d + amix_pad(v)] = dr;
    L.im[d + amix_pad(v)] = di;
  }
}

template <int S>
AMIX_HD void amix_cols_store(const AmixArgs& A, const AmixLds& L, int item, int g, int j) {
  constexpr int TG = AmixGeo<S>::TG, P = AmixPasses<S>::OUT;
  const int per = 3 * (A.b + 1);
  if (item >= A.N * per) return;
  const int n = item / per, cu = item % per, c = cu / (A.b + 1), u = cu - c * (A.b + 1);
  if (amix_partner(A, n) < 0) return;
  const int s = amix_base<S, 2>(g, 0, P);
  float* dst = A.corr + (((size_t)n * 3 + c) * S * (A.b + 1) + u) * 2;
  for (int y = j; y < S; y += TG) {
    dst[(size_t)y * (A.b + 1) * 2] = L.re[s + amix_pad(y)];
    dst[(size_t)y * (A.b + 1) * 2 + 1] = L.im[s + amix_pad(y)];
  }
}

// ------------------------------------------------------------------------------------------------ finish pass
// item = (n, row pair).  Za, Zb: the correction columns of rows y, y + 1 (half spectra; their Hermitian extension is real in x):
// W = Za + i Zb over the whole circle -> the inverse transform holds row y in re and row y + 1 in im.
template <int S>
AMIX_HD void amix_finish_load(const AmixArgs& A, const AmixLds& L, int item, int g, int j) {
  constexpr int TG = AmixGeo<S>::TG;
  const bool valid = item < A.N * (S / 2);
  const int n = valid ? item / (S / 2) : 0, y = valid ? 2 * (item % (S / 2)) : 0;
  const bool active = valid && amix_partner(A, n) >= 0;
  const size_t line = (size_t)(A.b + 1) * 2;
  for (int i = j; i < S; i += TG) {
    const int u = i <= S / 2 ? i : S - i;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float wr = 0.f, wi = 0.f;
      if (active && u <= A.b) {
        const float* za = A.corr + (((size_t)n * 3 + c) * S + y) * line + (size_t)u * 2;
        const float* zb = za + line;
        if (u == 0 || u == S / 2) { wr = za[0]; wi = zb[0]; }                 // real by symmetry: the imaginary parts are rounding
        else if (i == u) { wr = za[0] - zb[1]; wi = za[1] + zb[0]; }
        else { wr = za[0] + zb[1]; wi = zb[0] - za[1]; }                      // conj(Za) + i conj(Zb)
      }
      const int at = amix_base<S, 3>(g, c, 0) + amix_pad(i);
      L.re[at] = wr;
      L.im[at] = wi;
    }
  }
}

AMIX_HD unsigned char amix_round_u8(float v) {
  v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
  return (unsigned char)rintf(v);                 // half to even, as numpy's rint
}

template <int S>
AMIX_HD void amix_finish_store(const AmixArgs& A, const AmixLds& L, int item, int g, int j) {
  constexpr int TG = AmixGeo<S>::TG, P = AmixPasses<S>::OUT;
  if (item >= A.N * (S / 2)) return;
  const int n = item / (S / 2), y = 2 * (item % (S / 2));
  const bool active = amix_partner(A, n) >= 0;
  const size_t row = ((size_t)n * S + y) * S * 3, next = (size_t)S * 3;
  for (int e = j; e < 3 * S; e += TG) {
    const int x = e / 3, c = e - 3 * x;
    const int at = amix_base<S, 3>(g, c, P) + amix_pad(x);
    const float v0 = (float)A.img[row + e] + (active ? L.re[at] : 0.f);
    const float v1 = (float)A.img[row + next + e] + (active ? L.im[at] : 0.f);
    A.out_u8[row + e] = amix_round_u8(v0);
    A.out_u8[row + next + e] = amix_round_u8(v1);
    if (A.out_f32) {
      A.out_f32[row + e] = v0;
      A.out_f32[row + next + e] = v1;
    }
  }
}

// ------------------------------------------------------------------------------------------------ kernels
template <int S, int KS>
struct AmixShared {
  static constexpr int FLOATS = AmixGeo<S>::NG * KS * 2 * AmixGeo<S>::PS;
};

#define AMIX_LDS(S, KS)                                             \
  __shared__ float lds_re[AmixShared<S, KS>::FLOATS];               \
  __shared__ float lds_im[AmixShared<S, KS>::FLOATS];               \
  __shared__ float lds_twr[S];                                      \
  __shared__ float lds_twi[S];                                      \
  const AmixLds L = {lds_re, lds_im, lds_twr, lds_twi};             \
  const int tid = threadIdx.x, g = tid / AmixGeo<S>::TG, j = tid % AmixGeo<S>::TG; \
  const int item = (int)blockIdx.x * AmixGeo<S>::NG + g

template <int S>
__global__ __launch_bounds__(256) void amix_rows_k(const AmixArgs A) {
  AMIX_LDS(S, 3);
  amix_load_twiddle<S>(A, L, tid);
  amix_rows_load<S>(A, L, item, g, j);
  amix_fft<S, 3, 3, false>(L, g, j);
  amix_rows_store<S>(A, L, item, g, j);
}

template <int S>
__global__ __launch_bounds__(256) void amix_cols_k(const AmixArgs A) {
  AMIX_LDS(S, 2);
  amix_load_twiddle<S>(A, L, tid);
  amix_cols_load<S>(A, L, item, g, j);
  amix_fft<S, 2, 2, false>(L, g, j);
  amix_cols_mix<S>(A, L, item, g, j);
  amix_fft<S, 2, 1, true>(L, g, j);
  amix_cols_store<S>(A, L, item, g, j);
}

template <int S>
__global__ __launch_bounds__(256) void amix_finish_k(const AmixArgs A) {
  AMIX_LDS(S, 3);
  amix_load_twiddle<S>(A, L, tid);
  amix_finish_load<S>(A, L, item, g, j);
  amix_fft<S, 3, 3, true>(L, g, j);
  amix_finish_store<S>(A, L, item, g, j);
}

// ================================================================================================ C ABI (include/wtpse_hip.h)
static bool amix_shape_ok(int N, int S, int b) {
  return N > 0 && N <= 65535 && (S == 32 || S == 64 || S == 128 || S == 256 || S == 512) && b >= 0 && b <= S / 2;
}

// floats of one of the two workspace halves: [N][3][b + 1][S] complex
static long long amix_half(int N, int S, int b) { return (long long)N * 3 * (b + 1) * S * 2; }

extern "C" int wtpse_amix_workspace(int N, int S, int b) {
  WTPSE_REQUIRE(amix_shape_ok(N, S, b));
  const long long floats = 2 * amix_half(N, S, b);
  WTPSE_REQUIRE(floats <= 0x7FFFFFFFLL);
  return (int)floats;
}

template <int S>
static void amix_launch(const AmixArgs& A, hipStream_t st) {
  constexpr int NG = AmixGeo<S>::NG;
  const unsigned pairs = (unsigned)(((long long)A.N * (S / 2) + NG - 1) / NG);
  const unsigned cols = (unsigned)(((long long)A.N * 3 * (A.b + 1) + NG - 1) / NG);
  hipLaunchKernelGGL(amix_rows_k<S>, dim3(pairs), dim3(256), 0, st, A);
  hipLaunchKernelGGL(amix_cols_k<S>, dim3(cols), dim3(256), 0, st, A);
  hipLaunchKernelGGL(amix_finish_k<S>, dim3(pairs), dim3(256), 0, st, A);
}

extern "C" int wtpse_amplitude_mix(const unsigned char* img, const int* partner, const float* lam, const float* twiddle,
                                   unsigned char* out_u8, float* out_f32, float* work, int N, int S, int b, void* stream) {
  WTPSE_REQUIRE(amix_shape_ok(N, S, b) && 2 * amix_half(N, S, b) <= 0x7FFFFFFFLL);
  WTPSE_REQUIRE(img && partner && lam && twiddle && out_u8 && work && img != out_u8 && ((uintptr_t)work & 15) == 0);
  AmixArgs A;
  A.img = img; A.partner = partner; A.lam = lam; A.twiddle = twiddle; A.out_u8 = out_u8; A.out_f32 = out_f32;
  A.spec = work; A.corr = work + amix_half(N, S, b);
  A.N = N; A.b = b;
  const hipStream_t st = (hipStream_t)stream;
  switch (S) {
    case 32: amix_launch<32>(A, st); break;
    case 64: amix_launch<64>(A, st); break;
    case 128: amix_launch<128>(A, st); break;
    case 256: amix_launch<256>(A, st); break;
    default: amix_launch<512>(A, st); break;
  }
  return wtpse_status();
}
