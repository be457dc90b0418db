// Test-time views (wtpse_hip/views.py; validate.predict_pair_views): the eight symmetries of the square applied to the network
// input, and the merge of the V x K logit maps the views give back.  Two launches:
//
//   views_gen_k   : out[v][n] = view(x[n], codes[v]) for every plane — a pure permutation, bit for bit views.view_host.
//   views_merge_k : every map logits[v][b][k], given in its view's own frame, is turned back (views.unview_host), and per pixel the
//                   V K sigmoids are folded into mean, population spread (the running Welford update of shape_samples_k: equal
//                   samples give exactly 0) and vote count, the logits into their float32 sum.  One pass: each input map is read
//                   once, the un-viewed maps are written once when asked for, and a pixel's results are written once.
//
// What was chosen, and why.  A workgroup (256 lanes) owns one 32 x 32 tile of one OUTPUT plane; lane (qx = tid & 7, ly = tid >> 3)
// owns the quad of four consecutive pixels (row ly, columns 4 qx .. 4 qx + 3) of it and keeps the quad's state — mean, M2, votes,
// logit sum: 16 registers — across all V K maps.  Both kernels get their tile through unview_quad():
//   * a view that does not transpose: an output row is a source row read forwards or backwards, so the lane loads its quad with one
//     16-byte load (at column S - 4 - j and reversed in registers under a column flip; S % 4 == 0 keeps that aligned).  Eight
//     lanes cover the 128 contiguous bytes of a tile row.  No LDS.
//   * a transposing view: an output row is a source COLUMN.  The workgroup loads the source tile the same row-contiguous way (lane
//     (qx, ly) takes source row <- output column j0 + ly, source columns <- output rows i0 + 4 qx ..), writes it to LDS as
//     tile[ly][4 qx + e] with 33 words per row, and after one barrier reads its own quad as tile[4 qx + e][ly].  ds_write_b32 /
//     ds_read_b32 bank on (address / 4) % 32 within 32-lane halves; a half is 8 quads x 4 rows, so the writes fall on banks
//     (ly + 4 qx + e) % 32 and the reads on (4 qx + e + ly) % 32 — 32 different banks either way: the pad of one word makes the
//     column reads conflict-free.  Two tile buffers alternate, so one barrier per map suffices (a lane that writes buffer p again
//     has passed the barrier of the map in between, which every lane reaches only behind its reads of p).
// Source coordinates are DERIVED from output coordinates (i -> S - 1 - i under a flip, rows <-> columns under a transpose), and a
// lane takes part only when its output quad lies inside the plane.  A partial output tile at the right or bottom edge (S % 32 != 0)
// therefore reads a source tile that is partial on the mirrored and / or swapped side without any case of its own: every source
// index is the reflection of a valid output index and lies in [0, S).  S % 4 == 0 makes a quad wholly inside or wholly outside.
// The generator is the same gather with the inverse code (view(c) = unview(inverse(c)): bits 0 and 1 swapped when bit 2 is set).
//
// The float32 mean logit has no fused multiply-add in it: the sum starts from the first map and takes one addition per map, the
// factor 1 / (V K) is formed on the host and applied with one multiplication (views.merge_host states the same; the device matches
// it bit for bit).  No atomics, plain vector stores; a tile's results depend on its own index alone, so the grid (at most 2^20
// workgroups, grid-stride over the tiles) does not enter them.  All element indices are 64-bit.
#include "common.h"

#define VW_MAX_V 8
#define VW_MAX_MAPS 64                 // US_MAX_K of uncertainty.hip: the votes are a byte, the per-sample post-processing one set of launches
#define VW_TILE 32
#define VW_LDW 33                      // words per LDS tile row

static bool vw_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

__device__ __forceinline__ f32x4 vw_load_quad(const float* __restrict__ row, int col, int S, bool flip) {
  // the four source values that land on four consecutive destination positions starting at destination index `col`
  const f32x4 v = *reinterpret_cast<const f32x4*>(row + (flip ? S - 4 - col : col));
  f32x4 r = {v[3], v[2], v[1], v[0]};
  return flip ? r : v;
}

// The quad (row i0 + ly, columns j0 + 4 qx ..) of unview(src, c), src one [S][S] plane.  Every lane of the workgroup calls (c is
// uniform; a transposing c holds a barrier); lanes whose quad lies outside the plane get zeros.  par: the LDS buffer to use next.
__device__ __forceinline__ f32x4 unview_quad(const float* __restrict__ src, int c, int S, int i0, int j0, int qx, int ly,
                                             float (*lds)[VW_TILE * VW_LDW], int& par) {
  f32x4 q = {0.f, 0.f, 0.f, 0.f};
  const bool flip_r = (c & 2) != 0, flip_c = (c & 1) != 0;
  if (!(c & 4)) {
    const int i = i0 + ly, j = j0 + 4 * qx;
    if (i < S && j < S) q = vw_load_quad(src + (long long)(flip_r ? S - 1 - i : i) * S, j, S, flip_c);
    return q;
  }
  // out[i][j] = src[flip_r ? S-1-j : j][flip_c ? S-1-i : i]: the source row follows the output column, the source column the output row
  float* t = lds[par];
  par ^= 1;
  const int sj = j0 + ly, si = i0 + 4 * qx;                       // output column / first output row this lane loads for
  if (sj < S && si < S) {
    const f32x4 v = vw_load_quad(src + (long long)(flip_r ? S - 1 - sj : sj) * S, si, S, flip_c);
#pragma unroll
    for (int e = 0; e < 4; ++e) t[ly * VW_LDW + 4 * qx + e] = v[e];
  }
  __syncthreads();
  if (i0 + ly < S && j0 + 4 * qx < S) {
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = t[(4 * qx + e) * VW_LDW + ly];
  }
  return q;
}

__global__ __launch_bounds__(256) void views_gen_k(const float* __restrict__ x, float* __restrict__ out, unsigned inv_codes, long long N,
                                                   int S, int tiles, long long nitems) {
  __shared__ float lds[2][VW_TILE * VW_LDW];
  int par = 0;
  const int qx = threadIdx.x & 7, ly = threadIdx.x >> 3;
  const long long plane = (long long)S * S, tt = (long long)tiles * tiles;
  for (long long item = blockIdx.x; item < nitems; item += gridDim.x) {
    const long long vn = item / tt;                               // v * N + n
    const int tile = (int)(item - vn * tt);
    const int v = (int)(vn / N);
    const long long n = vn - (long long)v * N;
    const int i0 = (tile / tiles) * VW_TILE, j0 = (tile % tiles) * VW_TILE;
    const f32x4 q = unview_quad(x + n * plane, (int)((inv_codes >> (3 * v)) & 7u), S, i0, j0, qx, ly, lds, par);
    const int i = i0 + ly, j = j0 + 4 * qx;
    if (i < S && j < S) *reinterpret_cast<f32x4*>(out + vn * plane + (long long)i * S + j) = q;
  }
}

__global__ __launch_bounds__(256) void views_merge_k(const float* __restrict__ logits, unsigned codes, int V, int B, int K, int S,
                                                     float threshold, float inv_vk, float* __restrict__ logits_out,
                                                     float* __restrict__ mean, float* __restrict__ std_, unsigned char* __restrict__ votes,
                                                     float* __restrict__ mean_logit, int tiles, long long nitems) {
  __shared__ float lds[2][VW_TILE * VW_LDW];
  int par = 0;
  const int qx = threadIdx.x & 7, ly = threadIdx.x >> 3;
  const long long plane = (long long)S * S, tt = (long long)tiles * tiles;
  for (long long item = blockIdx.x; item < nitems; item += gridDim.x) {
    const long long b = item / tt;
    const int tile = (int)(item - b * tt);
    const int i0 = (tile / tiles) * VW_TILE, j0 = (tile % tiles) * VW_TILE;
    const int i = i0 + ly, j = j0 + 4 * qx;
    const bool valid = i < S && j < S;
    const long long pix = (long long)i * S + j;                   // of the quad within a plane
    float mean_[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f}, sum[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned nv[4] = {0u, 0u, 0u, 0u};
    int s = 0;
    for (int v = 0; v < V; ++v) {
      const int c = (int)((codes >> (3 * v)) & 7u);
      for (int k = 0; k < K; ++k, ++s) {
        const f32x4 l = unview_quad(logits + (((long long)v * B + b) * K + k) * plane, c, S, i0, j0, qx, ly, lds, par);
        if (!valid) continue;
        const float inv_n = 1.f / (float)(s + 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float pr = sigmoidf_(l[e]);
          const float d = pr - mean_[e];                          // Welford: equal samples leave d = 0 from the second on
          mean_[e] = fmaf(d, inv_n, mean_[e]);
          m2[e] = fmaf(d, pr - mean_[e], m2[e]);
          nv[e] += pr > threshold ? 1u : 0u;
          sum[e] = s == 0 ? l[e] : sum[e] + l[e];
        }
        if (logits_out) *reinterpret_cast<f32x4*>(logits_out + (b * ((long long)V * K) + s) * plane + pix) = l;
      }
    }
    if (!valid) continue;
    f32x4 mo, so, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      mo[e] = mean_[e];
      so[e] = sqrtf(fmaxf(m2[e], 0.f) * inv_vk);
      lo[e] = sum[e] * inv_vk;
    }
    const long long o = b * plane + pix;
    *reinterpret_cast<f32x4*>(mean + o) = mo;
    *reinterpret_cast<f32x4*>(std_ + o) = so;
    *reinterpret_cast<unsigned*>(votes + o) = nv[0] | (nv[1] << 8) | (nv[2] << 16) | (nv[3] << 24);
    if (mean_logit) *reinterpret_cast<f32x4*>(mean_logit + o) = lo;
  }
}

static unsigned vw_blocks(long long nitems) { return (unsigned)(nitems > (1LL << 20) ? (1LL << 20) : nitems); }

// codes[0 .. V) checked and packed three bits each (inverse: the code of the inverse view); -1: a code outside 0..7
static int vw_pack(const int* codes, int V, bool inverse, unsigned* packed) {
  unsigned p = 0;
  for (int v = 0; v < V; ++v) {
    int c = codes[v];
    if (c < 0 || c > 7) return -1;
    if (inverse && (c & 4)) c = 4 | ((c & 1) << 1) | ((c >> 1) & 1);
    p |= (unsigned)c << (3 * v);
  }
  *packed = p;
  return 0;
}

extern "C" int wtpse_dihedral_views(const float* x, float* out, const int* codes, int V, int N, int S, void* stream) {
  WTPSE_REQUIRE(x && out && codes && V >= 1 && V <= VW_MAX_V && N >= 1 && S >= 4 && S % 4 == 0);
  WTPSE_REQUIRE(vw_aligned(x, 16) && vw_aligned(out, 16));
  unsigned packed;
  WTPSE_REQUIRE(vw_pack(codes, V, true, &packed) == 0);
  const int tiles = ceil_div(S, VW_TILE);
  const long long nitems = (long long)V * N * tiles * tiles;
  hipLaunchKernelGGL(views_gen_k, dim3(vw_blocks(nitems)), dim3(256), 0, (hipStream_t)stream, x, out, packed, (long long)N, S, tiles,
                     nitems);
  return wtpse_status();
}

extern "C" int wtpse_views_merge(const float* logits, const int* codes, int V, int B, int K, int S, float threshold, float* logits_out,
                                 float* mean, float* std_, unsigned char* votes, float* mean_logit, void* stream) {
  WTPSE_REQUIRE(logits && codes && mean && std_ && votes);
  WTPSE_REQUIRE(V >= 1 && V <= VW_MAX_V && K >= 1 && (long long)V * K <= VW_MAX_MAPS && B >= 1 && S >= 4 && S % 4 == 0);
  WTPSE_REQUIRE(vw_aligned(logits, 16) && vw_aligned(logits_out, 16) && vw_aligned(mean, 16) && vw_aligned(std_, 16) &&
                vw_aligned(mean_logit, 16) && vw_aligned(votes, 4));
  unsigned packed;
  WTPSE_REQUIRE(vw_pack(codes, V, false, &packed) == 0);
  const int tiles = ceil_div(S, VW_TILE);
  const long long nitems = (long long)B * tiles * tiles;
  hipLaunchKernelGGL(views_merge_k, dim3(vw_blocks(nitems)), dim3(256), 0, (hipStream_t)stream, logits, packed, V, B, K, S, threshold,
                     1.f / (float)(V * K), logits_out, mean, std_, votes, mean_logit, tiles, nitems);
  return wtpse_status();
}
