// What crosses translation units of the library without being part of the C ABI (include/wtpse_hip.h): declared once, here.
// C++ linkage, so the linker checks the types, and hidden visibility: the library exports the header's names only.
// The host side of the convolutions lives here: ConvCall / WgradCall (what an entry point asks for), conv_run / wgrad_run (check, then
// the launcher of the kernel family) and the tiling functions that size queries and launches share.
#pragma once
#include <cstdlib>
#include "common.h"

#define WTPSE_INTERNAL __attribute__((visibility("hidden")))

WTPSE_INTERNAL extern int g_x3_terms;      // conv_x3.hip: wtpse_x3_terms()

// One forward or data-gradient convolution as its entry point describes it: the nine extern "C" entry points of conv.hip / conv_x3.hip
// fill the fields they were given by name and hand the call to conv_run(), which checks it (conv_check: every precondition once, the
// per-layout ones keyed on the layout) and passes it to the launcher of its kernel family, the only place that fills that family's
// kernel argument struct.  Every default means "none"; a data gradient is the forward kernel on dY (in0 = dy, mask_ref = bn_y).
struct BnbArgs {   // BatchNorm-backward epilogue over output channels [c0, c1) (mean == null: none)
  const float* ss = nullptr;
  const float* mean = nullptr;
  int relu = 0, c0 = 0, c1 = 0;
};
struct ConvCall {
  const float* in0 = nullptr; int C0 = 0;
  const float* in1 = nullptr; int C1 = 0;         // virtual concat behind in0
  const void* w = nullptr;                        // packed weights in the layout's format
  const float* bias = nullptr;
  const float* pro0 = nullptr; const float* pro1 = nullptr; int pro_relu = 0;
  float* out0 = nullptr; float* out1 = nullptr; int Csplit = 0;      // one output: Csplit == Cout
  float* stats = nullptr;
  const float* mask_ref = nullptr;
  float* gram = nullptr;
  const unsigned* in_amax0 = nullptr; const unsigned* in_amax1 = nullptr;
  int in_is_grad = 0;
  unsigned* out_amax = nullptr;
  BnbArgs bn;
  BnbTail tail = bnb_tail_none();
  BnfTail ftail = bnf_tail_none();
  int B = 0, H = 0, W = 0, Cout = 0, ksize = 0, relu_out = 0;
};
enum { CONV_FP32 = 0, CONV_X3 = 1, CONV_C16 = 2 };     // = `layout` of wtpse_conv_fwd_bnf / wtpse_dgrad_bnb_coef (include/wtpse_hip.h)
WTPSE_INTERNAL int conv_run(const ConvCall& c, int layout, hipStream_t st);    // conv.hip
WTPSE_INTERNAL int conv_launch_x3(const ConvCall& c, hipStream_t st);           // conv_x3.hip

// Tiling of a launch: decided in one function per kernel family, which the size query and the launch both call.
struct Tiling {
  int TW, TH, tiles_x, tiles_y, tiles;
};
static inline Tiling make_tiling(int B, int H, int W, bool narrow, int pixels) {
  Tiling t;
  t.TW = narrow ? 16 : 32; t.TH = pixels / t.TW;
  t.tiles_x = ceil_div(W, t.TW); t.tiles_y = ceil_div(H, t.TH); t.tiles = B * t.tiles_x * t.tiles_y;
  return t;
}
// conv_fwd_k / conv_wgrad_k (conv.hip): 256 pixels, 16x16 for the deepest levels, 8x32 otherwise; the x3 kernels: 256 or 128 pixels
static inline Tiling conv_tiling(int B, int H, int W, int pixels = 256) { return make_tiling(B, H, W, W <= 16, pixels); }
// conv_x3_k / conv_x3r_k (conv_x3.hip: x3_tiling)
struct X3Tiling {
  int mt;           // 32-channel blocks per workgroup: 1 | 2
  int px;           // pixels per tile: 128 | 256
  int half;         // 64-channel blocks on 128-pixel tiles (then mt == 2)
  int small;        // 32-channel blocks on 128-pixel tiles (then mt == 1)
  Tiling t;
};
WTPSE_INTERNAL X3Tiling x3_tiling(int B, int H, int W, int Cout, int ksize);

// One weight gradient as its entry point describes it, like ConvCall: the four extern "C" entry points (conv.hip, conv_x3.hip,
// wgrad_r.hip) fill the fields by name and return wgrad_run(): wgrad_check (every precondition once, the per-family ones keyed on the
// family), the family's launcher (the only place that fills its kernel argument struct), the fold of the slabs (wgrad_fold).
struct WgradCall {
  const float* dy = nullptr;                      // the _bn form of WGRAD_R (bn_y, bn_coef): the masked incoming gradient g
  const float* x0 = nullptr; int C0 = 0;
  const float* x1 = nullptr; int C1 = 0;          // virtual concat behind x0
  const float* pro0 = nullptr; const float* pro1 = nullptr; int pro_relu = 0;
  float* slab = nullptr; float* dbias_slab = nullptr; int nslab = 0;       // the k-split (FP32, X3) or slab count (R) the caller sized them for
  float* dw = nullptr; float* dbias = nullptr; int accumulate = 0;
  const float* bn_y = nullptr; const float* bn_coef = nullptr; const unsigned* dy_amax = nullptr;
  const unsigned* x_amax0 = nullptr; const unsigned* x_amax1 = nullptr;
  int B = 0, H = 0, W = 0, Cout = 0, ksize = 0;
};
enum { WGRAD_FP32 = 0, WGRAD_X3 = 1, WGRAD_R = 2 };
WTPSE_INTERNAL int wgrad_run(const WgradCall& c, int family, hipStream_t st);    // conv.hip
WTPSE_INTERNAL int wgrad_launch_x3(const WgradCall& c, hipStream_t st);          // conv_x3.hip
WTPSE_INTERNAL int wgrad_launch_r(const WgradCall& c, hipStream_t st);           // wgrad_r.hip

// Geometry of a weight-gradient launch, one function per kernel family: the size query answers its default `ksplit` / its `nslab`,
// wgrad_check bounds the caller's count with it, the launcher takes its grid from it.
struct WgradX3Geometry {   // conv_wgrad_x3_k: blk x blk channels per workgroup (quadrants: 64 on 64-pixel tiles, else 32 on 128-pixel tiles)
  Tiling t;
  int q, blk, nci, nx, ksplit;     // nci: cin blocks; nx: (cout block, cin block) pairs, the grid's x extent
};
WTPSE_INTERNAL WgradX3Geometry wgrad_x3_geometry(int B, int H, int W, int Cin, int Cout);     // conv_x3.hip
struct WgradRPlan {        // wgrad_r_k; nslab = wpp / nw: workgroups, and so slabs, per (cout block, cin block) pair
  int mf, nf, nw, pairs, nci, wpp, nseg, rseg, units, strips, nslab;
};
WTPSE_INTERNAL bool wgrad_r_plan(int B, int H, int W, int Cin, int Cout, WgradRPlan& p);      // wgrad_r.hip

// Folding the statistics inside the launch makes every workgroup live ~2.5 us longer (its partials must be visible before it takes
// its ticket: store acknowledgement + one L2 atomic round trip).  Measured on the step (back to back, profiles/r03_*): with the
// fold in every launch the convolutions took 2.4 ms more per step than the 346 finalize launches it replaced took (2.2 ms).  A CU
// slot sees nWG / (256 x 2..3) workgroups in a row, so the hand-off wins where that is about one or less; beyond the threshold the
// entry points launch the stand-alone finalize kernel themselves.
// (Round 6: with the fold's loads all in flight at once — tail_fold — the hand-off is cheaper than the stand-alone kernel up to the
// 8192-workgroup launches of the step as well: 41.54 vs 41.66 ms per step, three alternations on one box; the threshold moves there.)
static inline bool tail_in_launch(long long workgroups) {
  static const long long max_wgs = [] { const char* e = getenv("WTPSE_TAIL_MAX_WGS"); return e ? atoll(e) : 8192ll; }();
  return workgroups <= max_wgs;
}
// after a launch whose tails were switched off for size: the same results from the stand-alone kernels (a: ConvArgs | ConvX3Args as
// the launcher filled it)
template <class Args>
static inline int tail_after_launch(const Args& a, int nblk, hipStream_t stream) {
  const BnbTail& tl = a.tail;
  const BnfTail& fl = a.ftail;
  const long long count = (long long)a.B * a.H * a.W;
  if (tl.tickets && tl.dbias)
    return wtpse_bn_bwd_finalize_coef_frozen(a.stats, nblk, a.bn_c1 - a.bn_c0, tl.gamma, tl.invstd, tl.coef, tl.dgamma, tl.dbeta,
                                             tl.dbias, tl.accumulate, stream);
  if (tl.tickets)
    return wtpse_bn_bwd_finalize_coef(a.stats, nblk, a.bn_c1 - a.bn_c0, count, tl.gamma, a.bn_mean, tl.invstd, tl.coef, tl.dgamma,
                                      tl.dbeta, tl.accumulate, stream);
  if (fl.tickets)
    return wtpse_bn_finalize(a.stats, nblk, a.Cout, count, fl.gamma, fl.beta, fl.rmean, fl.rvar, fl.nbt, fl.momentum, fl.eps,
                             fl.scale_shift, fl.save_mean, fl.save_invstd, fl.act_amax, stream);
  return 0;
}
