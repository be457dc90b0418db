// What crosses translation units of the library without being part of the C ABI (include/wtpse_hip.h): declared once, here.
// C++ linkage, so the linker checks the types, and hidden visibility: the library exports the header's names only.
#pragma once
#include <cstdlib>
#include "common.h"

#define WTPSE_INTERNAL __attribute__((visibility("hidden")))

WTPSE_INTERNAL extern int g_x3_terms;      // conv_x3.hip: wtpse_x3_terms()

// conv_x3.hip: wtpse_conv_fwd_bnf / wtpse_dgrad_bnb_coef (conv.hip), x3 layout
WTPSE_INTERNAL int conv_fwd_x3_ftail(const float* in0, int C0, const float* in1, int C1, const unsigned short* wpacked,
                                     const float* bias, const float* pro0, const float* pro1, int pro_relu, float* out0,
                                     float* stats, const BnfTail* ftail, int B, int H, int W, int Cout, int ksize,
                                     const unsigned* in_amax0, const unsigned* in_amax1, void* stream);
WTPSE_INTERNAL int dgrad_x3_bnb_tail(const float* dy, int C, const unsigned short* wpacked, float* out0, float* out1, int Csplit,
                                     const float* bn_y, const float* bn_ss, const float* bn_mean, int bn_relu, int bn_c0,
                                     int bn_c1, float* stats, const BnbTail* tail, int B, int H, int W, int Cout, int ksize,
                                     const unsigned* in_amax, void* stream);

// conv.hip: fold of the k-split weight-gradient slabs; the second with the bias-gradient slabs folded in the same launch
WTPSE_INTERNAL void wgrad_reduce_launch(const float* slab, int ksplit, int n, float* dw, int accumulate, void* stream);
WTPSE_INTERNAL void wgrad_reduce_launch2(const float* slab, int ksplit, int n, float* dw, int accumulate, const float* slab_b,
                                         int n_b, float* db, void* stream);

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
// after a launch whose tails were switched off for size: the same results from the stand-alone kernels
static inline int tail_after_launch(const BnbTail& tl, const BnfTail& fl, float* stats, int nblk, int Cout, int bn_c0, int bn_c1,
                                    const float* bn_mean, long long count, void* stream) {
  if (tl.tickets && tl.dbias)
    return wtpse_bn_bwd_finalize_coef_frozen(stats, nblk, bn_c1 - bn_c0, tl.gamma, tl.invstd, tl.coef, tl.dgamma, tl.dbeta, tl.dbias,
                                             tl.accumulate, stream);
  if (tl.tickets)
    return wtpse_bn_bwd_finalize_coef(stats, nblk, bn_c1 - bn_c0, count, tl.gamma, bn_mean, tl.invstd, tl.coef, tl.dgamma, tl.dbeta,
                                      tl.accumulate, stream);
  if (fl.tickets)
    return wtpse_bn_finalize(stats, nblk, Cout, count, fl.gamma, fl.beta, fl.rmean, fl.rvar, fl.nbt, fl.momentum, fl.eps,
                             fl.scale_shift, fl.save_mean, fl.save_invstd, fl.act_amax, stream);
  return 0;
}
