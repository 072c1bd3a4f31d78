/* l2o_confocal_unroll_abi.h -- the fused persistent unroll of problems.confocal_microscopy_3d: the part of the C ABI of
 * libl2o_hip.so that was added after ABI v15 for it.  Conventions (error codes, l2o_last_error, l2o_last_unroll_form ==
 * L2O_FORM_CONFOCAL_UNROLL after a launch) and the structs l2o_net_cfg / l2o_confocal: l2o_abi.h, which this header includes.
 * (A header of its own: l2o_abi.h's list of exports is the v15 list.) */
#ifndef L2O_CONFOCAL_UNROLL_ABI_H
#define L2O_CONFOCAL_UNROLL_ABI_H

#include "l2o_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The fused unroll of the confocal optimizee: T x { fx_t = loss(x_t * s); g = s * grad; delta, state = net(g, state) for
 * each of the 6 num_points + 1 variables (one shared net); x += delta } then fx_T, as ONE persistent launch (k_cf_unroll:
 * one workgroup per batch row -- the rows are independent problems --, batch of the device's CUs busy) followed by the
 * fixed-order batch mean of the per-row losses.  No workgroup waits for another: there is no status word and no workspace
 * header; two calls from the same start are bit-identical.
 *   x, st, m, v, x_scale, sim   HOST arrays of 6 num_points + 1 pointers in l2o_confocal_fg's variable order.  x / m / v /
 *             x_scale / sim entries: device [batch]; st entries: the variable's own packed state, l2o_state_floats(1, batch)
 *             floats (row b is coordinate b), exactly what l2o_cwlstm_step keeps for it.  m, v: RNNProp only (else NULL);
 *             x_scale may be NULL or hold NULLs (= 1); sim is NULL (ignored) with inference = 1.  x, st, m, v are updated
 *             in place.
 *   fx        device [T + 1]: the loss (mean over batch) of every evaluation
 *   scratch   device [l2o_confocal_unroll_scratch_floats(net, T)], 8-byte aligned; nothing is kept in it between calls
 * l2o_confocal_unroll_supported() != 0 for the (20, 20) LSTM nets (both kinds, the three preprocess kinds) and the shapes
 * l2o_confocal_fg takes; everything else returns L2O_ERR_UNSUPPORTED and launches nothing.
 * l2o_confocal_unroll_record also writes what the meta-gradient needs (T + 1 gradient evaluations), per variable k:
 *   hist.st[k]  [T][l2o_state_floats(1, batch)]  the packed LSTM state BEFORE step t
 *   hist.g[k]   [T + 1][batch]                   the gradient at x_t (times x_scale), slot T = at x_T
 *   hist.m[k], hist.v[k]  [T + 1][batch]         RNNProp: the moments AFTER step t in slot t + 1 (slot 0 is not written);
 *                                                NULL for the DM nets
 * Added after ABI v15 and not in L2O_ABI_VERSION 15's list: test for the symbol. */
#define L2O_CONFOCAL_MAX_VARS 49     /* 6 * 8 points + 1 */
typedef struct l2o_confocal_hist {
  float* st[L2O_CONFOCAL_MAX_VARS];
  float* g[L2O_CONFOCAL_MAX_VARS];
  float* m[L2O_CONFOCAL_MAX_VARS];
  float* v[L2O_CONFOCAL_MAX_VARS];
} l2o_confocal_hist;
int l2o_confocal_unroll_supported(const l2o_net_cfg* cfg, const l2o_confocal* net, void* stream);
size_t l2o_confocal_unroll_scratch_floats(const l2o_confocal* net, int32_t T);
int l2o_confocal_unroll(const l2o_net_cfg* cfg, const float* wpack /* device */, const l2o_confocal* net, float* const* x,
                        float* const* st, float* const* m, float* const* v, const float* const* x_scale,
                        const float* const* sim, int32_t T, int32_t step0, float* fx, float* scratch, void* stream);
int l2o_confocal_unroll_record(const l2o_net_cfg* cfg, const float* wpack /* device */, const l2o_confocal* net,
                               float* const* x, float* const* st, float* const* m, float* const* v,
                               const float* const* x_scale, const float* const* sim, int32_t T, int32_t step0, float* fx,
                               const l2o_confocal_hist* hist, float* scratch, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* L2O_CONFOCAL_UNROLL_ABI_H */
