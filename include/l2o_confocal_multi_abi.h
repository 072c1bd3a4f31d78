/* l2o_confocal_multi_abi.h -- several instances of problems.confocal_microscopy_3d per fused launch: the part of the C ABI
 * of libl2o_hip.so that was added for replicas.Replicas' form "rows".  Conventions, l2o_net_cfg / l2o_confocal: l2o_abi.h;
 * the single-instance form, L2O_CONFOCAL_MAX_VARS and l2o_confocal_hist: l2o_confocal_unroll_abi.h, which this header
 * includes.  (A header of its own: the lists of exports of those two headers are fixed.) */
#ifndef L2O_CONFOCAL_MULTI_ABI_H
#define L2O_CONFOCAL_MULTI_ABI_H

#include "l2o_confocal_unroll_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The fused unroll of l2o_confocal_unroll on n_inst independent instances in ONE launch of k_cf_unroll: the rows of the
 * optimizee are independent problems, so workgroup i serves row i % batch of instance i / batch -- eight instances of
 * batch 32 are 256 workgroups.  No workgroup waits for another (more workgroups than CUs is fine): no status word, no
 * workspace header, nothing to recover from.  Per row the arithmetic is the single form's, and every instance's batch mean
 * is formed in the single form's order: the results are BIT-IDENTICAL to n_inst l2o_confocal_unroll calls.
 *   All instances share ONE descriptor (batch, num_points, roi, inference), one network (cfg, wpack) and one step0.
 *   inst      HOST array of n_inst instances; their pointer tables reach the kernel through `scratch` (written by small
 *             launches ahead of the unroll, in stream order: the host is not synchronised)
 *   scratch   device [l2o_confocal_unroll_multi_scratch_floats(net, n_inst, T)], 8-byte aligned; nothing is kept in it
 *             between calls
 * Supported where l2o_confocal_unroll_supported is, for 1 <= n_inst <= L2O_CONFOCAL_MAX_INSTANCES: everything else
 * returns L2O_ERR_UNSUPPORTED, launches nothing and writes nothing (the predicate and the scratch query return 0).  A
 * NULL buffer of a live variable is L2O_ERR_ARG, with nothing launched.  After a launch l2o_last_unroll_form() ==
 * L2O_FORM_CONFOCAL_MULTI | (1 << 8).
 * l2o_confocal_unroll_multi_record also writes every instance's history (hist[i] as l2o_confocal_unroll_record's hist).
 * Added after ABI v15 and not in L2O_ABI_VERSION 15's list: test for the symbol. */
#define L2O_CONFOCAL_MAX_INSTANCES 32
#define L2O_FORM_CONFOCAL_MULTI 13     /* k_cf_unroll, several instances per launch; no exchange */
typedef struct l2o_confocal_instance {
  float* x[L2O_CONFOCAL_MAX_VARS];           /* as l2o_confocal_unroll's x / st / m / v / x_scale / sim, per variable */
  float* st[L2O_CONFOCAL_MAX_VARS];
  float* m[L2O_CONFOCAL_MAX_VARS];           /* RNNProp only, else ignored */
  float* v[L2O_CONFOCAL_MAX_VARS];
  const float* x_scale[L2O_CONFOCAL_MAX_VARS]; /* entries may be NULL (= 1) */
  const float* sim[L2O_CONFOCAL_MAX_VARS];   /* ignored with inference = 1 */
  const float* img;                          /* inference = 1: THIS instance's [batch][V]; the descriptor's img is ignored */
  float* fx;                                 /* device [T + 1] */
} l2o_confocal_instance;
int l2o_confocal_unroll_multi_supported(const l2o_net_cfg* cfg, const l2o_confocal* net, int32_t n_inst, void* stream);
size_t l2o_confocal_unroll_multi_scratch_floats(const l2o_confocal* net, int32_t n_inst, int32_t T);
int l2o_confocal_unroll_multi(const l2o_net_cfg* cfg, const float* wpack /* device */, const l2o_confocal* net,
                              const l2o_confocal_instance* inst /* host [n_inst] */, int32_t n_inst, int32_t T,
                              int32_t step0, float* scratch, void* stream);
int l2o_confocal_unroll_multi_record(const l2o_net_cfg* cfg, const float* wpack /* device */, const l2o_confocal* net,
                                     const l2o_confocal_instance* inst /* host [n_inst] */, int32_t n_inst, int32_t T,
                                     int32_t step0, const l2o_confocal_hist* hist /* host [n_inst] */, float* scratch,
                                     void* stream);

#ifdef __cplusplus
}
#endif

#endif /* L2O_CONFOCAL_MULTI_ABI_H */
