/* l2o_nas_abi.h -- the NAS-cell optimizee on CIFAR-10 (problems.NAS): the part of the C ABI of libl2o_hip.so that was added
 * after ABI v15.  Conventions (error codes, l2o_last_error): l2o_abi.h, which this header includes.  (A header of its own:
 * l2o_abi.h's list of exports is the v15 list.) */
#ifndef L2O_NAS_ABI_H
#define L2O_NAS_ABI_H

#include "l2o_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define L2O_PROB_NAS 11        /* problems.NAS :540-634 (own entry point: l2o_nas_fg) */

/* problems.NAS (DM/problems.py:540-634; DM/util.py:185-190 "nas"): NHWC 32x32x3 images ->
 *   L(x; name) = relu([batch norm] (conv 3x3 stride 1 SAME (x, name/weights1 [3,3,cin,16]) + name/biases1))
 *   node0 = L(x; node0), n02 = L(node0; node0_onto_node2), node1 = L(node0; node1), n13 = L(node1; node1_onto_node3),
 *   node2 = avg_pool 3x3 stride 1 SAME (node1; divided by the number of VALID cells) + n02,  node3 = node2 + n13 + node0,
 *   nf = mean over the 1024 positions of node3 [batch, 16],  out = relu(nf fc_weights [16,10] + fc_bias),
 *   loss = mean_b sparse softmax cross-entropy(out_b, label_b).
 * Batch norm is tf.layers.batch_normalization(training=True): the statistics of the minibatch over batch x 1024 values per
 * channel, biased variance, eps 1e-3; the variance comes from merged per-sample (mean, M2) partials.
 * The step-granular evaluation only: loss + gradients of one minibatch.  The four convolutions, their input gradients and
 * their weight gradients are implicit GEMMs on v_mfma_f32_16x16x4_f32 (exact fp32 products, a k-ordered fmaf chain); every
 * reduction runs in an order that is a function of the minibatch size alone and there are no atomics: two calls on the
 * same inputs are bit-identical, and g == NULL (forward only) gives the same loss bits.  No fused unroll.
 * w / g: HOST arrays of device pointers in the reference's variable order, 18 with batch norm:
 *   node0/weights1 [3,3,3,16] (HWIO), node0/biases1 [16], batch_normalization/gamma [16], batch_normalization/beta [16],
 *   the same four of node0_onto_node2 ([3,3,16,16]; batch_normalization_1), node1 (_2) and node1_onto_node3 (_3),
 *   fc_weights [16,10], fc_bias [10]
 * and 10 without (no gamma / beta).  g may be NULL; every entry of every g[k] is written.  Under batch norm the gradient
 * of a conv bias is 0 in exact arithmetic (batch norm removes any per-channel shift): it is written as that analytic 0.
 * An index outside the data set is clamped into it.  batch in [2, 1024], flags 0, batch_norm 0 or 1, n_data >= 1, else
 * L2O_ERR_UNSUPPORTED (l2o_nas_scratch_floats: 0).  scratch 16-byte aligned; nothing is kept in it between calls and no
 * entry is read that the call has not written.  Its size in floats, every term rounded up to a multiple of 4:
 *   batch (3072 + 6 * 16384)      the gathered images; z of node0, of (n02, node1) [.,32] and of n13; dy of node1 and node0
 *   + 448                         four layers x (scale, shift, mean, rstd, gamma rstd, mean dy, mean dy xhat) x 16
 *   + 2 * 64 batch                the per-sample (mean, M2) and (sum dy, sum dy xhat) partials of up to 32 channels
 *   + 3 * 16 batch + batch        nf, dL/dout, dL/dnf / 1024 and the per-sample losses
 *   + min(4 batch, 256) * 4608    the weight-gradient partials [144][32] of the workgroups of the split */
typedef struct l2o_nas {
  int32_t batch;         /* minibatch size                            */
  int32_t n_data;        /* rows of `images`                          */
  int32_t batch_norm;    /* 0 / 1                                     */
  int32_t flags;         /* 0                                         */
  const float* images;   /* device [n_data, 3072] (NHWC 32x32x3)      */
  const int32_t* labels; /* device [n_data]                           */
} l2o_nas;
size_t l2o_nas_scratch_floats(const l2o_nas* net);
int l2o_nas_fg(const l2o_nas* net, const int32_t* indices /* device [batch] rows of the minibatch */,
               const float* const* w, float* loss /* device [1] */, float* const* g,
               float* scratch /* device [l2o_nas_scratch_floats] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* L2O_NAS_ABI_H */
