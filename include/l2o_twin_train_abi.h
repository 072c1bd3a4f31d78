/* l2o_twin_train_abi.h -- Twin-L2O meta-training: one segment of the reference's do_fit(should_train=True) -- its forward
 * with a history, and the meta-gradient of both networks from that history.  Part of the C ABI of libl2o_hip.so beside
 * l2o_twin_abi.h (objectives, network and state layouts, iteration rule: there).
 *
 * The segment.  Iterations iter0 .. iter0 + n_iter - 1 with iter0 odd and n_iter even (the reference: 2 unroll_unit), so a
 * segment starts with a min step and ends with a max step.  Its loss is
 *   total = sum_k (loss_k + loss_{k-1}) m[inst] loss_scale,   loss_k = +f after a min step, -f after a max step,
 * f at the point after iteration k, loss_{k-1} = 0 at the segment's first iteration, summed over the instances.  The LSTM
 * inputs are detached, the stepped variable is detached right after its loss is taken and the sign rule has derivative
 * zero: each network's gradient is a BPTT through its own (h1, c1, h2, c2) chain alone (multiplied by `rescale` before every
 * step), seeded per iteration and row by
 *   g_delta = w_k s_k out_mul (df / d own variable)(point after k) m[inst] loss_scale   (k > n_sign, else 0)
 * with s_k = +1 (min) / -1 (max) and w_k = 2, 1 at the segment's last iteration.
 * Gradients come back in torch's layouts (l2o_twin_net's); b_ih and b_hh of a cell get the same values.  Every entry is
 * written.  fp32 MFMA and fp32 VALU, except that the seed g_delta is evaluated in double and b_out's gradient, the plain sum
 * of the seeds, is their double sum rounded once; no atomics, a fixed summation order: two runs give the
 * same bits. */
#ifndef L2O_TWIN_TRAIN_ABI_H
#define L2O_TWIN_TRAIN_ABI_H

#include "l2o_twin_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define L2O_TWIN_TRAIN_MAX_ITER 64

typedef struct l2o_twin_segment {
  l2o_twin_run run;
  float loss_scale;                /* the reference: 1 / batch_size */
  const float* inst_weight;        /* NULL (all 1) | device [n_inst]: the curriculum's m */
} l2o_twin_segment;

typedef struct l2o_twin_grad {
  float *w_ih1, *w_hh1, *b_ih1, *b_hh1;
  float *w_ih2, *w_hh2, *b_ih2, *b_hh2;
  float *w_out, *b_out;
} l2o_twin_grad;

/* Floats of the work buffer of a segment of n_iter iterations (history of the forward, then scratch of the backward; the
 * layout is the library's own); 0 for what the two calls below refuse. */
size_t l2o_twin_train_floats(const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p, int32_t n_iter);

/* l2o_twin_unroll on the segment -- theta, both states, curve, fval and delta come out with its bits -- that also fills the
 * history part of `work` (16-byte aligned, l2o_twin_train_floats floats).
 * Refused before any launch: what l2o_twin_unroll refuses; iter0 even, n_iter odd, < 2 or > L2O_TWIN_TRAIN_MAX_ITER
 * (L2O_ERR_UNSUPPORTED); NULL weights or buffers, a misaligned `work` (L2O_ERR_ARG). */
int l2o_twin_train_forward(const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p,
                           const l2o_twin_segment* seg, float* theta, float* state_min, float* state_max,
                           float* curve, float* fval, float* delta, float* work, void* stream);

/* The gradient of the segment's loss with respect to every parameter of both networks, from the `work` buffer that
 * l2o_twin_train_forward filled with the same descriptors.  The weights are those of the forward. */
int l2o_twin_train_backward(const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p,
                            const l2o_twin_segment* seg, float* work, const l2o_twin_grad* grad_min,
                            const l2o_twin_grad* grad_max, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* L2O_TWIN_TRAIN_ABI_H */
