/* l2o_mlp_hvp_abi.h -- the Hessian-vector product of the problems.mnist optimizee: the part of the C ABI of libl2o_hip.so that
 * was added after ABI v15 for second_derivatives=True on an MLP optimizee.  Conventions (error codes, l2o_last_error) and the
 * struct l2o_mlp_deep: l2o_abi.h, which this header includes.  (A header of its own: l2o_abi.h's list of exports is the v15
 * list.) */
#ifndef L2O_MLP_HVP_ABI_H
#define L2O_MLP_HVP_ABI_H

#include "l2o_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = H(w; minibatch) u, with H the Hessian of the mean softmax cross-entropy that l2o_mlp_deep_fg differentiates (the
 * 1 / batch included) at the weights w on the minibatch rows `indices`: the FULL Hessian (not Gauss-Newton), computed
 * forward-over-reverse (Pearlmutter), two launches (csrc/l2o_mlp_hvp.h).
 *   mlp       one to three hidden layers of <= 32 units, sigmoid or relu, n_out <= 16, n_in <= 1024, batch <= 4096 -- what
 *             l2o_mlp_deep_fg takes; the one-hidden-layer optimizee (struct l2o_mlp) is n_hidden_layers = 1 here
 *   indices   device [batch] rows of the minibatch
 *   w, u, out HOST arrays of 2 (n_hidden_layers + 1) device pointers in Sonnet's order, as l2o_mlp_deep_fg takes them:
 *             linear_0/w [n_in, h0], linear_0/b [h0], ..., linear_L/w [h_{L-1}, n_out], linear_L/b [n_out].  out may not
 *             alias w or u; every entry of out is written
 *   scratch   device [l2o_mlp_hvp_scratch_floats(mlp)]; nothing is kept in it between calls and no entry is read that the
 *             call has not written
 * No atomics, sums over the minibatch in sample order: two calls on the same inputs are bit-identical.  A shape outside the
 * range returns L2O_ERR_UNSUPPORTED (l2o_mlp_hvp_scratch_floats: 0) and launches nothing.
 * Added after ABI v15 and not in L2O_ABI_VERSION 15's list: test for the symbol. */
size_t l2o_mlp_hvp_scratch_floats(const l2o_mlp_deep* mlp);
int l2o_mlp_hvp(const l2o_mlp_deep* mlp, const int32_t* indices /* device [batch] */, const float* const* w,
                const float* const* u, float* const* out, float* scratch /* device */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* L2O_MLP_HVP_ABI_H */
