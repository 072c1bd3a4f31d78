/* l2o_twin_abi.h -- Twin-L2O (Model_Free_L2O/L2O-Minimax/Twin-L2O.py): two per-coordinate two-layer LSTM optimizers that
 * alternate over an analytic saddle objective, the whole evaluation unroll in one launch: the part of the C ABI of
 * libl2o_hip.so that was added after ABI v15.  Conventions (error codes, l2o_last_error): l2o_abi.h, which this header
 * includes.  (A header of its own: l2o_abi.h's list of exports is the v15 list.)
 *
 * Objectives (l2o_twin_problem.kind; u = theta_min, v = theta_max):
 *   1 saddle          a u^2 - b v^2              2 rotated saddle   a u^2 - b v^2 + 2 u v
 *   3 seesaw          -b v sin(a pi u)           4 matrix game      u^T A v   (dim >= 1; A [dim][dim] row-major)
 * Rows are coordinates: row = instance * dim + coordinate, n_inst * dim of them, all sharing the two networks.
 * Network (torch layouts, device pointers): LSTMCell(n_in, H) w_ih1 [4H][n_in], w_hh1 [4H][H], b_ih1, b_hh1 [4H];
 * LSTMCell(H, H) w_ih2, w_hh2 [4H][H], b_ih2, b_hh2 [4H]; Linear(H, 1) w_out [H], b_out [1].  The cell is torch's:
 *   z = x w_ih^T + b_ih + h w_hh^T + b_hh, split i, f, g, o;  c' = sigmoid(f) c + sigmoid(i) tanh(g);  h' = sigmoid(o) tanh(c')
 * Iteration k (1-based, global): odd k steps u with network `mn` on the input row [df/du, df/dv], even k steps v with
 * network `mx` on [df/dv, df/du] (n_in = 1: the first entry alone), both gradients at the current point.  A network's
 * (h1, c1, h2, c2) are multiplied by `rescale` before its step and replaced by it; delta = w_out . h2' + b_out; the
 * variable moves by sign(delta) sign_lr[k - 1] while k <= n_sign (sign(0) = 0) and by delta out_mul after that.
 * State (l2o_twin_state_floats(net, rows) = 4 H rows floats per network): unit-major, h1 [H][rows], c1 [H][rows],
 * h2 [H][rows], c2 [H][rows], without padding.
 * Accepted: hidden in [1, 96] for both networks (they may differ), n_in 1 or 2, dim in [1, 16], kinds 1-4, kinds 1-3 with
 * dim = 1 only, flags 0, n_inst >= 1; else l2o_twin_supported is 0, l2o_twin_state_floats is 0 and l2o_twin_unroll
 * returns L2O_ERR_UNSUPPORTED and launches nothing. */
#ifndef L2O_TWIN_ABI_H
#define L2O_TWIN_ABI_H

#include "l2o_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define L2O_TWIN_MAX_HIDDEN 96
#define L2O_TWIN_MAX_DIM 16
#define L2O_TWIN_SADDLE 1
#define L2O_TWIN_ROTATED_SADDLE 2
#define L2O_TWIN_SEESAW 3
#define L2O_TWIN_MATRIX_GAME 4

typedef struct l2o_twin_net {
  int32_t hidden, n_in;        /* n_in 1 | 2 */
  const float *w_ih1, *w_hh1, *b_ih1, *b_hh1;
  const float *w_ih2, *w_hh2, *b_ih2, *b_hh2;
  const float *w_out, *b_out;
} l2o_twin_net;

typedef struct l2o_twin_problem {
  int32_t kind, n_inst, dim, flags;
  const float* data;           /* kinds 1-3: [n_inst][2] = a, b; kind 4: [n_inst][dim][dim] */
} l2o_twin_problem;

typedef struct l2o_twin_run {
  int32_t iter0, n_iter, n_sign;   /* iterations iter0 .. iter0+n_iter-1 (1-based, global);
                                      k <= n_sign takes the sign rule */
  float rescale, out_mul;
  const float* sign_lr;            /* device, indexed k-1 (may be NULL when n_sign is 0) */
} l2o_twin_run;

int    l2o_twin_supported(const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p);
size_t l2o_twin_state_floats(const l2o_twin_net* net, int64_t rows);

/* Runs iterations iter0 .. iter0 + n_iter - 1 of every instance in one persistent launch: theta and the two states stay on
 * chip in between and are read once and written once.  Everything a later launch needs to continue is in theta, the two
 * state buffers and iter0: a run split into two launches gives the bits of one.  The gate products run on the matrix cores
 * in exact fp32 (v_mfma_f32_16x16x4_f32), everything else in fp32 VALU; no atomics, a fixed summation order.  Every entry
 * of every non-NULL output is written; nothing past n_inst * dim rows is read or written.  The call re-packs the weights
 * into a stream-ordered temporary (hipMallocAsync / hipFreeAsync on `stream`). */
int l2o_twin_unroll(const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p,
                    const l2o_twin_run* run,
                    float* theta,                    /* [n_inst][2][dim], in/out */
                    float* state_min, float* state_max,
                    float* curve,                    /* NULL | [n_iter][n_inst][2 dim]: the point after each iteration */
                    float* fval,                     /* NULL | [n_iter][n_inst]: f(u, v) after each iteration */
                    float* delta,                    /* NULL | [n_iter][n_inst][dim]: the raw delta of each iteration */
                    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* L2O_TWIN_ABI_H */
