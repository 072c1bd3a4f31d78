/* l2o_klstm_abi.h -- KernelDeepLSTM (networks.KernelDeepLSTM; DM/networks.py:303-351), the optimizer network for
 * convolution filters: the part of the C ABI of libl2o_hip.so that was added after ABI v15.  Conventions (error codes,
 * l2o_last_error): l2o_abi.h, which this header includes.  (A header of its own: l2o_abi.h's list of exports is the v15
 * list.) */
#ifndef L2O_KLSTM_ABI_H
#define L2O_KLSTM_ABI_H

#include "l2o_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define L2O_KLSTM_MAX_SIDE 7      /* kw, kh in [1, 7]                           */
#define L2O_KLSTM_MAX_LAYERS 2
#define L2O_KLSTM_MAX_HIDDEN 32   /* every width a multiple of 4 in [4, 32]     */

/* A variable w [kw, kh, c_in, c_out] (row-major) is a [K = kw kh][N = c_in c_out] matrix in memory: entry (j, n) at
 * j N + n, j = a kh + b the patch position, n = ci c_out + co the filter.  So are its gradient and its update.  One LSTM
 * per filter n, all filters sharing the weights:
 *   x_n = the K gradients of the patch (L2O_PRE_IDENTITY), or their 2K LogAndSign features (L2O_PRE_LOGSIGN: column 2j
 *         max(log(|g| + eps) / k, -1), column 2j + 1 clip(g e^k, -1, 1), eps = 2^-23); in = K or 2K
 *   per layer (snt.LSTM): z = [x, h] w_gates + b_gates, split i, j, f, o; c' = sigmoid(f + 1) c + sigmoid(i) tanh(j);
 *         h' = tanh(c') sigmoid(o); x <- h'
 *   out = h_L w_lin [H_L, K] + b_lin [K];  x[j N + n] += scale out[n, j]  (scale tanh(out) with tanh_output)
 * Weights: device pointers in Sonnet's layouts, w_gates[l] [in_l + H_l, 4 H_l], b_gates[l] [4 H_l].
 * State: l2o_klstm_state_floats(net, N) floats, unit-major: per layer h [H_l][N] then c [H_l][N]; zero at reset.  The
 * carries of the backward step have the same layout (dL/dh_l, dL/dc_l).
 * Accepted: kw, kh in [1, 7], 1 or 2 layers, every width a multiple of 4 in [4, 32], preprocess identity or LogAndSign,
 * flags 0, N >= 1; else l2o_klstm_supported is 0, l2o_klstm_state_floats is 0 and the entry points return
 * L2O_ERR_UNSUPPORTED and launch nothing. */
typedef struct l2o_klstm_net {
  int32_t kw, kh;
  int32_t n_layers;
  int32_t hidden[L2O_KLSTM_MAX_LAYERS];
  int32_t preprocess;    /* L2O_PRE_IDENTITY | L2O_PRE_LOGSIGN */
  int32_t tanh_output;   /* 0 / 1 */
  int32_t flags;         /* 0 */
  double logsign_k;
  double scale;
  const float* w_gates[L2O_KLSTM_MAX_LAYERS];
  const float* b_gates[L2O_KLSTM_MAX_LAYERS];
  const float* w_lin;    /* [H_L, K] */
  const float* b_lin;    /* [K]      */
} l2o_klstm_net;

int l2o_klstm_supported(const l2o_klstm_net* net);
size_t l2o_klstm_state_floats(const l2o_klstm_net* net, int64_t N);

/* One optimizer step on N filters: reads g [K][N] and state_in, writes state_out (which may be state_in, or any buffer
 * that does not otherwise overlap it) and adds the update into x [K][N].  The gate products run on the matrix cores in
 * exact fp32 (v_mfma_f32_16x16x4_f32), everything else in fp32 VALU; no atomics, a fixed summation order: two calls on the
 * same inputs give the same bits.  Every entry of state_out is written; nothing past N is read or written. */
int l2o_klstm_step(const l2o_klstm_net* net, const float* g, const float* state_in, float* state_out, float* x,
                   int64_t N, void* stream);

/* One step of back-propagation through time of the first-order meta-gradient (g is a constant of it): recomputes the
 * step from st_prev and g, takes dx_next = dL/d(delta_t) [K][N] and the carries from step t + 1, writes the carries for
 * step t - 1 (carry_out must not be carry_in) and the operands of the weight gradients, every entry of each:
 *   act[l] [N][in_l + H_l] = [input_l | h_l(t-1)],  dz[l] [N][4 H_l] = dL/d(gate pre-activations, order i, j, f, o),
 *   h_last [N][H_L],  dd [N][K] = dL/d(Linear output)
 * so that dL/dw_gates[l] += act[l]^T dz[l], dL/db_gates[l] += column sums of dz[l], dL/dw_lin += h_last^T dd,
 * dL/db_lin += column sums of dd.  tc: scratch of sum_l H_l * N floats; nothing in it is read before it is written. */
typedef struct l2o_klstm_bwd_io {
  const float* g;
  const float* st_prev;
  const float* dx_next;
  const float* carry_in;
  float* carry_out;
  float* act[L2O_KLSTM_MAX_LAYERS];
  float* dz[L2O_KLSTM_MAX_LAYERS];
  float* tc;
  float* h_last;
  float* dd;
} l2o_klstm_bwd_io;
int l2o_klstm_bwd_step(const l2o_klstm_net* net, const l2o_klstm_bwd_io* io, int64_t N, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* L2O_KLSTM_ABI_H */
