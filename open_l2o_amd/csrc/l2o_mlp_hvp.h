// l2o_mlp_hvp.h -- Hessian-vector product of the problems.mnist loss on one minibatch (l2o_mlp_hvp): out = H(w) u with H the
// Hessian of the mean softmax cross-entropy l2o_mlp_deep_fg differentiates (1 / batch included).  What second_derivatives=True
// adds to the meta-gradient of an MLP optimizee (DM/meta.py:322-329 without the tf.stop_gradient).  Builds on
// l2o_mlp_deep.h (its limits and its layer order); written for gfx950 only.
//
// The FULL Hessian (not Gauss-Newton), forward-over-reverse (Pearlmutter's R-operator).  Per sample, tangents Vw_l, Vb_l = u:
//   z_l = a_{l-1} W_l + b_l          Rz_l = Ra_{l-1} W_l + a_{l-1} Vw_l + Vb_l     (Ra_{-1} = 0: the image has no tangent)
//   a_l = phi(z_l)                   Ra_l = phi'(z_l) Rz_l
//   d_L = (p - y) / B                Rd_L = (p * Rz_L - p sum_o p_o Rz_L,o) / B
//   back = d_{l+1} W_{l+1}^T         d_l = back * phi'
//   Rd_l = (Rd_{l+1} W_{l+1}^T + d_{l+1} Vw_{l+1}^T) * phi' + back * phi''(z_l) * Rz_l
//   out_Wl = sum_s (Ra_{l-1}^T d_l + a_{l-1}^T Rd_l)      out_bl = sum_s Rd_l
// sigmoid: phi' = a (1 - a), phi'' = a (1 - a)(1 - 2 a); relu: phi' = [a > 0] as k_mlp_deep_sample decides it, phi'' = 0.
//
// Two launches, the shape of l2o_mlp_deep.h:
//   k_mlp_hvp_sample   one workgroup per minibatch sample: gather the image row, the forward with tangents (the first layer
//                      split over eight k-slices), the backward with R-deltas; a, Ra, d, Rd -> scratch
//   k_mlp_hvp_reduce   one thread per weight / bias coordinate: the sum over the samples IN SAMPLE ORDER, eight samples'
//                      loads in flight, accumulated in double (the bias sums of a small-weight net cancel to a few ulp of
//                      their terms in fp32).  No atomics: two calls on the same inputs are bit-identical; every scratch entry
//                      that is read was written by this call, every output entry is written.
#pragma once
#include "l2o_mlp_deep.h"

#include "../../include/l2o_mlp_hvp_abi.h"

namespace l2o {

struct MlpHvpArgs {
  int n_in, n_out, batch, act, nh;       // nh hidden layers
  int width[kMdMaxHidden + 1];           // units of layer l (the last entry: n_out)
  const float* images;
  const int* labels;
  const int* idx;                        // [batch]
  const float* w[kMdMaxHidden + 1];      // layer l: [n_prev, width[l]]
  const float* b[kMdMaxHidden + 1];
  const float* vw[kMdMaxHidden + 1];     // the tangent u, same shapes
  const float* vb[kMdMaxHidden + 1];
  float* ow[kMdMaxHidden + 1];           // out = H u, same shapes
  float* ob[kMdMaxHidden + 1];
  float* acts;                           // [nh][batch][32]      a_l
  float* racts;                          // [nh][batch][32]      Ra_l
  float* deltas;                         // [nh + 1][batch][32]  d_l  (already / batch)
  float* rdeltas;                        // [nh + 1][batch][32]  Rd_l
};

__global__ __launch_bounds__(kMdThreads) void k_mlp_hvp_sample(MlpHvpArgs a) {
  __shared__ float xs[kMdMaxIn];
  __shared__ float part[8][kMdMaxWidth], rpart[8][kMdMaxWidth];
  __shared__ float act[kMdMaxHidden + 1][kMdMaxWidth], ract[kMdMaxHidden + 1][kMdMaxWidth];   // a_l, Ra_l (last: z_L, Rz_L)
  __shared__ float rz[kMdMaxHidden + 1][kMdMaxWidth];
  __shared__ float dl[kMdMaxHidden + 1][kMdMaxWidth], rdl[kMdMaxHidden + 1][kMdMaxWidth];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int row = a.idx[s];
  const int L = a.nh, sig = a.act == 0;
  for (int k = tid; k < a.n_in; k += kMdThreads) xs[k] = a.images[(size_t)row * a.n_in + k];
  __syncthreads();
  // layer 0: thread = (unit h, k-slice p): k = p, p + 8, ... ascending, then the eight slices in order (k_mlp_deep_sample's)
  {
    const int h = tid & 31, p = tid >> 5, H = a.width[0];
    float acc = 0.0f, racc = 0.0f;
    if (h < H)
      for (int k = p; k < a.n_in; k += 8) {
        const float x = xs[k];
        acc = __builtin_fmaf(x, a.w[0][(size_t)k * H + h], acc);
        racc = __builtin_fmaf(x, a.vw[0][(size_t)k * H + h], racc);
      }
    part[p][h] = acc;
    rpart[p][h] = racc;
    __syncthreads();
    if (tid < H) {
      float z = a.b[0][tid], r = a.vb[0][tid];
      for (int q = 0; q < 8; ++q) { z += part[q][tid]; r += rpart[q][tid]; }
      const float hv = sig ? sigmoidf_(z) : fmaxf(z, 0.0f);       // (nh >= 1: layer 0 is a hidden layer)
      rz[0][tid] = r;
      act[0][tid] = hv;
      ract[0][tid] = sig ? hv * (1.0f - hv) * r : (hv > 0.0f ? r : 0.0f);
    }
    __syncthreads();
  }
  for (int l = 1; l <= L; ++l) {
    const int Hp = a.width[l - 1], H = a.width[l];
    if (tid < H) {
      float z = a.b[l][tid], r = a.vb[l][tid];
      for (int k = 0; k < Hp; ++k) {
        const float wk = a.w[l][k * H + tid];
        z = __builtin_fmaf(act[l - 1][k], wk, z);
        r = __builtin_fmaf(ract[l - 1][k], wk, r);
        r = __builtin_fmaf(act[l - 1][k], a.vw[l][k * H + tid], r);
      }
      rz[l][tid] = r;
      if (l == L) { act[l][tid] = z; ract[l][tid] = r; }
      else {
        const float hv = sig ? sigmoidf_(z) : fmaxf(z, 0.0f);
        act[l][tid] = hv;
        ract[l][tid] = sig ? hv * (1.0f - hv) * r : (hv > 0.0f ? r : 0.0f);
      }
    }
    __syncthreads();
  }
  // the logits: d_L = (softmax - onehot) / B and its tangent
  const int O = a.n_out;
  const float invB = 1.0f / (float)a.batch;
  if (tid == 0) {
    const int lab = a.labels[row];
    float zmax = act[L][0];
    for (int o = 1; o < O; ++o) zmax = fmaxf(zmax, act[L][o]);
    float se = 0.0f;
    for (int o = 0; o < O; ++o) se += expf(act[L][o] - zmax);
    const float lse = zmax + logf(se);
    float pr = 0.0f;                                         // sum_o p_o Rz_o
    for (int o = 0; o < O; ++o) {
      const float p = expf(act[L][o] - lse);
      part[0][o] = p;
      pr = __builtin_fmaf(p, rz[L][o], pr);
    }
    for (int o = 0; o < O; ++o) {
      const float p = part[0][o];
      dl[L][o] = (p - (o == lab ? 1.0f : 0.0f)) * invB;
      rdl[L][o] = p * (rz[L][o] - pr) * invB;
    }
  }
  __syncthreads();
  for (int l = L - 1; l >= 0; --l) {
    const int H = a.width[l], Hn = a.width[l + 1];
    if (tid < H) {
      float back = 0.0f, rb = 0.0f;
      for (int o = 0; o < Hn; ++o) {
        const float wo = a.w[l + 1][tid * Hn + o];
        back = __builtin_fmaf(dl[l + 1][o], wo, back);
        rb = __builtin_fmaf(rdl[l + 1][o], wo, rb);
        rb = __builtin_fmaf(dl[l + 1][o], a.vw[l + 1][tid * Hn + o], rb);
      }
      const float hv = act[l][tid];
      if (sig) {
        const float d1 = hv * (1.0f - hv);
        dl[l][tid] = back * d1;
        rdl[l][tid] = __builtin_fmaf(rb, d1, back * (d1 * (1.0f - 2.0f * hv)) * rz[l][tid]);
      } else {
        dl[l][tid] = hv > 0.0f ? back : 0.0f;
        rdl[l][tid] = hv > 0.0f ? rb : 0.0f;
      }
    }
    __syncthreads();
  }
  for (int l = 0; l <= L; ++l)
    if (tid < a.width[l]) {
      const size_t at = ((size_t)l * a.batch + s) * kMdMaxWidth + tid;
      a.deltas[at] = dl[l][tid];
      a.rdeltas[at] = rdl[l][tid];
      if (l < L) { a.acts[at] = act[l][tid]; a.racts[at] = ract[l][tid]; }
    }
}

constexpr int kMhInFlight = 8;           // samples whose loads one thread of k_mlp_hvp_reduce issues before it adds them

__global__ __launch_bounds__(kMdThreads) void k_mlp_hvp_reduce(MlpHvpArgs a) {
  long i = (long)blockIdx.x * kMdThreads + threadIdx.x;
  const int B = a.batch;
  for (int l = 0; l <= a.nh; ++l) {
    const int np = l == 0 ? a.n_in : a.width[l - 1], H = a.width[l];
    const long nw = (long)np * H;
    const float* d = a.deltas + (size_t)l * B * kMdMaxWidth;
    const float* rd = a.rdeltas + (size_t)l * B * kMdMaxWidth;
    if (i < nw) {
      const int k = (int)(i / H), h = (int)(i - (long)k * H);
      double g = 0.0;
      if (l == 0) {                                          // the image has no tangent: x^T Rd_0
        int s = 0;
        for (; s + kMhInFlight <= B; s += kMhInFlight) {
          float x[kMhInFlight], r[kMhInFlight];
#pragma unroll
          for (int j = 0; j < kMhInFlight; ++j) {
            x[j] = a.images[(size_t)a.idx[s + j] * a.n_in + k];
            r[j] = rd[(size_t)(s + j) * kMdMaxWidth + h];
          }
#pragma unroll
          for (int j = 0; j < kMhInFlight; ++j) g = __builtin_fma((double)x[j], (double)r[j], g);
        }
        for (; s < B; ++s)
          g = __builtin_fma((double)a.images[(size_t)a.idx[s] * a.n_in + k], (double)rd[(size_t)s * kMdMaxWidth + h], g);
      } else {
        const float* ap = a.acts + (size_t)(l - 1) * B * kMdMaxWidth;
        const float* rap = a.racts + (size_t)(l - 1) * B * kMdMaxWidth;
        int s = 0;
        for (; s + kMhInFlight <= B; s += kMhInFlight) {
          float x[kMhInFlight], rx[kMhInFlight], dd[kMhInFlight], r[kMhInFlight];
#pragma unroll
          for (int j = 0; j < kMhInFlight; ++j) {
            x[j] = ap[(size_t)(s + j) * kMdMaxWidth + k];
            rx[j] = rap[(size_t)(s + j) * kMdMaxWidth + k];
            dd[j] = d[(size_t)(s + j) * kMdMaxWidth + h];
            r[j] = rd[(size_t)(s + j) * kMdMaxWidth + h];
          }
#pragma unroll
          for (int j = 0; j < kMhInFlight; ++j) {
            g = __builtin_fma((double)rx[j], (double)dd[j], g);
            g = __builtin_fma((double)x[j], (double)r[j], g);
          }
        }
        for (; s < B; ++s) {
          g = __builtin_fma((double)rap[(size_t)s * kMdMaxWidth + k], (double)d[(size_t)s * kMdMaxWidth + h], g);
          g = __builtin_fma((double)ap[(size_t)s * kMdMaxWidth + k], (double)rd[(size_t)s * kMdMaxWidth + h], g);
        }
      }
      a.ow[l][i] = (float)g;
      return;
    }
    i -= nw;
    if (i < H) {
      double g = 0.0;
      int s = 0;
      for (; s + kMhInFlight <= B; s += kMhInFlight) {
        float r[kMhInFlight];
#pragma unroll
        for (int j = 0; j < kMhInFlight; ++j) r[j] = rd[(size_t)(s + j) * kMdMaxWidth + (int)i];
#pragma unroll
        for (int j = 0; j < kMhInFlight; ++j) g += (double)r[j];
      }
      for (; s < B; ++s) g += (double)rd[(size_t)s * kMdMaxWidth + (int)i];
      a.ob[l][i] = (float)g;
      return;
    }
    i -= H;
  }
}

}  // namespace l2o
