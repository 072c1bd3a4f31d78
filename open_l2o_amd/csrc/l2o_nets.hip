// l2o_nets.hip -- the image-net optimizees of the C ABI: loss and gradient of one minibatch of problems.mnist_conv,
// problems.cifar10, problems.LeNet (include/l2o_abi.h), problems.vgg16_cifar10 (include/l2o_vgg16_abi.h) and problems.NAS
// (include/l2o_nas_abi.h).  This unit owns the kernels of l2o_mnist_conv.h, l2o_cifar_conv.h, l2o_lenet.h, l2o_vgg16.h and
// l2o_nas.h (the four batch-norm nets share the reductions of l2o_conv_bn.h).  Written for gfx950 only.
#include "l2o_host.h"
#include "l2o_mnist_conv.h"
#include "l2o_cifar_conv.h"
#include "l2o_lenet.h"
#include "l2o_vgg16.h"
#include "l2o_nas.h"

extern "C" {

// ---- problems.mnist_conv (csrc/l2o_mnist_conv.h) ----------------------------------------------------------------------
static bool mnist_conv_ok(const l2o_mnist_conv* m) {
  return m && m->batch >= 2 && m->batch <= kCvMaxBatch && m->n_data >= 1 && (m->batch_norm == 0 || m->batch_norm == 1);
}
static size_t mnist_conv_per_sample() {
  return (size_t)2 * kCvZ1 + 2 * kCvA1 + 2 * kCvZ2 + kCvNF + 16 + 1 + 2 * kCvC1 * 2 + 2 * kCvC2 * 2 + kCvPW2 + kCvPW1;
}
size_t l2o_mnist_conv_scratch_floats(const l2o_mnist_conv* m) {
  if (!mnist_conv_ok(m)) return 0;
  return (size_t)m->batch * mnist_conv_per_sample() + 2 * (kCvC1 + kCvC2);
}
int l2o_mnist_conv_fg(const l2o_mnist_conv* m, const int32_t* indices, const float* const* w, float* loss, float* const* g,
                      float* scratch, void* stream) {
  if (!mnist_conv_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mnist_conv_fg: batch in [2, %d], batch_norm 0 or 1, n_data >= 1", kCvMaxBatch);
  if (!indices || !w || !loss || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_mnist_conv_fg: NULL argument");
  const int bn = m->batch_norm, nv = bn ? 10 : 6;
  for (int k = 0; k < nv; ++k)
    if (!w[k] || (g && !g[k])) return fail(L2O_ERR_ARG, "l2o_mnist_conv_fg: NULL buffer of variable %d", k);
  MnistConvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.batch = m->batch; a.bn = bn; a.want_grad = g ? 1 : 0;
  a.images = m->images; a.labels = m->labels; a.idx = indices;
  // variable order of the reference's graph: conv_layer1/{weights1, biases1}, [batch_normalization/{gamma, beta}],
  // conv_layer2/{weights1, biases1}, [batch_normalization_1/{gamma, beta}], fc_weights, fc_bias
  const int k2 = bn ? 4 : 2, kf = bn ? 8 : 4;
  a.w1 = w[0]; a.b1 = w[1]; a.w2 = w[k2]; a.b2 = w[k2 + 1]; a.wf = w[kf]; a.bf = w[kf + 1];
  if (bn) { a.g1 = w[2]; a.be1 = w[3]; a.g2 = w[6]; a.be2 = w[7]; }
  if (g) {
    a.gw1 = g[0]; a.gb1 = g[1]; a.gw2 = g[k2]; a.gb2 = g[k2 + 1]; a.gwf = g[kf]; a.gbf = g[kf + 1];
    if (bn) { a.gg1 = g[2]; a.gbe1 = g[3]; a.gg2 = g[6]; a.gbe2 = g[7]; }
  }
  const size_t B = (size_t)a.batch;
  float* p = scratch;
  a.z1 = p; p += B * kCvZ1;
  a.d1 = p; p += B * kCvZ1;
  a.p1 = p; p += B * kCvA1;
  a.am1 = reinterpret_cast<int*>(p); p += B * kCvA1;
  a.z2 = p; p += B * kCvZ2;
  a.d2 = p; p += B * kCvZ2;
  a.f = p; p += B * kCvNF;
  a.dlog = p; p += B * 16;
  a.loss_s = p; p += B;
  a.st1 = p; p += B * kCvC1 * 2;
  a.bw1 = p; p += B * kCvC1 * 2;
  a.st2 = p; p += B * kCvC2 * 2;
  a.bw2 = p; p += B * kCvC2 * 2;
  a.pw2 = p; p += B * kCvPW2;
  a.pw1 = p; p += B * kCvPW1;
  a.stat = p;
  a.loss = loss;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(a.batch), blk(kCvThreads);
  hipLaunchKernelGGL(k_cv_conv1, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_cv_conv2, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_cv_head, grid, blk, 0, s, a);
  if (g) {
    hipLaunchKernelGGL(k_cv_mid, grid, blk, 0, s, a);
    hipLaunchKernelGGL(k_cv_first, grid, blk, 0, s, a);
  }
  const long nthreads = g ? kCvGradThreads : 1;
  hipLaunchKernelGGL(k_cv_grad, dim3((unsigned)((nthreads + kCvThreads - 1) / kCvThreads)), blk, 0, s, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- problems.cifar10 (csrc/l2o_cifar_conv.h) -------------------------------------------------------------------------
static bool cifar_conv_ok(const l2o_cifar_conv* m) {
  return m && m->batch >= 2 && m->batch <= kCcMaxBatch && m->n_data >= 1 && (m->batch_norm == 0 || m->batch_norm == 1);
}
static size_t cifar_conv_per_sample() {
  return (size_t)2 * kCcZ1 + 2 * kCcA1 + 3 * kCcZ2 + kCcNF + 16 + 1 + 2 * kCcC1 * 2 + 2 * kCcC2 * 2 + kCcPW1;
}
size_t l2o_cifar_conv_scratch_floats(const l2o_cifar_conv* m) {
  if (!cifar_conv_ok(m)) return 0;
  return (size_t)m->batch * cifar_conv_per_sample() + 2 * (kCcC1 + kCcC2);
}
int l2o_cifar_conv_fg(const l2o_cifar_conv* m, const int32_t* indices, const float* const* w, float* loss, float* const* g,
                      float* scratch, void* stream) {
  if (!cifar_conv_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_cifar_conv_fg: batch in [2, %d], batch_norm 0 or 1, n_data >= 1", kCcMaxBatch);
  if (!indices || !w || !loss || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_cifar_conv_fg: NULL argument");
  const int bn = m->batch_norm, nv = bn ? 10 : 6;
  for (int k = 0; k < nv; ++k)
    if (!w[k] || (g && !g[k])) return fail(L2O_ERR_ARG, "l2o_cifar_conv_fg: NULL buffer of variable %d", k);
  CifarConvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.batch = m->batch; a.bn = bn; a.want_grad = g ? 1 : 0;
  a.images = m->images; a.labels = m->labels; a.idx = indices;
  // variable order of the reference's graph: conv_layer1/{weights1, biases1}, [batch_normalization/{gamma, beta}],
  // conv_layer2/{weights1, biases1}, [batch_normalization_1/{gamma, beta}], fc_weights, fc_bias
  const int k2 = bn ? 4 : 2, kf = bn ? 8 : 4;
  a.w1 = w[0]; a.b1 = w[1]; a.w2 = w[k2]; a.b2 = w[k2 + 1]; a.wf = w[kf]; a.bf = w[kf + 1];
  if (bn) { a.g1 = w[2]; a.be1 = w[3]; a.g2 = w[6]; a.be2 = w[7]; }
  if (g) {
    a.gw1 = g[0]; a.gb1 = g[1]; a.gw2 = g[k2]; a.gb2 = g[k2 + 1]; a.gwf = g[kf]; a.gbf = g[kf + 1];
    if (bn) { a.gg1 = g[2]; a.gbe1 = g[3]; a.gg2 = g[6]; a.gbe2 = g[7]; }
  }
  const size_t B = (size_t)a.batch;
  float* p = scratch;
  a.z1 = p; p += B * kCcZ1;
  a.d1 = p; p += B * kCcZ1;
  a.p1 = p; p += B * kCcA1;
  a.am1 = reinterpret_cast<int*>(p); p += B * kCcA1;
  a.z2 = p; p += B * kCcZ2;
  a.d2 = p; p += B * kCcZ2;
  a.dz2 = p; p += B * kCcZ2;
  a.f = p; p += B * kCcNF;
  a.dlog = p; p += B * 16;
  a.loss_s = p; p += B;
  a.st1 = p; p += B * kCcC1 * 2;
  a.bw1 = p; p += B * kCcC1 * 2;
  a.st2 = p; p += B * kCcC2 * 2;
  a.bw2 = p; p += B * kCcC2 * 2;
  a.pw1 = p; p += B * kCcPW1;
  a.stat = p;
  a.loss = loss;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(a.batch), blk(kCcThreads);
  hipLaunchKernelGGL(k_cc_conv1, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_cc_conv2, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_cc_head, dim3((a.batch + kCcHeadSamples - 1) / kCcHeadSamples), blk, 0, s, a);
  if (g) {
    hipLaunchKernelGGL(k_cc_mid, grid, blk, 0, s, a);
    hipLaunchKernelGGL(k_cc_first, grid, blk, 0, s, a);
  }
  const long nthreads = g ? kCcGradThreads : 1;
  const unsigned nblocks = (unsigned)((nthreads + kCcThreads - 1) / kCcThreads) + (g ? kCcW2Blocks : 0);
  hipLaunchKernelGGL(k_cc_grad, dim3(nblocks), blk, 0, s, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- problems.LeNet (csrc/l2o_lenet.h) --------------------------------------------------------------------------------
static bool lenet_ok(const l2o_lenet* m) {
  return m && m->batch >= 2 && m->batch <= kLnMaxBatch && m->n_data >= 1 && (m->batch_norm == 0 || m->batch_norm == 1);
}
// every per-sample region is a multiple of 4 floats (the kernels read some of them as float4); loss_s and stat come last
static size_t lenet_per_sample() {
  return (size_t)2 * kLnZ1 + 2 * kLnA1 + 2 * kLnZ2 + 2 * kLnF + 3 * kLnN1 + 3 * kLnN2 + 16 + 2 * kLnC1 * 2 + 2 * kLnC2 * 2 +
         kLnPW1 + kLnPW2 + 1;
}
size_t l2o_lenet_scratch_floats(const l2o_lenet* m) {
  if (!lenet_ok(m)) return 0;
  return (size_t)m->batch * lenet_per_sample() + kLnStat;
}
int l2o_lenet_fg(const l2o_lenet* m, const int32_t* indices, const float* const* w, float* loss, float* const* g,
                 float* scratch, void* stream) {
  if (!lenet_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_lenet_fg: batch in [2, %d], batch_norm 0 or 1, n_data >= 1", kLnMaxBatch);
  if (!indices || !w || !loss || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_lenet_fg: NULL argument");
  if ((uintptr_t)scratch & 15) return fail(L2O_ERR_ARG, "l2o_lenet_fg: scratch must be 16-byte aligned");
  const int bn = m->batch_norm, nv = bn ? 14 : 10;
  for (int k = 0; k < nv; ++k)
    if (!w[k] || (g && !g[k])) return fail(L2O_ERR_ARG, "l2o_lenet_fg: NULL buffer of variable %d", k);
  LenetArgs a;
  std::memset(&a, 0, sizeof(a));
  a.batch = m->batch; a.bn = bn; a.want_grad = g ? 1 : 0;
  a.images = m->images; a.labels = m->labels; a.idx = indices;
  // variable order of the reference's graph: conv_2d_0/{w, b}, [batch_norm_0/beta], conv_2d_1/{w, b}, [batch_norm_1/beta],
  // linear_0/{w, b}, [mlp/batch_norm/beta], linear_1/{w, b}, [mlp/batch_norm_1/beta], linear_2/{w, b}
  const int st = bn ? 3 : 2, k2 = st, k3 = 2 * st, k4 = 3 * st, k5 = 4 * st;
  a.w1 = w[0]; a.b1 = w[1]; a.w2 = w[k2]; a.b2 = w[k2 + 1]; a.wl0 = w[k3]; a.bl0 = w[k3 + 1]; a.wl1 = w[k4]; a.bl1 = w[k4 + 1];
  a.wl2 = w[k5]; a.bl2 = w[k5 + 1];
  if (bn) { a.be1 = w[2]; a.be2 = w[5]; a.bel0 = w[8]; a.bel1 = w[11]; }
  if (g) {
    a.gw1 = g[0]; a.gb1 = g[1]; a.gw2 = g[k2]; a.gb2 = g[k2 + 1]; a.gwl0 = g[k3]; a.gbl0 = g[k3 + 1]; a.gwl1 = g[k4];
    a.gbl1 = g[k4 + 1]; a.gwl2 = g[k5]; a.gbl2 = g[k5 + 1];
    if (bn) { a.gbe1 = g[2]; a.gbe2 = g[5]; a.gbel0 = g[8]; a.gbel1 = g[11]; }
  }
  const size_t B = (size_t)a.batch;
  float* p = scratch;
  a.z1 = p; p += B * kLnZ1;
  a.d1 = p; p += B * kLnZ1;
  a.p1 = p; p += B * kLnA1;
  a.am1 = reinterpret_cast<int*>(p); p += B * kLnA1;
  a.z2 = p; p += B * kLnZ2;
  a.d2 = p; p += B * kLnZ2;
  a.f = p; p += B * kLnF;
  a.am2 = reinterpret_cast<int*>(p); p += B * kLnF;
  a.h1 = p; p += B * kLnN1;
  a.a1 = p; p += B * kLnN1;
  a.dh1 = p; p += B * kLnN1;
  a.h2 = p; p += B * kLnN2;
  a.a2 = p; p += B * kLnN2;
  a.dh2 = p; p += B * kLnN2;
  a.dlog = p; p += B * 16;
  a.st1 = p; p += B * kLnC1 * 2;
  a.bw1 = p; p += B * kLnC1 * 2;
  a.st2 = p; p += B * kLnC2 * 2;
  a.bw2 = p; p += B * kLnC2 * 2;
  a.pw1 = p; p += B * kLnPW1;
  a.pw2 = p; p += B * kLnPW2;
  a.loss_s = p; p += B;
  a.stat = p;
  a.loss = loss;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(a.batch), blk(kLnThreads);
  hipLaunchKernelGGL(k_ln_conv1, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_ln_conv2, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_ln_pool2, grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_ln_fc<0>, dim3(kLnN1 / kLnU), blk, 0, s, a);
  hipLaunchKernelGGL(k_ln_fc<1>, dim3(kLnN2 / kLnU), blk, 0, s, a);
  hipLaunchKernelGGL(k_ln_out, dim3((a.batch + kLnOutSamples - 1) / kLnOutSamples), blk, 0, s, a);
  if (g) {
    hipLaunchKernelGGL(k_ln_fcb<1>, dim3(kLnN2 / kLnU), blk, 0, s, a);
    hipLaunchKernelGGL(k_ln_fcb<0>, dim3(kLnN1 / kLnU), blk, 0, s, a);
    hipLaunchKernelGGL(k_ln_mid, grid, blk, 0, s, a);
    hipLaunchKernelGGL(k_ln_mid2, grid, blk, 0, s, a);
    hipLaunchKernelGGL(k_ln_first, grid, blk, 0, s, a);
  }
  const long nthreads = g ? kLnGradThreads : 1;
  hipLaunchKernelGGL(k_ln_grad, dim3((unsigned)((nthreads + kLnThreads - 1) / kLnThreads)), blk, 0, s, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- problems.vgg16_cifar10 (csrc/l2o_vgg16.h, include/l2o_vgg16_abi.h) -------------------------------------------------
static bool vgg16_ok(const l2o_vgg16* m) {
  if (!m || m->batch < 2 || m->batch > kVgMaxBatch || m->n_data < 1) return false;
  for (int b = 0; b < 5; ++b)
    if (m->channels[b] < 8 || m->channels[b] > 512 || m->channels[b] % 8) return false;
  return true;
}
// The scratch of one call, in floats from its start: the gathered images, the output of every conv layer and of pools 1-4,
// pool 5's output, dz, the per-sample losses, two gradient buffers of the largest activation and the weight-gradient
// partials.  Every size is a multiple of 4 floats.
struct VgScratch {
  size_t x0, act[kVgLayers], pool[4], pooled, dz, loss_s, grad[2], part, total;
};
static VgScratch vgg16_scratch(const l2o_vgg16* m, const VgLayer* L) {
  VgScratch s;
  const size_t B = (size_t)m->batch;
  size_t p = 0, gmax = 0, pmax = 0;
  auto take = [&](size_t n) { const size_t at = p; p += (n + 3) & ~(size_t)3; return at; };
  s.x0 = take(B * 3072);
  int np = 0;
  for (int l = 0; l < kVgLayers; ++l) {
    const size_t n = (B << (2 * L[l].lw)) * L[l].cout;
    s.act[l] = take(n);
    if (L[l].pool && l != kVgLayers - 1) s.pool[np++] = take(n / 4);
    if (n > gmax) gmax = n;
    int per;
    const size_t pn = (size_t)vg_wgrad_splits(m->batch, L[l], &per) * (9 * L[l].cin + 1) * L[l].cout;
    if (pn > pmax) pmax = pn;
  }
  s.pooled = take(B * m->channels[4]);
  s.dz = take(B * 16);
  s.loss_s = take(B);
  s.grad[0] = take(gmax);
  s.grad[1] = take(gmax);
  s.part = take(pmax);
  s.total = p;
  return s;
}
size_t l2o_vgg16_scratch_floats(const l2o_vgg16* m) {
  if (!vgg16_ok(m)) return 0;
  VgLayer L[kVgLayers];
  vg_plan(m->channels, L);
  return vgg16_scratch(m, L).total;
}
int l2o_vgg16_fg(const l2o_vgg16* m, const int32_t* indices, const float* const* w, float* loss, float* const* g,
                 float* scratch, void* stream) {
  if (!vgg16_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_vgg16_fg: batch in [2, %d], channels multiples of 8 in [8, 512], n_data >= 1",
                kVgMaxBatch);
  if (!indices || !w || !loss || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_vgg16_fg: NULL argument");
  if ((uintptr_t)scratch & 15) return fail(L2O_ERR_ARG, "l2o_vgg16_fg: scratch must be 16-byte aligned");
  for (int k = 0; k < L2O_VGG16_VARS; ++k)
    if (!w[k] || (g && !g[k])) return fail(L2O_ERR_ARG, "l2o_vgg16_fg: NULL buffer of variable %d", k);
  VgLayer L[kVgLayers];
  vg_plan(m->channels, L);
  const VgScratch sc = vgg16_scratch(m, L);
  hipStream_t s = (hipStream_t)stream;
  const int B = m->batch;
  const dim3 blk(kVgThreads);
  auto blocks = [](size_t n) { return dim3((unsigned)((n + kVgThreads - 1) / kVgThreads)); };
  auto tiles = [](int n, int t) { return (unsigned)((n + t - 1) / t); };
  // ---- forward
  hipLaunchKernelGGL(k_vg_gather, dim3(B), blk, 0, s, m->images, indices, m->n_data, scratch + sc.x0);
  const float* in[kVgLayers];                  // the input of every conv layer
  const float* x = scratch + sc.x0;
  int np = 0;
  for (int l = 0; l < kVgLayers; ++l) {
    const int M = B << (2 * L[l].lw);
    in[l] = x;
    VgGemm a{x, w[2 * l], w[2 * l + 1], scratch + sc.act[l], M, L[l].lw, L[l].cin, L[l].cout, 0};
    hipLaunchKernelGGL(k_vg_gemm<VG_FWD>, dim3(tiles(M, kVgBM), tiles(L[l].cout, kVgBN)), blk, 0, s, a);
    x = scratch + sc.act[l];
    if (L[l].pool && l != kVgLayers - 1) {
      const size_t total = (size_t)(M / 4) * L[l].cout;
      hipLaunchKernelGGL(k_vg_pool, blocks(total), blk, 0, s, x, scratch + sc.pool[np], L[l].lw, L[l].cout, total);
      x = scratch + sc.pool[np++];
    }
  }
  float* dy = scratch + sc.grad[0];            // gradient w.r.t. the pre-activation of the layer in hand
  float* other = scratch + sc.grad[1];
  VgHead h;
  std::memset(&h, 0, sizeof(h));
  h.a13 = scratch + sc.act[kVgLayers - 1]; h.wfc = w[26]; h.bfc = w[27]; h.labels = m->labels; h.idx = indices;
  h.pooled = scratch + sc.pooled; h.dz = scratch + sc.dz; h.loss_s = scratch + sc.loss_s; h.dy13 = g ? dy : nullptr;
  h.loss = loss; h.gwfc = g ? g[26] : nullptr; h.gbfc = g ? g[27] : nullptr;
  h.B = B; h.C = m->channels[4]; h.n_data = m->n_data;
  hipLaunchKernelGGL(k_vg_head, dim3(B), dim3(64), 0, s, h);
  hipLaunchKernelGGL(k_vg_head_sum, dim3(g ? 1 + tiles(h.C * kVgClasses + kVgClasses, kVgThreads) : 1), blk, 0, s, h);
  // ---- backward: per layer the weight (and bias) gradient, then the gradient w.r.t. its input, masked by the ReLU of the
  // layer below -- directly, or on the way back through the pool between them
  for (int l = kVgLayers - 1; g && l >= 0; --l) {
    const int M = B << (2 * L[l].lw), K9 = 9 * L[l].cin;
    int per;
    const int splits = vg_wgrad_splits(B, L[l], &per);
    VgGemm a{in[l], dy, nullptr, scratch + sc.part, M, L[l].lw, L[l].cin, L[l].cout, per};
    hipLaunchKernelGGL(k_vg_gemm<VG_WGRAD>, dim3(tiles(K9, kVgBM), tiles(L[l].cout, kVgBN), splits), blk, 0, s, a);
    hipLaunchKernelGGL(k_vg_wsum, blocks((size_t)(K9 + 1) * L[l].cout), blk, 0, s, scratch + sc.part, splits,
                       K9 * L[l].cout, L[l].cout, g[2 * l], g[2 * l + 1]);
    if (l == 0) break;
    const bool pooled_input = L[l - 1].pool != 0;
    VgGemm d{dy, w[2 * l], pooled_input ? nullptr : in[l], other, M, L[l].lw, L[l].cin, L[l].cout, 0};
    hipLaunchKernelGGL(k_vg_gemm<VG_DGRAD>, dim3(tiles(M, kVgBM), tiles(L[l].cin, kVgBN)), blk, 0, s, d);
    if (pooled_input) {
      const size_t total = (size_t)M * L[l].cin;
      hipLaunchKernelGGL(k_vg_pool_bwd, blocks(total), blk, 0, s, scratch + sc.act[l - 1], other, dy, L[l - 1].lw, L[l].cin,
                         total);
    } else {
      std::swap(dy, other);
    }
  }
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- problems.NAS (csrc/l2o_nas.h, include/l2o_nas_abi.h) ----------------------------------------------------------------
static bool nas_ok(const l2o_nas* m) {
  return m && m->batch >= 2 && m->batch <= kNsMaxBatch && m->n_data >= 1 && m->flags == 0 &&
         (m->batch_norm == 0 || m->batch_norm == 1);
}
// The scratch of one call, in floats from its start (include/l2o_nas_abi.h has the formula).  Every size is a multiple of
// 4 floats.
struct NsScratch {
  size_t x0, z0, zz, z13, dy1, dy0, P, stat, bsum, nf, dlog, v, loss_s, part, total;
};
static NsScratch nas_scratch(int batch) {
  NsScratch s;
  const size_t B = (size_t)batch, M = B * kNsPix;
  size_t p = 0;
  auto take = [&](size_t n) { const size_t at = p; p += (n + 3) & ~(size_t)3; return at; };
  s.x0 = take(B * 3072);
  s.z0 = take(M * 16);
  s.zz = take(M * 32);
  s.z13 = take(M * 16);
  s.dy1 = take(M * 16);
  s.dy0 = take(M * 16);
  s.P = take(kNsLayers * kNsP);
  s.stat = take(B * 64);
  s.bsum = take(B * 64);
  s.nf = take(B * 16);
  s.dlog = take(B * 16);
  s.v = take(B * 16);
  s.loss_s = take(B);
  s.part = take((size_t)ns_wgrad_groups(batch) * kNsWPart);
  s.total = p;
  return s;
}
size_t l2o_nas_scratch_floats(const l2o_nas* m) { return nas_ok(m) ? nas_scratch(m->batch).total : 0; }
int l2o_nas_fg(const l2o_nas* m, const int32_t* indices, const float* const* w, float* loss, float* const* g, float* scratch,
               void* stream) {
  if (!nas_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_nas_fg: batch in [2, %d], batch_norm 0 or 1, flags 0, n_data >= 1", kNsMaxBatch);
  if (!indices || !w || !loss || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_nas_fg: NULL argument");
  if ((uintptr_t)scratch & 15) return fail(L2O_ERR_ARG, "l2o_nas_fg: scratch must be 16-byte aligned");
  const int bn = m->batch_norm, per = bn ? 4 : 2, nvars = kNsLayers * per + 2;
  for (int k = 0; k < nvars; ++k)
    if (!w[k] || (g && !g[k])) return fail(L2O_ERR_ARG, "l2o_nas_fg: NULL buffer of variable %d", k);
  const NsScratch sc = nas_scratch(m->batch);
  hipStream_t s = (hipStream_t)stream;
  const int B = m->batch;
  const dim3 blk(kNsThreads), strips(4 * B), samples(B), one(1);
  float* x0 = scratch + sc.x0;
  float* z0 = scratch + sc.z0;
  float* zz = scratch + sc.zz;           // [M][32]: n02 in columns 0-15, node1 in 16-31
  float* z13 = scratch + sc.z13;
  float* dy1 = scratch + sc.dy1;
  float* dy0 = scratch + sc.dy0;
  float* P = scratch + sc.P;
  float* v = scratch + sc.v;
  // layer l (node0, n02, node1, n13): its variables
  auto W = [&](int l) { return w[l * per]; };
  auto Bi = [&](int l) { return w[l * per + 1]; };
  auto src = [](const float* z, int ldz, const float* dy, const float* Pl) { NsSrc r{z, dy, Pl, ldz}; return r; };
  const NsSrc none = src(nullptr, 0, nullptr, nullptr);
  // batch norm of layers l .. l + C / 16 - 1 whose z is the [M][C] array `z`
  auto norm = [&](const float* z, int l, int C) {
    if (!bn) return;
    NsBn a{scratch + sc.stat, {w[l * per + 2], C == 32 ? w[(l + 1) * per + 2] : nullptr},
           {w[l * per + 3], C == 32 ? w[(l + 1) * per + 3] : nullptr}, P + l * kNsP, B};
    if (C == 32) {
      hipLaunchKernelGGL(k_ns_stats<32>, samples, blk, 0, s, z, scratch + sc.stat);
      hipLaunchKernelGGL(k_ns_bn<32>, one, blk, 0, s, a);
    } else {
      hipLaunchKernelGGL(k_ns_stats<16>, samples, blk, 0, s, z, scratch + sc.stat);
      hipLaunchKernelGGL(k_ns_bn<16>, one, blk, 0, s, a);
    }
  };
  // ---- forward
  hipLaunchKernelGGL(k_vg_gather, samples, dim3(kVgThreads), 0, s, m->images, indices, m->n_data, x0);
  if (!bn) hipLaunchKernelGGL(k_ns_identity, one, blk, 0, s, P);
  {
    NsConv a{{src(x0, 3, nullptr, nullptr), none}, v, {W(0), nullptr}, {Bi(0), nullptr}, z0, nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL((k_ns_conv<3, 16, NS_RAW>), strips, blk, 0, s, a);
    norm(z0, 0, 16);
  }
  {
    NsConv a{{src(z0, 16, nullptr, P), none}, v, {W(1), W(2)}, {Bi(1), Bi(2)}, zz, nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL((k_ns_conv<16, 32, NS_ACT>), strips, blk, 0, s, a);
    norm(zz, 1, 32);
  }
  {
    NsConv a{{src(zz + 16, 32, nullptr, P + 2 * kNsP), none}, v, {W(3), nullptr}, {Bi(3), nullptr}, z13, nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL((k_ns_conv<16, 16, NS_ACT>), strips, blk, 0, s, a);
    norm(z13, 3, 16);
  }
  NsHead h;
  std::memset(&h, 0, sizeof(h));
  h.z0 = z0; h.zz = zz; h.z13 = z13; h.P = P; h.wfc = w[nvars - 2]; h.bfc = w[nvars - 1]; h.labels = m->labels; h.idx = indices;
  h.nf = scratch + sc.nf; h.dlog = scratch + sc.dlog; h.v = v; h.loss_s = scratch + sc.loss_s; h.loss = loss;
  h.gwfc = g ? g[nvars - 2] : nullptr; h.gbfc = g ? g[nvars - 1] : nullptr; h.B = B; h.n_data = m->n_data;
  hipLaunchKernelGGL(k_ns_head, samples, blk, 0, s, h);
  hipLaunchKernelGGL(k_ns_head_sum, one, blk, 0, s, h);
  if (g) {
    // ---- backward.  The sums of a layer (or of n02 and node1 together): the two means of its NsP block(s) and the
    // gradients of gamma, beta and the bias
    auto sums = [&](const NsSrc& s0, const NsSrc& s1, int l, int C) {
      NsBwd a;
      std::memset(&a, 0, sizeof(a));
      a.src[0] = s0; a.src[1] = s1; a.v = v; a.part = scratch + sc.bsum; a.P = P + l * kNsP; a.B = B; a.bn = bn;
      for (int i = 0; i < C / 16; ++i) {
        a.gbias[i] = g[(l + i) * per + 1];
        if (bn) { a.ggamma[i] = g[(l + i) * per + 2]; a.gbeta[i] = g[(l + i) * per + 3]; }
      }
      if (C == 32) {
        hipLaunchKernelGGL(k_ns_bwd_sums<32>, samples, blk, 0, s, a);
        hipLaunchKernelGGL(k_ns_bwd_fin<32>, one, blk, 0, s, a);
      } else {
        hipLaunchKernelGGL(k_ns_bwd_sums<16>, samples, blk, 0, s, a);
        hipLaunchKernelGGL(k_ns_bwd_fin<16>, one, blk, 0, s, a);
      }
    };
    const int groups = ns_wgrad_groups(B);
    float* part = scratch + sc.part;
    auto wsum = [&](int K, int NOUT, float* g0, float* g1) {
      hipLaunchKernelGGL(k_ns_wsum, dim3((K * NOUT + kNsWsE - 1) / kNsWsE), blk, 0, s, part, groups, K, NOUT, g0, g1);
    };
    const NsSrc d13 = src(z13, 16, nullptr, P + 3 * kNsP);           // dy = u / 1024 under n13's mask
    const NsSrc d02 = src(zz, 32, nullptr, P + 1 * kNsP);
    const NsSrc d1 = src(zz + 16, 32, dy1, P + 2 * kNsP);
    const NsSrc d0 = src(z0, 16, dy0, P);
    // n13
    sums(d13, none, 3, 16);
    {
      NsWgrad a{src(zz + 16, 32, nullptr, P + 2 * kNsP), {d13, none}, v, part, 4 * B};
      hipLaunchKernelGGL((k_ns_wgrad<16, 16>), dim3(groups), blk, 0, s, a);
      wsum(144, 16, g[3 * per], g[3 * per]);
      NsConv c{{d13, none}, v, {W(3), nullptr}, {nullptr, nullptr}, dy1, zz + 16, P + 2 * kNsP, 32, 1};
      hipLaunchKernelGGL((k_ns_conv<16, 16, NS_DZ>), strips, blk, 0, s, c);
    }
    // n02 and node1
    sums(d02, d1, 1, 32);
    {
      NsWgrad a{src(z0, 16, nullptr, P), {d02, d1}, v, part, 4 * B};
      hipLaunchKernelGGL((k_ns_wgrad<16, 32>), dim3(groups), blk, 0, s, a);
      wsum(144, 32, g[1 * per], g[2 * per]);
      NsConv c{{d02, d1}, v, {W(1), W(2)}, {nullptr, nullptr}, dy0, z0, P, 16, 0};
      hipLaunchKernelGGL((k_ns_conv<32, 16, NS_DZ>), strips, blk, 0, s, c);
    }
    // node0
    sums(d0, none, 0, 16);
    {
      NsWgrad a{src(x0, 3, nullptr, nullptr), {d0, none}, v, part, 4 * B};
      hipLaunchKernelGGL((k_ns_wgrad<3, 16>), dim3(groups), blk, 0, s, a);
      wsum(27, 16, g[0], g[0]);
    }
  }
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

}  // extern "C"
