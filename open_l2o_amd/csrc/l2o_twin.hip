// l2o_twin.hip -- one translation unit of libl2o_hip.so: the Twin-L2O entry points of include/l2o_twin_abi.h -- descriptor
// checks, the weight re-pack and the one launch of k_twin_unroll (l2o_twin.h) -- and the meta-training entry points of
// include/l2o_twin_train_abi.h: the recording forward, the BPTT and the weight-gradient contraction of one segment
// (l2o_twin_train.h).  Written for gfx950 only.
#include "l2o_host.h"
#include "l2o_twin_train.h"
#include "../../include/l2o_twin_abi.h"
#include "../../include/l2o_twin_train_abi.h"

static bool twin_net_ok(const l2o_twin_net* n) {
  return n && n->hidden >= 1 && n->hidden <= L2O_TWIN_MAX_HIDDEN && (n->n_in == 1 || n->n_in == 2);
}
static bool twin_ok(const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p) {
  if (!twin_net_ok(mn) || !twin_net_ok(mx) || !p || p->flags != 0 || p->n_inst < 1) return false;
  if (p->kind < L2O_TWIN_SADDLE || p->kind > L2O_TWIN_MATRIX_GAME) return false;
  if (p->dim < 1 || p->dim > L2O_TWIN_MAX_DIM) return false;
  return p->kind == L2O_TWIN_MATRIX_GAME || p->dim == 1;
}
static bool twin_net_has_weights(const l2o_twin_net* n) {
  return n->w_ih1 && n->w_hh1 && n->b_ih1 && n->b_hh1 && n->w_ih2 && n->w_hh2 && n->b_ih2 && n->b_hh2 && n->w_out && n->b_out;
}
static int twin_pack(const l2o_twin_net* n, float* out, hipStream_t s) {
  TwPackParams pp;
  pp.H = n->hidden; pp.n_in = n->n_in;
  pp.w_ih1 = n->w_ih1; pp.w_hh1 = n->w_hh1; pp.b_ih1 = n->b_ih1; pp.b_hh1 = n->b_hh1;
  pp.w_ih2 = n->w_ih2; pp.w_hh2 = n->w_hh2; pp.b_ih2 = n->b_ih2; pp.b_hh2 = n->b_hh2;
  pp.w_out = n->w_out; pp.b_out = n->b_out; pp.out = out;
  const int blocks = (tw_pack_floats(pp.H) + 255) / 256;
  hipLaunchKernelGGL(k_twin_pack, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, pp);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

extern "C" {

int l2o_twin_supported(const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p) {
  return twin_ok(mn, mx, p) ? 1 : 0;
}
size_t l2o_twin_state_floats(const l2o_twin_net* net, int64_t rows) {
  if (!twin_net_ok(net) || rows < 1) return 0;
  return 4 * (size_t)net->hidden * (size_t)rows;
}

}  // extern "C"

// The checks of l2o_twin_unroll and its launch; hist: NULL (k_twin_unroll) or the history k_twin_record fills.
static int twin_forward(const char* who, const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p,
                        const l2o_twin_run* run, float* theta, float* state_min, float* state_max, float* curve, float* fval,
                        float* delta, float* hist, long rec_stride, void* stream) {
  if (!twin_ok(mn, mx, p))
    return fail(L2O_ERR_UNSUPPORTED, "%s: hidden in [1, %d], n_in 1 or 2, kinds 1-4, dim in [1, %d] (1 for kinds "
                "1-3), flags 0, n_inst >= 1", who, L2O_TWIN_MAX_HIDDEN, L2O_TWIN_MAX_DIM);
  if (!run || run->n_iter < 0) return fail(L2O_ERR_UNSUPPORTED, "%s: n_iter >= 0", who);
  if (run->iter0 < 1 || run->n_sign < 0 || (long long)run->iter0 + run->n_iter > 0x7fffffffLL)
    return fail(L2O_ERR_ARG, "%s: iter0 >= 1, n_sign >= 0", who);
  if (!twin_net_has_weights(mn) || !twin_net_has_weights(mx)) return fail(L2O_ERR_ARG, "%s: NULL weights", who);
  if (!p->data || !theta || !state_min || !state_max) return fail(L2O_ERR_ARG, "%s: NULL argument", who);
  if (run->n_sign >= run->iter0 && !run->sign_lr) return fail(L2O_ERR_ARG, "%s: the sign rule needs sign_lr", who);
  if (run->n_iter == 0) return L2O_OK;
  hipStream_t s = (hipStream_t)stream;
  TwParams kp;
  std::memset(&kp, 0, sizeof(kp));
  const l2o_twin_net* nets[2] = {mn, mx};
  float* states[2] = {state_min, state_max};
  size_t pack_floats = 0;
  for (int n = 0; n < 2; ++n) pack_floats += (size_t)tw_pack_floats(nets[n]->hidden);
  float* pack = nullptr;
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&pack), sizeof(float) * pack_floats, s));
  float* at = pack;
  int rc = L2O_OK;
  for (int n = 0; n < 2 && rc == L2O_OK; ++n) {
    TwNetParams& np = kp.net[n];
    np.H = nets[n]->hidden; np.nt = tw_nt(np.H); np.ntp = tw_ntp(np.H); np.n_in = nets[n]->n_in;
    np.pack = at; np.state = states[n];
    rc = twin_pack(nets[n], at, s);
    at += tw_pack_floats(np.H);
  }
  if (rc == L2O_OK) {
    kp.kind = p->kind; kp.n_inst = p->n_inst; kp.dim = p->dim; kp.ipt = 16 / p->dim;
    kp.iter0 = run->iter0; kp.n_iter = run->n_iter; kp.n_sign = run->n_sign;
    kp.rescale = run->rescale; kp.out_mul = run->out_mul; kp.sign_lr = run->sign_lr;
    kp.data = p->data; kp.theta = theta; kp.curve = curve; kp.fval = fval; kp.delta = delta;
    const int tiles = (p->n_inst + kp.ipt - 1) / kp.ipt;
    const size_t lds = sizeof(float) * (size_t)tw_lds_floats(kp);
    if (hist) rc = launch(k_twin_record, dim3((unsigned)tiles), dim3(kTwThreads), lds, s, kp, hist, rec_stride);
    else rc = launch(k_twin_unroll, dim3((unsigned)tiles), dim3(kTwThreads), lds, s, kp);
  }
  const hipError_t e = hipFreeAsync(pack, s);
  if (rc == L2O_OK && e != hipSuccess) return fail(L2O_ERR_HIP, "hipFreeAsync: %s", hipGetErrorString(e));
  return rc;
}

// ---- meta-training: the work buffer is [tiles][n_iter] records, then [tiles][n_iter] backward scratch
static int twin_tiles(const l2o_twin_problem* p) { const int ipt = 16 / p->dim; return (p->n_inst + ipt - 1) / ipt; }
static int twin_nt_max(const l2o_twin_net* mn, const l2o_twin_net* mx) {
  return tw_nt(mn->hidden > mx->hidden ? mn->hidden : mx->hidden);
}
static bool twin_segment_ok(const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p, long long iter0,
                            long long n_iter) {
  return twin_ok(mn, mx, p) && (iter0 & 1) && iter0 >= 1 && !(n_iter & 1) && n_iter >= 2 && n_iter <= L2O_TWIN_TRAIN_MAX_ITER;
}
static int twin_segment_check(const char* who, const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p,
                              const l2o_twin_segment* seg, const float* work) {
  if (!seg || !twin_segment_ok(mn, mx, p, seg->run.iter0, seg->run.n_iter))
    return fail(L2O_ERR_UNSUPPORTED, "%s: what l2o_twin_unroll accepts, iter0 odd, n_iter even in [2, %d]", who,
                L2O_TWIN_TRAIN_MAX_ITER);
  if (!twin_net_has_weights(mn) || !twin_net_has_weights(mx)) return fail(L2O_ERR_ARG, "%s: NULL weights", who);
  if (!work || ((uintptr_t)work & 15)) return fail(L2O_ERR_ARG, "%s: work is NULL or not 16-byte aligned", who);
  return L2O_OK;
}

extern "C" {

int l2o_twin_unroll(const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p, const l2o_twin_run* run,
                    float* theta, float* state_min, float* state_max, float* curve, float* fval, float* delta,
                    void* stream) {
  return twin_forward("l2o_twin_unroll", mn, mx, p, run, theta, state_min, state_max, curve, fval, delta, nullptr, 0, stream);
}

size_t l2o_twin_train_floats(const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p, int32_t n_iter) {
  if (!twin_segment_ok(mn, mx, p, 1, n_iter)) return 0;
  const int ntm = twin_nt_max(mn, mx);
  return (size_t)twin_tiles(p) * (size_t)n_iter * (size_t)(tw_rec_floats(ntm) + tw_dz_floats(ntm));
}

int l2o_twin_train_forward(const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p,
                           const l2o_twin_segment* seg, float* theta, float* state_min, float* state_max, float* curve,
                           float* fval, float* delta, float* work, void* stream) {
  const int rc = twin_segment_check("l2o_twin_train_forward", mn, mx, p, seg, work);
  if (rc != L2O_OK) return rc;
  return twin_forward("l2o_twin_train_forward", mn, mx, p, &seg->run, theta, state_min, state_max, curve, fval, delta, work,
                      tw_rec_floats(twin_nt_max(mn, mx)), stream);
}

int l2o_twin_train_backward(const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p,
                            const l2o_twin_segment* seg, float* work, const l2o_twin_grad* grad_min,
                            const l2o_twin_grad* grad_max, void* stream) {
  int rc = twin_segment_check("l2o_twin_train_backward", mn, mx, p, seg, work);
  if (rc != L2O_OK) return rc;
  const l2o_twin_grad* grads[2] = {grad_min, grad_max};
  for (int n = 0; n < 2; ++n) {
    const l2o_twin_grad* g = grads[n];
    if (!g || !g->w_ih1 || !g->w_hh1 || !g->b_ih1 || !g->b_hh1 || !g->w_ih2 || !g->w_hh2 || !g->b_ih2 || !g->b_hh2 ||
        !g->w_out || !g->b_out)
      return fail(L2O_ERR_ARG, "l2o_twin_train_backward: NULL gradient");
  }
  if (!p->data) return fail(L2O_ERR_ARG, "l2o_twin_train_backward: NULL argument");
  hipStream_t s = (hipStream_t)stream;
  const l2o_twin_net* nets[2] = {mn, mx};
  const int tiles = twin_tiles(p), ntm = twin_nt_max(mn, mx), n_iter = seg->run.n_iter;
  TwBpParams bp;
  TwWgParams wp;
  std::memset(&bp, 0, sizeof(bp));
  std::memset(&wp, 0, sizeof(wp));
  float* packt = nullptr;
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&packt),
                         sizeof(float) * ((size_t)tw_packt_floats(mn->hidden) + (size_t)tw_packt_floats(mx->hidden)), s));
  float* at = packt;
  for (int n = 0; n < 2; ++n) {
    const int H = nets[n]->hidden;
    TwPackTParams pp;
    pp.H = H; pp.w_hh1 = nets[n]->w_hh1; pp.w_ih2 = nets[n]->w_ih2; pp.w_hh2 = nets[n]->w_hh2; pp.out = at;
    const int blocks = (tw_packt_floats(H) + 255) / 256;
    hipLaunchKernelGGL(k_twin_pack_t, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, pp);
    TwBpNet& b = bp.net[n];
    b.H = H; b.nt = tw_nt(H); b.ntp = tw_ntp(H); b.n_in = nets[n]->n_in; b.packt = at; b.w_out = nets[n]->w_out;
    TwWgNet& w = wp.net[n];
    const l2o_twin_grad* g = grads[n];
    w.H = H; w.nt = tw_nt(H); w.n_in = nets[n]->n_in;
    w.w_ih1 = g->w_ih1; w.w_hh1 = g->w_hh1; w.b_ih1 = g->b_ih1; w.b_hh1 = g->b_hh1;
    w.w_ih2 = g->w_ih2; w.w_hh2 = g->w_hh2; w.b_ih2 = g->b_ih2; w.b_hh2 = g->b_hh2; w.w_out = g->w_out; w.b_out = g->b_out;
    at += tw_packt_floats(H);
  }
  bp.kind = p->kind; bp.n_inst = p->n_inst; bp.dim = p->dim; bp.ipt = 16 / p->dim;
  bp.iter0 = seg->run.iter0; bp.n_iter = n_iter; bp.n_sign = seg->run.n_sign;
  bp.rescale = seg->run.rescale; bp.out_mul = seg->run.out_mul; bp.loss_scale = seg->loss_scale;
  bp.data = p->data; bp.inst_weight = seg->inst_weight;
  bp.hist = work; bp.rec_stride = tw_rec_floats(ntm);
  bp.dz = work + (size_t)tiles * (size_t)n_iter * (size_t)tw_rec_floats(ntm); bp.dz_stride = tw_dz_floats(ntm);
  wp.tiles = tiles; wp.iter0 = bp.iter0; wp.n_iter = n_iter; wp.rescale = bp.rescale;
  wp.hist = bp.hist; wp.rec_stride = bp.rec_stride; wp.dz = bp.dz; wp.dz_stride = bp.dz_stride;
  rc = hipGetLastError() == hipSuccess ? L2O_OK : fail(L2O_ERR_HIP, "l2o_twin_train_backward: k_twin_pack_t launch");
  if (rc == L2O_OK) rc = launch(k_twin_bptt, dim3(2u * (unsigned)tiles), dim3(kTwThreads), 0, s, bp);
  if (rc == L2O_OK)
    rc = launch(k_twin_wgrad, dim3((unsigned)(tw_wg_jobs(mn->hidden) + tw_wg_jobs(mx->hidden))), dim3(64), 0, s, wp);
  const hipError_t e = hipFreeAsync(packt, s);
  if (rc == L2O_OK && e != hipSuccess) return fail(L2O_ERR_HIP, "hipFreeAsync: %s", hipGetErrorString(e));
  return rc;
}

}  // extern "C"
