// l2o_twin.hip -- one translation unit of libl2o_hip.so: the Twin-L2O entry points of include/l2o_twin_abi.h -- descriptor
// checks, the weight re-pack and the one launch of k_twin_unroll (l2o_twin.h).  Written for gfx950 only.
#include "l2o_host.h"
#include "l2o_twin.h"
#include "../../include/l2o_twin_abi.h"

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

int l2o_twin_unroll(const l2o_twin_net* mn, const l2o_twin_net* mx, const l2o_twin_problem* p, const l2o_twin_run* run,
                    float* theta, float* state_min, float* state_max, float* curve, float* fval, float* delta,
                    void* stream) {
  if (!twin_ok(mn, mx, p))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_twin_unroll: hidden in [1, %d], n_in 1 or 2, kinds 1-4, dim in [1, %d] (1 for kinds "
                "1-3), flags 0, n_inst >= 1", L2O_TWIN_MAX_HIDDEN, L2O_TWIN_MAX_DIM);
  if (!run || run->n_iter < 0) return fail(L2O_ERR_UNSUPPORTED, "l2o_twin_unroll: n_iter >= 0");
  if (run->iter0 < 1 || run->n_sign < 0 || (long long)run->iter0 + run->n_iter > 0x7fffffffLL)
    return fail(L2O_ERR_ARG, "l2o_twin_unroll: iter0 >= 1, n_sign >= 0");
  if (!twin_net_has_weights(mn) || !twin_net_has_weights(mx)) return fail(L2O_ERR_ARG, "l2o_twin_unroll: NULL weights");
  if (!p->data || !theta || !state_min || !state_max) return fail(L2O_ERR_ARG, "l2o_twin_unroll: NULL argument");
  if (run->n_sign >= run->iter0 && !run->sign_lr) return fail(L2O_ERR_ARG, "l2o_twin_unroll: the sign rule needs sign_lr");
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
    rc = launch(k_twin_unroll, dim3((unsigned)tiles), dim3(kTwThreads), sizeof(float) * (size_t)tw_lds_floats(kp), s, kp);
  }
  const hipError_t e = hipFreeAsync(pack, s);
  if (rc == L2O_OK && e != hipSuccess) return fail(L2O_ERR_HIP, "hipFreeAsync: %s", hipGetErrorString(e));
  return rc;
}

}  // extern "C"
