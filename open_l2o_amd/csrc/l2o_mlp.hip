// l2o_mlp.hip -- the MNIST MLP optimizee of the C ABI of include/l2o_abi.h: its loss and gradient (l2o_mlp_fg; with several
// hidden layers l2o_mlp_deep_fg), its Hessian-vector product (l2o_mlp_hvp, include/l2o_mlp_hvp_abi.h) and the fused
// persistent unrolls (l2o_mlp_unroll*: one instance over the whole chip; l2o_mlp_unroll_multi*: one instance per XCD).
// This unit owns the kernels of l2o_mlp.h, l2o_mlp_unroll.h, l2o_mlp_xcd.h, l2o_mlp_deep.h and l2o_mlp_hvp.h.
// Written for gfx950 only.
#include "l2o_host.h"
#include "l2o_mlp.h"
#include "l2o_mlp_unroll.h"
#include "l2o_mlp_xcd.h"
#include "l2o_mlp_deep.h"
#include "l2o_mlp_hvp.h"

extern "C" {

int l2o_mlp_fg(const l2o_mlp* mlp, const int32_t* indices, const float* w1, const float* b1, const float* w2,
               const float* b2, float* loss, float* gw1, float* gb1, float* gw2, float* gb2, float* scratch,
               void* stream) {
  OptScope opt_scope((mlp && (mlp->flags & L2O_MLP_GENERIC)) ? L2O_OPTW(L2O_OPT_MLP_GENERIC, 1) : 0);
  if (!mlp || !indices || !w1 || !b1 || !w2 || !b2 || !loss || !mlp->images || !mlp->labels)
    return fail(L2O_ERR_ARG, "l2o_mlp_fg: NULL argument");
  const bool want_g = gw1 || gb1 || gw2 || gb2;
  if (want_g && !(gw1 && gb1 && gw2 && gb2)) return fail(L2O_ERR_ARG, "l2o_mlp_fg: pass all four gradients or none");
  if (mlp->n_hidden < 1 || mlp->n_hidden > kMlpMaxH || mlp->n_out < 1 || mlp->n_out > kMlpMaxO ||
      mlp->batch < 1 || mlp->batch > 256 || mlp->n_in < 1 || mlp->n_in > kMlpTPS * kMlpKPT)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_fg: sizes n_in=%d hidden=%d out=%d batch=%d not implemented",
                mlp->n_in, mlp->n_hidden, mlp->n_out, mlp->batch);
  if (!scratch) return fail(L2O_ERR_ARG, "l2o_mlp_fg: NULL scratch (l2o_mlp_scratch_floats)");
  MlpParams p;
  p.n_in = mlp->n_in; p.H = mlp->n_hidden; p.O = mlp->n_out; p.batch = mlp->batch; p.act = mlp->activation;
  p.images = mlp->images; p.labels = mlp->labels; p.idx = indices;
  p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2; p.loss = loss;
  p.gw1 = gw1; p.gb1 = gb1; p.gw2 = gw2; p.gb2 = gb2;
  p.scratch = scratch;
  hipStream_t s = (hipStream_t)stream;
  const int HP = p.H == 20 ? 20 : kMlpMaxH;             // padded hidden width of the kernels' hot loops
  const int HS = HP | 1;
  const size_t lds_f = sizeof(float) * ((HP == 20 ? 0 : (size_t)p.n_in * HS) + (size_t)kMlpSPB * kMlpTPS * HP + (size_t)kMlpSPB * p.H +
                                        (size_t)kMlpSPB * p.O + (size_t)p.H * p.O + p.H + p.O);
  size_t lds_b = sizeof(float) * ((size_t)p.batch * HP + (size_t)p.batch + 4 * (size_t)kMlpKPB * HP);
  const size_t lds_small = sizeof(float) * (size_t)p.batch * (2 * p.H + p.O + 1);   // the small-tensor workgroup's copy of scratch
  if (lds_small > lds_b) lds_b = lds_small;
  if (lds_f > 160 * 1024 || lds_b > 160 * 1024)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_fg: needs %zu / %zu bytes of LDS", lds_f, lds_b);
  if (p.H == kMlp20 && !opt(L2O_OPT_MLP_GENERIC)) {       // the reference's width: barrier-free forward, scalar-operand backward
    hipLaunchKernelGGL(k_mlp_fwd20, dim3(p.batch), dim3(64), 0, s, p);
    HIP_TRY(hipGetLastError());
    const int nkb20 = (p.n_in + 63) / 64;
    size_t lds20 = sizeof(float) * (size_t)kMlpBwdWaves * 64 * (kMlp20 + 1);
    if (lds_small > lds20) lds20 = lds_small;
    return launch(k_mlp_bwd20, dim3(nkb20 + 1), dim3(64 * kMlpBwdWaves), lds20, s, p);
  }
  void (*ffwd)(MlpParams) = HP == 20 ? k_mlp_fwd<20> : k_mlp_fwd<kMlpMaxH>;
  void (*fbwd)(MlpParams) = HP == 20 ? k_mlp_bwd<20> : k_mlp_bwd<kMlpMaxH>;
  const int rc = launch(ffwd, dim3((p.batch + kMlpSPB - 1) / kMlpSPB), dim3(256), lds_f, s, p);
  if (rc) return rc;
  const int nkb = (p.n_in + kMlpKPB - 1) / kMlpKPB;
  return launch(fbwd, dim3(nkb + 1), dim3(256), lds_b, s, p);
}

size_t l2o_mlp_scratch_floats(const l2o_mlp* mlp) {
  if (!mlp || mlp->batch < 1) return 0;
  return (size_t)mlp->batch * (2 * (size_t)mlp->n_hidden + mlp->n_out + 1);
}

// ---- the fused persistent unroll of the MLP optimizee (csrc/l2o_mlp_unroll.h) ---------------------------
struct MlpUnrollLayout { int n[4], tile_begin[5], nwg, nw1, R, hier_R1; bool fast; size_t NO, NSM, p_off, s_off, sm_off, hs_off, x_off, s1_off, total; };
static bool mlp_unroll_layout(const l2o_mlp* mlp, MlpUnrollLayout* L) {
  if (!mlp) return false;
  const int H = mlp->n_hidden, O = mlp->n_out;
  if (H < kMuMinH || H > kMuMaxH || O < 1 || O > kMuMaxO || mlp->batch < 1 || mlp->batch > kMuMaxBatch || mlp->n_in < 1)
    return false;
  L->n[0] = mlp->n_in * H; L->n[1] = H; L->n[2] = H * O; L->n[3] = O;
  if (L->n[0] % 64) return false;                        // the w1 coordinates fill whole workgroups
  L->tile_begin[0] = 0;
  for (int v = 0; v < 4; ++v) L->tile_begin[v + 1] = L->tile_begin[v] + tiles_per_problem(L->n[v]);
  L->nwg = (L->tile_begin[4] + 3) / 4;
  L->nw1 = L->n[0] / 64;
  L->NO = (size_t)mlp->batch * H;
  L->NSM = (size_t)H + (size_t)H * O + O;
  L->R = (int)((L->NO + L->nwg - 1) / L->nwg);
  L->R = (L->R + 1) & ~1;                                // even: the fast path moves granules in pairs
  // one 64-byte line per (source, reducer): R = 8 measured best (profiles/archive_r01_r03/r02l: R = 6 / 8 / 12 / 16 -> 1.32 / 1.35 /
  // 1.28 / 1.24 G on config 5)
  if (L->R < 8 && L->NO >= 8 * 32) L->R = 8;
  if (L->R > kMuMaxR) return false;
  L->fast = H == 20 && O == 10 && mlp->batch == 64;
  L->p_off = sizeof(MlpWs);
  // XCD-hierarchical all-reduce (fast path; l2o_mlp_unroll.h): group g = wg % 8, every group needs enough w1 owners to
  // reduce all NO outputs in slices of R1 (even) <= kMuHierR1Max
  L->hier_R1 = 0;
  if (L->fast && opt(L2O_OPT_MLP_HIER) && L->nwg <= 256 && L->nw1 >= 2 * kMuHierG && (L->nwg + kMuHierG - 1) / kMuHierG <= kMuHierM) {
    const int min_cnt = L->nw1 / kMuHierG;                 // the smallest group
    int r1 = (int)((L->NO + min_cnt - 1) / min_cnt);
    r1 = (r1 + 1) & ~1;
    if (r1 <= kMuHierR1Max) L->hier_R1 = r1;
  }
  // P: generic [nw1][NO]; fast path: one inbox per reducing workgroup, [nwg][nw1][R]; hierarchical: [8][M][M][R1]
  const size_t pg = (size_t)L->nw1 * L->NO, pf = (size_t)L->nwg * L->nw1 * L->R;
  const size_t ph = L->hier_R1 ? (size_t)kMuHierG * kMuHierM * kMuHierM * L->hier_R1 : 0;
  size_t pmax = pg > pf ? pg : pf;
  if (ph > pmax) pmax = ph;
  L->s_off = L->p_off + sizeof(unsigned long long) * pmax;
  L->sm_off = L->s_off + sizeof(unsigned long long) * 2 * L->NO;
  L->hs_off = L->sm_off + sizeof(unsigned long long) * 2 * ((L->NSM + 1) & ~(size_t)1);
  L->x_off = L->hs_off + sizeof(unsigned long long) * 256;
  L->s1_off = L->x_off + sizeof(unsigned long long) * 2 * kMuHierG * kMuHierM * kMuHierR1Max;
  L->total = L->s1_off + sizeof(unsigned long long) * 2 * kMuHierG * kMuHierS;
  return true;
}

int l2o_mlp_unroll_supported(const l2o_net_cfg* cfg, const l2o_mlp* mlp, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  MlpUnrollLayout L;
  if (!cfg || !net_ok_for_mfma(cfg) || !opt(L2O_OPT_MLP_UNROLL) || !mlp_unroll_layout(mlp, &L)) return 0;
  if (L.nwg > coresident_cus((hipStream_t)stream)) return 0;     // one workgroup per CU, all co-resident
  return L.fast ? 2 : 1;                                           // 2: the reference's shape (static loop bounds, paired granules)
}

size_t l2o_mlp_unroll_workspace_bytes(const l2o_mlp* mlp) {
  MlpUnrollLayout L;
  return mlp_unroll_layout(mlp, &L) ? L.total : 0;
}

static int mlp_unroll_launch(const l2o_net_cfg* cfg, const float* wpack, const l2o_mlp* mlp, const int32_t* indices,
                             float* const* x, float* const* st, float* const* m, float* const* v,
                             const float* const* x_scale, int32_t T, int32_t step0, float* fx, const l2o_mlp_hist* hist,
                             void* workspace, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !wpack || !mlp || !indices || !x || !st || !fx || !workspace || T < 0 || !mlp->images || !mlp->labels)
    return fail(L2O_ERR_ARG, "l2o_mlp_unroll: bad argument");
  hipStream_t s = (hipStream_t)stream;
  MlpUnrollLayout L;
  if (!net_ok_for_mfma(cfg) || !mlp_unroll_layout(mlp, &L) || L.nwg > coresident_cus(s))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_unroll: no fused kernel for n_in=%d hidden=%d out=%d batch=%d net(layers=%d)",
                mlp->n_in, mlp->n_hidden, mlp->n_out, mlp->batch, cfg->n_layers);
  const bool rn = cfg->preprocess == L2O_PRE_FC_ELU;
  MlpUnrollArgs a;
  std::memset(&a, 0, sizeof(a));
  a.np = make_net_params(cfg, wpack);
  a.n_in = mlp->n_in; a.H = mlp->n_hidden; a.O = mlp->n_out; a.batch = mlp->batch; a.act = mlp->activation;
  a.images = mlp->images; a.labels = mlp->labels; a.idx = indices;
  for (int k = 0; k < 4; ++k) {
    if (!x[k] || !st[k] || (rn && (!m || !v || !m[k] || !v[k]))) return fail(L2O_ERR_ARG, "l2o_mlp_unroll: NULL buffer of variable %d", k);
    a.x[k] = x[k]; a.st[k] = st[k]; a.m[k] = rn ? m[k] : nullptr; a.v[k] = rn ? v[k] : nullptr;
    a.xscale[k] = x_scale ? x_scale[k] : nullptr;
    a.n[k] = L.n[k];
  }
  for (int k = 0; k < 5; ++k) a.tile_begin[k] = L.tile_begin[k];
  a.T = T;
  pow_ff(cfg->beta1, step0, &a.p1_hi, &a.p1_lo);
  pow_ff(cfg->beta2, step0, &a.p2_hi, &a.p2_lo);
  a.fx = fx;
  char* wsb = static_cast<char*>(workspace);
  a.ws = reinterpret_cast<MlpWs*>(wsb);
  a.P = reinterpret_cast<unsigned long long*>(wsb + L.p_off);
  a.S = reinterpret_cast<unsigned long long*>(wsb + L.s_off);
  a.Sm = reinterpret_cast<unsigned long long*>(wsb + L.sm_off);
  a.nwg = L.nwg; a.nw1 = L.nw1; a.R = L.R;
  a.hier_R1 = L.hier_R1;
  a.HS = reinterpret_cast<unsigned long long*>(wsb + L.hs_off);
  a.X = reinterpret_cast<unsigned long long*>(wsb + L.x_off);
  a.S1 = reinterpret_cast<unsigned long long*>(wsb + L.s1_off);
  a.use_salt = T + 1 < 0xffff ? 1u : 0u;
  if (hist) {
    for (int k = 0; k < 4; ++k) {
      if (!hist->st[k] || !hist->g[k] || (rn && (!hist->m[k] || !hist->v[k])))
        return fail(L2O_ERR_ARG, "l2o_mlp_unroll_record: NULL history buffer of variable %d", k);
      a.hist_st[k] = hist->st[k]; a.hist_g[k] = hist->g[k];
      a.hist_m[k] = rn ? hist->m[k] : nullptr; a.hist_v[k] = rn ? hist->v[k] : nullptr;
    }
  }
  HIP_TRY(hipMemsetAsync(wsb + L.p_off, 0, L.total - L.p_off, s));   // the granules only: the header survives
  const dim3 grid(L.nwg), block(256);
  void (*fn)(MlpUnrollArgs) = with_pre(cfg->preprocess, [&](auto pre) -> void (*)(MlpUnrollArgs) {
    constexpr int PRE = decltype(pre)::value;
    if (hist) return L.fast ? k_mlp_unroll<PRE, true, true> : k_mlp_unroll<PRE, false, true>;
    return L.fast ? k_mlp_unroll<PRE, true> : k_mlp_unroll<PRE, false>;
  });
  hipLaunchKernelGGL(fn, grid, block, 0, s, a);
  HIP_TRY(hipGetLastError());
  note_form(!L.fast ? L2O_FORM_MLP_UNROLL_GENERIC : (a.hier_R1 ? L2O_FORM_MLP_UNROLL_HIER : L2O_FORM_MLP_UNROLL));
  return L2O_OK;
}

int l2o_mlp_unroll(const l2o_net_cfg* cfg, const float* wpack, const l2o_mlp* mlp, const int32_t* indices,
                   float* const* x, float* const* st, float* const* m, float* const* v, const float* const* x_scale,
                   int32_t T, int32_t step0, float* fx, void* workspace, void* stream) {
  return mlp_unroll_launch(cfg, wpack, mlp, indices, x, st, m, v, x_scale, T, step0, fx, nullptr, workspace, stream);
}
int l2o_mlp_unroll_record(const l2o_net_cfg* cfg, const float* wpack, const l2o_mlp* mlp, const int32_t* indices,
                          float* const* x, float* const* st, float* const* m, float* const* v,
                          const float* const* x_scale, int32_t T, int32_t step0, float* fx, const l2o_mlp_hist* hist,
                          void* workspace, void* stream) {
  if (!hist) return fail(L2O_ERR_ARG, "l2o_mlp_unroll_record: NULL hist");
  return mlp_unroll_launch(cfg, wpack, mlp, indices, x, st, m, v, x_scale, T, step0, fx, hist, workspace, stream);
}

// ---- problems.mnist with several hidden layers (csrc/l2o_mlp_deep.h) ---------------------------------------------------
static bool mlp_deep_ok(const l2o_mlp_deep* m) {
  if (!m || m->n_hidden_layers < 1 || m->n_hidden_layers > kMdMaxHidden || m->n_in < 1 || m->n_in > kMdMaxIn) return false;
  if (m->n_out < 1 || m->n_out > kMdMaxOut || m->batch < 1 || m->batch > 4096) return false;
  for (int l = 0; l < m->n_hidden_layers; ++l)
    if (m->hidden[l] < 1 || m->hidden[l] > kMdMaxWidth) return false;
  return true;
}
size_t l2o_mlp_deep_scratch_floats(const l2o_mlp_deep* m) {
  if (!mlp_deep_ok(m)) return 0;
  return (size_t)m->batch * kMdMaxWidth * (2 * m->n_hidden_layers + 1) + m->batch;
}
int l2o_mlp_deep_fg(const l2o_mlp_deep* m, const int32_t* indices, const float* const* w, float* loss, float* const* g,
                    float* scratch, void* stream) {
  if (!mlp_deep_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_deep_fg: 1-3 hidden layers of <= 32 units, n_in <= 1024, n_out <= 16, batch <= 4096");
  if (!indices || !w || !loss || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_mlp_deep_fg: NULL argument");
  MlpDeepArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n_in = m->n_in; a.n_out = m->n_out; a.batch = m->batch; a.act = m->activation; a.nh = m->n_hidden_layers;
  for (int l = 0; l < a.nh; ++l) a.width[l] = m->hidden[l];
  a.width[a.nh] = m->n_out;
  a.images = m->images; a.labels = m->labels; a.idx = indices;
  long ncoord = 0;
  for (int l = 0; l <= a.nh; ++l) {
    if (!w[2 * l] || !w[2 * l + 1] || (g && (!g[2 * l] || !g[2 * l + 1]))) return fail(L2O_ERR_ARG, "l2o_mlp_deep_fg: NULL buffer of layer %d", l);
    a.w[l] = w[2 * l]; a.b[l] = w[2 * l + 1];
    if (g) { a.gw[l] = g[2 * l]; a.gb[l] = g[2 * l + 1]; }
    ncoord += (long)(l == 0 ? a.n_in : a.width[l - 1]) * a.width[l] + a.width[l];
  }
  a.acts = scratch;
  a.deltas = a.acts + (size_t)a.nh * a.batch * kMdMaxWidth;
  a.loss_s = a.deltas + (size_t)(a.nh + 1) * a.batch * kMdMaxWidth;
  a.loss = loss;
  a.want_grad = g ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mlp_deep_sample, dim3(a.batch), dim3(kMdThreads), 0, s, a);
  const long nthreads = g ? ncoord : 1;
  hipLaunchKernelGGL(k_mlp_deep_grad, dim3((unsigned)((nthreads + kMdThreads - 1) / kMdThreads)), dim3(kMdThreads), 0, s, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- second derivatives of problems.mnist: the Hessian-vector product (csrc/l2o_mlp_hvp.h, include/l2o_mlp_hvp_abi.h) ------
size_t l2o_mlp_hvp_scratch_floats(const l2o_mlp_deep* m) {
  if (!mlp_deep_ok(m)) return 0;
  return (size_t)m->batch * kMdMaxWidth * (4 * m->n_hidden_layers + 2);
}
int l2o_mlp_hvp(const l2o_mlp_deep* m, const int32_t* indices, const float* const* w, const float* const* u, float* const* out,
                float* scratch, void* stream) {
  if (!mlp_deep_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_hvp: 1-3 hidden layers of <= 32 units, n_in <= 1024, n_out <= 16, batch <= 4096");
  if (m->activation != 0 && m->activation != 1) return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_hvp: activation 0 (sigmoid) or 1 (relu)");
  if (!indices || !w || !u || !out || !scratch || !m->images || !m->labels) return fail(L2O_ERR_ARG, "l2o_mlp_hvp: NULL argument");
  MlpHvpArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n_in = m->n_in; a.n_out = m->n_out; a.batch = m->batch; a.act = m->activation; a.nh = m->n_hidden_layers;
  for (int l = 0; l < a.nh; ++l) a.width[l] = m->hidden[l];
  a.width[a.nh] = m->n_out;
  a.images = m->images; a.labels = m->labels; a.idx = indices;
  long ncoord = 0;
  for (int l = 0; l <= a.nh; ++l) {
    for (int q = 2 * l; q < 2 * l + 2; ++q)
      if (!w[q] || !u[q] || !out[q]) return fail(L2O_ERR_ARG, "l2o_mlp_hvp: NULL buffer of layer %d", l);
    a.w[l] = w[2 * l]; a.b[l] = w[2 * l + 1];
    a.vw[l] = u[2 * l]; a.vb[l] = u[2 * l + 1];
    a.ow[l] = out[2 * l]; a.ob[l] = out[2 * l + 1];
    ncoord += (long)(l == 0 ? a.n_in : a.width[l - 1]) * a.width[l] + a.width[l];
  }
  const size_t per = (size_t)a.batch * kMdMaxWidth;
  a.acts = scratch;
  a.racts = a.acts + (size_t)a.nh * per;
  a.deltas = a.racts + (size_t)a.nh * per;
  a.rdeltas = a.deltas + (size_t)(a.nh + 1) * per;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mlp_hvp_sample, dim3(a.batch), dim3(kMdThreads), 0, s, a);
  hipLaunchKernelGGL(k_mlp_hvp_reduce, dim3((unsigned)((ncoord + kMdThreads - 1) / kMdThreads)), dim3(kMdThreads), 0, s, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

#ifndef L2O_MLP_XCD_DEFAULT_FOUR
#define L2O_MLP_XCD_DEFAULT_FOUR 0     // (set from the A/B measurement: profiles/r06_c5_xcd_forms_ab.txt)
#endif
// ---- one optimizee instance per XCD (csrc/l2o_mlp_xcd.h) ------------------------------------------------------------
struct MlpXcdLayout { int n[4], tile_begin[5], nw1; size_t team_off, inst_off, p_bytes, s_bytes, sm_bytes, inst_bytes, total; };
static bool mlp_xcd_layout(const l2o_mlp* mlp, int n_inst, MlpXcdLayout* L) {
  if (!mlp || n_inst < 1 || n_inst > kMxMaxInst) return false;
  if (mlp->n_hidden != kMxH || mlp->n_out != kMxO || (mlp->batch != 64 && mlp->batch != 128) || mlp->n_in < 1) return false;
  const int NO = mlp->batch * kMxH;                   // MxShape<batch>::kNO
  L->n[0] = mlp->n_in * kMxH; L->n[1] = kMxH; L->n[2] = kMxH * kMxO; L->n[3] = kMxO;
  L->tile_begin[0] = 0;
  for (int v = 0; v < 4; ++v) L->tile_begin[v + 1] = L->tile_begin[v] + tiles_per_problem(L->n[v]);
  // members 0 .. 30: the w1 tiles (32 each); member 31: b1 | w2 | b2
  if (L->tile_begin[1] > (kMxMembers - 1) * kMxSlots || L->tile_begin[4] - L->tile_begin[1] > kMxSlots) return false;
  L->nw1 = (L->n[0] + kMxCoords - 1) / kMxCoords;
  L->team_off = sizeof(MlpWs);
  L->inst_off = L->team_off + 64;
  L->p_bytes = sizeof(unsigned long long) * kMxMembers * kMxMembers * (NO / kMxMembers);
  L->s_bytes = sizeof(unsigned long long) * 2 * NO;
  L->sm_bytes = sizeof(unsigned long long) * 2 * kMxNSMp;
  L->inst_bytes = (L->p_bytes + L->s_bytes + L->sm_bytes + 255) & ~(size_t)255;
  L->total = L->inst_off + (size_t)n_inst * L->inst_bytes;
  return true;
}

// the four-wave form (k_mlp_xcd<PRE, 4>): L2O_OPT_MLP_XCD_WAVES = 2, or the build's default for RNNProp
static bool mlp_xcd_four(const l2o_net_cfg* cfg) {
  const int wopt = (int)opt(L2O_OPT_MLP_XCD_WAVES);
  return wopt == 2 || (wopt == 0 && cfg->preprocess == L2O_PRE_FC_ELU && L2O_MLP_XCD_DEFAULT_FOUR);
}

int l2o_mlp_unroll_multi_supported(const l2o_net_cfg* cfg, const l2o_mlp* mlp, int32_t n_inst, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  MlpXcdLayout L;
  if (!cfg || !net_ok_for_mfma(cfg) || !opt(L2O_OPT_MLP_UNROLL) || !mlp_xcd_layout(mlp, n_inst, &L)) return 0;
  if (mlp->batch != 64 && mlp_xcd_four(cfg)) return 0;      // (the four-wave form has no batch-128 instantiation)
  // every XCD's 32 CUs must be able to host one workgroup each at the same time
  return coresident_cus((hipStream_t)stream) >= kMxMaxInst * kMxMembers ? 1 : 0;
}

size_t l2o_mlp_unroll_multi_workspace_bytes(const l2o_mlp* mlp, int32_t n_inst) {
  MlpXcdLayout L;
  return mlp_xcd_layout(mlp, n_inst, &L) ? L.total : 0;
}

static int mlp_unroll_multi_launch(const l2o_net_cfg* cfg, const float* wpack, const l2o_mlp* mlp, const l2o_mlp_instance* inst,
                                   int32_t n_inst, int32_t T, int32_t step0, const l2o_mlp_hist* hist, void* workspace, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !wpack || !mlp || !inst || !workspace || T < 0 || !mlp->images || !mlp->labels)
    return fail(L2O_ERR_ARG, "l2o_mlp_unroll_multi: bad argument");
  hipStream_t s = (hipStream_t)stream;
  MlpXcdLayout L;
  if (!net_ok_for_mfma(cfg) || !mlp_xcd_layout(mlp, n_inst, &L) || coresident_cus(s) < kMxMaxInst * kMxMembers)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_unroll_multi: no one-XCD kernel for n_in=%d hidden=%d out=%d batch=%d x %d instances "
                "(needs the reference's shape and all 8 x 32 CUs)", mlp->n_in, mlp->n_hidden, mlp->n_out, mlp->batch, (int)n_inst);
  // which form: four waves per member stepping tile PAIRS (a lone wave per SIMD with two independent chains; RNNProp: no
  // spills at 438 registers) or eight waves stepping single tiles (two waves per SIMD; the DM nets' pair form spills)
  const bool four = mlp_xcd_four(cfg);
  if (four && mlp->batch != 64)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_mlp_unroll_multi: the four-wave one-XCD form serves batch 64 only (batch %d)", mlp->batch);
  const bool rn = cfg->preprocess == L2O_PRE_FC_ELU;
  MlpXcdHistArgs a;                                   // (the plain form is launched with its MlpXcdArgs part)
  std::memset(&a, 0, sizeof(a));
  a.np = make_net_params(cfg, wpack);
  a.n_in = mlp->n_in; a.act = mlp->activation; a.T = T; a.ninst = n_inst;
  a.images = mlp->images; a.labels = mlp->labels;
  for (int k = 0; k < 4; ++k) a.n[k] = L.n[k];
  for (int k = 0; k < 5; ++k) a.tile_begin[k] = L.tile_begin[k];
  a.nw1 = L.nw1;
  pow_ff(cfg->beta1, step0, &a.p1_hi, &a.p1_lo);
  pow_ff(cfg->beta2, step0, &a.p2_hi, &a.p2_lo);
  char* wsb = static_cast<char*>(workspace);
  a.ws = reinterpret_cast<MlpWs*>(wsb);
  a.team = reinterpret_cast<unsigned*>(wsb + L.team_off);
  for (int j = 0; j < n_inst; ++j) {
    const l2o_mlp_instance& in = inst[j];
    MxInst& o = a.inst[j];
    if (!in.indices || !in.fx) return fail(L2O_ERR_ARG, "l2o_mlp_unroll_multi: NULL indices / fx of instance %d", j);
    o.idx = in.indices; o.fx = in.fx;
    for (int k = 0; k < 4; ++k) {
      if (!in.x[k] || !in.st[k] || (rn && (!in.m[k] || !in.v[k])))
        return fail(L2O_ERR_ARG, "l2o_mlp_unroll_multi: NULL buffer of variable %d of instance %d", k, j);
      o.x[k] = in.x[k]; o.st[k] = in.st[k]; o.m[k] = rn ? in.m[k] : nullptr; o.v[k] = rn ? in.v[k] : nullptr;
      o.xscale[k] = in.x_scale[k];
    }
    char* ib = wsb + L.inst_off + (size_t)j * L.inst_bytes;
    o.P = reinterpret_cast<unsigned long long*>(ib);
    o.S = reinterpret_cast<unsigned long long*>(ib + L.p_bytes);
    o.Sm = reinterpret_cast<unsigned long long*>(ib + L.p_bytes + L.s_bytes);
    if (hist) {
      const l2o_mlp_hist& h = hist[j];
      MxHist& oh = a.hist[j];
      for (int k = 0; k < 4; ++k) {
        if (!h.st[k] || !h.g[k] || (rn && (!h.m[k] || !h.v[k])))
          return fail(L2O_ERR_ARG, "l2o_mlp_unroll_multi_record: NULL history buffer of variable %d of instance %d", k, j);
        oh.st[k] = h.st[k]; oh.g[k] = h.g[k];
        oh.m[k] = rn ? h.m[k] : nullptr; oh.v[k] = rn ? h.v[k] : nullptr;
      }
    }
  }
  HIP_TRY(hipMemsetAsync(wsb + L.team_off, 0, L.total - L.team_off, s));   // team counters + granules: the header survives
  const bool b128 = mlp->batch == 128;
  // one workgroup per CU of the whole chip: the 32 that land on XCD j < n_inst form instance j's team, the others exit
  const dim3 grid(kMxMaxInst * kMxMembers), block(four ? kMxThreads4 : kMxThreads);
  const int rc = with_pre(cfg->preprocess, [&](auto pre) {
    constexpr int PRE = decltype(pre)::value;
    const size_t lds = b128 ? mlp_xcd_lds_bytes<PRE, 128>() : mlp_xcd_lds_bytes<PRE, 64>();
    if (hist) {
      void (*fn)(MlpXcdHistArgs) = b128 ? k_mlp_xcd<PRE, 8, true, 128> : four ? k_mlp_xcd<PRE, 4, true> : k_mlp_xcd<PRE, 8, true>;
      return launch(fn, grid, block, lds, s, a);
    }
    void (*fn)(MlpXcdArgs) = b128 ? k_mlp_xcd<PRE, 8, false, 128> : four ? k_mlp_xcd<PRE, 4> : k_mlp_xcd<PRE, 8>;
    return launch(fn, grid, block, lds, s, static_cast<const MlpXcdArgs&>(a));
  });
  if (rc) return rc;
  note_form(L2O_FORM_MLP_XCD);
  return L2O_OK;
}

int l2o_mlp_unroll_multi(const l2o_net_cfg* cfg, const float* wpack, const l2o_mlp* mlp, const l2o_mlp_instance* inst,
                         int32_t n_inst, int32_t T, int32_t step0, void* workspace, void* stream) {
  return mlp_unroll_multi_launch(cfg, wpack, mlp, inst, n_inst, T, step0, nullptr, workspace, stream);
}
int l2o_mlp_unroll_multi_record(const l2o_net_cfg* cfg, const float* wpack, const l2o_mlp* mlp, const l2o_mlp_instance* inst,
                                int32_t n_inst, int32_t T, int32_t step0, const l2o_mlp_hist* hist, void* workspace,
                                void* stream) {
  if (!hist) return fail(L2O_ERR_ARG, "l2o_mlp_unroll_multi_record: NULL hist");
  return mlp_unroll_multi_launch(cfg, wpack, mlp, inst, n_inst, T, step0, hist, workspace, stream);
}

}  // extern "C"
