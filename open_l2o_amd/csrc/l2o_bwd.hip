// l2o_bwd.hip -- the backward side of the optimizer nets and the nets that have no fused form, of the C ABI of
// include/l2o_abi.h: BPTT through the (20, 20) LSTM step (l2o_cwlstm_bwd_*), the generic-`layers` step and its backward
// (l2o_cwlstm_step_generic, l2o_cwlstm_bwd_step_generic) and KernelDeepLSTM (l2o_klstm_*, include/l2o_klstm_abi.h).  This
// unit owns the kernels of l2o_bwd.h, l2o_bwd_mfma.h, l2o_generic.h and l2o_klstm.h.  Written for gfx950 only.
#include "l2o_host.h"
#include "l2o_bwd.h"
#include "l2o_bwd_mfma.h"
#include "l2o_generic.h"
#include "l2o_klstm.h"
#include "../../include/l2o_klstm_abi.h"

// ---- generic-`layers` optimizer step (csrc/l2o_generic.h) --------------------------------------------------
static int check_gen_net(const l2o_net_cfg* cfg, const l2o_gen_net* net) {
  if (!cfg || !net) return fail(L2O_ERR_ARG, "generic net: NULL argument");
  if (net->n_layers < 1 || net->n_layers > kGenMaxL)
    return fail(L2O_ERR_UNSUPPORTED, "generic net: 1..%d LSTM layers (got %d)", kGenMaxL, net->n_layers);
  for (int l = 0; l < net->n_layers; ++l) {
    if (net->hidden[l] < 1 || net->hidden[l] > kGenMaxH)
      return fail(L2O_ERR_UNSUPPORTED, "generic net: hidden sizes 1..%d (layer %d has %d)", kGenMaxH, l, net->hidden[l]);
    if (!net->w_gates[l] || !net->b_gates[l]) return fail(L2O_ERR_ARG, "generic net: NULL weights of layer %d", l);
  }
  if (!net->w_lin || !net->b_lin) return fail(L2O_ERR_ARG, "generic net: NULL output Linear");
  const int want = cfg->preprocess == L2O_PRE_FC_ELU ? net->in_dim : (cfg->preprocess == L2O_PRE_LOGSIGN ? 2 : 1);
  if (net->in_dim != want || net->in_dim < 1 || net->in_dim > kGenMaxH)
    return fail(L2O_ERR_ARG, "generic net: in_dim %d does not match the preprocessing (%d)", net->in_dim, want);
  if (cfg->preprocess == L2O_PRE_FC_ELU && (!net->w_fc || !net->b_fc)) return fail(L2O_ERR_ARG, "generic net: fc weights");
  return L2O_OK;
}

// ---- KernelDeepLSTM: one LSTM per convolution filter (csrc/l2o_klstm.h, include/l2o_klstm_abi.h) ----------------------------
static bool klstm_ok(const l2o_klstm_net* n) {
  if (!n || n->flags != 0) return false;
  if (n->kw < 1 || n->kw > L2O_KLSTM_MAX_SIDE || n->kh < 1 || n->kh > L2O_KLSTM_MAX_SIDE) return false;
  if (n->n_layers < 1 || n->n_layers > L2O_KLSTM_MAX_LAYERS) return false;
  for (int l = 0; l < n->n_layers; ++l)
    if (n->hidden[l] < 4 || n->hidden[l] > L2O_KLSTM_MAX_HIDDEN || n->hidden[l] % 4) return false;
  return n->preprocess == L2O_PRE_IDENTITY || n->preprocess == L2O_PRE_LOGSIGN;
}
static int klstm_check(const char* who, const l2o_klstm_net* n, int64_t N) {
  if (!klstm_ok(n) || N < 1)
    return fail(L2O_ERR_UNSUPPORTED, "%s: kw, kh in [1, %d], 1 or 2 layers of a width that is a multiple of 4 in [4, %d], "
                "preprocess identity or LogAndSign, flags 0, N >= 1", who, L2O_KLSTM_MAX_SIDE, L2O_KLSTM_MAX_HIDDEN);
  for (int l = 0; l < n->n_layers; ++l)
    if (!n->w_gates[l] || !n->b_gates[l]) return fail(L2O_ERR_ARG, "%s: NULL weights of layer %d", who, l);
  if (!n->w_lin || !n->b_lin) return fail(L2O_ERR_ARG, "%s: NULL output Linear", who);
  return L2O_OK;
}

extern "C" {

size_t l2o_gen_state_floats(const l2o_gen_net* net, int64_t N) {
  if (!net || N <= 0 || net->n_layers < 1 || net->n_layers > kGenMaxL) return 0;
  size_t n = 0;
  for (int l = 0; l < net->n_layers; ++l) n += 2 * (size_t)N * (size_t)net->hidden[l];
  return n;
}

int l2o_cwlstm_step_generic(const l2o_net_cfg* cfg, const l2o_gen_net* net, const float* g, const float* m_tilde, float* m,
                            float* v, double pow1, double pow2, float* state, float* x, int64_t N, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  int rc = check_gen_net(cfg, net);
  if (rc) return rc;
  if (!g || !state || !x || N <= 0) return fail(L2O_ERR_ARG, "l2o_cwlstm_step_generic: bad argument");
  const bool fc = cfg->preprocess == L2O_PRE_FC_ELU;
  if (fc && net->direct_inputs && !m_tilde) return fail(L2O_ERR_ARG, "l2o_cwlstm_step_generic: direct inputs need m_tilde");
  if (fc && !net->direct_inputs && (!m || !v)) return fail(L2O_ERR_ARG, "l2o_cwlstm_step_generic: RNNProp needs m and v");
  GenParams p;
  std::memset(&p, 0, sizeof(p));
  p.n_layers = net->n_layers;
  for (int l = 0; l < net->n_layers; ++l) { p.H[l] = net->hidden[l]; p.wg[l] = net->w_gates[l]; p.bg[l] = net->b_gates[l]; }
  p.in_dim = net->in_dim; p.pre = cfg->preprocess; p.direct = net->direct_inputs; p.tanh_output = cfg->tanh_output;
  p.scale = (float)cfg->scale;
  p.k_inv = cfg->logsign_k != 0.0 ? (float)(1.0 / cfg->logsign_k) : 0.0f;
  p.exp_k = (float)std::exp(cfg->logsign_k);
  p.beta1 = (float)cfg->beta1; p.beta2 = (float)cfg->beta2;
  p.omb1 = (float)(1.0 - cfg->beta1); p.omb2 = (float)(1.0 - cfg->beta2);
  p.om1 = (float)(1.0 - pow1); p.om2 = (float)(1.0 - pow2);
  p.wl = net->w_lin; p.bl = net->b_lin; p.wfc = net->w_fc; p.bfc = net->b_fc;
  p.g = g; p.m_in = m_tilde; p.m = m; p.v = v; p.state = state; p.x = x; p.N = (long)N;
  hipLaunchKernelGGL(k_cwlstm_generic, dim3((unsigned)((N + kGenThreads - 1) / kGenThreads)), dim3(kGenThreads), 0,
                     (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

int l2o_cwlstm_bwd_step_generic(const l2o_net_cfg* cfg, const l2o_gen_net* net, const l2o_gen_bwd_io* io, double pow1,
                                double pow2, int64_t N, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  int rc = check_gen_net(cfg, net);
  if (rc) return rc;
  if (!io || N <= 0 || !io->g || !io->st_prev || !io->dx_next || !io->carry_in || !io->carry_out || !io->tc ||
      !io->h_last || !io->dd)
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_step_generic: bad argument");
  if (net->direct_inputs) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_step_generic: direct inputs have no moments to chain through");
  const bool fc = cfg->preprocess == L2O_PRE_FC_ELU;
  if (fc && (!io->m || !io->v || !io->feats || !io->du))
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_step_generic: RNNProp needs m, v, feats and du");
  if (fc && io->dg) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_step_generic: the input adjoint of RNNProp is formed by the host from du");
  GenBwdParams p;
  std::memset(&p, 0, sizeof(p));
  p.n_layers = net->n_layers;
  for (int l = 0; l < net->n_layers; ++l) {
    if (!io->act[l] || !io->dz[l]) return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_step_generic: NULL act / dz of layer %d", l);
    p.H[l] = net->hidden[l]; p.wg[l] = net->w_gates[l]; p.bg[l] = net->b_gates[l];
    p.act[l] = io->act[l]; p.dz[l] = io->dz[l];
  }
  p.in_dim = net->in_dim; p.pre = cfg->preprocess; p.tanh_output = cfg->tanh_output;
  p.scale = (float)cfg->scale;
  p.k_inv = cfg->logsign_k != 0.0 ? (float)(1.0 / cfg->logsign_k) : 0.0f;
  p.exp_k = (float)std::exp(cfg->logsign_k);
  p.om1 = (float)(1.0 - pow1); p.om2 = (float)(1.0 - pow2);
  p.wl = net->w_lin; p.bl = net->b_lin; p.wfc = net->w_fc; p.bfc = net->b_fc;
  p.g = io->g; p.m = io->m; p.v = io->v; p.st_prev = io->st_prev; p.dx_next = io->dx_next;
  p.carry_in = io->carry_in; p.carry_out = io->carry_out; p.tc = io->tc; p.h_last = io->h_last; p.dd = io->dd;
  p.feats = io->feats; p.du = io->du; p.dg = io->dg; p.N = (long)N;
  hipLaunchKernelGGL(k_cwlstm_generic_bwd, dim3((unsigned)((N + kGenThreads - 1) / kGenThreads)), dim3(kGenThreads), 0,
                     (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

int l2o_klstm_supported(const l2o_klstm_net* net) { return klstm_ok(net) ? 1 : 0; }
size_t l2o_klstm_state_floats(const l2o_klstm_net* net, int64_t N) {
  if (!klstm_ok(net) || N < 1) return 0;
  size_t n = 0;
  for (int l = 0; l < net->n_layers; ++l) n += 2 * (size_t)N * (size_t)net->hidden[l];
  return n;
}
int l2o_klstm_step(const l2o_klstm_net* net, const float* g, const float* state_in, float* state_out, float* x, int64_t N,
                   void* stream) {
  int rc = klstm_check("l2o_klstm_step", net, N);
  if (rc) return rc;
  if (!g || !state_in || !state_out || !x) return fail(L2O_ERR_ARG, "l2o_klstm_step: NULL argument");
  KlParams p;
  std::memset(&p, 0, sizeof(p));
  p.K = net->kw * net->kh;
  p.pre = net->preprocess;
  p.in = p.pre == L2O_PRE_LOGSIGN ? 2 * p.K : p.K;
  p.in_pad = (p.in + 3) / 4 * 4;
  p.n_layers = net->n_layers;
  for (int l = 0; l < net->n_layers; ++l) { p.H[l] = net->hidden[l]; p.wg[l] = net->w_gates[l]; p.bg[l] = net->b_gates[l]; }
  p.tanh_output = net->tanh_output;
  p.scale = (float)net->scale;
  p.k_inv = net->logsign_k != 0.0 ? (float)(1.0 / net->logsign_k) : 0.0f;
  p.exp_k = (float)std::exp(net->logsign_k);
  p.wl = net->w_lin; p.bl = net->b_lin;
  p.g = g; p.st_in = state_in; p.st_out = state_out; p.x = x; p.N = (long)N;
  const int64_t ntiles = (N + 15) / 16;
  if (ntiles > 0x7fffffff / 16) return fail(L2O_ERR_UNSUPPORTED, "l2o_klstm_step: N %lld is too large", (long long)N);
  p.ntiles = (int)ntiles;
  const int64_t wgs = (ntiles + kKlWaves - 1) / kKlWaves;
  return launch(k_klstm_step, dim3((unsigned)(wgs < kKlMaxBlocks ? wgs : kKlMaxBlocks)), dim3(kKlThreads),
                sizeof(float) * (size_t)kl_lds_floats(p), (hipStream_t)stream, p);
}
int l2o_klstm_bwd_step(const l2o_klstm_net* net, const l2o_klstm_bwd_io* io, int64_t N, void* stream) {
  int rc = klstm_check("l2o_klstm_bwd_step", net, N);
  if (rc) return rc;
  if (!io || !io->g || !io->st_prev || !io->dx_next || !io->carry_in || !io->carry_out || !io->tc || !io->h_last || !io->dd ||
      io->carry_in == io->carry_out)
    return fail(L2O_ERR_ARG, "l2o_klstm_bwd_step: bad argument");
  KlBwdParams p;
  std::memset(&p, 0, sizeof(p));
  p.K = net->kw * net->kh;
  p.pre = net->preprocess;
  p.in = p.pre == L2O_PRE_LOGSIGN ? 2 * p.K : p.K;
  p.n_layers = net->n_layers;
  for (int l = 0; l < net->n_layers; ++l) {
    if (!io->act[l] || !io->dz[l]) return fail(L2O_ERR_ARG, "l2o_klstm_bwd_step: NULL act / dz of layer %d", l);
    p.H[l] = net->hidden[l]; p.wg[l] = net->w_gates[l]; p.bg[l] = net->b_gates[l];
    p.act[l] = io->act[l]; p.dz[l] = io->dz[l];
  }
  p.tanh_output = net->tanh_output;
  p.scale = (float)net->scale;
  p.k_inv = net->logsign_k != 0.0 ? (float)(1.0 / net->logsign_k) : 0.0f;
  p.exp_k = (float)std::exp(net->logsign_k);
  p.wl = net->w_lin; p.bl = net->b_lin;
  p.g = io->g; p.st_prev = io->st_prev; p.dx_next = io->dx_next; p.carry_in = io->carry_in; p.carry_out = io->carry_out;
  p.tc = io->tc; p.h_last = io->h_last; p.dd = io->dd; p.N = (long)N;
  hipLaunchKernelGGL(k_klstm_bwd_step, dim3((unsigned)((N + kKlBwdThreads - 1) / kKlBwdThreads)), dim3(kKlBwdThreads), 0,
                     (hipStream_t)stream, p);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

static int launch_bwd_tile(const BwdParams& p, int pre, hipStream_t s) {
  size_t nblk = ((size_t)p.tile_end[p.nseg - 1] + 3) / 4;
  size_t cap = (size_t)device_cu_count(s);              // persistent: one workgroup per CU walks the tile groups
  if (opt(L2O_OPT_BWD_BLOCKS) > 0) cap = (size_t)opt(L2O_OPT_BWD_BLOCKS);
  if (nblk > cap && p.T <= 1) nblk = cap;                  // (a T-step launch keeps one workgroup per four tiles: each lives T steps)
  const dim3 grid((unsigned)nblk), block(256);
  const bool mfma = p.wpack && opt(L2O_OPT_BWD_KERNEL) == 0;   // the matrix-core form needs the packed weights
  return with_pre(pre, [&](auto pr) {
    constexpr int PRE = decltype(pr)::value;
    if (mfma) return launch(k_cwlstm_bwd_mfma<PRE>, grid, block, sizeof(float) * BwdMfmaGeom<PRE>::kLdsFloats, s, p);
    return launch(k_cwlstm_bwd_tile<PRE>, grid, block, sizeof(float) * BwdTileGeom<PRE>::kLdsFloats, s, p);
  });
}

static void fill_bwd_net(BwdParams& p, const l2o_net_cfg* cfg, const l2o_net_weights* w, double pow1, double pow2) {
  p.pre = cfg->preprocess; p.tanh_output = cfg->tanh_output; p.n_layers = cfg->n_layers;
  p.scale = (float)cfg->scale;
  p.k_inv = cfg->logsign_k != 0.0 ? (float)(1.0 / cfg->logsign_k) : 0.0f;
  p.exp_k = (float)std::exp(cfg->logsign_k);
  p.beta1 = (float)cfg->beta1; p.beta2 = (float)cfg->beta2;
  p.om1 = (float)(1.0 - pow1); p.om2 = (float)(1.0 - pow2);
  p.wg1 = w->w_gates1; p.bg1 = w->b_gates1; p.wg2 = w->w_gates2; p.bg2 = w->b_gates2;
  p.wl = w->w_lin; p.bl = w->b_lin; p.wfc = w->w_fc; p.bfc = w->b_fc;
  p.wpack = w->wpack;
}

int l2o_cwlstm_bwd_multi(const l2o_net_cfg* cfg, const l2o_net_weights* w, const l2o_bwd_seg* segs, int32_t nseg,
                         const float* carry_in, float* carry_out, float* A, float* Bm, double pow1, double pow2,
                         void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !w || !segs || nseg < 1 || !carry_in || !carry_out || !A || !Bm)
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_multi: bad argument");
  if (nseg > 8) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_multi: at most 8 panels");
  if (!net_ok_for_mfma(cfg) || cfg->n_layers == 0)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_multi: only layers=(20,20) nets");
  if (!w->w_gates1 || !w->b_gates1 || !w->w_gates2 || !w->b_gates2 || !w->w_lin || !w->b_lin)
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_multi: NULL weights");
  const int pre = cfg->preprocess;
  if (pre == L2O_PRE_FC_ELU && (!w->w_fc || !w->b_fc)) return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_multi: fc weights");
  if (((uintptr_t)A & 15) || ((uintptr_t)Bm & 15)) return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_multi: A / Bm must be 16-byte aligned");
  BwdParams p;
  std::memset(&p, 0, sizeof(p));
  fill_bwd_net(p, cfg, w, pow1, pow2);
  p.carry_in = carry_in; p.carry_out = carry_out; p.act1 = A; p.dz1 = Bm;
  p.nseg = nseg;
  long tiles = 0;
  for (int i = 0; i < nseg; ++i) {
    const l2o_bwd_seg& sgm = segs[i];
    if (!sgm.g || !sgm.st_prev || !sgm.dx_next || sgm.B <= 0 || sgm.D <= 0 ||
        (pre == L2O_PRE_FC_ELU && (!sgm.m || !sgm.v)))
      return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_multi: bad panel %d", i);
    if (sgm.D % kTile != 0 && sgm.B != 1)
      return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_multi: panel %d needs D %% 16 == 0 or B == 1", i);
    const long n = (long)(sgm.B * sgm.D);
    tiles += (n + kTile - 1) / kTile;
    if (tiles > INT32_MAX / kTile) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_multi: too many coordinates");
    p.tile_end[i] = (int)tiles;
    p.seg_n[i] = n;
    p.seg_d[i] = n; p.seg_tpp[i] = (int)((n + kTile - 1) / kTile);   // (tile-aligned or one row: the flat numbering)
    p.seg_g[i] = sgm.g; p.seg_m[i] = sgm.m; p.seg_v[i] = sgm.v; p.seg_st[i] = sgm.st_prev; p.seg_dx[i] = sgm.dx_next;
  }
  p.rows_total = tiles * kTile;
  return launch_bwd_tile(p, pre, (hipStream_t)stream);
}

static int bwd_unroll_impl(const l2o_net_cfg* cfg, const l2o_net_weights* w, const l2o_bwd_unroll_seg* segs,
                           int32_t nseg, const float* const* table, int32_t T, int64_t step0, const float* carry_in,
                           float* carry_out, float* A, float* Bm, void* stream, int compact);
int l2o_cwlstm_bwd_unroll(const l2o_net_cfg* cfg, const l2o_net_weights* w, const l2o_bwd_unroll_seg* segs,
                          int32_t nseg, const float* const* table, int32_t T, int64_t step0, const float* carry_in,
                          float* carry_out, float* A, float* Bm, void* stream) {
  return bwd_unroll_impl(cfg, w, segs, nseg, table, T, step0, carry_in, carry_out, A, Bm, stream, 0);
}
int l2o_cwlstm_bwd_unroll_compact(const l2o_net_cfg* cfg, const l2o_net_weights* w, const l2o_bwd_unroll_seg* segs,
                                  int32_t nseg, const float* const* table, int32_t T, int64_t step0, const float* carry_in,
                                  float* carry_out, float* Ac, float* Bm, void* stream) {
  return bwd_unroll_impl(cfg, w, segs, nseg, table, T, step0, carry_in, carry_out, Ac, Bm, stream, 1);
}
static int bwd_unroll_impl(const l2o_net_cfg* cfg, const l2o_net_weights* w, const l2o_bwd_unroll_seg* segs,
                           int32_t nseg, const float* const* table, int32_t T, int64_t step0, const float* carry_in,
                           float* carry_out, float* A, float* Bm, void* stream, int compact) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !w || !segs || nseg < 1 || !table || T < 1 || step0 < 0 || !A || !Bm)
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_unroll: bad argument");
  if (nseg > 8) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_unroll: at most 8 panels");
  if (!net_ok_for_mfma(cfg) || cfg->n_layers == 0)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_unroll: only layers=(20,20) nets");
  if (!w->wpack) return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_unroll: needs l2o_net_weights.wpack");
  if (((uintptr_t)A & 15) || ((uintptr_t)Bm & 15)) return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_unroll: A / Bm must be 16-byte aligned");
  const int pre = cfg->preprocess;
  BwdParams p;
  std::memset(&p, 0, sizeof(p));
  fill_bwd_net(p, cfg, w, 0.0, 0.0);
  p.carry_in = carry_in; p.carry_out = carry_out; p.act1 = A; p.dz1 = Bm;
  p.nseg = nseg; p.T = T; p.table = table;
  if (compact && opt(L2O_OPT_BWD_KERNEL) != 0)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_unroll_compact: the matrix-core BPTT kernel only (L2O_OPT_BWD_KERNEL = 0)");
  p.compact_a = compact;
  p.pw1_last = std::pow((double)p.beta1, (double)(step0 + T - 1));
  p.pw2_last = std::pow((double)p.beta2, (double)(step0 + T - 1));
  long tiles = 0;
  for (int i = 0; i < nseg; ++i) {
    const l2o_bwd_unroll_seg& sgm = segs[i];
    if (sgm.B <= 0 || sgm.D <= 0) return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_unroll: bad panel %d", i);
    const long n = (long)(sgm.B * sgm.D);
    const long tpp = (long)tiles_per_problem(sgm.D);        // per-problem tiles, the packed-state layout of the forward
    tiles += (long)sgm.B * tpp;
    if (tiles > INT32_MAX / kTile) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_unroll: too many coordinates");
    p.tile_end[i] = (int)tiles;
    p.seg_n[i] = n;
    p.seg_d[i] = (long)sgm.D;
    p.seg_tpp[i] = (int)tpp;
    p.seg_gfinal[i] = sgm.g_final;
  }
  p.rows_total = tiles * kTile;
  return launch_bwd_tile(p, pre, (hipStream_t)stream);
}

int l2o_cwlstm_bwd_step(const l2o_net_cfg* cfg, const l2o_net_weights* w, const l2o_bwd_io* io, double pow1,
                        double pow2, int64_t B, int64_t D, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !w || !io || B <= 0 || D <= 0 || !io->g || !io->dx_next || !io->act1 || !io->dd || !w->w_lin ||
      !w->b_lin)
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_step: bad argument");
  BwdParams p;
  std::memset(&p, 0, sizeof(p));
  p.B = (int)B; p.D = (int)D; p.tpp = tiles_per_problem(D);
  p.pre = cfg->preprocess; p.tanh_output = cfg->tanh_output; p.n_layers = cfg->n_layers;
  p.scale = (float)cfg->scale;
  p.k_inv = cfg->logsign_k != 0.0 ? (float)(1.0 / cfg->logsign_k) : 0.0f;
  p.exp_k = (float)std::exp(cfg->logsign_k);
  p.beta1 = (float)cfg->beta1; p.beta2 = (float)cfg->beta2;
  p.om1 = (float)(1.0 - pow1); p.om2 = (float)(1.0 - pow2);
  p.wg1 = w->w_gates1; p.bg1 = w->b_gates1; p.wg2 = w->w_gates2; p.bg2 = w->b_gates2;
  p.wl = w->w_lin; p.bl = w->b_lin; p.wfc = w->w_fc; p.bfc = w->b_fc;
  p.wpack = w->wpack;
  p.g = io->g; p.m = io->m; p.v = io->v; p.st_prev = io->st_prev; p.dx_next = io->dx_next;
  p.carry_in = io->carry_in; p.carry_out = io->carry_out; p.act1 = io->act1; p.dz1 = io->dz1;
  p.act2 = io->act2; p.dz2 = io->dz2; p.h2o = io->h2; p.dd = io->dd; p.feats = io->feats; p.du = io->du;
  p.dg = io->dg;
  if (io->dg && cfg->preprocess == L2O_PRE_FC_ELU)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_step: the input adjoint (dg) is implemented for the DM nets (identity / LogAndSign)");
  {
    const int pre_ = cfg->preprocess;
    const long P_ = cfg->n_layers == 0 ? 2 : (pre_ == L2O_PRE_FC_ELU ? kH : (pre_ == L2O_PRE_LOGSIGN ? 2 : 1));
    const long K1_ = cfg->n_layers == 0 ? 2 : P_ + kH;
    const long as = (long)io->a_stride, bs = (long)io->b_stride;
    p.s_act1 = as ? as : K1_; p.s_act2 = as ? as : 2 * kH; p.s_h2 = as ? as : kH; p.s_feats = as ? as : 2;
    p.s_dz1 = bs ? bs : 4 * kH; p.s_dz2 = bs ? bs : 4 * kH; p.s_dd = bs ? bs : 1; p.s_du = bs ? bs : kH;
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t N = (size_t)B * D;
  if (cfg->n_layers == 0) {
    if (cfg->kind != L2O_NET_CW || cfg->preprocess == L2O_PRE_FC_ELU)
      return fail(L2O_ERR_UNSUPPORTED, "layers=() is implemented for CoordinateWiseDeepLSTM only");
    const dim3 grid((unsigned)((N + 255) / 256));
    if (cfg->preprocess == L2O_PRE_LOGSIGN) hipLaunchKernelGGL(k_linear_bwd_step<L2O_PRE_LOGSIGN>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_linear_bwd_step<L2O_PRE_IDENTITY>, grid, dim3(256), 0, s, p);
    HIP_TRY(hipGetLastError());
    return L2O_OK;
  }
  if (!net_ok_for_mfma(cfg)) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_bwd_step: only layers=(20,20) / () nets");
  if (!w->w_gates1 || !w->b_gates1 || !w->w_gates2 || !w->b_gates2 || !io->st_prev || !io->carry_in ||
      !io->carry_out || !io->dz1 || !io->act2 || !io->dz2 || !io->h2)
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_step: NULL LSTM buffer");
  const int pre = cfg->preprocess;
  // fast path: tile-aligned panel + the interleaved A / Bm layout -> the quad / LDS-tile kernel
  {
    const int Pq = pre == L2O_PRE_FC_ELU ? kH : (pre == L2O_PRE_LOGSIGN ? 2 : 1);
    const int K1q = Pq + kH;
    const long KA = K1q + 3 * kH + (pre == L2O_PRE_FC_ELU ? 2 : 0) + 1, KB = 8 * kH + 1 + (pre == L2O_PRE_FC_ELU ? kH : 0);
    const bool layout = io->a_stride == KA && io->b_stride == KB && io->act2 == io->act1 + K1q &&
                        io->h2 == io->act1 + K1q + 2 * kH && io->dz2 == io->dz1 + 4 * kH && io->dd == io->dz1 + 8 * kH &&
                        (pre != L2O_PRE_FC_ELU || (io->feats == io->act1 + K1q + 3 * kH && io->du == io->dz1 + 8 * kH + 1 &&
                                                   io->m && io->v && w->w_fc && w->b_fc));
    if (layout && (D % kTile == 0 || B == 1) && ((uintptr_t)io->act1 & 15) == 0 && ((uintptr_t)io->dz1 & 15) == 0 &&
        opt(L2O_OPT_BWD_KERNEL) != 2 && !io->dg) {           // (the input adjoint is emitted by the generic kernel)
      p.nseg = 1;
      p.tile_end[0] = (int)((N + kTile - 1) / kTile);
      p.seg_n[0] = (long)N;
      p.seg_d[0] = (long)N; p.seg_tpp[0] = p.tile_end[0];
      p.seg_g[0] = io->g; p.seg_m[0] = io->m; p.seg_v[0] = io->v; p.seg_st[0] = io->st_prev; p.seg_dx[0] = io->dx_next;
      p.rows_total = (long)N;
      return launch_bwd_tile(p, pre, s);
    }
  }
  const size_t lds = 0;                                   // static LDS only (the per-thread input column)
  const dim3 grid((unsigned)((N + 63) / 64)), block(64);
  if (pre != L2O_PRE_IDENTITY && pre != L2O_PRE_LOGSIGN && (!io->m || !io->v || !io->feats || !io->du || !w->w_fc || !w->b_fc))
    return fail(L2O_ERR_ARG, "l2o_cwlstm_bwd_step: RNNProp needs m, v, feats, du and the fc weights");
  with_pre(pre, [&](auto pr) { hipLaunchKernelGGL(k_cwlstm_bwd_step<decltype(pr)::value>, grid, block, lds, s, p); });
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

}  // extern "C"
