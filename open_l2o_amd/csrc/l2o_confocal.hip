// l2o_confocal.hip -- the confocal_microscopy_3d optimizee of the C ABI: its loss and gradient (l2o_confocal_fg,
// include/l2o_abi.h), the fused persistent unroll (l2o_confocal_unroll*, include/l2o_confocal_unroll_abi.h) and several
// instances per fused launch (l2o_confocal_unroll_multi*, include/l2o_confocal_multi_abi.h).  This unit owns the kernels of
// l2o_confocal.h and l2o_confocal_unroll.h.  Written for gfx950 only.
#include "l2o_host.h"
#include "l2o_confocal.h"
#include "l2o_confocal_unroll.h"

// the loss reduction of l2o_util_kernels.h: code in l2o_core.hip, the launch binds to its host stub
__global__ void k_reduce_fx(const float* __restrict__ fx_part, int T1, int B_local, float inv_bg, float* __restrict__ fx);

// the fused unroll of the confocal optimizee (csrc/l2o_confocal_unroll.h): one workgroup per batch row
template <int PRE>
static int launch_confocal_unroll(const CfUnrollArgs& a, bool hist, size_t lds, hipStream_t s) {
  void (*fn)(CfUnrollArgs) = hist ? k_cf_unroll<PRE, true> : k_cf_unroll<PRE, false>;
  return launch(fn, dim3(a.batch), dim3(kCfThreads), lds, s, a);
}

// ... and several instances per launch: n_inst x batch workgroups, the pointers out of the tables in device scratch
template <int PRE>
static int launch_confocal_unroll_multi(const CfUnrollMultiArgs& a, int n_inst, bool hist, size_t lds, hipStream_t s) {
  void (*fn)(CfUnrollMultiArgs) = hist ? k_cf_unroll<PRE, true, true> : k_cf_unroll<PRE, false, true>;
  return launch(fn, dim3(n_inst * a.batch), dim3(kCfThreads), lds, s, a);
}

extern "C" {

// ---- problems.confocal_microscopy_3d (csrc/l2o_confocal.h) ------------------------------------------------------------
static bool confocal_ok(const l2o_confocal* m) {
  if (!m || m->batch < 1 || m->batch > kCfMaxBatch || m->num_points < 1 || m->num_points > kCfMaxPts) return false;
  for (int k = 0; k < 3; ++k)
    if (m->roi[k] < kCfMinEdge || m->roi[k] > kCfMaxEdge) return false;
  return m->inference == 0 || m->inference == 1;
}
// planes of iy per workgroup: about kCfTargetWgs workgroups in all, a row never split further than one plane per slab
static void confocal_slabs(const l2o_confocal* m, int* slab, int* nslab) {
  int want = (kCfTargetWgs + m->batch - 1) / m->batch;
  if (want > m->roi[1]) want = m->roi[1];
  *slab = (m->roi[1] + want - 1) / want;
  *nslab = (m->roi[1] + *slab - 1) / *slab;
}
size_t l2o_confocal_scratch_floats(const l2o_confocal* m) {
  if (!confocal_ok(m)) return 0;
  int slab, nslab;
  confocal_slabs(m, &slab, &nslab);
  return (size_t)nslab * kCfPart * m->batch + m->batch;
}
int l2o_confocal_fg(const l2o_confocal* m, const float* const* theta, const float* const* sim, float* loss, float* const* g,
                    float* scratch, void* stream) {
  if (!confocal_ok(m))
    return fail(L2O_ERR_UNSUPPORTED, "l2o_confocal_fg: batch in [1, %d], num_points in [1, %d], roi edges in [%d, %d], "
                "inference 0 or 1", kCfMaxBatch, kCfMaxPts, kCfMinEdge, kCfMaxEdge);
  if (!theta || !loss || !scratch) return fail(L2O_ERR_ARG, "l2o_confocal_fg: NULL argument");
  if (m->inference ? !m->img : !sim) return fail(L2O_ERR_ARG, "l2o_confocal_fg: inference needs img, simulation needs sim");
  const int nv = 6 * m->num_points + 1;
  for (int k = 0; k < nv; ++k)
    if (!theta[k] || (g && !g[k]) || (!m->inference && !sim[k]))
      return fail(L2O_ERR_ARG, "l2o_confocal_fg: NULL buffer of variable %d", k);
  CfArgs a;
  std::memset(&a, 0, sizeof(a));
  a.batch = m->batch; a.P = m->num_points; a.rx = m->roi[0]; a.ry = m->roi[1]; a.rz = m->roi[2];
  a.inference = m->inference; a.want_grad = g ? 1 : 0;
  confocal_slabs(m, &a.slab, &a.nslab);
  a.img = m->inference ? m->img : nullptr;
  a.part = scratch;
  a.inv = scratch + (size_t)a.nslab * kCfPart * a.batch;
  a.loss = loss;
  for (int k = 0; k < nv; ++k) {
    a.th[k] = theta[k];
    a.sim[k] = m->inference ? nullptr : sim[k];
    a.g[k] = g ? g[k] : nullptr;
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kCfThreads);
  if (a.inference) hipLaunchKernelGGL(k_cf_norm, dim3(a.batch), blk, 0, s, a);
  hipLaunchKernelGGL(k_cf_slab, dim3(a.batch, a.nslab), blk, 0, s, a);
  const int nred = g ? (nv * a.batch + kCfThreads - 1) / kCfThreads : 1;
  hipLaunchKernelGGL(k_cf_reduce, dim3(nred), blk, 0, s, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- the fused unroll of the confocal optimizee (csrc/l2o_confocal_unroll.h) ----------------------------------------------
static bool confocal_unroll_ok(const l2o_net_cfg* cfg, const l2o_confocal* m) {
  return cfg && net_ok_for_mfma(cfg) && confocal_ok(m);
}
int l2o_confocal_unroll_supported(const l2o_net_cfg* cfg, const l2o_confocal* m, void* /*stream*/) {
  return confocal_unroll_ok(cfg, m) ? 1 : 0;
}
// fx_part [T + 1][batch] (rounded up to whole pointers), then the history pointer table of a recording launch
static size_t confocal_unroll_fx_floats(const l2o_confocal* m, int T) { return (((size_t)T + 1) * m->batch + 1) & ~(size_t)1; }
size_t l2o_confocal_unroll_scratch_floats(const l2o_confocal* m, int32_t T) {
  if (!confocal_ok(m) || T < 0) return 0;
  return confocal_unroll_fx_floats(m, T) + 2 * 4 * (size_t)kCfMaxVars;
}
static int confocal_unroll_launch(const char* who, const l2o_net_cfg* cfg, const float* wpack, const l2o_confocal* m,
                                  float* const* x, float* const* st, float* const* mm, float* const* vv,
                                  const float* const* x_scale, const float* const* sim, int32_t T, int32_t step0, float* fx,
                                  const l2o_confocal_hist* hist, float* scratch, void* stream) {
  if (!confocal_unroll_ok(cfg, m))
    return fail(L2O_ERR_UNSUPPORTED, "%s: the (20, 20) LSTM nets; batch in [1, %d], num_points in [1, %d], roi edges in "
                "[%d, %d], inference 0 or 1", who, kCfMaxBatch, kCfMaxPts, kCfMinEdge, kCfMaxEdge);
  if (!wpack || !x || !st || !fx || !scratch || T < 0) return fail(L2O_ERR_ARG, "%s: NULL argument or T < 0", who);
  if (m->inference ? !m->img : !sim) return fail(L2O_ERR_ARG, "%s: inference needs img, simulation needs sim", who);
  const bool rn = cfg->preprocess == L2O_PRE_FC_ELU;
  if (rn && (!mm || !vv)) return fail(L2O_ERR_ARG, "%s: RNNProp needs m and v", who);
  const int nv = 6 * m->num_points + 1;
  CfUnrollArgs a;
  std::memset(&a, 0, sizeof(a));
  CfHistPtrs hp;
  std::memset(&hp, 0, sizeof(hp));
  for (int k = 0; k < nv; ++k) {
    if (!x[k] || !st[k] || (rn && (!mm[k] || !vv[k])) || (!m->inference && !sim[k]))
      return fail(L2O_ERR_ARG, "%s: NULL buffer of variable %d", who, k);
    a.x[k] = x[k]; a.st[k] = st[k];
    a.m[k] = rn ? mm[k] : nullptr; a.v[k] = rn ? vv[k] : nullptr;
    a.xs[k] = x_scale ? x_scale[k] : nullptr;
    a.sim[k] = m->inference ? nullptr : sim[k];
    if (hist) {
      if (!hist->st[k] || !hist->g[k] || (rn && (!hist->m[k] || !hist->v[k])))
        return fail(L2O_ERR_ARG, "%s: NULL history buffer of variable %d", who, k);
      hp.p[0][k] = hist->st[k]; hp.p[1][k] = hist->g[k];
      hp.p[2][k] = rn ? hist->m[k] : nullptr; hp.p[3][k] = rn ? hist->v[k] : nullptr;
    }
  }
  a.np = make_net_params(cfg, wpack);
  a.batch = m->batch; a.P = m->num_points; a.rx = m->roi[0]; a.ry = m->roi[1]; a.rz = m->roi[2];
  a.inference = m->inference; a.T = T;
  a.rb = 1.0f / (float)m->batch;
  pow_ff(cfg->beta1, step0, &a.p1_hi, &a.p1_lo);
  pow_ff(cfg->beta2, step0, &a.p2_hi, &a.p2_lo);
  a.img = m->inference ? m->img : nullptr;
  a.fx_part = scratch;
  float** tab = reinterpret_cast<float**>(scratch + confocal_unroll_fx_floats(m, T));
  a.htab = hist ? tab : nullptr;
  hipStream_t s = (hipStream_t)stream;
  if (hist) hipLaunchKernelGGL(k_cf_hist_table, dim3(1), dim3(256), 0, s, hp, tab);
  const size_t lds = sizeof(float) * (size_t)a.rx * a.ry * a.rz;
  const int rc = with_pre(cfg->preprocess, [&](auto pre) { return launch_confocal_unroll<decltype(pre)::value>(a, hist != nullptr, lds, s); });
  if (rc != L2O_OK) return rc;
  hipLaunchKernelGGL(k_reduce_fx, dim3(T + 1), dim3(64), 0, s, a.fx_part, (int)(T + 1), (int)a.batch, a.rb, fx);
  HIP_TRY(hipGetLastError());
  note_form(L2O_FORM_CONFOCAL_UNROLL);
  return L2O_OK;
}
int l2o_confocal_unroll(const l2o_net_cfg* cfg, const float* wpack, const l2o_confocal* m, float* const* x, float* const* st,
                        float* const* mm, float* const* vv, const float* const* x_scale, const float* const* sim, int32_t T,
                        int32_t step0, float* fx, float* scratch, void* stream) {
  return confocal_unroll_launch("l2o_confocal_unroll", cfg, wpack, m, x, st, mm, vv, x_scale, sim, T, step0, fx, nullptr,
                                scratch, stream);
}
int l2o_confocal_unroll_record(const l2o_net_cfg* cfg, const float* wpack, const l2o_confocal* m, float* const* x,
                               float* const* st, float* const* mm, float* const* vv, const float* const* x_scale,
                               const float* const* sim, int32_t T, int32_t step0, float* fx, const l2o_confocal_hist* hist,
                               float* scratch, void* stream) {
  if (!hist) return fail(L2O_ERR_ARG, "l2o_confocal_unroll_record: NULL hist");
  return confocal_unroll_launch("l2o_confocal_unroll_record", cfg, wpack, m, x, st, mm, vv, x_scale, sim, T, step0, fx, hist,
                                scratch, stream);
}

// ---- several confocal instances per fused launch (include/l2o_confocal_multi_abi.h) ------------------------------------------
static bool confocal_unroll_multi_ok(const l2o_net_cfg* cfg, const l2o_confocal* m, int32_t n_inst) {
  return confocal_unroll_ok(cfg, m) && n_inst >= 1 && n_inst <= L2O_CONFOCAL_MAX_INSTANCES;
}
int l2o_confocal_unroll_multi_supported(const l2o_net_cfg* cfg, const l2o_confocal* m, int32_t n_inst, void* /*stream*/) {
  return confocal_unroll_multi_ok(cfg, m, n_inst) ? 1 : 0;
}
// n_inst x fx_part [T + 1][batch] (each rounded up to whole pointers), then the n_inst pointer tables
size_t l2o_confocal_unroll_multi_scratch_floats(const l2o_confocal* m, int32_t n_inst, int32_t T) {
  if (!confocal_ok(m) || T < 0 || n_inst < 1 || n_inst > L2O_CONFOCAL_MAX_INSTANCES) return 0;
  return (size_t)n_inst * (confocal_unroll_fx_floats(m, T) + 2 * (size_t)kCfInstPtrs);
}
static int confocal_unroll_multi_launch(const char* who, const l2o_net_cfg* cfg, const float* wpack, const l2o_confocal* m,
                                        const l2o_confocal_instance* inst, int32_t n_inst, int32_t T, int32_t step0,
                                        const l2o_confocal_hist* hist, float* scratch, void* stream) {
  if (!confocal_unroll_multi_ok(cfg, m, n_inst))
    return fail(L2O_ERR_UNSUPPORTED, "%s: the (20, 20) LSTM nets; batch in [1, %d], num_points in [1, %d], roi edges in "
                "[%d, %d], inference 0 or 1; 1 to %d instances", who, kCfMaxBatch, kCfMaxPts, kCfMinEdge, kCfMaxEdge,
                L2O_CONFOCAL_MAX_INSTANCES);
  if (!wpack || !inst || !scratch || T < 0) return fail(L2O_ERR_ARG, "%s: NULL argument or T < 0", who);
  const bool rn = cfg->preprocess == L2O_PRE_FC_ELU;
  const int nv = 6 * m->num_points + 1;
  // every instance is checked before anything is launched
  for (int i = 0; i < n_inst; ++i) {
    const l2o_confocal_instance& in = inst[i];
    if (!in.fx || (m->inference && !in.img)) return fail(L2O_ERR_ARG, "%s: instance %d: NULL fx, or inference without img", who, i);
    for (int k = 0; k < nv; ++k) {
      if (!in.x[k] || !in.st[k] || (rn && (!in.m[k] || !in.v[k])) || (!m->inference && !in.sim[k]))
        return fail(L2O_ERR_ARG, "%s: instance %d: NULL buffer of variable %d", who, i, k);
      if (hist && (!hist[i].st[k] || !hist[i].g[k] || (rn && (!hist[i].m[k] || !hist[i].v[k]))))
        return fail(L2O_ERR_ARG, "%s: instance %d: NULL history buffer of variable %d", who, i, k);
    }
  }
  const size_t fx_floats = confocal_unroll_fx_floats(m, T);
  float** tab = reinterpret_cast<float**>(scratch + (size_t)n_inst * fx_floats);
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < n_inst; ++i) {
    const l2o_confocal_instance& in = inst[i];
    CfInstPtrs ip;
    std::memset(&ip, 0, sizeof(ip));
    CfHistPtrs hp;
    std::memset(&hp, 0, sizeof(hp));
    for (int k = 0; k < nv; ++k) {
      ip.p[0][k] = in.x[k]; ip.p[1][k] = in.st[k];
      ip.p[2][k] = rn ? in.m[k] : nullptr; ip.p[3][k] = rn ? in.v[k] : nullptr;
      ip.p[4][k] = const_cast<float*>(in.x_scale[k]);
      ip.p[5][k] = m->inference ? nullptr : const_cast<float*>(in.sim[k]);
      if (hist) {
        hp.p[0][k] = hist[i].st[k]; hp.p[1][k] = hist[i].g[k];
        hp.p[2][k] = rn ? hist[i].m[k] : nullptr; hp.p[3][k] = rn ? hist[i].v[k] : nullptr;
      }
    }
    ip.img = m->inference ? const_cast<float*>(in.img) : nullptr;
    ip.fx_part = scratch + (size_t)i * fx_floats;
    ip.fx = in.fx;
    float** it = tab + (size_t)i * kCfInstPtrs;
    hipLaunchKernelGGL(k_cf_inst_table, dim3(1), dim3(320), 0, s, ip, it);
    if (hist) hipLaunchKernelGGL(k_cf_hist_table, dim3(1), dim3(256), 0, s, hp, it + kCfTabHist);
  }
  HIP_TRY(hipGetLastError());
  CfUnrollMultiArgs a;
  std::memset(&a, 0, sizeof(a));
  a.np = make_net_params(cfg, wpack);
  a.batch = m->batch; a.P = m->num_points; a.rx = m->roi[0]; a.ry = m->roi[1]; a.rz = m->roi[2];
  a.inference = m->inference; a.T = T;
  a.rb = 1.0f / (float)m->batch;
  pow_ff(cfg->beta1, step0, &a.p1_hi, &a.p1_lo);
  pow_ff(cfg->beta2, step0, &a.p2_hi, &a.p2_lo);
  a.tab = tab;
  const size_t lds = sizeof(float) * (size_t)a.rx * a.ry * a.rz;
  const int rc = with_pre(cfg->preprocess, [&](auto pre) { return launch_confocal_unroll_multi<decltype(pre)::value>(a, n_inst, hist != nullptr, lds, s); });
  if (rc != L2O_OK) return rc;
  hipLaunchKernelGGL(k_cf_reduce_fx_multi, dim3(T + 1, n_inst), dim3(64), 0, s, tab, (int)a.batch, a.rb);
  HIP_TRY(hipGetLastError());
  note_form(L2O_FORM_CONFOCAL_MULTI);
  return L2O_OK;
}
int l2o_confocal_unroll_multi(const l2o_net_cfg* cfg, const float* wpack, const l2o_confocal* m,
                              const l2o_confocal_instance* inst, int32_t n_inst, int32_t T, int32_t step0, float* scratch,
                              void* stream) {
  return confocal_unroll_multi_launch("l2o_confocal_unroll_multi", cfg, wpack, m, inst, n_inst, T, step0, nullptr, scratch,
                                      stream);
}
int l2o_confocal_unroll_multi_record(const l2o_net_cfg* cfg, const float* wpack, const l2o_confocal* m,
                                     const l2o_confocal_instance* inst, int32_t n_inst, int32_t T, int32_t step0,
                                     const l2o_confocal_hist* hist, float* scratch, void* stream) {
  if (!hist) return fail(L2O_ERR_ARG, "l2o_confocal_unroll_multi_record: NULL hist");
  return confocal_unroll_multi_launch("l2o_confocal_unroll_multi_record", cfg, wpack, m, inst, n_inst, T, step0, hist,
                                      scratch, stream);
}

}  // extern "C"
