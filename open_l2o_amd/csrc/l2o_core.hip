// l2o_core.hip -- the part of the C ABI of include/l2o_abi.h that belongs to no optimizee: version / build id / last error,
// the weight packer, Adam, state pack and unpack, the weight-gradient contraction G = A^T B, the loss reduction and the
// small vector passes of the meta-gradient.  This unit owns the kernels that are no templates of l2o_util_kernels.h (the
// two that the unroll launches and k_reduce_fx of the confocal unroll are declared where they are launched), l2o_atb.h
// (and its g_atb_phase) and l2o_vecops.h.  Written for gfx950 only.
#include "l2o_host.h"
#include "l2o_util_kernels.h"
#include "l2o_atb.h"
#include "l2o_vecops.h"

extern "C" {

int l2o_abi_version(void) { return L2O_ABI_VERSION; }
const char* l2o_last_error(void) { return g_err; }
#ifndef L2O_BUILD_ID
#define L2O_BUILD_ID "unknown"
#endif
const char* l2o_build_id(void) { return L2O_BUILD_ID; }
int l2o_last_unroll_form(void) { return g_last_form; }
int l2o_last_unroll_variant(void) { return g_last_variant; }

size_t l2o_wpack_floats(const l2o_net_cfg* cfg) {
  if (!cfg) return 0;
  if (cfg->n_layers == 0) return 4;
  if (!net_ok_for_mfma(cfg)) return 0;
  return (size_t)wp_rows(cfg->preprocess) * 64 + (size_t)bx::words(cfg->preprocess) + (size_t)bxb::words(cfg->preprocess);
}

int l2o_wpack_host(const l2o_net_cfg* cfg, const float* wg1, const float* bg1, const float* wg2,
                   const float* bg2, const float* wl, const float* bl, const float* wfc, const float* bfc,
                   float* out) {
  if (!cfg || !out || !wl || !bl) return fail(L2O_ERR_ARG, "l2o_wpack_host: NULL argument");
  if (cfg->n_layers == 0) {
    // Linear(P -> 1) on the preprocessed gradient, P = 1 (identity) or 2 (LogAndSign)
    if (cfg->kind != L2O_NET_CW || cfg->preprocess == L2O_PRE_FC_ELU)
      return fail(L2O_ERR_UNSUPPORTED, "layers=() is implemented for CoordinateWiseDeepLSTM only");
    out[0] = wl[0];
    out[1] = cfg->preprocess == L2O_PRE_LOGSIGN ? wl[1] : 0.0f;
    out[2] = bl[0];
    out[3] = 0.0f;
    return L2O_OK;
  }
  if (!net_ok_for_mfma(cfg))
    return fail(L2O_ERR_UNSUPPORTED, "MFMA kernels implement layers=(20,20) (got n_layers=%d hidden=%d kind=%d pre=%d)",
                cfg->n_layers, cfg->hidden, cfg->kind, cfg->preprocess);
  if (!wg1 || !bg1 || !wg2 || !bg2) return fail(L2O_ERR_ARG, "l2o_wpack_host: NULL LSTM weights");
  const int pre = cfg->preprocess;
  const bool fc = pre == L2O_PRE_FC_ELU;
  if (fc && (!wfc || !bfc)) return fail(L2O_ERR_ARG, "l2o_wpack_host: fc preprocess needs input_projection");
  std::memset(out, 0, sizeof(float) * l2o_wpack_floats(cfg));
  for (int l = 0; l < 64; ++l) wpack_lane(pre, l, 0, kNT, 0, bxb::ntiles(pre), wg1, bg1, wg2, bg2, wl, bl, wfc, bfc, out);
  return L2O_OK;
}

int l2o_wpack_device(const l2o_net_cfg* cfg, const l2o_net_weights* w, float* wpack, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  if (!cfg || !w || !wpack) return fail(L2O_ERR_ARG, "l2o_wpack_device: NULL argument");
  if (!net_ok_for_mfma(cfg) || cfg->n_layers == 0)
    return fail(L2O_ERR_UNSUPPORTED, "l2o_wpack_device: layers=(20,20) nets only");
  const bool fc = cfg->preprocess == L2O_PRE_FC_ELU;
  if (!w->w_gates1 || !w->b_gates1 || !w->w_gates2 || !w->b_gates2 || !w->w_lin || !w->b_lin ||
      (fc && (!w->w_fc || !w->b_fc)))
    return fail(L2O_ERR_ARG, "l2o_wpack_device: NULL weight pointer");
  hipStream_t s = (hipStream_t)stream;
  if (!opt(L2O_OPT_WPACK_NO_CLEAR)) HIP_TRY(hipMemsetAsync(wpack, 0, sizeof(float) * l2o_wpack_floats(cfg), s));
  hipLaunchKernelGGL(k_wpack, dim3(kNT * bx::nchunks(cfg->preprocess) + 4 * bxb::ntiles(cfg->preprocess)), dim3(64), 0, s, (int)cfg->preprocess, w->w_gates1, w->b_gates1, w->w_gates2,
                     w->b_gates2, w->w_lin, w->b_lin, w->w_fc, w->b_fc, wpack);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

static int adam_launch(float* w, float* m, float* v, const float* g, int64_t n, float lr_t, double beta1, double beta2,
                       double epsilon, const unsigned* guard, void* stream, const int* map = nullptr) {
  if (!w || !m || !v || !g || n < 0) return fail(L2O_ERR_ARG, "l2o_adam_step: bad argument");
  if (n == 0) return L2O_OK;
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, m, v, g, (long)n,
                     lr_t, (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)epsilon, guard, map);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}
int l2o_adam_step(float* w, float* m, float* v, const float* g, int64_t n, float lr_t, double beta1, double beta2,
                  double epsilon, void* stream) {
  return adam_launch(w, m, v, g, n, lr_t, beta1, beta2, epsilon, nullptr, stream);
}
int l2o_adam_step_gather(float* w, float* m, float* v, const float* G, const int32_t* map, int64_t n, float lr_t,
                         double beta1, double beta2, double epsilon, const void* unroll_workspace, void* stream) {
  if (!map) return fail(L2O_ERR_ARG, "l2o_adam_step_gather: NULL map");
  return adam_launch(w, m, v, G, n, lr_t, beta1, beta2, epsilon, static_cast<const unsigned*>(unroll_workspace), stream, map);
}
int l2o_adam_step_guarded(float* w, float* m, float* v, const float* g, int64_t n, float lr_t, double beta1,
                          double beta2, double epsilon, const void* unroll_workspace, void* stream) {
  // (the status word is the first member of the workspace header: l2o_unroll_status reads the same 4 bytes)
  return adam_launch(w, m, v, g, n, lr_t, beta1, beta2, epsilon, static_cast<const unsigned*>(unroll_workspace), stream);
}

size_t l2o_state_floats(int64_t B, int64_t D) {
  if (B <= 0 || D <= 0) return 0;
  return (size_t)B * tiles_per_problem(D) * kStateFloatsPerTile;
}

static int state_repack(float* h1, float* c1, float* h2, float* c2, float* st, int64_t B, int64_t D,
                        void* stream, int to_packed) {
  if (!h1 || !c1 || !h2 || !c2 || !st || B <= 0 || D <= 0) return fail(L2O_ERR_ARG, "state repack: bad argument");
  const int tpp = tiles_per_problem(D);
  const size_t total = (size_t)B * tpp * 64 * 20;
  hipLaunchKernelGGL(k_state_repack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h1,
                     c1, h2, c2, st, (int)B, (int)D, tpp, to_packed);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}
int l2o_state_pack(const float* h1, const float* c1, const float* h2, const float* c2, float* st, int64_t B,
                   int64_t D, void* stream) {
  return state_repack(const_cast<float*>(h1), const_cast<float*>(c1), const_cast<float*>(h2),
                      const_cast<float*>(c2), st, B, D, stream, 1);
}
int l2o_state_unpack(const float* st, float* h1, float* c1, float* h2, float* c2, int64_t B, int64_t D,
                     void* stream) {
  return state_repack(h1, c1, h2, c2, const_cast<float*>(st), B, D, stream, 0);
}

// ---- G = A^T B, the weight-gradient contraction of the meta-gradient (csrc/l2o_atb.h) ----------------------
static int atb_groups(int64_t R, int wgs_per_cu, hipStream_t s) {
  const int64_t nblk = (R + kAtbRows - 1) / kAtbRows;
  int g = wgs_per_cu * device_cu_count(s);                // persistent workgroups (k_atb: 72 KB of LDS each, k_atb_bx3: 52 | 58)
  if (g <= 0 || g > kAtbMaxGroups) g = kAtbMaxGroups;
  return (int)(nblk < g ? nblk : g);
}
size_t l2o_atb_workspace_bytes(int64_t R, int32_t KA, int32_t KB) {
  if (R <= 0 || KA <= 0 || KB <= 0) return 0;
  return sizeof(float) * (size_t)kAtbMaxGroups * KA * KB;
}
// mask 0: the dense product (fp32 matrix pipe, exact products).  mask 1 | 2: the weight-gradient blocks -- on the
// bf16 pipe (k_atb_bx3) unless the call asks for exact gates (L2O_OPT_EXACT_GATES: the fp32 pipe, bit-equal to the
// dense product on those blocks)
// compact_rows > 0 (mask 1 | 2, bf16 pipe only): A is the COMPACT operand of l2o_cwlstm_bwd_unroll_compact -- T + 1 blocks of
// compact_rows rows of KA - 40 floats -- and R = T * compact_rows rows of B (csrc/l2o_atb.h: atb_compact_off)
static int atb_launch(const float* A, const float* B, int64_t R, int KA, int KB, int mask, float* out, void* workspace,
                      hipStream_t s, int64_t compact_rows = 0, int P = 0) {
  float* part = static_cast<float*>(workspace);
  const int MT = (KA + 15) / 16, NT = (KB + 15) / 16;
  void (*fn)(const float*, const float*, long, int, int, float*) = nullptr;
  void (*fx)(const float*, const float*, long, int, int, float*, int, unsigned, int) = nullptr;
  int wgs = L2O_ATB_WGS_PER_CU;
  const bool bx3 = mask != 0 && !opt(L2O_OPT_EXACT_GATES);
  if (compact_rows > 0 && !bx3) return fail(L2O_ERR_UNSUPPORTED, "the compact A operand is read by the bf16x3 contraction only");
  if (mask == 1) {
    if (bx3) { fx = k_atb_bx3<6, 11, 1>; wgs = atb_bx3_wgs_per_cu<6, 11>(); } else fn = k_atb<6, 11, 1>;
  } else if (mask == 2) {
    if (bx3) { fx = k_atb_bx3<7, 12, 2>; wgs = atb_bx3_wgs_per_cu<7, 12>(); } else fn = k_atb<7, 12, 2>;
  } else if (MT <= 1 && NT <= 1) fn = k_atb<1, 1>;
  else if (MT <= 6 && NT <= 11) fn = k_atb<6, 11>;
  else fn = k_atb<7, 12>;
  const int groups = atb_groups(R, wgs, s);
  if (fx) {
    const int KAs = compact_rows > 0 ? KA - 2 * kH : KA;
    const uint64_t slice = compact_rows > 0 ? (uint64_t)compact_rows * KAs * sizeof(float) : 0;
    if (slice > 0xf0000000ull) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_wgrad_compact: %lld rows per step is too many", (long long)compact_rows);
    hipLaunchKernelGGL(fx, dim3(groups), dim3(256), 0, s, A, B, (long)R, KA, KB, part, KAs, (unsigned)slice, P);
  } else {
    hipLaunchKernelGGL(fn, dim3(groups), dim3(256), 0, s, A, B, (long)R, KA, KB, part);
  }
  HIP_TRY(hipGetLastError());
  const int n = KA * KB;
  hipLaunchKernelGGL(k_atb_reduce, dim3((n + 31) / 32), dim3(256), 0, s, part, groups, n, out, mask,
                     mask == 2 ? 12 : 11, KB);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

int l2o_atb(const float* A, const float* B, int64_t R, int32_t KA, int32_t KB, float* out, void* workspace, void* stream) {
  if (!A || !B || !out || !workspace || R <= 0 || KA <= 0 || KB <= 0) return fail(L2O_ERR_ARG, "l2o_atb: bad argument");
  if (KA > 112 || KB > 192) return fail(L2O_ERR_UNSUPPORTED, "l2o_atb: KA <= 112 and KB <= 192 (got %d x %d)", KA, KB);
  return atb_launch(A, B, R, KA, KB, 0, out, workspace, (hipStream_t)stream);
}

int32_t l2o_cwlstm_wgrad_dims(const l2o_net_cfg* cfg, int32_t* KA, int32_t* KB) {
  if (!cfg || !net_ok_for_mfma(cfg) || cfg->n_layers == 0) return fail(L2O_ERR_UNSUPPORTED, "l2o_cwlstm_wgrad: layers=(20,20) nets only");
  const bool fc = cfg->preprocess == L2O_PRE_FC_ELU;
  const int P = fc ? kH : (cfg->preprocess == L2O_PRE_LOGSIGN ? 2 : 1);
  if (KA) *KA = P + kH + 3 * kH + (fc ? 2 : 0) + 1;         // act1 | act2 | h2 | feats | 1   (BwdTileGeom::KA)
  if (KB) *KB = 8 * kH + 1 + (fc ? kH : 0);                 // dz1 | dz2 | dd | du             (BwdTileGeom::KB)
  return L2O_OK;
}

int l2o_cwlstm_wgrad(const l2o_net_cfg* cfg, const float* A, const float* Bm, int64_t R, float* G, void* workspace,
                     void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  int32_t KA = 0, KB = 0;
  const int rc = l2o_cwlstm_wgrad_dims(cfg, &KA, &KB);
  if (rc) return rc;
  if (!A || !Bm || !G || !workspace || R <= 0) return fail(L2O_ERR_ARG, "l2o_cwlstm_wgrad: bad argument");
  return atb_launch(A, Bm, R, KA, KB, cfg->preprocess == L2O_PRE_FC_ELU ? 2 : 1, G, workspace, (hipStream_t)stream);
}

int l2o_cwlstm_wgrad_compact(const l2o_net_cfg* cfg, const float* Ac, const float* Bm, int32_t T, int64_t rows, float* G,
                             void* workspace, void* stream) {
  OptScope opt_scope(cfg_optw(cfg));
  int32_t KA = 0, KB = 0;
  const int rc = l2o_cwlstm_wgrad_dims(cfg, &KA, &KB);
  if (rc) return rc;
  if (!Ac || !Bm || !G || !workspace || T <= 0 || rows <= 0) return fail(L2O_ERR_ARG, "l2o_cwlstm_wgrad_compact: bad argument");
  const bool fc = cfg->preprocess == L2O_PRE_FC_ELU;
  const int P = fc ? kH : (cfg->preprocess == L2O_PRE_LOGSIGN ? 2 : 1);
  return atb_launch(Ac, Bm, (int64_t)T * rows, KA, KB, fc ? 2 : 1, G, workspace, (hipStream_t)stream, rows, P);
}

int l2o_reduce_fx(const float* fx_part, int32_t T1, int32_t B_local, int32_t B_global, float* fx, void* stream) {
  if (!fx_part || !fx || T1 <= 0 || B_local <= 0 || B_global < B_local)
    return fail(L2O_ERR_ARG, "l2o_reduce_fx: bad argument");
  hipLaunchKernelGGL(k_reduce_fx, dim3(T1), dim3(64), 0, (hipStream_t)stream, fx_part, (int)T1, (int)B_local,
                     1.0f / (float)B_global, fx);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

// ---- small vector passes of the meta-gradient (csrc/l2o_vecops.h; ABI v11) ---------------------------------
int l2o_suffix_sums(const float* const* g, const float* g_final, float* out, int64_t n, int32_t T, void* stream) {
  if (!g || !g_final || !out || n <= 0 || T < 0) return fail(L2O_ERR_ARG, "l2o_suffix_sums: bad argument");
  if (T == 0) return L2O_OK;
  hipLaunchKernelGGL(k_suffix_sums, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g, g_final, out,
                     (long)n, (int)T);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}
size_t l2o_colsum_scratch_floats(int64_t batch, int32_t cols) {
  if (batch <= 0 || cols <= 0) return 0;
  return (size_t)batch * kColsumSplit * (size_t)cols;
}
int l2o_colsum(const float* A, int64_t batch, int64_t rows, int32_t cols, float* out, int32_t accumulate, float* scratch,
               void* stream) {
  if (!A || !out || !scratch || batch <= 0 || rows <= 0 || cols <= 0 || batch > 65535)
    return fail(L2O_ERR_ARG, "l2o_colsum: bad argument");
  const unsigned gx = (unsigned)((cols + 255) / 256);
  hipLaunchKernelGGL(k_colsum_part, dim3(gx, kColsumSplit, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, A, (long)rows,
                     (int)cols, scratch);
  hipLaunchKernelGGL(k_colsum_final, dim3(gx, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, scratch, (int)cols, out,
                     (int)accumulate);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}
int l2o_lincomb(float* out, const float* a, float ca, const float* b, float cb, const float* c, float cc, int64_t n,
                void* stream) {
  if (!out || !a || n <= 0) return fail(L2O_ERR_ARG, "l2o_lincomb: bad argument");
  hipLaunchKernelGGL(k_lincomb, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, a, ca, b, cb, c, cc,
                     (long)n);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}
int l2o_rnnprop_input_adjoint(const float* Bm, int64_t ldb, int32_t du_col, int32_t H, const float* w_fc, const float* g,
                              const float* m, const float* v, double pow1, double pow2, double beta1, double beta2,
                              float* dm, float* dv, float* dg, int64_t n, void* stream) {
  if (!Bm || !w_fc || !g || !m || !v || !dm || !dv || !dg || n <= 0 || H <= 0 || du_col < 0 || ldb < du_col + H)
    return fail(L2O_ERR_ARG, "l2o_rnnprop_input_adjoint: bad argument");
  RnnpropAdjArgs a;
  a.Bm = Bm; a.ldb = (long)ldb; a.du_col = du_col; a.H = H; a.w_fc = w_fc; a.g = g; a.m = m; a.v = v;
  a.om1 = (float)(1.0 - pow1); a.om2 = (float)(1.0 - pow2);
  a.b1 = (float)beta1; a.b2 = (float)beta2;
  a.omb1 = 1.0f - a.b1; a.omb2 = 1.0f - a.b2;               // (fp32, like the forward's 1 - beta)
  a.dm = dm; a.dv = dv; a.dg = dg; a.n = (long)n;
  hipLaunchKernelGGL(k_rnnprop_input_adjoint, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return L2O_OK;
}

}  // extern "C"
