// l2o_step.h -- the step-granular optimizer step: k_cwlstm_step (state in HBM) and the Linear-only k_linear_step.
#pragma once
#include "l2o_lstm_bx3.h"
#include "l2o_params.h"

// ---------------------------------------------------------------------------
// K1: step-granular optimizer step on a gradient panel (state in HBM).
// One wave per 16-coordinate tile, grid-stride over tiles; weights live in VGPRs.
// HBM traffic per coordinate: 320 B state read + 320 B write + g + x r/w.
// ---------------------------------------------------------------------------
// s_waitcnt vmcnt(n) for a run-time n from the small set the step kernel needs
__device__ __forceinline__ void wait_vmcnt_le(int n) {
#define L2O_VMCASE(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
  switch (n) {
    L2O_VMCASE(0) L2O_VMCASE(5) L2O_VMCASE(7) L2O_VMCASE(9) L2O_VMCASE(10) L2O_VMCASE(12) L2O_VMCASE(14)
    L2O_VMCASE(15) L2O_VMCASE(17) L2O_VMCASE(18) L2O_VMCASE(19) L2O_VMCASE(22) L2O_VMCASE(23) L2O_VMCASE(24)
    L2O_VMCASE(28) L2O_VMCASE(29) L2O_VMCASE(33)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
#undef L2O_VMCASE
}

constexpr int kStepRing = 4;       // LDS ring slots per wave
constexpr int kStepAhead = 3;      // tiles in flight ahead of the one being computed

// up to kMaxStepSegs (variable, state) panels updated by one launch of the same network
constexpr int kMaxStepSegs = 8;
struct StepSegs {
  int n;
  int tile_end[kMaxStepSegs];     // running tile count (exclusive end) per segment
  int tpp[kMaxStepSegs], D[kMaxStepSegs];
  const float* g[kMaxStepSegs];
  float* m[kMaxStepSegs];
  float* v[kMaxStepSegs];
  float* st[kMaxStepSegs];
  float* x[kMaxStepSegs];
  float* st_out[kMaxStepSegs];    // where the new state / moments go (== st / m / v unless the caller records history)
  float* m_out[kMaxStepSegs];
  float* v_out[kMaxStepSegs];
};

template <int PRE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_cwlstm_step(
    NetParams np, StepSegs sg, float om1, float om2) {
  // One wave per SIMD (the bf16x3 weights take 180-240 registers), so memory latency is
  // hidden by DEPTH instead of occupancy: a wave walks its tiles with the next three tiles'
  // inputs in flight as LDS-DMA (global_load_lds: packed state 5 x dwordx4 per lane, and
  // g / x / m / v one dword each -- no staging registers), consumed after a counted
  // s_waitcnt.  VMEM operations retire in issue order, so "at most N outstanding" with
  // N = (later prefetches) x (loads per prefetch) + (later tiles' state stores) guarantees
  // that this tile has landed; the masked x / m / v stores only make the wait stricter.
  constexpr int NL = PRE == L2O_PRE_FC_ELU ? 9 : 7;              // VMEM loads per prefetched tile
  constexpr int kSlotF4 = 5 * 64 + 64;                           // float4 per slot: state + {g,x,m,v} rows
  __shared__ float4 sbuf[4][kStepRing][kSlotF4];
  __shared__ __attribute__((aligned(16))) float bias_s[bx::kBiasWords];   // the gate biases = accumulator inits
  bx::stage_bias(bias_s, np.wpack, PRE, threadIdx.x, blockDim.x);       // (ordered by the __syncthreads() of the fragment staging)
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // scalar: the waits below branch on it
  const int c = lane & 15, q = lane >> 4;
  const int wave = blockIdx.x * (blockDim.x >> 6) + wv;
  const int nwaves = gridDim.x * (blockDim.x >> 6);
  const int ntiles = sg.tile_end[sg.n - 1];
  // ---- the bf16x3 weight fragments (60 / 80 KB) reach the four waves through LDS: one DMA copy per
  // workgroup instead of four L2 reads; the staging area is the (not yet used) prefetch ring
  constexpr bool PK = bx::packed_default(PRE);
  bx::NetWB<PRE, PK> w;
  {
    constexpr int kFrags = bx::nchunks(PRE) * kNT * bx::frags(PK);   // 1 KB each = one wave-wide dwordx4
    static_assert(kFrags * 1024 <= (int)sizeof(sbuf), "staging area");
    float4* stage = &sbuf[0][0][0];
    const float* src = np.wpack + bx::frag_off(PRE, PK, 0, 0, 0) + lane * 4;
#pragma unroll
    for (int f = 0; f < (kFrags + 3) / 4; ++f) {
      const int fr = 4 * f + wv;
      if (fr < kFrags)
        __builtin_amdgcn_global_load_lds((gbl_void*)(src + fr * bx::kFragWords), (lds_void*)(stage + fr * 64), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int ch = 0; ch < bx::NetWB<PRE, PK>::NCH; ++ch)
#pragma unroll
      for (int t = 0; t < kNT; ++t)
#pragma unroll
        for (int s3 = 0; s3 < bx::frags(PK); ++s3) {
          const float4 v4 = stage[((ch * kNT + t) * bx::frags(PK) + s3) * 64 + lane];
          w.a[ch][t][s3] = __builtin_bit_cast(bx::u32x4, v4);
        }
    __syncthreads();                                               // everyone holds its copy: the ring may be used
#pragma unroll
    for (int ch = 0; ch < bx::NetWB<PRE, PK>::NCH; ++ch)           // fragments -> AGPRs (MFMA reads them there)
#pragma unroll
      for (int t = 0; t < kNT; ++t)
#pragma unroll
        for (int s3 = 0; s3 < bx::frags(PK); ++s3) asm volatile("" : "+a"(w.a[ch][t][s3]));
  }
  if (wave >= ntiles) return;
  const int ntl = (ntiles - wave + nwaves - 1) / nwaves;         // tiles of this wave
  // global tile index -> segment (wave-uniform scalar work)
  struct Loc { const float* g; float *m, *v, *st, *x, *st_out, *m_out, *v_out; int tile, tpp, D; };
  Loc L0;                                                        // the common single-panel launch: fields read once
  L0.tile = 0; L0.g = sg.g[0]; L0.m = sg.m[0]; L0.v = sg.v[0]; L0.st = sg.st[0]; L0.x = sg.x[0];
  L0.st_out = sg.st_out[0]; L0.m_out = sg.m_out[0]; L0.v_out = sg.v_out[0];
  L0.tpp = sg.tpp[0]; L0.D = sg.D[0];
  const bool single = sg.n == 1;
  auto locate = [&](int tile) {
    Loc L = L0;
    if (single) {
      L.tile = tile;
      return L;
    }
    int sidx = 0;
    while (sidx + 1 < sg.n && tile >= sg.tile_end[sidx]) ++sidx;
    L.tile = tile - (sidx ? sg.tile_end[sidx - 1] : 0);
    L.g = sg.g[sidx]; L.m = sg.m[sidx]; L.v = sg.v[sidx]; L.st = sg.st[sidx]; L.x = sg.x[sidx];
    L.st_out = sg.st_out[sidx]; L.m_out = sg.m_out[sidx]; L.v_out = sg.v_out[sidx];
    L.tpp = sg.tpp[sidx]; L.D = sg.D[sidx];
    return L;
  };
  bx::load_netw<PRE, false>(w, np.wpack, lane);                  // the small fp32 weights
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // weights landed: the VMEM queue is empty
  bx::set_bias(w, bias_s, q);
  // dead lanes (j >= D in the last tile of a problem) read the problem's last coordinate:
  // branch-free loads, masked where they are used
  auto prefetch = [&](int k, int kslot) {
    const Loc L = locate(wave + k * nwaves);
    const int tile = L.tile, tpp = L.tpp, D = L.D;
    const float *g = L.g, *x = L.x, *mbuf = L.m, *vbuf = L.v, *st = L.st;
    float4* slot = sbuf[wv][kslot % kStepRing];
    const float* src = st + (size_t)tile * kStateFloatsPerTile + lane * 4;
#pragma unroll
    for (int jj = 0; jj < 5; ++jj)
      __builtin_amdgcn_global_load_lds((gbl_void*)(src + jj * 256), (lds_void*)(slot + jj * 64), 16, 0, 0);
    const int b_ = tile / tpp, tw_ = tile - b_ * tpp;
    const size_t idx_ = (size_t)b_ * D + min(tw_ * kTile + c, D - 1);
    float* aux = reinterpret_cast<float*>(slot + 5 * 64);
    __builtin_amdgcn_global_load_lds((gbl_void*)(g + idx_), (lds_void*)(aux), 4, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void*)(x + idx_), (lds_void*)(aux + 64), 4, 0, 0);
    if (PRE == L2O_PRE_FC_ELU) {
      __builtin_amdgcn_global_load_lds((gbl_void*)(mbuf + idx_), (lds_void*)(aux + 128), 4, 0, 0);
      __builtin_amdgcn_global_load_lds((gbl_void*)(vbuf + idx_), (lds_void*)(aux + 192), 4, 0, 0);
    }
  };
  // unconditional prologue (a wave with fewer than three tiles re-fetches its last one): a
  // static VMEM count keeps hipcc from draining the queue at the loop entry
#pragma unroll
  for (int k = 0; k < kStepAhead; ++k) prefetch(min(k, ntl - 1), k);
  for (int k = 0; k < ntl; ++k) {
    const Loc L = locate(wave + k * nwaves);
    const int tile = L.tile, tpp = L.tpp, D = L.D;
    float *x = L.x, *mbuf = L.m_out, *vbuf = L.v_out, *st = L.st_out;
    const int b = tile / tpp, tw = tile - b * tpp;
    const int j = tw * kTile + c;
    const bool live = j < D;
    const size_t idx = (size_t)b * D + j;
#ifndef L2O_ABLATE_STEP_LOAD
    wait_vmcnt_le(NL * min(kStepAhead - 1, ntl - 1 - k) + 5 * min(k, kStepAhead));
#endif
    // the slot is read with inline-asm ds_reads: hipcc cannot tell the ring slots apart and
    // would drain the whole VMEM queue (vmcnt(0)) before an ordinary LDS read of sbuf
    const unsigned slot_addr =
        (unsigned)(size_t)(__attribute__((address_space(3))) char*)(&sbuf[wv][k % kStepRing][0]) + lane * 16;
    const unsigned aux_addr = slot_addr - lane * 12 + 5 * 1024;
    TileState s;
    float gv, xv, m = 0.f, v = 0.f;
    {
      float4 v0, v1, v2, v3, v4;
      if (PRE == L2O_PRE_FC_ELU)
        asm volatile(
            "ds_read_b128 %0, %9\n\tds_read_b128 %1, %9 offset:1024\n\tds_read_b128 %2, %9 offset:2048\n\t"
            "ds_read_b128 %3, %9 offset:3072\n\tds_read_b128 %4, %9 offset:4096\n\t"
            "ds_read_b32 %5, %10\n\tds_read_b32 %6, %10 offset:256\n\tds_read_b32 %7, %10 offset:512\n\t"
            "ds_read_b32 %8, %10 offset:768\n\ts_waitcnt lgkmcnt(0)"
            : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3), "=&v"(v4), "=&v"(gv), "=&v"(xv), "=&v"(m), "=&v"(v)
            : "v"(slot_addr), "v"(aux_addr)
            : "memory");
      else
        asm volatile(
            "ds_read_b128 %0, %7\n\tds_read_b128 %1, %7 offset:1024\n\tds_read_b128 %2, %7 offset:2048\n\t"
            "ds_read_b128 %3, %7 offset:3072\n\tds_read_b128 %4, %7 offset:4096\n\t"
            "ds_read_b32 %5, %8\n\tds_read_b32 %6, %8 offset:256\n\ts_waitcnt lgkmcnt(0)"
            : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3), "=&v"(v4), "=&v"(gv), "=&v"(xv)
            : "v"(slot_addr), "v"(aux_addr)
            : "memory");
      // slot k is in registers now; slot (k+3)%4 = (k-1)%4 is free for the next prefetch
      const float e[20] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y,
                           v2.z, v2.w, v3.x, v3.y, v3.z, v3.w, v4.x, v4.y, v4.z, v4.w};
#pragma unroll
      for (int t = 0; t < kNT; ++t) { s.h1[t] = e[t]; s.c1[t] = e[5 + t]; s.h2[t] = e[10 + t]; s.c2[t] = e[15 + t]; }
    }
    if (!live) { gv = 0.0f; m = 0.0f; v = 0.0f; }
#ifndef L2O_ABLATE_STEP_LOAD
    if (k + kStepAhead < ntl) prefetch(k + kStepAhead, k + kStepAhead);
#endif
    float in0, in1;
    if (PRE == L2O_PRE_FC_ELU) {
      rnnprop_inputs(gv, m, v, np.beta1, np.beta2, np.omb1, np.omb2, om1, om2, in0, in1);
      if (!live) { in0 = 0.0f; in1 = 0.0f; }
      if (live && q == 0) { mbuf[idx] = m; vbuf[idx] = v; }
    } else {
      preprocess_grad<PRE>(gv, np.k_inv_ln2, np.exp_k, in0, in1);
    }
    float d = bx::tile_step<PRE>(w, s, in0, in1, q);
    if (np.tanh_output) d = tanhf_(d);
    d *= np.scale;
    if (live && q == 0) x[idx] = xv + d;
#ifndef L2O_ABLATE_STEP_STORE
    store_tile_state(s, st + (size_t)tile * kStateFloatsPerTile, lane);
#else
    if (d == 1234.5f) store_tile_state(s, st + (size_t)tile * kStateFloatsPerTile, lane);
#endif
  }
}

// layers == (): StandardDeepLSTM with no cores = Linear on the preprocessed gradient
// (DM/networks.py:225-232 with an empty DeepRNN; used by the meta_test.py:50-69 KAT).
// lw = {w0, w1, b}
template <int PRE>
__global__ void k_linear_step(NetParams np, const float* __restrict__ g, float* __restrict__ x, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float w0 = np.wpack[0], w1 = np.wpack[1], bl = np.wpack[2];
  float in0, in1;
  preprocess_grad<PRE>(g[i], np.k_inv_ln2, np.exp_k, in0, in1);
  float d = __builtin_fmaf(in1, w1, in0 * w0) + bl;
  if (np.tanh_output) d = tanhf_(d);
  x[i] += d * np.scale;
}
