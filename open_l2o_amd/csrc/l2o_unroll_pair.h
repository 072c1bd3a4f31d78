// l2o_unroll_pair.h -- the fused persistent unroll with every problem split over TWO
// workgroups (two CUs).  Launched by l2o_unroll.hip (launch_unroll_ch).
//
// Why: a batch of B <= #CU/2 problems (BASELINE config 2: B = 128 on 256 CUs) leaves half
// the chip idle with one problem per CU, and the per-step critical path of a problem is
// bound by its own SIMDs' fp32 issue cycles.  Splitting the coordinates (tiles) of a problem
// over two CUs halves that path; the price is ONE exchange per step between the two partner
// workgroups: each half multiplies ITS columns of W with its part of the scaled iterate and
// the halves swap the partial residuals (one granule per row, 128 each way for d = 128).
//
// Exchange protocol (placement independent, MI355X_MICROARCH.md "valid forms"): data-tagged
// 8-byte granules {float x, uint tag = launch salt | step + 1} written with ONE agent-scope relaxed atomic
// 64-bit store (global_store_dwordx2 sc1: write-through) and polled with agent-scope relaxed
// 64-bit loads (sc1: L1 bypass).  A granule is self-validating, so no flag, no fence.  Two
// parity buffers: a workgroup can publish step t+2 only after it has consumed the partner's
// step t+1, which the partner publishes only after it consumed ours of step t+1 -- the
// buffer of parity (t+2)&1 = t&1 is therefore free.  The granule area is zeroed by a
// hipMemsetAsync ahead of every launch (tag 0 is never valid) and the tags carry the launch
// sequence number of the workspace header on top.  Every spin is bounded: on timeout the kernel
// raises the STICKY ws->status and stops waiting (results are then garbage and the host reports
// L2O_ERR_HIP) -- a non-resident partner can never hang the GPU.  Confirmed same-XCD partners
// publish with plain stores (see the handshake below; L2O_OPT_PAIR_PLAIN_STORES).
//
// The matrix never touches LDS: a half keeps its SQ x SQ/2 column block of W twice in
// registers (row-major for the partial residual, column-major for the gradient: 2 x SQ/4
// floats per lane), because with W in LDS the two GEMV passes were LDS-bandwidth bound
// (1 KB per wave ds_read_b128 x 32 per wave per pass = 1024 cycles per CU).
#pragma once
#include "l2o_lstm_bx3.h"
#include "l2o_params.h"

struct PairWs {               // header of the caller-owned workspace (never cleared by the library)
  unsigned status;            // 0 ok, 1 = partner timeout.  STICKY: raised by the kernel, cleared by the caller
  unsigned seq;               // launch sequence number: read by every workgroup of a launch (tag salt), advanced
                              // by k_combine_halves after it -- the library keeps no host-side launch state
  unsigned fault;             // TEST HOOK (ABI v12; 0 in production): non-zero = every workgroup behaves as if its partner
                              // never showed up -- raises `status` at once and stops polling.  Lets a test force the
                              // timeout path (and the host's recovery from it) deterministically; the caller clears it.
  unsigned pad0;
  long long ticks;            // ABI v12 (bytes 16..23): shader-clock cycles (s_memtime) wave 0 of workgroup 0 spent in the step
                              // loop of the LAST launch on this workspace -- T steps + the final loss evaluation.  What
                              // bench.py's roofline block divides its work model by: measured cycles, no clock assumption
  long long ticks_total;      // (bytes 24..31) the same wave from kernel entry to its last store: prologue and epilogue included
  unsigned pad[8];            // -DL2O_PROFILE_PHASES build: the launch marks of wave 0 of workgroup 0 outside the step loop, cycles
                              // since kernel entry (L2O_LAUNCH_MARK; scripts/phase_profile.py names them); else unused
  long long phases[16];       // phase clock dump of the -DL2O_PROFILE_PHASES build (else unused)
};
static_assert(sizeof(PairWs) == 64 + 128, "workspace header layout (include/l2o_abi.h)");

struct UnrollPairArgs {
  UnrollArgs u;
  PairWs* ws;
  unsigned long long* xbuf;   // [B][2 halves][2 parities][SQ] granules (partial residuals)
  float* fx_half;             // [(T+1)][B][2 * NWH]: one partial per (step, problem, wave)
  unsigned use_salt;          // tags carry the launch sequence in their upper bits (T + 1 < 65 535): a granule left by an
                              // earlier launch never matches, on top of the memset of the granule area ahead of every launch
  unsigned plain_stores;      // L2O_OPT_PAIR_PLAIN_STORES: a confirmed same-XCD pair publishes with plain stores
  int b0, nb;                 // this launch steps problems [b0, b0 + nb) of the shard: a batch of more than #CU / 2 problems
                              // runs as consecutive launches of <= #CU / 2 (exchange granules and loss partials are per launch)
  unsigned fast_load;         // the FAST kernel only (the launcher sets it for a problem of full tiles, M = D = SQ): load W without
                              // predicates.  LAST: the gather kernel's argument block keeps the layout its code was tuned at
};

__device__ __forceinline__ unsigned long long pack_granule(float v, unsigned tag) {
  return ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v);
}

// N ds_read_b128 at p, p + 64 B, ... issued together, then one s_waitcnt lgkmcnt(0).
// NOT directly behind MFMAs: the hazard recognizer does not see loads inside inline asm, so nothing would keep
// their data from landing in a register an in-flight MFMA still reads as SrcC (the allocator hands dead chain
// registers out at once).  Every use below sits behind an LDS barrier (>= the 18 wait states of the longest
// MFMA WAR hazard); an experiment in k_mlp_unroll that issued such reads right after 60 MFMAs produced NaNs
// (profiles/archive_r01_r03/r02u_mlp_variants.txt).
template <int N>
__device__ __forceinline__ void lds_read_f4(float4 (&v)[N], const float* p) {
  const unsigned addr = (unsigned)(size_t)(__attribute__((address_space(3))) const char*)p;
  static_assert(N == 1 || N == 2 || N == 4 || N == 8, "");
  if constexpr (N == 1)
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v[0]) : "v"(addr) : "memory");
  if constexpr (N == 2)
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:64\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]) : "v"(addr) : "memory");
  if constexpr (N == 4)
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:64\n\tds_read_b128 %2, %4 offset:128\n\t"
                 "ds_read_b128 %3, %4 offset:192\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]) : "v"(addr) : "memory");
  if constexpr (N == 8)
    asm volatile("ds_read_b128 %0, %8\n\tds_read_b128 %1, %8 offset:64\n\tds_read_b128 %2, %8 offset:128\n\t"
                 "ds_read_b128 %3, %8 offset:192\n\tds_read_b128 %4, %8 offset:256\n\tds_read_b128 %5, %8 offset:320\n\t"
                 "ds_read_b128 %6, %8 offset:384\n\tds_read_b128 %7, %8 offset:448\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
                 : "v"(addr) : "memory");
}

// Round 4: compiler-visible 16-byte LDS reads (the compiler places the s_waitcnt itself) in front of independent VALU
// work of the caller, ordered with sched_group_barrier: N ds_read_b128 back to back, then the VALU block that hides their
// latency.  (A first attempt with two asm statements -- issue / wait with the destinations as tied operands -- was WRONG:
// the register allocator split the live ranges and copied the destinations between the two statements, i.e. before the
// data had landed.)
template <int N>
__device__ __forceinline__ void lds_load_f4(l2o::f32x4 (&v)[N], const float* p) {
  const auto* q = reinterpret_cast<const __attribute__((address_space(3))) l2o::f32x4*>(
      (const __attribute__((address_space(3))) float*)p);
#pragma unroll
  for (int m = 0; m < N; ++m) v[m] = q[4 * m];             // (+64 bytes per read: the row / column chunk of tile m)
}
// (dot4 of l2o_params.h with the LDS operand as an ext-vector register quad: no float4 <-> f32x4 copies)
__device__ __forceinline__ void dot4v(const float4 a, const l2o::f32x4 b, float4& acc) {
  acc.x = __builtin_fmaf(a.x, b[0], acc.x);
  acc.y = __builtin_fmaf(a.y, b[1], acc.y);
  acc.z = __builtin_fmaf(a.z, b[2], acc.z);
  acc.w = __builtin_fmaf(a.w, b[3], acc.w);
}

// The same four chains as two v_pk_fma_f32 (lanes x,y | z,w): half the GEMV's instructions; the operands are register
// quads (W packed once in the prologue, x / r straight from ds_read_b128), so the halves are sub-registers, no copies.
// hsum4pk adds in hsum4's order: bit-identical to dot4v + hsum4.  (L2O_GEMV_PK=0 restores the scalar FMAs.)
// Measured (profiles/archive_r04/r04aa_*): config 2, ONE wave per SIMD -- the wave is issue-bound and 32 fewer instructions per step are
// worth 4 % (8.78 -> 9.15 G); with TWO waves per SIMD (k_unroll_lds) the VALU pipe is the limit, a packed FMA
// occupies it twice as long, and the packed form is 1.5-3 % SLOWER: those keep the scalar FMAs.
#ifndef L2O_GEMV_PK
#define L2O_GEMV_PK 1
#endif
#ifndef L2O_GEMV_PK_G
#define L2O_GEMV_PK_G L2O_GEMV_PK   // the g pass alone (the 16 FMAs behind barrier B2; profiles/r09_split_beside_mfma_ab.txt)
#endif
struct Acc4pk { l2o::bx::f32x2 lo, hi; };
__device__ __forceinline__ void dot4pk(const l2o::f32x4 a, const l2o::f32x4 b, Acc4pk& acc) {
  acc.lo = __builtin_elementwise_fma(__builtin_shufflevector(a, a, 0, 1), __builtin_shufflevector(b, b, 0, 1), acc.lo);
  acc.hi = __builtin_elementwise_fma(__builtin_shufflevector(a, a, 2, 3), __builtin_shufflevector(b, b, 2, 3), acc.hi);
}
__device__ __forceinline__ float hsum4pk(const Acc4pk& a) { return (a.lo.x + a.lo.y) + (a.hi.x + a.hi.y); }
__device__ __forceinline__ l2o::f32x4 as_quad(const float4 v) { return l2o::f32x4{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ void dot4q(const l2o::f32x4 a, const l2o::f32x4 b, float4& acc) {
  acc.x = __builtin_fmaf(a[0], b[0], acc.x);
  acc.y = __builtin_fmaf(a[1], b[1], acc.y);
  acc.z = __builtin_fmaf(a[2], b[2], acc.z);
  acc.w = __builtin_fmaf(a[3], b[3], acc.w);
}

// HIST: also record the per-step history for the meta-gradient (l2o_unroll_record); a template
// parameter so that the plain unroll carries none of it
// EXACT (L2O_OPT_EXACT_GATES): the fp32 MFMA gate GEMM (bit-equal to an fmaf chain) instead of the bf16x3 split
#ifndef L2O_PAIR_LDS_BARRIERS
#define L2O_PAIR_LDS_BARRIERS 0
#endif
// (round 4 also ran this body with the fragments in LDS and two workgroups per CU -- k_unroll_pair2; it measured like
//  k_unroll_lds and was removed in round 5)
// Launch marks (the -DL2O_PROFILE_PHASES build only; the product build compiles them to nothing): where wave 0 of workgroup 0
// stands, in cycles since kernel entry, at the stations of the prologue and the epilogue.  A mark pins the schedule
// (nothing moves across it); the `landed` form also drains the wave's outstanding memory operations first.
//   0 salt known | 1 W / fragment loads issued | 2 every prologue load landed | 3 handshake done | 4 loop entry |
//   5 loop exit | 6 last store issued | 7 last store acknowledged
#ifdef L2O_PROFILE_PHASES
#define L2O_LAUNCH_MARK(i)                                                                  \
  do {                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    launch_marks[i] = (unsigned)(__builtin_readcyclecounter() - kernel_t0);                 \
    __builtin_amdgcn_sched_barrier(0);                                                      \
  } while (0)
#define L2O_LAUNCH_MARK_LANDED(i)                                                           \
  do {                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                      \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                             \
    L2O_LAUNCH_MARK(i);                                                                     \
  } while (0)
#else
#define L2O_LAUNCH_MARK(i) do {} while (0)
#define L2O_LAUNCH_MARK_LANDED(i) do {} while (0)
#endif

// Two bodies, one step loop (l2o_unroll_pair_loop.h).  unroll_pair_body_gather is the prologue every shape ran until round 8
// and ragged shapes still run (FAST = false): per-element predicated loads of W, its load phases one behind the other.
// unroll_pair_body (FAST = true) is the prologue of a problem of full tiles, M = D = SQ -- the launcher picks it.
template <int PRE, int KIND, int CH, bool HIST, bool EXACT>
__device__ __forceinline__ void unroll_pair_body_gather(const UnrollPairArgs& pa) {
  const long long kernel_t0 = __builtin_readcyclecounter();
#ifdef L2O_PROFILE_PHASES
  unsigned launch_marks[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  constexpr int SQ = 16 * CH;            // padded rows (and columns) of the problem
  constexpr int NWH = CH / 2;            // waves (tiles) per half; tiles beyond the real count idle
  constexpr int NC = 16 * NWH;           // columns (coordinates) owned by a half = SQ / 2
  __shared__ __attribute__((aligned(16))) float xs[NC];   // this half's scaled iterate
  __shared__ __attribute__((aligned(16))) float rs[SQ];   // the full residual
  const UnrollArgs& a = pa.u;
  const ProbParams& pp = a.pp;
  const int D = pp.D, M = pp.M;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  // partner workgroups are blockIdx b and b + 8 inside a group of 16 (same XCD under the
  // observed round-robin placement -- a speed choice only)
  const int bid = blockIdx.x;
  const unsigned salt = pa.use_salt ? ((pa.ws->seq + 1u) & 0x7fffu) << 16 : 0u;
#ifdef L2O_PROFILE_PHASES
  asm volatile("" ::"s"(salt));                         // (the mark waits for the sequence word)
#endif
  L2O_LAUNCH_MARK(0);
  const int half = (bid >> 3) & 1;
  const int bl = ((bid >> 4) << 3) | (bid & 7);         // problem index inside this launch's chunk
  if (bl >= pa.nb) return;                              // padding blocks of the last group of 16 (both halves)
  const int b = pa.b0 + bl;                             // problem index inside the batch shard
  const int tile_in_prob = half * NWH + wv;             // this wave's coordinate tile
  // GEMV role of a lane = its LSTM role: row / column gr = c, 16-byte chunk gq = q.  The four chunk partial sums
  // of a row / column then sit on the lanes (c, 0..3) and two permlane swaps add them INTO the lanes that feed
  // the gradient to the network -- no ds_bpermute (an LDS round trip) between the g pass and the gate math.
  const int gq = q, gr = c;

  // ---- the matrix lives in registers: no LDS bandwidth in the two GEMV passes -------------
  //  wr[p][m] : row (2 wv + p) 16 + gr, own columns 16 m + 4 gq + {0..3}     (partial r = W xs)
  //  wt[m]    : own column wv 16 + gr,   rows       16 m + 4 gq + {0..3}     (g = W^T r)
  const float* Wb = pp.W + (pp.w_shared ? (size_t)0 : (size_t)b * M * D);
  const int col0 = half * NC;
  float4 wr[2][NWH], wt[CH];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int row = (2 * wv + p) * kTile + gr;
#pragma unroll
    for (int m = 0; m < NWH; ++m) {
      float e[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int col = col0 + 16 * m + 4 * gq + k;
        e[k] = (row < M && col < D) ? Wb[(size_t)row * D + col] : 0.0f;
      }
      wr[p][m] = make_float4(e[0], e[1], e[2], e[3]);
    }
  }
  {
    const int col = col0 + wv * kTile + gr;
#pragma unroll
    for (int m = 0; m < CH; ++m) {
      float e[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = 16 * m + 4 * gq + k;
        e[k] = (row < M && col < D) ? Wb[(size_t)row * D + col] : 0.0f;
      }
      wt[m] = make_float4(e[0], e[1], e[2], e[3]);
    }
  }
  constexpr bool kPk = L2O_GEMV_PK != 0;                    // packed GEMV FMAs: one wave per SIMD (see dot4pk)
  l2o::f32x4 wrq[2][NWH], wtq[CH];                          // (the same values as register quads for the packed FMAs)
#pragma unroll
  for (int m = 0; m < NWH; ++m) { wrq[0][m] = as_quad(wr[0][m]); wrq[1][m] = as_quad(wr[1][m]); }
#pragma unroll
  for (int m = 0; m < CH; ++m) wtq[m] = as_quad(wt[m]);
  // the residual rows this lane finishes: gq == 0 -> p = 0, gq == 1 -> p = 1 (gq 2, 3 idle)
  const int myrow = (2 * wv + (gq & 1)) * kTile + gr;
  const float myy = (gq < 2 && myrow < M) ? pp.y[(size_t)b * M + myrow] : 0.0f;
  const bool row_counted = gq < 2 && (half == 0 ? (myrow < NC) : (myrow >= NC));   // every row once per pair

  // ---- per-lane persistent registers -------------------------------------
  // <= 4 waves per workgroup: bf16x3 gate GEMM, weights in VGPR + AGPR
  using Core = LstmCorePair<PRE, !EXACT, false>;
  Core core;
  core.load(a.np.wpack, lane);
  core.pin();   // fragments -> AGPRs (MFMA reads them there): the VGPRs hold W, the state and the gate math
  __shared__ __attribute__((aligned(16))) float bias_s[Core::kBiasFloats];   // the gate biases = accumulator inits
  core.stage_bias(bias_s, a.np.wpack, tid, blockDim.x, q);   // (the handshake's __syncthreads() below orders it)
  L2O_LAUNCH_MARK(1);
  const int j = tile_in_prob * kTile + c;
  const bool live = j < D;
  const size_t idx = (size_t)b * D + j;
  const int tpp = (D + kTile - 1) / kTile;
  const bool tile_real = tile_in_prob < tpp;            // the padded tile of an odd tile count is idle
  TileState s;
  float* st_tile = a.st + ((size_t)b * tpp + (tile_real ? tile_in_prob : 0)) * kStateFloatsPerTile;
  if (tile_real && !a.zero_state) load_tile_state(s, st_tile, lane);
  else {
#pragma unroll
    for (int t = 0; t < kNT; ++t) s.h1[t] = s.c1[t] = s.h2[t] = s.c2[t] = 0.0f;
  }
  float xv = live ? (a.x_in ? a.x_in : a.x)[idx] : 0.0f;
  const float sc = (live && pp.x_scale) ? pp.x_scale[idx] : 1.0f;
  float cj = 0.0f;
  constexpr bool kCos = KIND == L2O_PROB_RASTRIGIN || KIND == L2O_PROB_SQUARE_COS;
  if (kCos) cj = live ? pp.C[idx] : 0.0f;
  float mv = 0.0f, vv = 0.0f;
  if (PRE == L2O_PRE_FC_ELU && !a.zero_state) { mv = live ? a.m[idx] : 0.0f; vv = live ? a.v[idx] : 0.0f; }
  float p1h = a.p1_hi, p1l = a.p1_lo, p2h = a.p2_hi, p2l = a.p2_lo;
  constexpr bool kSq = KIND == L2O_PROB_QUADRATIC || KIND == L2O_PROB_SQUARE_COS;
  const float coef = kSq ? 1.0f : 0.5f;
  const float cg = (KIND == L2O_PROB_QUADRATIC ? 2.0f : 1.0f) * pp.inv_bg;   // x2 folded in (exact)
  const float kTwoPi = pp.twopi;
  const float* xsq = xs + 4 * gq;
  const float* rsq = rs + 4 * gq;
  unsigned long long* mine = pa.xbuf + ((size_t)bl * 2 + half) * 2 * SQ;
  const unsigned long long* theirs = pa.xbuf + ((size_t)bl * 2 + (half ^ 1)) * 2 * SQ;
  bool dead = false;                                             // partner timed out
  if (pa.ws->fault != 0) {                                       // (test hook: the injected timeout, see PairWs)
    dead = true;
    if (tid == 0) atomicExch(&pa.ws->status, 1u);
  }
  L2O_LAUNCH_MARK_LANDED(2);
  // ---- handshake: do the two halves of this problem run on the same XCD?  HIP promises nothing about
  // placement (observed: block b on XCD b % 8, hence the b / b + 8 pairing above), so the halves tell each
  // other their XCC_ID once, through the coherent (agent-scope) path, in a granule slot that the step loop
  // does not touch before step 1.  Only a confirmed same-XCD pair uses the L2-resident plain stores.
  __shared__ __attribute__((aligned(16))) int same_xcd_s4[4];
  int& same_xcd_s = same_xcd_s4[0];
  if (tid == 0) {
    unsigned my_xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(my_xcc));
    my_xcc &= 0xfu;
    const unsigned kHsTag = 0x80000000u | salt | 0xffffu;
    __hip_atomic_store(mine + SQ, ((unsigned long long)kHsTag << 32) | my_xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned long long g = 0;
    int spins = 0;
    bool ok = true;
#pragma nounroll
    for (;;) {
      g = __hip_atomic_load(theirs + SQ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((unsigned)(g >> 32) == kHsTag) break;
      if (dead || ++spins > (1 << 20)) { ok = false; break; }       // (the step loop reports a missing partner)
      __builtin_amdgcn_s_sleep(1);
    }
    same_xcd_s = ok && pa.plain_stores && ((unsigned)g & 0xfu) == my_xcc;
  }
  __syncthreads();
  const bool same_xcd = same_xcd_s != 0;
  L2O_LAUNCH_MARK(3);

  constexpr bool kBiasRegs = kPairBiasRegs<PRE, KIND, CH, HIST, EXACT, false>;
  constexpr int kL2bLate = kPairL2bLate<PRE, KIND, CH, HIST, EXACT, false>;
  constexpr bool kL2aUnderSplit = kPairL2aUnderSplit<PRE, KIND, CH, HIST, EXACT, false>;
#define L2O_PAIR_FX_PTR 0
#include "l2o_unroll_pair_loop.h"
#undef L2O_PAIR_FX_PTR
}

// FAST: the prologue for full tiles (the launcher guarantees M = D = SQ; the kernel itself checks the matrix's alignment and
// falls back to the gather in place): unpredicated matrix loads, every other load issued behind them, ONE drain, the
// handshake granule published in front of it and the partner's polled behind it.
template <int PRE, int KIND, int CH, bool HIST, bool EXACT>
__device__ __forceinline__ void unroll_pair_body(const UnrollPairArgs& pa) {
  const long long kernel_t0 = __builtin_readcyclecounter();
#ifdef L2O_PROFILE_PHASES
  unsigned launch_marks[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  constexpr int SQ = 16 * CH;            // padded rows (and columns) of the problem
  constexpr int NWH = CH / 2;            // waves (tiles) per half; tiles beyond the real count idle
  constexpr int NC = 16 * NWH;           // columns (coordinates) owned by a half = SQ / 2
  __shared__ __attribute__((aligned(16))) float xs[NC];   // this half's scaled iterate
  __shared__ __attribute__((aligned(16))) float rs[SQ];   // the full residual
  const UnrollArgs& a = pa.u;
  const ProbParams& pp = a.pp;
  const int D = pp.D, M = pp.M;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  // partner workgroups are blockIdx b and b + 8 inside a group of 16 (same XCD under the
  // observed round-robin placement -- a speed choice only)
  const int bid = blockIdx.x;
  const int half = (bid >> 3) & 1;
  const int bl = ((bid >> 4) << 3) | (bid & 7);         // problem index inside this launch's chunk
  if (bl >= pa.nb) return;                              // padding blocks of the last group of 16 (both halves)
  const int b = pa.b0 + bl;                             // problem index inside the batch shard
  const int tile_in_prob = half * NWH + wv;             // this wave's coordinate tile
  // GEMV role of a lane = its LSTM role: row / column gr = c, 16-byte chunk gq = q.  The four chunk partial sums
  // of a row / column then sit on the lanes (c, 0..3) and two permlane swaps add them INTO the lanes that feed
  // the gradient to the network -- no ds_bpermute (an LDS round trip) between the g pass and the gate math.
  const int gq = q, gr = c;

  // ---- prologue, part zero: the bf16 gate fragments, ONCE per workgroup (round 13).  Every wave needs all of the 60 KB
  // image in its AGPRs; loaded per wave (core.load) a CU pulled it NWH times through its L1, 60 dwordx4 loads per wave in
  // the prologue's burst.  Here each wave copies its 1 / NWH of the image into LDS (LDS-DMA: no destination registers, 1 KiB
  // per instruction, lane-linear = the layout the lanes read back), FIRST, so that the copies fly under everything else
  // the prologue issues; behind the one drain and a barrier every wave reads its 60 x 16 bytes per lane from LDS, under the
  // poll of the partner's handshake granule.  One wave per workgroup (CH = 2) has nobody to share with and keeps its loads.
  using Core = LstmCorePair<PRE, !EXACT, true>;
  constexpr bool kStage = Core::kStageFrags > 0 && NWH >= 2;
  __shared__ float4 frag_stage[kStage ? Core::kStageFrags * 64 : 1];
  static_assert(sizeof(frag_stage) + sizeof(float) * (NC + SQ + Core::kBiasFloats + 4) <= 64 * 1024, "static LDS");
  if constexpr (kStage) {
    const int wvs = __builtin_amdgcn_readfirstlane(wv);   // (the LDS destination is wave-uniform base + lane x 16)
    const float* src = a.np.wpack + Core::kStageOff + lane * 4;
#pragma unroll
    for (int f = 0; f < (Core::kStageFrags + NWH - 1) / NWH; ++f) {
      const int fr = NWH * f + wvs;
      if (Core::kStageFrags % NWH == 0 || fr < Core::kStageFrags)
        __builtin_amdgcn_global_load_lds((gbl_void*)(src + fr * bx::kFragWords), (lds_void*)(frag_stage + fr * 64), 16, 0, 0);
    }
  }

  // ---- the matrix lives in registers: no LDS bandwidth in the two GEMV passes -------------
  //  wr[p][m] : row (2 wv + p) 16 + gr, own columns 16 m + 4 gq + {0..3}     (partial r = W xs)
  //  wt[m]    : own column wv 16 + gr,   rows       16 m + 4 gq + {0..3}     (g = W^T r)
  const float* Wb = pp.W + (pp.w_shared ? (size_t)0 : (size_t)b * M * D);
  const int col0 = half * NC;
  float4 wr[2][NWH], wt[CH];
  // ---- prologue, part one: the matrix.
  // Full tiles (M = D = SQ, the matrix 16-byte aligned: one uniform branch): every element is inside the matrix, so
  // the row-major copy is 2 x NWH 16-byte loads and the column-major one 4 x CH dword loads at compile-time strides --
  // no predicate, no exec-masked region, a tenth of the instructions of the gather below.  The same bits either way
  // (L2O_OPT_PAIR_FAST_LOAD = 0 keeps full tiles on the gather: tests/test_pair_launch_paths.py compares the two).
  if (pa.fast_load && M == SQ && D == SQ && (reinterpret_cast<size_t>(pp.W) & 15) == 0) {
    const float4* Wq = reinterpret_cast<const float4*>(Wb + (size_t)(2 * wv * kTile + gr) * SQ + col0 + 4 * gq);
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int m = 0; m < NWH; ++m) wr[p][m] = Wq[(p * kTile * SQ + 16 * m) / 4];
    const float* Wc = Wb + (size_t)(4 * gq) * SQ + col0 + wv * kTile + gr;
#pragma unroll
    for (int m = 0; m < CH; ++m)
      wt[m] = make_float4(Wc[(16 * m + 0) * SQ], Wc[(16 * m + 1) * SQ], Wc[(16 * m + 2) * SQ], Wc[(16 * m + 3) * SQ]);
  } else {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int row = (2 * wv + p) * kTile + gr;
#pragma unroll
      for (int m = 0; m < NWH; ++m) {
        float e[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int col = col0 + 16 * m + 4 * gq + k;
          e[k] = (row < M && col < D) ? Wb[(size_t)row * D + col] : 0.0f;
        }
        wr[p][m] = make_float4(e[0], e[1], e[2], e[3]);
      }
    }
    const int col = col0 + wv * kTile + gr;
#pragma unroll
    for (int m = 0; m < CH; ++m) {
      float e[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = 16 * m + 4 * gq + k;
        e[k] = (row < M && col < D) ? Wb[(size_t)row * D + col] : 0.0f;
      }
      wt[m] = make_float4(e[0], e[1], e[2], e[3]);
    }
  }
  // ---- the rest of the prologue's global loads, issued back to back behind the matrix; the wave drains them ONCE
  // (profiles/r08_launch_fixed_cost.txt).  The two header words first: loads return in order, so the wait for the tag
  // salt -- the handshake below publishes with it -- leaves everything behind them in flight.
  // (read through an address the compiler cannot see to be uniform: the two words stay in vector registers, in flight,
  //  until the readfirstlane at the handshake -- as uniform loads they are moved to scalar registers, and waited for, at once)
  unsigned hdr_lane = 0;
  asm volatile("" : "+v"(hdr_lane));
  const unsigned* hdr = &pa.ws->seq + hdr_lane;
  const unsigned seq_v = hdr[0], fault_v = hdr[1];
  static_assert(offsetof(PairWs, fault) == offsetof(PairWs, seq) + sizeof(unsigned), "seq and fault are neighbours");
  // the per-lane scalars: lanes outside the problem read a clamped (valid) address and drop the value with a select --
  // no exec-masked region, no wait of their own
  // the residual rows this lane finishes: gq == 0 -> p = 0, gq == 1 -> p = 1 (gq 2, 3 idle)
  const int myrow = (2 * wv + (gq & 1)) * kTile + gr;
  const float y_ld = pp.y[(size_t)b * M + (myrow < M ? myrow : 0)];
  const bool row_counted = gq < 2 && (half == 0 ? (myrow < NC) : (myrow >= NC));   // every row once per pair
  const int j = tile_in_prob * kTile + c;
  const bool live = j < D;
  const size_t idx = (size_t)b * D + j;
  const size_t idx_ld = (size_t)b * D + (live ? j : 0);
  const int tpp = (D + kTile - 1) / kTile;
  const bool tile_real = tile_in_prob < tpp;            // the padded tile of an odd tile count is idle
  // (the state tile is read whatever it holds -- the kernel stores it at the end, so the memory is there -- and dropped
  //  below when the launch starts from the zero state: no branch around five loads.  Round 13 measured the uniform branch:
  //  the loads it saves are not what the burst waits for, and the loop behind it scheduled 2 % slower --
  //  profiles/r13_launch_fixed_cost.txt)
  float* st_tile = a.st + ((size_t)b * tpp + (tile_real ? tile_in_prob : 0)) * kStateFloatsPerTile;
  float4 st_ld[5];
  fetch_tile_state(st_ld, st_tile, lane);
  const float x_ld = (a.x_in ? a.x_in : a.x)[idx_ld];
  float sc_ld = 1.0f;
  if (pp.x_scale) sc_ld = pp.x_scale[idx_ld];
  constexpr bool kCos = KIND == L2O_PROB_RASTRIGIN || KIND == L2O_PROB_SQUARE_COS;
  float cj_ld = 0.0f;
  if (kCos) cj_ld = pp.C[idx_ld];
  float m_ld = 0.0f, v_ld = 0.0f;
  if (PRE == L2O_PRE_FC_ELU && !a.zero_state) { m_ld = a.m[idx_ld]; v_ld = a.v[idx_ld]; }

  // ---- per-lane persistent registers -------------------------------------
  // <= 4 waves per workgroup: bf16x3 gate GEMM, weights in VGPR + AGPR
  Core core;
  float bias_ld[kStage ? (Core::kBiasFloats + 64 * NWH - 1) / (64 * NWH) : 1];
  if constexpr (kStage) {
    core.load_small(a.np.wpack, lane);
    // (the bias table rides in this burst too: hipcc drains the vector memory queue at the first use of a loaded value
    //  while a copy into LDS is in flight -- the salt below -- so a load issued behind that point is a round trip of its own)
    core.template fetch_bias<64 * NWH>(bias_ld, a.np.wpack, tid);
    // (and the one kernel argument that is first used behind the stage reads is fetched here: a scalar load shares its
    //  counter with the LDS reads and returns out of order, so its use waits for every ds_read issued in front of it)
    asm volatile("" ::"s"(a.zero_state));
  } else
    core.load(a.np.wpack, lane);
  __builtin_amdgcn_sched_barrier(0);                    // (everything above is issue only; the uses start below)
  L2O_LAUNCH_MARK(1);

  // ---- handshake, first half: do the two halves of this problem run on the same XCD?  HIP promises nothing about
  // placement (observed: block b on XCD b % 8, hence the b / b + 8 pairing above), so the halves tell each
  // other their XCC_ID once, through the coherent (agent-scope) path, in a granule slot that the step loop
  // does not touch before step 1.  Only a confirmed same-XCD pair uses the L2-resident plain stores.
  // The granule is PUBLISHED here, the moment the salt is known, and POLLED in front of the loop, behind the drain:
  // the partner's round trip runs under this wave's own loads.
  if constexpr (kStage) {
    // the completion point of this wave's fragment copies (they count in its vmcnt) -- and the prologue's one drain: with a
    // copy into LDS in flight hipcc waits for vmcnt(0), not for a count, at the first use of a loaded value, which is the
    // salt right below.  Said here in so many words; the granule's store is issued BEHIND it and nothing waits for that.
    L2O_LAUNCH_MARK_LANDED(2);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  const unsigned seq_w = __builtin_amdgcn_readfirstlane(seq_v), fault_w = __builtin_amdgcn_readfirstlane(fault_v);
  const unsigned salt = pa.use_salt ? ((seq_w + 1u) & 0x7fffu) << 16 : 0u;
  unsigned long long* mine = pa.xbuf + ((size_t)bl * 2 + half) * 2 * SQ;
  const unsigned long long* theirs = pa.xbuf + ((size_t)bl * 2 + (half ^ 1)) * 2 * SQ;
  const unsigned kHsTag = 0x80000000u | salt | 0xffffu;
  unsigned my_xcc = 0;
  if (tid == 0) {
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(my_xcc));
    my_xcc &= 0xfu;
    __hip_atomic_store(mine + SQ, ((unsigned long long)kHsTag << 32) | my_xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  L2O_LAUNCH_MARK(0);
  __builtin_amdgcn_sched_barrier(0);
  __shared__ __attribute__((aligned(16))) float bias_s[Core::kBiasFloats];   // the gate biases = accumulator inits
  // (64 * NWH = the workgroup size the launcher uses: a compile-time stride, one masked load per thread instead of a loop)
  if constexpr (kStage) core.template put_bias<64 * NWH>(bias_s, bias_ld, tid, q);
  else core.stage_bias(bias_s, a.np.wpack, tid, 64 * NWH, q);     // (the handshake's __syncthreads() below orders it)
  if constexpr (kStage) {
    // every wave has drained its copies in front of the salt; behind this barrier it knows that the others have too, and
    // only then is the stage read -- nothing else orders a ds_read behind a copy in flight.  A bare s_barrier (the asm
    // statements fence the compiler): __syncthreads() would wait for the granule's store on top.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    core.read_stage(frag_stage, lane);
    __builtin_amdgcn_sched_barrier(0);                  // (the reads are issued HERE; they land under the poll below)
  } else
    core.pin();   // fragments -> AGPRs (MFMA reads them there): the VGPRs hold W, the state and the gate math
  constexpr bool kPk = L2O_GEMV_PK != 0;                    // packed GEMV FMAs: one wave per SIMD (see dot4pk)
  l2o::f32x4 wrq[2][NWH], wtq[CH];                          // (the same values as register quads for the packed FMAs)
#pragma unroll
  for (int m = 0; m < NWH; ++m) { wrq[0][m] = as_quad(wr[0][m]); wrq[1][m] = as_quad(wr[1][m]); }
#pragma unroll
  for (int m = 0; m < CH; ++m) wtq[m] = as_quad(wt[m]);
  TileState s;
  unpack_tile_state(s, st_ld);
  if (!(tile_real && !a.zero_state)) {
#pragma unroll
    for (int t = 0; t < kNT; ++t) s.h1[t] = s.c1[t] = s.h2[t] = s.c2[t] = 0.0f;
  }
  const float myy = (gq < 2 && myrow < M) ? y_ld : 0.0f;
  float xv = live ? x_ld : 0.0f;
  const float sc = live ? sc_ld : 1.0f;
  const float cj = live ? cj_ld : 0.0f;
  float mv = live ? m_ld : 0.0f, vv = live ? v_ld : 0.0f;
  float p1h = a.p1_hi, p1l = a.p1_lo, p2h = a.p2_hi, p2l = a.p2_lo;
  constexpr bool kSq = KIND == L2O_PROB_QUADRATIC || KIND == L2O_PROB_SQUARE_COS;
  const float coef = kSq ? 1.0f : 0.5f;
  const float cg = (KIND == L2O_PROB_QUADRATIC ? 2.0f : 1.0f) * pp.inv_bg;   // x2 folded in (exact)
  const float kTwoPi = pp.twopi;
  const float* xsq = xs + 4 * gq;
  const float* rsq = rs + 4 * gq;
  bool dead = false;                                             // partner timed out
  if (fault_w != 0) {                                            // (test hook: the injected timeout, see PairWs)
    dead = true;
    if (tid == 0) atomicExch(&pa.ws->status, 1u);
  }
  if constexpr (!kStage) L2O_LAUNCH_MARK_LANDED(2);
  // ---- handshake, second half: the partner's granule (published at ITS salt, a prologue ago)
  __shared__ __attribute__((aligned(16))) int same_xcd_s4[4];
  int& same_xcd_s = same_xcd_s4[0];
  if (tid == 0) {
    unsigned long long g = 0;
    int spins = 0;
    bool ok = true;
#pragma nounroll
    for (;;) {
      g = __hip_atomic_load(theirs + SQ, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((unsigned)(g >> 32) == kHsTag) break;
      if (dead || ++spins > (1 << 20)) { ok = false; break; }       // (the step loop reports a missing partner)
      __builtin_amdgcn_s_sleep(1);
    }
    same_xcd_s = ok && pa.plain_stores && ((unsigned)g & 0xfu) == my_xcc;
  }
  __syncthreads();
  const bool same_xcd = same_xcd_s != 0;
  if constexpr (kStage) core.pin();                     // (the staged fragments, landed by now)
  L2O_LAUNCH_MARK(3);

  constexpr bool kBiasRegs = kPairBiasRegs<PRE, KIND, CH, HIST, EXACT, true>;
  constexpr int kL2bLate = kPairL2bLate<PRE, KIND, CH, HIST, EXACT, true>;
  constexpr bool kL2aUnderSplit = kPairL2aUnderSplit<PRE, KIND, CH, HIST, EXACT, true>;
#define L2O_PAIR_FX_PTR 1
#include "l2o_unroll_pair_loop.h"
#undef L2O_PAIR_FX_PTR
}

template <int PRE, int KIND, int CH, bool HIST, bool EXACT = false, bool FAST = false>
__global__ __launch_bounds__(256) void k_unroll_pair(UnrollPairArgs pa) {
  if constexpr (FAST) unroll_pair_body<PRE, KIND, CH, HIST, EXACT>(pa);
  else unroll_pair_body_gather<PRE, KIND, CH, HIST, EXACT>(pa);
}
