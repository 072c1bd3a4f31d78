// l2o_util_kernels.h -- the small kernels that are no templates (emitted by the one translation unit that includes this:
// l2o_core.hip): state repack, loss reductions, the co-residency probe, the weight packer, Adam.  l2o_unroll.hip launches
// k_combine_halves and k_coresident_probe, l2o_confocal.hip k_reduce_fx, each through a declaration of its own.
#pragma once
#include "l2o_bwd_mfma.h"
#include "l2o_unroll_pair.h"

// ---------------------------------------------------------------------------
// small utility kernels
// ---------------------------------------------------------------------------
// reference layout [B*D, 20] x 4  <->  packed tile layout
__global__ void k_state_repack(float* __restrict__ h1, float* __restrict__ c1, float* __restrict__ h2,
                               float* __restrict__ c2, float* __restrict__ st, int B, int D, int tpp,
                               int to_packed) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)B * tpp * 64 * 20;
  if (gid >= total) return;
  const int e = gid % 20;                 // element of the lane: 4*jv + wv
  const int lane = (gid / 20) % 64;
  const size_t tile = gid / (20 * 64);
  const int b = tile / tpp, tw = tile % tpp;
  const int c = lane & 15, q = lane >> 4;
  const int j = tw * kTile + c;
  const int arr = e / 5, t = e % 5, u = 4 * t + q;
  const size_t paddr = tile * kStateFloatsPerTile + ((size_t)(e >> 2) * 64 + lane) * 4 + (e & 3);
  float* ref = arr == 0 ? h1 : (arr == 1 ? c1 : (arr == 2 ? h2 : c2));
  if (j < D) {
    const size_t raddr = ((size_t)b * D + j) * kH + u;
    if (to_packed) st[paddr] = ref[raddr];
    else ref[raddr] = st[paddr];
  } else if (to_packed) {
    st[paddr] = 0.0f;
  }
}

// fx[t] = (sum_b fx_part[t][b]) / B_global, fixed order: each wave sums a strided slice
// sequentially, then a fixed butterfly.
__global__ void k_reduce_fx(const float* __restrict__ fx_part, int T1, int B_local, float inv_bg,
                            float* __restrict__ fx) {
  const int t = blockIdx.x;
  const int lane = threadIdx.x;   // 64 threads
  float acc = 0.0f;
  for (int b = lane; b < B_local; b += 64) acc += fx_part[(size_t)t * B_local + b];
  acc = wave_sum64(acc);
  if (lane == 0) fx[t] = acc * inv_bg;
}

// The epilogue of a two-CU unroll, one workgroup (64 threads) per step t; runs after every workgroup of the unroll
// has finished:
//   fx_part[t][b] = sum of the 2 x NWH per-wave partials of (step t, problem b), fixed order
//   fx[t]         = (sum_b fx_part[t][b]) / B_global, the summation order of k_reduce_fx (optional)
//   the exchange granules are zeroed for the NEXT launch (tag 0 is never valid; no memset launch per unroll)
//   the launch sequence word the next launch salts its tags with advances
__global__ __launch_bounds__(256) void k_combine_halves(const float* __restrict__ fx_half, float* __restrict__ fx_part,
                                                        int nb, int nparts, float inv_bg, float* __restrict__ fx,
                                                        unsigned long long* __restrict__ xbuf, long xwords, PairWs* ws,
                                                        int b0, int B_local) {
  // nb problems of this launch = problems [b0, b0 + nb) of the shard (fx_part rows have B_local entries).  256 threads:
  // waves 1..3 zero the granules, wave 0 forms the sums.  The kernel sits between two unrolls of a bench step, so what
  // counts is its chain of dependent memory round trips (round 13): the sequence word is fetched at entry, not in front
  // of its store; a lane has the partials of BOTH its problems (nb <= 128: lane and lane + 64) in flight before its first
  // add -- clamped addresses and selects, no loop whose loads wait for its counter; the granules go out 16 bytes per
  // store, from waves that have no load pending (stores and loads share the wave's memory counter: in one wave the second
  // round of stores waited for the loads).  The adds and their order are what they were: per problem ((p0 + p1) + p2) +
  // ..., per lane 0 + f(lane) + f(lane + 64), then wave_sum64.
  const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (tid >= 64) {
    // block t zeroes pairs [t per2, (t + 1) per2) of the xwords / 2 whole pairs of granules (the area is 16-byte aligned:
    // it follows the 192-byte header); the last granule of an odd count is wave 0's, below
    const long npairs = xwords >> 1;
    const long per2 = (npairs + gridDim.x - 1) / gridDim.x;
    const long lo = (long)t * per2, hi = lo + per2 < npairs ? lo + per2 : npairs;
    ulonglong2* xpair = reinterpret_cast<ulonglong2*>(xbuf);
    for (long e = lo + (tid - 64); e < hi; e += 192) xpair[e] = make_ulonglong2(0ull, 0ull);
    return;
  }
  const bool bump = t == 0 && tid == 0;
  unsigned seq0 = 0;
  if (bump) seq0 = ws->seq;
  float acc = 0.0f;
  if (nb <= 128 && (nparts == 2 || nparts == 4 || nparts == 8)) {
    const int bA = lane, bB = lane + 64;
    const bool hA = bA < nb, hB = bB < nb;
    const float* pA = fx_half + ((size_t)t * nb + (hA ? bA : 0)) * nparts;
    const float* pB = fx_half + ((size_t)t * nb + (hB ? bB : 0)) * nparts;
    float fA, fB;
    if (nparts == 8) {
      const float4 a0 = *reinterpret_cast<const float4*>(pA), a1 = *reinterpret_cast<const float4*>(pA + 4);
      const float4 c0 = *reinterpret_cast<const float4*>(pB), c1 = *reinterpret_cast<const float4*>(pB + 4);
      fA = ((a0.x + a0.y) + a0.z) + a0.w;
      fA = (((fA + a1.x) + a1.y) + a1.z) + a1.w;
      fB = ((c0.x + c0.y) + c0.z) + c0.w;
      fB = (((fB + c1.x) + c1.y) + c1.z) + c1.w;
    } else if (nparts == 4) {
      const float4 a0 = *reinterpret_cast<const float4*>(pA), c0 = *reinterpret_cast<const float4*>(pB);
      fA = ((a0.x + a0.y) + a0.z) + a0.w;
      fB = ((c0.x + c0.y) + c0.z) + c0.w;
    } else {
      const float2 a0 = *reinterpret_cast<const float2*>(pA), c0 = *reinterpret_cast<const float2*>(pB);
      fA = a0.x + a0.y;
      fB = c0.x + c0.y;
    }
    if (hA) { fx_part[(size_t)t * B_local + b0 + bA] = fA; acc += fA; }
    if (hB) { fx_part[(size_t)t * B_local + b0 + bB] = fB; acc += fB; }
  } else {
    for (int b = lane; b < nb; b += 64) {                  // (any other shape: the loop of rounds 7-12)
      const float* p = fx_half + ((size_t)t * nb + b) * nparts;
      float f = p[0];
      for (int k = 1; k < nparts; ++k) f += p[k];
      fx_part[(size_t)t * B_local + b0 + b] = f;
      acc += f;
    }
  }
  if (fx) {                                               // (single-launch batches only: nb == B_local)
    acc = l2o::wave_sum64(acc);
    if (lane == 0) fx[t] = acc * inv_bg;
  }
  if (bump) {
    if (xwords & 1) xbuf[xwords - 1] = 0ull;
    ws->seq = seq0 + 1u;
  }
}

// The probe: one workgroup per CU (100 KB of LDS each), every workgroup counts itself, waits a FIXED ~30 us (the
// dispatch of a grid this size takes a few) and records how many had arrived by then; the minimum over the workgroups
// is the number that were resident together (a second wave of workgroups sees the full count, the first wave its own
// size).  Bounded: no workgroup waits for another.
__global__ __launch_bounds__(256) void k_coresident_probe(unsigned* ctr, unsigned* min_seen) {
  extern __shared__ float probe_lds[];
  if (threadIdx.x == 0) {
    probe_lds[0] = 1.0f;
    atomicAdd(ctr, 1u);
    for (int i = 0; i < 8; ++i) __builtin_amdgcn_s_sleep(127);        // 8 x 127 x 64 clocks ~ 28 us
    const unsigned v = __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicMin(min_seen, v);
  }
}

extern "C" {   // (k_wpack and k_adam keep their unmangled names)
// ---- bf16x3 section of wpack (l2o_lstm_bx3.h) --------------------------------
__host__ __device__ static inline uint16_t bf16_rne(float f) {
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__host__ __device__ static inline double bf16_value(uint16_t h) {
  return (double)__builtin_bit_cast(float, (uint32_t)h << 16);
}
__host__ __device__ static inline void bf16_split3(double v, uint16_t (&out)[3]) {
  for (int s = 0; s < 3; ++s) {
    out[s] = bf16_rne((float)v);
    v -= bf16_value(out[s]);
  }
}

// Lane l's share of the packed weights (the buffer is zero beforehand): the host packer runs it for
// l = 0..63, the device packer (l2o_wpack_device, the meta-training step) with one thread per lane.
// The lanes write disjoint words.
// [t_lo, t_hi): unit slices of the forward sections, [tile_lo, tile_hi): M-tiles of the BPTT section (the device
// packer gives every (lane, slice) and (lane, tile) its own thread: the float64 splits are the cost).
// (ch_lo, ch_hi): the gate-GEMM chunks of slices [t_lo, t_hi) this call packs -- everything of a slice that is not a
// chunk fragment rides with chunk 0; (r_lo, r_hi): the gate types of the BPTT M-tiles [tile_lo, tile_hi).  The host
// packer passes the full ranges; k_wpack one (slice, chunk) or one (tile, gate type) per block.
__host__ __device__ static void wpack_lane(int pre, int l, int t_lo, int t_hi, int tile_lo, int tile_hi,
                                           const float* wg1, const float* bg1, const float* wg2,
                                           const float* bg2, const float* wl, const float* bl, const float* wfc,
                                           const float* bfc, float* out, int ch_lo = 0, int ch_hi = 4, int r_lo = 0,
                                           int r_hi = 4) {
  const bool fc = pre == L2O_PRE_FC_ELU;
  const int P = fc ? kH : (pre == L2O_PRE_LOGSIGN ? 2 : 1);
  const int G = 4 * kH;
  auto col = [](int t, int rho) { return (rho & 3) * kH + 4 * t + (rho >> 2); };
  const int rho = l & 15, kq = l >> 4;   // A-fragment view of the lane
  const int q = l >> 4;                  // C/D + B view of the lane
  for (int t = t_lo; t < t_hi && ch_lo == 0; ++t) {
    const int cA = col(t, rho);
    // layer 1
    if (fc) {
      for (int kk = 0; kk < 10; ++kk) {
        const int row = kk < 5 ? 4 * kk + kq : kH + 4 * (kk - 5) + kq;   // fc features, then h1
        out[(wp_row_a1(pre) + kk * kNT + t) * 64 + l] = wg1[row * G + cA];
      }
    } else {
      for (int kk = 0; kk < 5; ++kk)
        out[(wp_row_a1(pre) + kk * kNT + t) * 64 + l] = wg1[(P + 4 * kk + kq) * G + cA];
      float v = 0.0f;
      if (kq == 0) v = wg1[0 * G + cA];
      else if (kq == 1) v = P == 2 ? wg1[1 * G + cA] : 0.0f;
      else if (kq == 2) v = bg1[cA];
      out[(wp_row_a1(pre) + 5 * kNT + t) * 64 + l] = v;
    }
    // layer 2: kk 0..4 <- h1 (rows 0..19), kk 5..9 <- h2 (rows 20..39)
    for (int kk = 0; kk < 10; ++kk) {
      const int row = kk < 5 ? 4 * kk + kq : kH + 4 * (kk - 5) + kq;
      out[(wp_row_a2(pre) + kk * kNT + t) * 64 + l] = wg2[row * G + cA];
    }
    for (int r = 0; r < 4; ++r) {
      const int cD = col(t, 4 * q + r);
      out[(wp_row_b1(pre) + t * 4 + r) * 64 + l] = fc ? bg1[cD] : 0.0f;
      out[(wp_row_b2(pre) + t * 4 + r) * 64 + l] = bg2[cD];
    }
    out[(wp_row_wl(pre) + t) * 64 + l] = wl[4 * t + q];
    if (fc) {
      out[(wp_row_fc(pre) + t) * 64 + l] = wfc[0 * kH + 4 * t + q];
      out[(wp_row_fc(pre) + kNT + t) * 64 + l] = wfc[1 * kH + 4 * t + q];
      out[(wp_row_fc(pre) + 2 * kNT + t) * 64 + l] = bfc[4 * t + q];
    }
  }
  if (t_lo == 0 && t_hi > 0 && ch_lo == 0) out[wp_row_bl(pre) * 64 + l] = bl[0];
  // ---- bf16x3 fragments: gate rows pre-scaled to exp2 arguments, split from float64 ----
  {
    uint32_t* ow = reinterpret_cast<uint32_t*>(out);
    constexpr double kL2E = 1.4426950408889634074;
    auto gscale = [&](int r) { return r == 1 ? 2.0 * kL2E : -kL2E; };      // rows i, j, f, o
    for (int t = t_lo; t < t_hi; ++t) {
      const int cA = col(t, rho), r = rho & 3;
      for (int ch = ch_lo; ch < ch_hi && ch < bx::nchunks(pre); ++ch) {
        uint16_t sl[5][3], bs[3] = {0, 0, 0};
        for (int i = 0; i < 5; ++i) {
          const int u = 4 * i + kq;
          double v;
          if (ch == bx::kChL1H) v = wg1[(P + u) * G + cA];
          else if (ch == bx::kChL2A) v = wg2[u * G + cA];
          else if (ch == bx::kChL2B) v = wg2[(kH + u) * G + cA];
          else v = wg1[u * G + cA];                              // kChL1X: the fc features
          bf16_split3(v * gscale(r), sl[i]);
        }
        // (the bias slots of the fragments stay ZERO since round 3: the bias is the accumulator init, bx::bias_off)
        // 6-product form: K-slots 0..4 = the units, slot 7 = the bias (q == 0), one fragment per split level
        for (int sp = 0; sp < 3; ++sp)
          for (int rg = 0; rg < 4; ++rg) {
            auto slot = [&](int i) -> uint32_t { return i < 5 ? sl[i][sp] : (i == 7 && kq == 0 ? bs[sp] : 0); };
            ow[bx::frag_off(pre, false, ch, t, sp) + l * 4 + rg] = slot(2 * rg) | (slot(2 * rg + 1) << 16);
          }
        // packed K-slots (l2o_lstm_bx3.h, slot_desc): the weight level that multiplies the slot's activation level
        {
          for (int j = 0; j < bx::kPack; ++j)
            for (int rg = 0; rg < 4; ++rg) {
              uint32_t word = 0;
              for (int h = 0; h < 2; ++h) {
                const bx::SlotDesc d = bx::slot_desc(j, rg, h);
                uint16_t v16 = 0;
                if (d.unit < 5) v16 = sl[d.unit][d.w];
                else if (bx::bias_level(kq, h) >= 0) v16 = bs[bx::bias_level(kq, h)];
                word |= (uint32_t)v16 << (16 * h);
              }
              ow[bx::frag_off(pre, true, ch, t, j) + l * 4 + rg] = word;
            }
        }
      }
      if (ch_lo != 0) continue;                                 // (the rest of the slice rides with chunk 0)
      if ((l & 15) == 0)                                        // one lane per lane group writes its 4 gate rows
        for (int rr = 0; rr < 4; ++rr) {
          const int cD = col(t, 4 * q + rr);
          const double fb = rr == 2 ? 1.0 : 0.0;                  // forget_bias
          out[bx::bias_off(pre) + ((0 * kNT + t) * 4 + q) * 4 + rr] = (float)(((double)bg1[cD] + fb) * gscale(rr));
          out[bx::bias_off(pre) + ((1 * kNT + t) * 4 + q) * 4 + rr] = (float)(((double)bg2[cD] + fb) * gscale(rr));
        }
      if (!fc)
        for (int rr = 0; rr < 4; ++rr) {
          const int cD = col(t, 4 * q + rr);
          out[bx::win_off(pre) + t * 256 + l * 4 + rr] = (float)((double)wg1[0 * G + cD] * gscale(rr));
          out[bx::win_off(pre) + (kNT + t) * 256 + l * 4 + rr] =
              P == 2 ? (float)((double)wg1[1 * G + cD] * gscale(rr)) : 0.0f;
        }
    }
  }
  // ---- bf16x3 fragments of the transposed products of the BPTT step (l2o_bwd_mfma.h): W itself,
  //      unscaled; M-tile rows = input rows of W, K-chunk r = gate type r (Sonnet column block) ----
  {
    uint32_t* ow = reinterpret_cast<uint32_t*>(out) + bxb::base(pre);
    for (int tile = tile_lo; tile < tile_hi; ++tile) {
      const bool l2 = tile < bxb::tiles2();
      const int m = l2 ? tile : tile - bxb::tiles2();
      const float* W = l2 ? wg2 : wg1;
      const int first = l2 ? 0 : (fc ? 0 : -1), second = l2 ? kH : (fc ? kH : P);
      const int row = bxb::src_row(m, rho, first, second);
      if (row < 0) continue;
      for (int r = r_lo; r < r_hi; ++r) {
        uint16_t sl[8][3];
        for (int i = 0; i < 8; ++i)
          for (int sp = 0; sp < 3; ++sp) sl[i][sp] = 0;
        for (int i = 0; i < 5; ++i) bf16_split3((double)W[row * G + r * kH + 4 * i + kq], sl[i]);
        for (int sp = 0; sp < 3; ++sp)
          for (int j = 0; j < 4; ++j)
            ow[bxb::frag_rel(tile, r, sp) + l * 4 + j] = (uint32_t)sl[2 * j][sp] | ((uint32_t)sl[2 * j + 1][sp] << 16);
      }
    }
  }
}

__global__ void k_wpack(int pre, const float* wg1, const float* bg1, const float* wg2, const float* bg2, const float* wl,
                        const float* bl, const float* wfc, const float* bfc, float* out) {
  // one block per (slice, chunk), then one per (BPTT M-tile, gate type): 35 / 44 blocks of one wave (10 / 11 blocks
  // before: 12.5 us on the critical path between the meta-step and the next unroll)
  const int b = blockIdx.x, nch = bx::nchunks(pre);
  if (b < kNT * nch) {
    const int t = b / nch, ch = b - t * nch;
    wpack_lane(pre, threadIdx.x, t, t + 1, 0, 0, wg1, bg1, wg2, bg2, wl, bl, wfc, bfc, out, ch, ch + 1, 0, 0);
  } else {
    const int e = b - kNT * nch, tile = e >> 2, r = e & 3;
    wpack_lane(pre, threadIdx.x, 0, 0, tile, tile + 1, wg1, bg1, wg2, bg2, wl, bl, wfc, bfc, out, 0, 0, r, r + 1);
  }
}

// tf.train.AdamOptimizer._apply_dense (TF 1.x) on one flat fp32 vector, every operation rounded separately
// like the NumPy expression it replaces (no contraction): bit-equal to the host update
// guard != nullptr: the status word of the unroll whose gradients these are (the head of its workspace); a non-zero
// status (a partner timeout: the recorded history is garbage) leaves w, m, v untouched
// map != nullptr: the gradient of weight i is g[map[i]] (map[i] < 0: zero) -- the weight-gradient blocks are read
// straight out of the contraction's [KA][KB] result (l2o_adam_step_gather)
__global__ void k_adam(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g,
                       long n, float lr_t, float b1, float omb1, float b2, float omb2, float eps,
                       const unsigned* __restrict__ guard, const int* __restrict__ map) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (guard && __builtin_nontemporal_load(guard) != 0u) return;
  float gi;
  if (map) { const int j = map[i]; gi = j >= 0 ? g[j] : 0.0f; }
  else gi = g[i];
  const float mi = __fadd_rn(__fmul_rn(b1, m[i]), __fmul_rn(omb1, gi));
  const float vi = __fadd_rn(__fmul_rn(b2, v[i]), __fmul_rn(__fmul_rn(omb2, gi), gi));
  m[i] = mi; v[i] = vi;
  w[i] = __fsub_rn(w[i], __fdiv_rn(__fmul_rn(lr_t, mi), __fadd_rn(__fsqrt_rn(vi), eps)));
}
}
