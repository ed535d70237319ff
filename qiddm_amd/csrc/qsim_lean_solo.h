// qsim_lean_solo.h -- the "solo" body of the lean sampling loop: ONE wavefront per (sample, step) item of the 8-qubit
// net without re-upload and with a compiled-in layer count (float32; the flagship QNN_noise(784, 8, 14)).
//
// Layout: all 256 amplitudes in one wavefront, four per lane, in one of TWO layouts that alternate from layer to layer
// (solo_amp below).  Index bits 0..3 are lane bits 0..3 in both.  Layout A: amplitude k = (r << 6) | logical_lane(lane),
// r = 0..3 -- the register bits are index bits 6 and 7, the WAVE bits of the four-wave decomposition (qsim_lean.h), so
// entry r * 64 + lane of a LeanTables<T, 8> layer is this lane's entry for register r.  Layout B: the register bits are
// index bits 5 and 4, lane bits 5 and 4 hold index bits 6 and 7.  Eight permlane swaps turn one into the other.
// What that buys:
//   * the RYs of a layer commute: a layer applies the two bits that are register bits where it starts, swaps, and
//     applies the two that are register bits where it ends -- every RY on index bits 4..7 is a packed FMA on register
//     pairs, no LDS exchange, no s_barrier, and nothing is swapped back (the layer before this one swapped (re, im) of
//     every amplitude there and back for bits 4 and 5: 16 swaps and 16 FMAs, 701 -> 571 ticks per layer with two
//     wavefronts on a SIMD, profiles/lean_pipeline/ubench_solo_layer.txt);
//   * every gate acts on 8 independent registers (4 amplitudes x re / im), so the wave issues back to back (~4 cycles
//     per vector instruction) instead of waiting ~11 cycles on its own previous result;
//   * the items of a launch (batch x n_steps: this instance's angles never reach the state, so its steps do not depend
//     on each other) are spread over all wavefronts of all workgroups, kSoloWaves per CU.  Every item is still
//     simulated in full.
// The per-workgroup setup fetches the tables from global memory ONCE and hands them to the eight wavefronts through LDS
// (one __syncthreads()).  linear_up is split by PIXELS, not by items: a lane owns two neighbouring pixels and keeps their
// weights in registers for the whole launch; the eight wavefronts meet once per round of eight items (one s_barrier) to
// exchange the read-outs, 64 bytes per item.  Every wave runs the same code -- one copy of it, and a pixel of every row
// is computed by the same instructions on the same operands, so every row of a launch is the same bits --; what depends
// on the wave number is which items it simulates and which pixels it writes.
#pragma once
#include "qsim_lean.h"

namespace qiddm {

// LDS of the solo body: the read-outs of a round's eight items [2 parities][kSoloWaves][8] as float64, the tangents
// [layers][8], the phase entries in the lanes' order.  (linear_up's weights and bias were here too, 57 KiB that every
// wavefront read in full for every item; they are in the registers of the lanes that own the pixels now, below.)
struct LeanSoloLds {
  static constexpr size_t kEvBytes = (size_t)2 * kSoloWaves * 8 * sizeof(double);
  __host__ __device__ static constexpr size_t un_bytes(int layers) { return (size_t)layers * 8 * sizeof(float); }
  // the phase entries of the simulated layers 1 .. layers - 1 in the order the lanes take them: [layer][2][64] units of
  // 16 bytes, unit (l, h, lane) = the lane's entries for registers 2 h and 2 h + 1 in the layout layer l starts in
  __host__ __device__ static constexpr size_t ph_bytes(int layers) { return (size_t)(layers - 1) * 256 * 2 * sizeof(float); }
  __host__ __device__ static constexpr size_t bytes(int layers) { return kEvBytes + un_bytes(layers) + ph_bytes(layers); }
};

// ---- who writes which pixels ---------------------------------------------------------------------------------------------
// linear_up by ownership: the Q <= 1024 pixels of a row are ceil(Q / 2) pairs (2 p, 2 p + 1); wavefront w of the workgroup
// owns solo_pairs_per_wave(Q) consecutive pairs (<= 64), its lane l < that the pair w * per_wave + l.  A lane keeps the
// two rows of w_up and the two biases of its pair in registers for the whole launch and stores a pair as 16 bytes.
// A wavefront's share is ceil(pairs / 8) rounded up to whole 64-byte lines (four pairs): with the bare quotient -- 49
// pairs, 784 bytes at Q = 784 -- neighbouring wavefronts split a 32-byte sector at four of a row's seven seams, and the
// write-through stores wrote those sectors twice (WRITE_SIZE 24 000 KiB per benchmark launch for 23 520 KiB of
// images).  The instructions of a wavefront do not depend on how many of its lanes hold a pair, so the uneven split --
// 7 x 52 + 28 at Q = 784 -- costs nothing.
constexpr int kSoloMaxPixels = 1024;
__host__ __device__ constexpr int solo_pairs(int q) { return (q + 1) / 2; }
__host__ __device__ constexpr int solo_pairs_per_wave(int q) {
  return ((solo_pairs(q) + kSoloWaves - 1) / kSoloWaves + 3) / 4 * 4;
}
// the pair of lane `lane` of wavefront `wave`, or -1: lanes beyond the wavefront's share and pairs beyond the row
__host__ __device__ constexpr int solo_pair_of(int q, int wave, int lane) {
  const int per = solo_pairs_per_wave(q), pr = wave * per + lane;
  return lane < per && pr < solo_pairs(q) ? pr : -1;
}
// for every Q in [q_lo, q_hi]: walking the (wavefront, lane) slots in order meets the pairs 0, 1, .. ceil(Q / 2) - 1 once
// each and nothing else -- every pixel has exactly one owner --, and no owned pixel is >= Q but the second half of an odd
// Q's last pair
__host__ __device__ constexpr bool solo_owners_cover(int q_lo, int q_hi) {
  for (int q = q_lo; q <= q_hi; ++q) {
    int next = 0;
    for (int w = 0; w < kSoloWaves; ++w)
      for (int l = 0; l < kWave; ++l) {
        const int pr = solo_pair_of(q, w, l);
        if (pr < 0) continue;
        if (pr != next || 2 * pr >= q) return false;
        if (2 * pr + 1 >= q && !(q % 2 == 1 && pr == solo_pairs(q) - 1)) return false;
        ++next;
      }
    if (next != solo_pairs(q)) return false;
  }
  return true;
}
// (in slices of 64 image sizes: one constant expression has a step limit)
#define QIDDM_SOLO_OWNERS(lo) static_assert(solo_owners_cover(lo, lo + 63), "pixel ownership, Q = " #lo " .. " #lo " + 63")
QIDDM_SOLO_OWNERS(1);
QIDDM_SOLO_OWNERS(65);
QIDDM_SOLO_OWNERS(129);
QIDDM_SOLO_OWNERS(193);
QIDDM_SOLO_OWNERS(257);
QIDDM_SOLO_OWNERS(321);
QIDDM_SOLO_OWNERS(385);
QIDDM_SOLO_OWNERS(449);
QIDDM_SOLO_OWNERS(513);
QIDDM_SOLO_OWNERS(577);
QIDDM_SOLO_OWNERS(641);
QIDDM_SOLO_OWNERS(705);
QIDDM_SOLO_OWNERS(769);
QIDDM_SOLO_OWNERS(833);
QIDDM_SOLO_OWNERS(897);
QIDDM_SOLO_OWNERS(961);
#undef QIDDM_SOLO_OWNERS
static_assert(961 + 63 == kSoloMaxPixels, "the slices end at the largest image");
static_assert(solo_pairs_per_wave(kSoloMaxPixels) == kWave && solo_pairs_per_wave(784) == 52, "a wavefront's share fits its lanes");

// 1: a pair in a 16-byte aligned row leaves as one write-through store (`buffer_store_dwordx4 ... sc1`): the image goes
// to memory while the launch runs instead of staying dirty in the L2s until the kernel boundary.  0 (A/B builds only):
// a plain 16-byte store.
#ifndef QIDDM_SOLO_WRITE_THROUGH
#define QIDDM_SOLO_WRITE_THROUGH 1
#endif

// The four DPP lane-bit gates (index bits 0..3) on eight registers: own += t_signed * partner, `v_fmac_f32_dpp` in place
// (qsim_lean.h: ry_t_dpp4).  A DPP read needs two wait states behind the vector instruction that wrote the register:
// inside the block a register is read eight instructions after it was written; `s_nop 1` in front covers whatever the
// compiler placed before the block, `s_nop 1` behind whatever it places after (a permlane swap follows).
#define QIDDM_SOLO_DPP8(ctrl, t)                                             \
  "v_fmac_f32_dpp %0, %0, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %1, %1, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %2, %2, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %3, %3, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %4, %4, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %5, %5, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %6, %6, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t" \
  "v_fmac_f32_dpp %7, %7, " t " " ctrl " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
__device__ __forceinline__ void solo_ry_dpp4(V2<float> (&a)[4], float t0, float t1, float t2, float t3) {
  float v0 = a[0].x, v1 = a[0].y, v2 = a[1].x, v3 = a[1].y, v4 = a[2].x, v5 = a[2].y, v6 = a[3].x, v7 = a[3].y;
  asm volatile(
      "s_nop 1\n\t"
      QIDDM_SOLO_DPP8("quad_perm:[1,0,3,2]", "%8")
      QIDDM_SOLO_DPP8("quad_perm:[2,3,0,1]", "%9")
      QIDDM_SOLO_DPP8("row_half_mirror", "%10")
      QIDDM_SOLO_DPP8("row_ror:8", "%11")
      "s_nop 1"
      : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(v6), "+v"(v7)
      : "v"(t0), "v"(t1), "v"(t2), "v"(t3));
  a[0] = V2<float>{v0, v1};
  a[1] = V2<float>{v2, v3};
  a[2] = V2<float>{v4, v5};
  a[3] = V2<float>{v6, v7};
}
#undef QIDDM_SOLO_DPP8

// RY (tangent form) on a register bit: the 2 x 2 on (member with the bit clear, member with it set)
__device__ __forceinline__ void solo_ry_reg(V2<float>& lo, V2<float>& hi, float t) {
  const V2<float> nlo = __builtin_elementwise_fma(bcast<float>(-t), hi, lo);
  const V2<float> nhi = __builtin_elementwise_fma(bcast<float>(t), lo, hi);
  lo = nlo;
  hi = nhi;
}

// exchange a register bit with lane bit Q (4 / 5): the permlane swap of (register with the bit clear, register with it
// set), on both components
template <int Q>
__device__ __forceinline__ void solo_swap_bit(V2<float>& lo, V2<float>& hi) {
  float lx = lo.x, ly = lo.y, hx = hi.x, hy = hi.y;
  swap_parts<Q>(lx, hx);
  swap_parts<Q>(ly, hy);
  lo = V2<float>{lx, ly};
  hi = V2<float>{hx, hy};
}

// ---- the two layouts ------------------------------------------------------------------------------------------------------
// Which amplitude register r (bit 0 = r0, bit 1 = r1) of the lane with logical number llane holds.  Index bits 0..3 are
// lane bits 0..3 in both layouts (the DPP gates and their lane signs do not care which one the wave is in);
//   layout A: index bits 4, 5 = lane bits 4, 5; index bits 6, 7 = r0, r1  -- k = (r << 6) | llane, the tables' own order;
//   layout B: index bits 4, 5 = r1, r0;         index bits 6, 7 = lane bits 5, 4.
// A `v_permlane32_swap` of (a[2 r1].c, a[2 r1 + 1].c) exchanges r0 with lane bit 5, a `v_permlane16_swap` of (a[r0].c,
// a[2 + r0].c) exchanges r1 with lane bit 4 (c = re, im): eight swaps turn either layout into the other.
constexpr int kSoloLayoutA = 0, kSoloLayoutB = 1;
__host__ __device__ constexpr int solo_amp(int layout, int r, int llane) {
  const int r0 = r & 1, r1 = (r >> 1) & 1, l4 = (llane >> 4) & 1, l5 = (llane >> 5) & 1, low = llane & 15;
  return layout == kSoloLayoutA ? (low | (l4 << 4) | (l5 << 5) | (r0 << 6) | (r1 << 7))
                                : (low | (r1 << 4) | (r0 << 5) | (l5 << 6) | (l4 << 7));
}
// entry of a LeanTables<float, 8> layer (thread order of the four-wave body: (wave << 6) | physical lane) that register r
// of physical lane `lane` multiplies by in `layout`
__host__ __device__ constexpr int solo_table_slot(int layout, int r, int lane) {
  const int k = solo_amp(layout, r, lane ^ (((lane >> 2) & 1) * 3));   // (logical_lane, an involution)
  return (k & ~63) | ((k & 63) ^ ((((k & 63) >> 2) & 1) * 3));
}
// where the eight swaps put the value of (r, llane): (r', llane') as (r' << 6) | llane'
__host__ __device__ constexpr int solo_swapped(int r, int llane) {
  const int r0 = r & 1, r1 = (r >> 1) & 1, l4 = (llane >> 4) & 1, l5 = (llane >> 5) & 1;
  return ((l5 | (l4 << 1)) << 6) | (llane & 15) | (r1 << 4) | (r0 << 5);
}
__host__ __device__ constexpr bool solo_layout_is_bijection(int layout) {
  bool seen[256] = {};
  for (int r = 0; r < 4; ++r)
    for (int l = 0; l < 64; ++l) {
      const int k = solo_amp(layout, r, l);
      if (k < 0 || k > 255 || seen[k]) return false;
      seen[k] = true;
    }
  return true;
}
__host__ __device__ constexpr bool solo_swaps_map(int from, int to) {
  for (int r = 0; r < 4; ++r)
    for (int l = 0; l < 64; ++l) {
      const int s = solo_swapped(r, l);
      if (solo_amp(from, r, l) != solo_amp(to, s >> 6, s & 63)) return false;
    }
  return true;
}
static_assert(solo_layout_is_bijection(kSoloLayoutA) && solo_layout_is_bijection(kSoloLayoutB),
              "each layout holds every amplitude 0..255 exactly once");
static_assert(solo_swaps_map(kSoloLayoutA, kSoloLayoutB) && solo_swaps_map(kSoloLayoutB, kSoloLayoutA),
              "the eight swaps turn layout A into layout B and back");
static_assert(solo_amp(kSoloLayoutA, 2, 37) == ((2 << 6) | 37) && solo_table_slot(kSoloLayoutA, 3, 21) == 3 * 64 + 21,
              "layout A reads the tables as they are");

// One layer on the four amplitudes of a lane: phase table entry (gathered by the layout the layer starts in), then RY on
// every index bit (tangent form: the cosines sit in the phase entry).  The RYs of a layer commute, so the two bits that
// are register bits NOW go first, the eight swaps change the layout, and the two bits that are register bits THEN
// follow: every RY on bits 4..7 is a packed FMA on register pairs and nothing is swapped back -- a layer that starts in A
// ends in B and the other way round.  ts: tangents of index bits 0..3 signed by this lane's bit; t4..t7: plain tangents.
// layout: the one the layer starts in (a constant once the layer sequence is unrolled).
__device__ __forceinline__ void solo_layer(int layout, V2<float> (&a)[4], const V2<float> (&ph)[4], const float (&ts)[4],
                                           float t4, float t5, float t6, float t7) {
  // (component by component, the products of cmul2: its packed form wants (ph.x, ph.x) and (ph.y, ph.y) as register
  //  pairs, which the compiler keeps across the loop for every layer -- twice the registers of the phase table)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float re = fmaf(-ph[r].y, a[r].y, ph[r].x * a[r].x), im = fmaf(ph[r].y, a[r].x, ph[r].x * a[r].y);
    a[r] = V2<float>{re, im};
  }
  solo_ry_dpp4(a, ts[0], ts[1], ts[2], ts[3]);
  const bool from_a = layout == kSoloLayoutA;
  const float in0 = from_a ? t6 : t5, in1 = from_a ? t7 : t4;     // r0 / r1 of the layout the layer starts in
  const float out0 = from_a ? t5 : t6, out1 = from_a ? t4 : t7;   // ... of the one it ends in
  solo_ry_reg(a[0], a[1], in0);
  solo_ry_reg(a[2], a[3], in0);
  solo_ry_reg(a[0], a[2], in1);
  solo_ry_reg(a[1], a[3], in1);
  solo_swap_bit<5>(a[0], a[1]);
  solo_swap_bit<5>(a[2], a[3]);
  solo_swap_bit<4>(a[0], a[2]);
  solo_swap_bit<4>(a[1], a[3]);
  solo_ry_reg(a[0], a[1], out0);
  solo_ry_reg(a[2], a[3], out0);
  solo_ry_reg(a[0], a[2], out1);
  solo_ry_reg(a[1], a[3], out1);
}

// The body of dense_lean_kernel<float, 8, PPT, false, LPR, false> at kSoloThreads threads per workgroup.
// Items: (sample, step) = item / n_steps, item % n_steps for item < batch * n_steps; wave g of the launch takes items
// g, g + (waves of the launch), ...: every item is simulated exactly once, no wave idles while another has two to do.
// Round r of workgroup b is the eight consecutive items (r * gridDim.x + b) * 8 + w of its wavefronts w: each simulates
// its own and leaves the eight <Z> in LDS, one s_barrier, and every wavefront writes ITS pixels (above) of all eight
// rows.  The read-outs alternate between two slots of LDS by the round's parity, so one barrier per round is enough: a
// wavefront writes round r + 1's only behind the barrier of round r, and reads round r's only behind that barrier too.
template <int LPR>
__device__ void dense_lean_solo_body(const double* __restrict__ wu, const double* __restrict__ bu,
                                                     double* __restrict__ y, const unsigned char* __restrict__ tables,
                                                     const QuadScalars& d, const KScalars& p) {
  using T = float;
  using C = V2<T>;
  using QT = LeanTables<T, 8>;
  using V4 = T __attribute__((ext_vector_type(4)));
  using D2 = double __attribute__((ext_vector_type(2)));
  static_assert(LPR > 1, "a compiled-in layer count with at least one simulated layer");
  // the layout simulated layer l (1 .. LPR - 1) starts in: they alternate, and the last one ends in A, where the
  // read-out expects the state
  auto layout_of = [](int l) { return (LPR - 1 - l) % 2 == 0 ? kSoloLayoutB : kSoloLayoutA; };
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int Q = d.out_features;
  double* s_ev = reinterpret_cast<double*>(smem_raw);                             // [2][kSoloWaves][8]
  T* s_un = reinterpret_cast<T*>(smem_raw + LeanSoloLds::kEvBytes);                // [LPR][8]
  C* s_ph = reinterpret_cast<C*>(smem_raw + LeanSoloLds::kEvBytes + LeanSoloLds::un_bytes(LPR));   // [LPR - 1][2][64][2]
  static_assert((LeanSoloLds::kEvBytes + LeanSoloLds::un_bytes(LPR)) % 16 == 0, "16-byte reads of the phase entries");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int llane = logical_lane(lane);
  const T* g_body = reinterpret_cast<const T*>(tables + kLeanHeaderDoubles * sizeof(double));
  const C* g_ph = reinterpret_cast<const C*>(g_body);
  const T* g_un = g_body + QT::ph_elems(LPR);
  const T* g_a0 = g_un + QT::un_elems(LPR);
  // diagnostics: wavefront 0 of workgroup 0 stamps s_memtime into words 0..7 (tools/stamp_lean_solo.py) -- [0] entry,
  // [1] setup loads issued, [2] barrier passed, [3] / [4] end of the layers and read-out / of the tail of its first round
  // (the tail starts at the round's barrier: it holds the wait for the slowest of the eight wavefronts, linear_up and
  // the stores), [5] / [6] of its second round, [7]: s_memrealtime (100 MHz) from entry to the last tail stamped, which
  // gives the ticks their length.
  // When the buffer holds 8 + 8 * gridDim.x words (d.stamp_words), wavefront 0 of EVERY workgroup b also stamps
  // s_memrealtime -- the same clock on every CU -- into words 8 + 8 b .. (tools/timeline_lean_solo.py): [0] entry,
  // [1] barrier passed, [2] / [3] end of the layers / of the tail of its first round, [4] / [5] of its second, [6] its
  // last instruction.
  // The test is wave-uniform (a scalar branch per stamp); lane 0 stores.
  const bool stamp_timeline = d.stamps != nullptr && (int64_t)d.stamp_words >= 8 + 8 * (int64_t)gridDim.x;
  const bool stamp_wave = d.stamps != nullptr && wv == 0 && (blockIdx.x == 0 || stamp_timeline);
  const unsigned long long stamp_rt0 = stamp_wave ? __builtin_amdgcn_s_memrealtime() : 0ull;
  auto stamp = [&](int word, int tword) {
    if (stamp_wave) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      const unsigned long long rt = __builtin_amdgcn_s_memrealtime();
      if (lane == 0) {
        if (blockIdx.x == 0 && word >= 0) {
          d.stamps[word] = t;
          if (word == 4 || word == 6) d.stamps[7] = rt - stamp_rt0;
        }
        if (stamp_timeline && tword >= 0) d.stamps[8 + 8 * (size_t)blockIdx.x + tword] = rt;
      }
    }
  };
  stamp(0, 0);

  // ---- per-launch setup ----------------------------------------------------------------------------------------------
  // The workgroup fetches everything ONCE -- the phase entries of the 13 simulated layers (26 KiB, gathered into the
  // lanes' own order) and the tangents -- and hands it over through LDS; behind the barrier every wavefront fills its
  // phase registers from the LDS copy with 16-byte reads.  (Each wavefront used to read the whole phase table from
  // global memory itself: eight times the bytes through the CU's vector L1, which took longer than an item's layers.)
  // Every global load of it is issued before anything waits.  linear_up's weights go straight to the registers of the
  // lanes that own the pixels (the two rows of a pair are 128 contiguous bytes of w_up), behind the barrier.
  constexpr int kPhEntries = (LPR - 1) * QT::TL;                                  // phase entries of layers 1 .. LPR - 1
  constexpr int kPhTrips = (kPhEntries + kSoloThreads - 1) / kSoloThreads;
  C phstage[kPhTrips];
#pragma unroll
  for (int k = 0; k < kPhTrips; ++k) {
    // LDS entry e = ((l - 1) * 2 + h) * 128 + lane * 2 + j: register r = 2 h + j of `lane` in layer l
    // (an entry beyond the table loads entry 0 and is not stored: no branch around a load, which would wait inside)
    const int e = tid + k * kSoloThreads, ec = e < kPhEntries ? e : 0;
    const int l = (ec >> 8) + 1, r = ((ec >> 6) & 2) | (ec & 1), ln = (ec >> 1) & 63;
    phstage[k] = g_ph[l * QT::TL + solo_table_slot(layout_of(l), r, ln)];
  }
  const T unreg = g_un[tid < LPR * 8 ? tid : 0];
  T a0r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) a0r[r] = g_a0[solo_table_slot(layout_of(1), r, lane)];
  __builtin_amdgcn_sched_barrier(0);   // (all loads are out)
  stamp(1, -1);
#pragma unroll
  for (int k = 0; k < kPhTrips; ++k) {
    const int e = tid + k * kSoloThreads;
    if (e < kPhEntries) s_ph[e] = phstage[k];
  }
  static_assert(LPR * 8 <= kSoloThreads, "one tangent per thread");
  if (tid < LPR * 8) s_un[tid] = unreg;
  T pm[4];   // +-1 by this lane's index bit
#pragma unroll
  for (int q = 0; q < 4; ++q) pm[q] = ((llane >> q) & 1) ? (T)1 : (T)-1;
  __syncthreads();
  stamp(2, 1);
  // linear_up's weights, behind the barrier: the first tail is an item's layers away, and in front of the barrier
  // these loads -- 16 bytes of up to 64 different lines each -- would stand in the queue before the phase entries.
  // (a lane without a pair loads pair 0's rows and the missing second row of an odd Q's last pair the row before it:
  //  no branch around a load, and neither is ever stored.  Q <= kSoloMaxPixels: the host checks)
  const int pair = solo_pair_of(Q, wv, lane);
  const int row_a = pair < 0 ? 0 : 2 * pair, row_b = row_a + 1 < Q ? row_a + 1 : Q - 1;
  const bool has_b = pair >= 0 && 2 * pair + 1 < Q;
  D2 wa[4], wb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    wa[j] = reinterpret_cast<const D2*>(wu)[row_a * 4 + j];
    wb[j] = reinterpret_cast<const D2*>(wu)[row_b * 4 + j];
  }
  const double bias_a = bu != nullptr ? bu[row_a] : 0.0, bias_b = bu != nullptr ? bu[row_b] : 0.0;
  // this lane's phase entries into registers, for all items of the wave (entry 0 unused: the first layer is generated)
  C phr[LPR][4];
#pragma unroll
  for (int l = 1; l < LPR; ++l) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const V4 v = reinterpret_cast<const V4*>(s_ph)[((l - 1) * 2 + h) * kWave + lane];
      phr[l][2 * h] = C{v.x, v.y};
      phr[l][2 * h + 1] = C{v.z, v.w};
    }
  }

  // ---- the rounds of this workgroup ----------------------------------------------------------------------------------
  const uint32_t n_steps = (uint32_t)d.n_steps;
  const uint32_t n_items = (uint32_t)p.batch * n_steps;         // < 2^31 (the host checks)
  const uint32_t stride = (uint32_t)gridDim.x * kSoloWaves;     // waves of the launch
  const uint32_t base0 = (uint32_t)blockIdx.x * kSoloWaves;     // the round's first item: wavefront w takes base + w
  const uint32_t stride_q = stride / n_steps, stride_r = stride - stride_q * n_steps;
  int64_t sample = (int64_t)(base0 / n_steps);                  // (sample, step) of the round's first item
  uint32_t step = base0 - (base0 / n_steps) * n_steps;
  int round = 0;
  // (the count of rounds is the same for the eight wavefronts: every one of them meets every barrier)
  for (uint32_t base = base0; base < n_items; base += stride, ++round) {
    asm volatile("" ::: "memory");   // (the LDS reads below stay inside the loop: hoisted, they would not fit registers)
    double* s_round = s_ev + (round & 1) * (kSoloWaves * 8);
    if (base + (uint32_t)wv < n_items) {   // (wave-uniform; a wavefront without an item in the last round skips to the barrier)
      C a[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = C{a0r[r], (T)0};
      // a layer's tangents are read one layer ahead (the fence keeps the compiler from reading all layers' up front)
      const V4* un4 = reinterpret_cast<const V4*>(s_un);
      V4 lo = un4[2], hi = un4[3];
#pragma unroll
      for (int l = 1; l < LPR; ++l) {
        const int ln = l + 1 < LPR ? l + 1 : l;
        const V4 nlo = un4[2 * ln], nhi = un4[2 * ln + 1];
        __builtin_amdgcn_sched_barrier(0);
        const T ts[4] = {lo.x * pm[0], lo.y * pm[1], lo.z * pm[2], lo.w * pm[3]};
        solo_layer(layout_of(l), a, phr[l], ts, hi.x, hi.y, hi.z, hi.w);
        lo = nlo;
        hi = nhi;
      }
      // ---- <Z_w>: the register-bit wires are signed in-lane sums, the lane-bit wires signed copies of the lane's total ----
      T pw[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) pw[r] = a[r].x * a[r].x + a[r].y * a[r].y;
      const T pt = (pw[0] + pw[1]) + (pw[2] + pw[3]);
      T ez[8];
      ez[0] = (pw[0] + pw[1]) - (pw[2] + pw[3]);   // wire 0 = index bit 7 = register bit 1
      ez[1] = (pw[0] + pw[2]) - (pw[1] + pw[3]);   // wire 1 = index bit 6 = register bit 0
#pragma unroll
      for (int w = 2; w < 8; ++w) ez[w] = ((llane >> (7 - w)) & 1) ? -pt : pt;
      const T tot = wave_reduce8<T>(ez, lane, llane);
      // (the lane of logical number 4 b0 + 2 b1 + b2 -> wire b0 b1 b2 holds that wire's total: qsim_adjoint.h)
      if (llane < 8) s_round[wv * 8 + (((llane & 1) << 2) | (llane & 2) | ((llane >> 2) & 1))] = (double)tot;
      if (round < 2) stamp(3 + 2 * round, 2 + 2 * round);
    }
    // the round's only barrier.  It waits for this wavefront's LDS traffic alone -- the read-out just written, the
    // reads of the round before --, not, as __syncthreads() may, for the image stores of the round before.
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // ---- linear_up: this lane's two pixels of the round's rows, two partial sums each with explicit fma (as
    // dense_lean_kernel); an item's eight <Z> are one address for all lanes, a broadcast read ------------------------------
    const uint32_t left = n_items - base, n_rows = left < (uint32_t)kSoloWaves ? left : (uint32_t)kSoloWaves;
    int64_t row_sample = sample;
    uint32_t row_step = step;
    const D2* ev2 = reinterpret_cast<const D2*>(s_round);
    D2 e01 = ev2[0], e23 = ev2[1], e45 = ev2[2], e67 = ev2[3];
    for (uint32_t k = 0; k < n_rows; ++k) {
      // (the next row's values are read while this one is computed; behind the last row, the last again)
      const uint32_t kn = k + 1 < (uint32_t)kSoloWaves ? k + 1 : k;
      const D2 n01 = ev2[4 * kn], n23 = ev2[4 * kn + 1], n45 = ev2[4 * kn + 2], n67 = ev2[4 * kn + 3];
      double a0 = bias_a, a1 = 0.0, b0 = bias_b, b1 = 0.0;
      a0 = fma(e01.x, wa[0].x, a0);
      a1 = fma(e01.y, wa[0].y, a1);
      a0 = fma(e23.x, wa[1].x, a0);
      a1 = fma(e23.y, wa[1].y, a1);
      a0 = fma(e45.x, wa[2].x, a0);
      a1 = fma(e45.y, wa[2].y, a1);
      a0 = fma(e67.x, wa[3].x, a0);
      a1 = fma(e67.y, wa[3].y, a1);
      a0 += a1;
      b0 = fma(e01.x, wb[0].x, b0);
      b1 = fma(e01.y, wb[0].y, b1);
      b0 = fma(e23.x, wb[1].x, b0);
      b1 = fma(e23.y, wb[1].y, b1);
      b0 = fma(e45.x, wb[2].x, b0);
      b1 = fma(e45.y, wb[2].y, b1);
      b0 = fma(e67.x, wb[3].x, b0);
      b1 = fma(e67.y, wb[3].y, b1);
      b0 += b1;
      double* yrow = y + (size_t)row_step * d.y_step_stride + row_sample * d.y_ld;
      // a whole pair of a 16-byte aligned row (a wave-uniform test) is one 16-byte store; a row that is not aligned
      // and the lone last pixel of an odd Q take plain 8-byte stores (an 8-byte write-through store is the slow form)
      const bool row_aligned = (reinterpret_cast<uintptr_t>(yrow) & 15) == 0;
      if (pair >= 0) {
        if (row_aligned && has_b) {
#if QIDDM_SOLO_WRITE_THROUGH
          // (the resource spans this row alone, Q * 8 <= 8 192 bytes: the 32-bit offset never limits the output's size)
          using U4 = unsigned __attribute__((ext_vector_type(4)));
          const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(yrow, 0, Q * 8, 0x00020000);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(U4, D2{a0, b0}), rsrc, pair * 16, 0, /*sc1*/ 16);
#else
          *reinterpret_cast<D2*>(yrow + 2 * pair) = D2{a0, b0};
#endif
        } else {
          yrow[2 * pair] = a0;
          if (has_b) yrow[2 * pair + 1] = b0;
        }
      }
      e01 = n01;
      e23 = n23;
      e45 = n45;
      e67 = n67;
      if (++row_step >= n_steps) {
        row_step = 0;
        ++row_sample;
      }
    }
    if (round < 2) stamp(4 + 2 * round, 3 + 2 * round);
    // the next round's first item
    sample += stride_q;
    step += stride_r;
    if (step >= n_steps) {
      step -= n_steps;
      ++sample;
    }
  }
  stamp(-1, 6);
}

}  // namespace qiddm
