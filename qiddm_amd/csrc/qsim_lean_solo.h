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
//     on each other) are spread over all wavefronts of all workgroups, WAVES = 8 or 16 per CU (two or four per SIMD;
//     the host picks the width, qiddm_lean.hip: launch_lean).
// This instance never reads the image (no re-upload: the encoders are a global phase), so a row of the output is a
// function of (tables, w_up, b_up) alone and every item of a launch has the same one -- and the eight <Z> are a function
// of the tables alone.  So the circuit is simulated when the tables are made, not when they are used:
//   * lean_solo_readout_kernel<LPR>, one wavefront, runs behind lean_tables_kernel (qiddm_dense_sample_lean_prepare).
//     It gathers the phase entries into LDS in the lanes' order, reads a layer's entries and tangents from there one
//     layer ahead, applies the LPR - 1 simulated layers, reduces the eight <Z> and leaves them as floats in the pad of
//     the tables' header (kLeanReadoutDouble ..) with the layer count as a tag behind them (kLeanReadoutTagDouble).
//   * dense_lean_solo_kernel<LPR, WAVES> executes no gate.  Its threads load linear_up's weights and biases straight
//     from global memory into registers, a thread the two rows of a pixel pair, and the read-out (32 bytes at a uniform
//     address); they compute their pair's two pixels and write them to an LDS row; behind the kernel's ONE barrier every
//     wavefront reads the row into registers, a lane the pairs lane + 64 g, once.  From there on a wavefront only
//     stores: per item the row, 16 contiguous bytes per lane and store.  A pixel is computed once per workgroup, by the
//     same instructions on the same operands in every workgroup of either width, so every row of a launch is the same
//     bits; what depends on the wave number is which items it takes.
// w_up and b_up stay operands of the launch: nothing but the tables is carried from one launch to the next.
#pragma once
#include "qsim_lean.h"

namespace qiddm {

// ---- which lane writes which pixels --------------------------------------------------------------------------------------
// linear_up by pixel pairs: the Q <= 1024 pixels of a row are ceil(Q / 2) pairs (2 pr, 2 pr + 1); lane l of the wavefront
// that writes an item's row takes the pairs l, l + 64, .. -- group g of solo_groups(Q) the pair solo_pair_of(g, l) -- and
// stores the solo_pair_pixels(Q, pr) pixels of a pair that exist: both (16 bytes), the first one of an odd Q's last pair,
// or none beyond the row.
constexpr int kSoloMaxPixels = 1024;
__host__ __device__ constexpr int solo_pairs(int q) { return (q + 1) / 2; }
__host__ __device__ constexpr int solo_pairs_padded(int q) { return (solo_pairs(q) + kWave - 1) / kWave * kWave; }
__host__ __device__ constexpr int solo_groups(int q) { return solo_pairs_padded(q) / kWave; }
__host__ __device__ constexpr int solo_pair_of(int group, int lane) { return lane + kWave * group; }
__host__ __device__ constexpr int solo_pair_pixels(int q, int pr) { return q - 2 * pr >= 2 ? 2 : q - 2 * pr == 1 ? 1 : 0; }
// Every pixel < Q is written by exactly one (group, lane) and no pixel >= Q is written, for every Q in 1 .. 1024: walking
// the (group, lane) slots in order meets the pairs 0, 1, 2, .. once each (whatever Q is: the map does not depend on it), a
// slot writes the pixels of its pair that are < Q and no others, and the groups a wavefront walks hold every pair of the
// row -- the last of them at least one.
__host__ __device__ constexpr bool solo_pairs_cover() {
  int next = 0;
  for (int g = 0; g < solo_groups(kSoloMaxPixels); ++g)
    for (int l = 0; l < kWave; ++l)
      if (solo_pair_of(g, l) != next++) return false;
  for (int q = 1; q <= kSoloMaxPixels; ++q) {
    const int pairs = solo_pairs(q), groups = solo_groups(q);
    if (groups * kWave < pairs || (groups - 1) * kWave >= pairs || groups * kWave > next) return false;
    for (int pr = (groups - 1) * kWave; pr < groups * kWave; ++pr) {   // (the groups before the last hold whole pairs)
      const int n = solo_pair_pixels(q, pr);
      if (n != (2 * pr + 1 < q ? 2 : 2 * pr < q ? 1 : 0)) return false;
    }
    if ((groups - 1) * kWave * 2 >= q || solo_pair_pixels(q, pairs - 1) != 2 - q % 2 || solo_pair_pixels(q, pairs) != 0) return false;
  }
  return true;
}
static_assert(solo_pairs_cover(), "pixel pairs: every pixel of every image size has exactly one writer");
static_assert(solo_groups(784) == 7 && solo_groups(kSoloMaxPixels) == 8, "7 groups for the flagship, 8 at most");

// LDS of the solo body: the workgroup's one row as 16-byte units [pairs padded] -- unit pr = pixels (2 pr, 2 pr + 1):
// consecutive lanes write and read consecutive 16 bytes.  linear_up's weights and bias are not here: they go from global
// memory to the registers of the thread that computes their pair.  Pad units and the missing second pixel of an odd Q's
// last pair hold finite values that are never stored.
struct LeanSoloLds {
  __host__ __device__ static constexpr size_t row_bytes(int q) { return (size_t)solo_pairs_padded(q) * 2 * sizeof(double); }
  __host__ __device__ static constexpr size_t bytes(int q) { return row_bytes(q); }
};
static_assert(LeanSoloLds::bytes(kSoloMaxPixels) == 8 * 1024, "the row of the largest image: 8 KiB");
// LDS of the read-out kernel: the tangents [layers][8] and the phase entries in the lanes' order
struct LeanReadoutLds {
  __host__ __device__ static constexpr size_t un_bytes(int layers) { return (size_t)layers * 8 * sizeof(float); }
  // the phase entries of the simulated layers 1 .. layers - 1 in the order the lanes take them: [layer][2][64] units of
  // 16 bytes, unit (l, h, lane) = the lane's entries for registers 2 h and 2 h + 1 in the layout layer l starts in
  __host__ __device__ static constexpr size_t ph_bytes(int layers) { return (size_t)(layers - 1) * 256 * 2 * sizeof(float); }
  __host__ __device__ static constexpr size_t bytes(int layers) { return un_bytes(layers) + ph_bytes(layers); }
};
// Where the read-out sits in the tables' header (qsim_lean.h: kLeanHeaderDoubles; doubles 0 .. 72 are max |t|, M and v
// of 8 qubits): eight floats <Z_0> .. <Z_7> in four doubles, and behind them the layer count they were made for as a
// double -- 0.0 (with zeros in the four) in tables that carry none.
constexpr int kLeanReadoutDouble = 73, kLeanReadoutTagDouble = 77;
static_assert(kLeanReadoutDouble >= 1 + 8 * 8 + 8 && kLeanReadoutTagDouble == kLeanReadoutDouble + 4 &&
                  kLeanReadoutTagDouble < kLeanHeaderDoubles && (kLeanReadoutDouble * sizeof(double)) % 4 == 0,
              "the read-out lies in the header's pad");

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

// ph * a, the products of cmul2 component by component -- re = fma(-ph.y, a.y, ph.x * a.x), im = fma(ph.y, a.x, ph.x * a.y)
// -- as two packed instructions: op_sel picks the half of a register pair that each component reads and neg_lo negates
// ph.y for the real part, so neither (ph.x, ph.x), (-ph.y, ph.y) nor (a.y, a.x) is ever built in registers (written in
// plain vector code the compiler builds two of them: a `v_xor` and a `v_mov` per amplitude).  Four scalar instructions
// before: 16 -> 8 of a layer's ~80.
__device__ __forceinline__ V2<float> solo_cmul(V2<float> ph, V2<float> a) {
  V2<float> prod, out;
  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(prod) : "v"(ph), "v"(a));   // ph.x * (a.x, a.y)
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]"           // (-ph.y a.y, ph.y a.x) + prod
      : "=&v"(out)
      : "v"(ph), "v"(a), "v"(prod));
  return out;
}

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
#pragma unroll
  for (int r = 0; r < 4; ++r) a[r] = solo_cmul(ph[r], a[r]);
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

// the layout simulated layer l (1 .. lpr - 1) starts in: they alternate, and the last one ends in A, where the read-out
// expects the state
__host__ __device__ constexpr int solo_layout_of(int lpr, int l) { return (lpr - 1 - l) % 2 == 0 ? kSoloLayoutB : kSoloLayoutA; }

// ---- the read-out, once per tables --------------------------------------------------------------------------------------
// One wavefront simulates the circuit of a LeanTables<float, 8> with LPR layers in one round (the layers, their order and
// their operands are those of the kernel that simulated in every workgroup of every launch: the eight <Z> are its bits)
// and writes them into the header of the tables it read (kLeanReadoutDouble ..).  It runs behind lean_tables_kernel on
// the same stream.  No address depends on the data: tables whose tangents are out of range give non-finite values
// there and nothing else (qiddm_dense_sample_lean_check turns such tables down).
template <int LPR>
__global__ __launch_bounds__(kWave) void lean_solo_readout_kernel(unsigned char* tables) {
  using T = float;
  using C = V2<T>;
  using QT = LeanTables<T, 8>;
  using V4 = T __attribute__((ext_vector_type(4)));
  static_assert(LPR > 1, "a compiled-in layer count with at least one simulated layer");
  __shared__ __attribute__((aligned(16))) unsigned char smem_raw[LeanReadoutLds::bytes(LPR)];
  T* s_un = reinterpret_cast<T*>(smem_raw);                                    // [LPR][8]
  C* s_ph = reinterpret_cast<C*>(smem_raw + LeanReadoutLds::un_bytes(LPR));    // [LPR - 1][2][64][2]
  static_assert(LeanReadoutLds::un_bytes(LPR) % 16 == 0, "16-byte reads of the tangents and the phase entries");
  const int lane = threadIdx.x;
  const int llane = logical_lane(lane);
  const T* g_body = reinterpret_cast<const T*>(tables + kLeanHeaderDoubles * sizeof(double));
  const C* g_ph = reinterpret_cast<const C*>(g_body);
  const T* g_un = g_body + QT::ph_elems(LPR);
  const T* g_a0 = g_un + QT::un_elems(LPR);
  // The phase entries of the LPR - 1 simulated layers (26 KiB at 14, gathered into the lanes' own order) and the
  // tangents go to LDS; the wavefront then reads a layer's entries from there with two 16-byte reads, one layer ahead.
  constexpr int kPhEntries = (LPR - 1) * QT::TL;                               // phase entries of layers 1 .. LPR - 1
  static_assert(kPhEntries % kWave == 0, "whole trips of the wavefront");
  constexpr int kPhTrips = kPhEntries / kWave, kUnTrips = (LPR * 8 + kWave - 1) / kWave;
#pragma unroll 4
  for (int k = 0; k < kPhTrips; ++k) {
    // LDS entry e = ((l - 1) * 2 + h) * 128 + lane * 2 + j: register r = 2 h + j of `lane` in layer l
    const int e = lane + k * kWave;
    const int l = (e >> 8) + 1, r = ((e >> 6) & 2) | (e & 1), ln = (e >> 1) & 63;
    s_ph[e] = g_ph[l * QT::TL + solo_table_slot(solo_layout_of(LPR, l), r, ln)];
  }
#pragma unroll
  for (int k = 0; k < kUnTrips; ++k) {
    const int e = lane + k * kWave;
    if (e < LPR * 8) s_un[e] = g_un[e];
  }
  T a0r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) a0r[r] = g_a0[solo_table_slot(solo_layout_of(LPR, 1), r, lane)];
  T pm[4];   // +-1 by this lane's index bit
#pragma unroll
  for (int q = 0; q < 4; ++q) pm[q] = ((llane >> q) & 1) ? (T)1 : (T)-1;
  __syncthreads();

  C a[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) a[r] = C{a0r[r], (T)0};
  // a layer's tangents and this lane's phase entries (two 16-byte units: registers 0, 1 and 2, 3) are read one layer
  // ahead (the fence keeps the compiler from reading all layers' up front)
  const V4* un4 = reinterpret_cast<const V4*>(s_un);
  const V4* ph4 = reinterpret_cast<const V4*>(s_ph) + lane;
  V4 lo = un4[2], hi = un4[3], p01 = ph4[0], p23 = ph4[kWave];
#pragma unroll
  for (int l = 1; l < LPR; ++l) {
    const int ln = l + 1 < LPR ? l + 1 : l;
    const V4 nlo = un4[2 * ln], nhi = un4[2 * ln + 1];
    const V4 np01 = ph4[(ln - 1) * 2 * kWave], np23 = ph4[((ln - 1) * 2 + 1) * kWave];
    __builtin_amdgcn_sched_barrier(0);
    const T ts[4] = {lo.x * pm[0], lo.y * pm[1], lo.z * pm[2], lo.w * pm[3]};
    const C ph[4] = {C{p01.x, p01.y}, C{p01.z, p01.w}, C{p23.x, p23.y}, C{p23.z, p23.w}};
    solo_layer(solo_layout_of(LPR, l), a, ph, ts, hi.x, hi.y, hi.z, hi.w);
    lo = nlo;
    hi = nhi;
    p01 = np01;
    p23 = np23;
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
  T ev[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) ev[w] = read_lane(tot, logical_lane(((w >> 2) & 1) | (w & 2) | ((w & 1) << 2)));
  // (plain vector stores from lane 0, as lean_tables_kernel writes its header; a float widens to the double that the
  //  sampler's linear_up multiplies by without rounding)
  if (lane == 0) {
    double* head = reinterpret_cast<double*>(tables);
    T* out = reinterpret_cast<T*>(head + kLeanReadoutDouble);
#pragma unroll
    for (int w = 0; w < 8; ++w) out[w] = ev[w];
    head[kLeanReadoutTagDouble] = (double)LPR;
  }
}

// The launches of dense_lean_kernel<float, 8, 4, false, LPR, false> that the host routes here, WAVES wavefronts per
// workgroup, one workgroup per CU.  The tables carry the read-out of lean_solo_readout_kernel<LPR> (the host's check
// has seen its tag).
// Items: (sample, step) = item / n_steps, item % n_steps for item < batch * n_steps; wave wv of workgroup b takes items
// wv * gridDim.x + b, + gridDim.x * WAVES, ...: consecutive items go to consecutive CUs, every item is written exactly
// once, by one wavefront, and no CU holds two items more than another.  Workgroup b exists only if item b does (the
// host's grid is <= ceil(items / 8)): its wavefront 0 always has an item.
constexpr int solo_threads(int waves) { return waves * kWave; }
// linear_up's operands: every thread of every wavefront takes a pixel pair, thread t the pair t: at either width the
// workgroup has a thread for every pair of the largest image, so the pairs take one trip
constexpr int solo_loaders(int waves) { return waves * kWave; }
constexpr int solo_pair_trips(int waves) { return (solo_pairs(kSoloMaxPixels) + solo_loaders(waves) - 1) / solo_loaders(waves); }
static_assert(solo_pair_trips(16) == 1 && solo_pair_trips(8) == 1, "the pairs of the largest image: one trip at both widths");
static_assert(solo_pair_trips(16) * solo_loaders(16) >= solo_pairs_padded(kSoloMaxPixels) &&
                  solo_pair_trips(8) * solo_loaders(8) >= solo_pairs_padded(kSoloMaxPixels),
              "every pair of the largest image, pad pairs included, has a thread");
static_assert(solo_loaders(8) % kWave == 0 && solo_pairs_padded(1) % kWave == 0,
              "a wavefront's 64 pairs are all inside the padded row or all beyond it");
// (word 8 + 8 * workgroups + b of a stamp buffer that long: see the stamps below)
__host__ __device__ constexpr int64_t solo_timeline_words(int64_t workgroups) { return 8 + 8 * workgroups; }
template <int LPR, int WAVES>
__global__ __launch_bounds__(solo_threads(WAVES)) void dense_lean_solo_kernel(
    const double* __restrict__ wu, const double* __restrict__ bu, double* __restrict__ y,
    const unsigned char* __restrict__ tables, const QuadScalars d, const KScalars p) {
  using D2 = double __attribute__((ext_vector_type(2)));
  static_assert(LPR > 1, "a compiled-in layer count with at least one simulated layer");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int Q = d.out_features, PairsP = solo_pairs_padded(Q);
  D2* s_row = reinterpret_cast<D2*>(smem_raw);                                      // [PairsP]
  static_assert(LeanSoloLds::row_bytes(1) % 16 == 0, "16-byte reads of the row");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  // diagnostics: wavefront 0 of workgroup 0 stamps s_memtime into words 0..7 (tools/stamp_lean_solo.py) -- [0] entry,
  // [1] the loads of linear_up's operands and of the read-out issued, [4] row barrier passed (the row is in LDS),
  // [5] the stores of its first item issued, [6] its last instruction, [7]: s_memrealtime (100 MHz) from entry to [6],
  // which gives the ticks their length.
  // When the buffer holds 8 + 8 * gridDim.x words (d.stamp_words), wavefront 0 of EVERY workgroup b also stamps
  // s_memrealtime -- the same clock on every CU -- into words 8 + 8 b .. (tools/timeline_lean_solo.py): [0] entry,
  // [1] loads issued, [3] row barrier passed, [4] the stores of its first item issued, ([2] and [5] are not written,)
  // [6] its last instruction; and the LAST wavefront of the workgroup (WAVES - 1, the youngest of its SIMD, which may
  // have no item), [7] its last instruction.  With one more word per workgroup behind those (9 * gridDim.x in all) the
  // last wavefront of workgroup b that HAD an item stamps its last instruction into word 8 + 8 * gridDim.x + b.
  // (Against the kernel that simulated in every workgroup no word moved: words [1] took the place of that kernel's
  // "setup loads issued" / "setup barrier passed", and its words [2], [3] (setup barrier, end of the simulation) and
  // timeline word [2] (end of the simulation) are gone with what they marked -- the tools read either library.)
  // The test is wave-uniform (a scalar branch per stamp); lane 0 stores.
  const bool stamp_timeline = d.stamps != nullptr && (int64_t)d.stamp_words >= solo_timeline_words(gridDim.x);
  const bool stamp_last_item = stamp_timeline && (int64_t)d.stamp_words >= solo_timeline_words(gridDim.x) + (int64_t)gridDim.x;
  const bool stamp_wave = d.stamps != nullptr && wv == 0 && (blockIdx.x == 0 || stamp_timeline);
  const unsigned long long stamp_rt0 = stamp_wave ? __builtin_amdgcn_s_memrealtime() : 0ull;
  auto stamp = [&](int word, int tword) {
    if (stamp_wave) {
      const unsigned long long t = __builtin_amdgcn_s_memtime();
      const unsigned long long rt = __builtin_amdgcn_s_memrealtime();
      if (lane == 0) {
        if (blockIdx.x == 0 && word >= 0) {
          d.stamps[word] = t;
          if (word == 6) d.stamps[7] = rt - stamp_rt0;
        }
        if (stamp_timeline && tword >= 0) d.stamps[8 + 8 * (size_t)blockIdx.x + tword] = rt;
      }
    }
  };
  stamp(0, 0);

  // ---- the workgroup's one row ---------------------------------------------------------------------------------------
  // A thread takes a pair: the pair's two rows of w_up are 128 contiguous bytes, eight 16-byte chunks (chunk u = the
  // weights (w[2 k], w[2 k + 1]), k = u & 3, of row 2 pr + (u >> 2)), and its two biases.  A chunk or a bias beyond
  // the image loads the last one; its pixel is never stored.  The 64 pairs of a wavefront are all inside the padded
  // row or all beyond it (a wave-uniform test): a wavefront beyond it loads nothing.  (Q <= kSoloMaxPixels: the host
  // checks.)  The eight <Z> come from the tables' header, the same 32 bytes for every thread.  Every load is issued
  // before anything waits.
  constexpr int kLoaders = solo_loaders(WAVES), kPairTrips = solo_pair_trips(WAVES);
  const D2* wu2 = reinterpret_cast<const D2*>(wu);
  D2 wreg[kPairTrips][8], breg[kPairTrips];
#pragma unroll
  for (int k = 0; k < kPairTrips; ++k) {
    const int pr = tid + k * kLoaders;
    if (pr < PairsP) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = 8 * pr + u;
        wreg[k][u] = wu2[i < 4 * Q ? i : 4 * Q - 1];
      }
      const int i0 = 2 * pr < Q ? 2 * pr : Q - 1, i1 = 2 * pr + 1 < Q ? 2 * pr + 1 : Q - 1;
      breg[k] = bu != nullptr ? D2{bu[i0], bu[i1]} : D2{0.0, 0.0};
    }
  }
  const float* g_ez = reinterpret_cast<const float*>(tables + kLeanReadoutDouble * sizeof(double));
  float ezf[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) ezf[w] = g_ez[w];
  __builtin_amdgcn_sched_barrier(0);   // (all loads are out)
  stamp(1, 1);
  double ev[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) ev[w] = (double)ezf[w];
  // ---- linear_up: per pixel two partial sums with explicit fma (as dense_lean_kernel) and one add --------------------
#pragma unroll
  for (int k = 0; k < kPairTrips; ++k) {
    const int pr = tid + k * kLoaders;
    if (pr < PairsP) {
      const D2 wa0 = wreg[k][0], wa1 = wreg[k][1], wa2 = wreg[k][2], wa3 = wreg[k][3];
      const D2 wb0 = wreg[k][4], wb1 = wreg[k][5], wb2 = wreg[k][6], wb3 = wreg[k][7];
      const D2 bias = breg[k];
      double a0 = bias.x, a1 = 0.0, b0 = bias.y, b1 = 0.0;
      a0 = fma(ev[0], wa0.x, a0);
      a1 = fma(ev[1], wa0.y, a1);
      a0 = fma(ev[2], wa1.x, a0);
      a1 = fma(ev[3], wa1.y, a1);
      a0 = fma(ev[4], wa2.x, a0);
      a1 = fma(ev[5], wa2.y, a1);
      a0 = fma(ev[6], wa3.x, a0);
      a1 = fma(ev[7], wa3.y, a1);
      a0 += a1;
      b0 = fma(ev[0], wb0.x, b0);
      b1 = fma(ev[1], wb0.y, b1);
      b0 = fma(ev[2], wb1.x, b0);
      b1 = fma(ev[3], wb1.y, b1);
      b0 = fma(ev[4], wb2.x, b0);
      b1 = fma(ev[5], wb2.y, b1);
      b0 = fma(ev[6], wb3.x, b0);
      b1 = fma(ev[7], wb3.y, b1);
      b0 += b1;
      s_row[pr] = D2{a0, b0};
    }
  }
  __syncthreads();   // (the row is in LDS: the kernel's one barrier)
  stamp(4, 3);

  // ---- the items of this wave: stores only ---------------------------------------------------------------------------
  // (a lane's units of the row, pair = lane + 64 g, read once; a group beyond the image re-reads group 0 and is not stored)
  const int groups = solo_groups(Q);
  constexpr int kMaxGroups = solo_groups(kSoloMaxPixels);
  D2 rowreg[kMaxGroups];
#pragma unroll
  for (int g = 0; g < kMaxGroups; ++g) rowreg[g] = s_row[solo_pair_of(g < groups ? g : 0, lane)];
  const uint32_t n_steps = (uint32_t)d.n_steps;
  const uint32_t stride = (uint32_t)gridDim.x * WAVES;          // waves of the launch
  const uint32_t g0 = (uint32_t)wv * gridDim.x + (uint32_t)blockIdx.x;
  const uint32_t stride_q = stride / n_steps, stride_r = stride - stride_q * n_steps;
  int64_t sample = (int64_t)(g0 / n_steps);
  uint32_t step = g0 - (g0 / n_steps) * n_steps;
  for (int item = 0; sample < p.batch; ++item) {
    double* yrow = y + (size_t)step * d.y_step_stride + sample * d.y_ld;
    // a whole pair of a 16-byte aligned row (a wave-uniform test) is one 16-byte store; a row that is not aligned and
    // the lone last pixel of an odd Q take plain 8-byte stores (an 8-byte write-through store is the slow form)
    const bool row_aligned = (reinterpret_cast<uintptr_t>(yrow) & 15) == 0;
#if QIDDM_SOLO_WRITE_THROUGH
    // (the resource spans this row alone, Q * 8 <= 8 192 bytes: the 32-bit offset never limits the output's size)
    using U4 = unsigned __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(yrow, 0, Q * 8, 0x00020000);
#endif
#pragma unroll
    for (int g = 0; g < kMaxGroups; ++g) {
      if (g < groups) {
        const int pr = solo_pair_of(g, lane), n_pix = solo_pair_pixels(Q, pr);
        if (row_aligned && n_pix == 2) {
#if QIDDM_SOLO_WRITE_THROUGH
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(U4, rowreg[g]), rsrc, pr * 16, 0, /*sc1*/ 16);
#else
          *reinterpret_cast<D2*>(yrow + 2 * pr) = rowreg[g];
#endif
        } else if (n_pix > 0) {
          yrow[2 * pr] = rowreg[g].x;
          if (n_pix == 2) yrow[2 * pr + 1] = rowreg[g].y;
        }
      }
    }
    if (item == 0) stamp(5, 4);
    // next item of this wave
    sample += stride_q;
    step += stride_r;
    if (step >= n_steps) {
      step -= n_steps;
      ++sample;
    }
  }
  stamp(6, 6);
  if (stamp_timeline && wv == WAVES - 1) {
    const unsigned long long rt = __builtin_amdgcn_s_memrealtime();
    if (lane == 0) d.stamps[8 + 8 * (size_t)blockIdx.x + 7] = rt;
  }
  // (the last wavefront of this workgroup with a first item: the next one's would lie beyond the launch's items)
  if (stamp_last_item) {
    const uint64_t n_items = (uint64_t)p.batch * n_steps;
    if (g0 < n_items && (wv == WAVES - 1 || (uint64_t)g0 + gridDim.x >= n_items)) {
      const unsigned long long rt = __builtin_amdgcn_s_memrealtime();
      if (lane == 0) d.stamps[solo_timeline_words(gridDim.x) + blockIdx.x] = rt;
    }
  }
}

}  // namespace qiddm
