// qsim_mixed_wide.h -- tile-fused density-matrix sweeps: forward execution of the programs of qsim_mixed.h at
// n = 7..10 wires (the reference's 28 x 28 noise study samples 10-wire models on default.mixed,
// src/fashion_noise.py:42-44, 207-225).
//
// rho of a sample is a vector on 2n index bits, k = (i << n) | j, and lives in a slab of the workspace.  A gate or
// channel on wire w acts on the bit pair (q, q + n), q = n - 1 - w.  A SWEEP is one launch over (tile, sample): a
// workgroup gathers the 2^12 elements whose 12 LOCAL bits are the pairs of six wires, keeps them in LDS (32 KiB in
// float32, 64 KiB in float64), applies a whole SEGMENT of the program and writes them back.  The other 2n - 12 bits
// are the tile number.  A segment holds
//   * ops that are diagonal on vec(rho) -- PHASE, CZ, PhaseDamping -- on any wires: the factor of an element depends
//     on its global index only (tile bits + local bits);
//   * GATE / RY / AmplitudeDamping / Depolarizing / the general channel on a tile wire, CNOT and the general two-wire
//     channel with both wires in the tile (2^12 / 16 = 256 blocks of 4 x 4: one per thread);
//   * ZERO / AMP_EMBED as its first op: the tile is generated instead of read.
// The host cuts the program into segments (plan_mixed_wide in qiddm_mixed.hip) and uploads it sorted by segment.
// Wires n-1 and n-2 (q = 0, 1) belong to every tile: the two lowest column bits are local, so a lane moves two
// consecutive elements (16 bytes in float32) and four lanes cover 64 contiguous bytes.
// Per 2 x 2 block and per element the arithmetic is that of mixed_apply_op (shared helpers in qsim_mixed.h).
// `dst_delta` (elements; 0 in the forward) moves the write-back to another set of slabs: the reverse sweep's replay
// (qsim_mixed_wide_adjoint.h) leaves the state in front of a channel segment behind as its snapshot.
#pragma once
#include "qsim_mixed.h"

namespace qiddm {

// Tile width: six wires.  -DQIDDM_WIDE_TILE_WIRES=5 builds the five-wire variant (2^10 elements a tile) for A/B runs;
// the loops below take their trip counts from it.
#ifndef QIDDM_WIDE_TILE_WIRES
#define QIDDM_WIDE_TILE_WIRES 6
#endif
constexpr int kWideTileWires = QIDDM_WIDE_TILE_WIRES;
constexpr int kWideLocalBits = 2 * kWideTileWires;
constexpr uint32_t kWideTile = 1u << kWideLocalBits;
constexpr int kWideMaxTileBits = 20 - kWideLocalBits;  // tile-number bits at 10 wires
constexpr int kWideHiBits = kWideLocalBits - 6;        // local bits above the low six
constexpr int kWidePairs = kWideTile / 512;            // element pairs per thread
constexpr int kWideBlocks = kWideTile / 1024;          // 2 x 2 blocks per thread
constexpr int kWideElems = kWideTile / 256;            // elements per thread
static_assert(kWideTileWires == 5 || kWideTileWires == 6, "tile width");

struct WideSegment {
  int32_t op_begin, op_end;   // into the uploaded (segment-sorted) program
  int32_t n_tile_bits, pad_;  // 2n - kWideLocalBits
  uint8_t lpos[12];           // global bit of local bit r, ascending; lpos[0] = 0, lpos[1] = 1
  uint8_t gpos[kWideMaxTileBits];  // global bit of tile-number bit r, ascending
};

template <typename T>
using V4 = T __attribute__((ext_vector_type(4)));

template <int COUNT>
__device__ __forceinline__ uint32_t wide_deposit(uint32_t v, const uint8_t* pos) {
  uint32_t out = 0;
#pragma unroll
  for (int r = 0; r < COUNT; ++r) out |= ((v >> r) & 1u) << pos[r];
  return out;
}
// rank of global bit `g` among the local bits (the planner guarantees it is there)
__device__ __forceinline__ int wide_local_rank(const WideSegment& sg, int g) {
  int r = 0;
#pragma unroll
  for (int i = 0; i < kWideLocalBits; ++i) r = sg.lpos[i] == g ? i : r;
  return r;
}

// |v|^2 of every resident sample's feature row (AMP_EMBED), in the order of the 8-wire kernel
__global__ __launch_bounds__(256) void mixed_wide_norms(const double* __restrict__ feats, double* __restrict__ norms,
                                                        const MixedScalars m, int64_t sample0) {
  __shared__ double s_red[256];
  const int64_t sample = sample0 + blockIdx.x;
  const double v = mixed_embed_norm2(feats + sample * m.feat_ld, s_red, m);
  if (threadIdx.x == 0) norms[blockIdx.x] = v;
}

// LEVEL (MixedLevel, qsim_mixed.h): the general-channel cases the instantiation carries; a segment is launched at the
// lowest level that holds its ops
template <typename T, int LEVEL>
__global__ __launch_bounds__(256) void mixed_wide_sweep(const MixedOp* __restrict__ prog,
                                                        const double* __restrict__ angle_rows,
                                                        const double* __restrict__ feats,
                                                        const double* __restrict__ gates,
                                                        const double* __restrict__ norms, V2<T>* __restrict__ slabs,
                                                        const MixedScalars m, const WideSegment sg, int64_t sample0,
                                                        int64_t dst_delta) {
  using C = V2<T>;
  extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];
  __shared__ uint32_t s_lo[64], s_hi[64];
  C* tile = reinterpret_cast<C*>(smem_raw);
  const int n = m.n, tid = threadIdx.x;
  const int64_t resident = blockIdx.y, sample = sample0 + resident;
  C* __restrict__ rho = slabs + ((size_t)resident << (2 * n));
  const uint32_t base = wide_deposit<kWideMaxTileBits>(blockIdx.x, sg.gpos);  // the tile number has n_tile_bits bits
  if (tid < 64) {
    s_lo[tid] = wide_deposit<6>(tid, sg.lpos);
    s_hi[tid] = wide_deposit<kWideHiBits>(tid, sg.lpos + 6);
  }
  __syncthreads();
  // a thread owns the element pairs l = 2 (tid + 256 i), l + 1: global k, k + 1 (lpos[0] = 0)
  uint32_t kown[kWidePairs];
#pragma unroll
  for (int i = 0; i < kWidePairs; ++i) {
    const uint32_t l = 2u * (tid + 256u * i);
    kown[i] = base | s_lo[l & 63u] | s_hi[l >> 6];
  }

  int oi = sg.op_begin;
  const int first_kind = prog[oi].kind;
  if (first_kind == kMixZero) {
#pragma unroll
    for (int i = 0; i < kWidePairs; ++i) {
      const uint32_t l = 2u * (tid + 256u * i);
      tile[l] = C{kown[i] == 0 ? (T)1 : (T)0, (T)0};
      tile[l + 1] = C{(T)0, (T)0};
    }
    ++oi;
  } else if (first_kind == kMixAmpEmbed) {
    const double* __restrict__ row = feats + sample * m.feat_ld;
    const double inv = 1.0 / norms[resident];
#pragma unroll
    for (int i = 0; i < kWidePairs; ++i) {
      const uint32_t l = 2u * (tid + 256u * i);
      tile[l] = mixed_embed_elem<T>(row, kown[i], inv, m);
      tile[l + 1] = mixed_embed_elem<T>(row, kown[i] + 1u, inv, m);
    }
    ++oi;
  } else {
#pragma unroll
    for (int i = 0; i < kWidePairs; ++i) {
      const uint32_t l = 2u * (tid + 256u * i);
      const V4<T> v = *reinterpret_cast<const V4<T>*>(rho + kown[i]);
      *reinterpret_cast<V4<T>*>(tile + l) = v;
    }
  }

  // Diagonal ops work on the elements their thread owns: no barrier between two of them.
  bool owned = true;
  for (; oi < sg.op_end; ++oi) {
    const MixedOp op = prog[oi];
    const int q = n - 1 - op.wire;
    const bool diag = op.kind == kMixPhase || op.kind == kMixCZ || op.kind == kMixPhaseDamp;
    if (!(diag && owned)) __syncthreads();
    owned = diag;
    switch (op.kind) {
      case kMixPhase: {
        C up, dn;
        mixed_phase_factors<T>(mixed_angle(op, angle_rows, m, sample), up, dn);
#pragma unroll
        for (int i = 0; i < kWidePairs; ++i) {
          const uint32_t l = 2u * (tid + 256u * i);
          tile[l] = mixed_phase_elem<T>(tile[l], kown[i], q, n, up, dn);
          tile[l + 1] = mixed_phase_elem<T>(tile[l + 1], kown[i] + 1u, q, n, up, dn);
        }
        break;
      }
      case kMixCZ: {
        const int qt = n - 1 - op.a;
#pragma unroll
        for (int i = 0; i < kWidePairs; ++i) {
          const uint32_t l = 2u * (tid + 256u * i);
          tile[l] = mixed_cz_elem<T>(tile[l], kown[i], q, qt, n);
          tile[l + 1] = mixed_cz_elem<T>(tile[l + 1], kown[i] + 1u, q, qt, n);
        }
        break;
      }
      case kMixPhaseDamp: {
        const T off = mixed_channel<T>(op.kind, mixed_angle(op, angle_rows, m, sample)).off;
#pragma unroll
        for (int i = 0; i < kWidePairs; ++i) {
          const uint32_t l = 2u * (tid + 256u * i);
          tile[l] = mixed_phase_damp_elem<T>(tile[l], kown[i], q, n, off);
          tile[l + 1] = mixed_phase_damp_elem<T>(tile[l + 1], kown[i] + 1u, q, n, off);
        }
        break;
      }
      case kMixRY:
      case kMixGate:
      case kMixAmpDamp:
      case kMixDepol: {
        const int a = wide_local_rank(sg, q), b = wide_local_rank(sg, q + n);
        const uint32_t cj = 1u << a, ci = 1u << b;
        const bool unitary = op.kind == kMixRY || op.kind == kMixGate;
        MixedU<T> u{};
        MixedChannel<T> ch{};
        if (unitary) u = mixed_unitary<T>(op, angle_rows, gates, m, sample);
        else ch = mixed_channel<T>(op.kind, mixed_angle(op, angle_rows, m, sample));
#pragma unroll
        for (int i = 0; i < kWideBlocks; ++i) {
          const uint32_t l = insert_two_bits(tid + 256u * i, a, b);
          C m00 = tile[l], m01 = tile[l | cj], m10 = tile[l | ci], m11 = tile[l | ci | cj];
          if (unitary) mixed_block_unitary<T>(u, m00, m01, m10, m11);
          else mixed_block_channel<T>(ch, m00, m01, m10, m11);
          tile[l] = m00;
          tile[l | cj] = m01;
          tile[l | ci] = m10;
          tile[l | ci | cj] = m11;
        }
        break;
      }
      case kMixChannel2: {
        if constexpr (LEVEL >= kLevelChannel2) {
          const int q2 = n - 1 - op.wire2;
          const MixedBlock2 b = mixed_block2(wide_local_rank(sg, q), wide_local_rank(sg, q2), wide_local_rank(sg, q + n),
                                             wide_local_rank(sg, q2 + n));
          const auto su = mixed_super2<T>(op, gates);
          for (uint32_t t = tid; t < kWideTile / 16; t += 256) mixed_block_super2<T, false>(su, tile, nullptr, mixed_block2_base(t, b), b);
        }
        break;
      }
      case kMixChannel: {
        if constexpr (LEVEL >= kLevelChannel) {
          const int a = wide_local_rank(sg, q), b = wide_local_rank(sg, q + n);
          const uint32_t cj = 1u << a, ci = 1u << b;
          const MixedSuper<T> su = mixed_super<T>(op, gates);
#pragma unroll
          for (int i = 0; i < kWideBlocks; ++i) {
            const uint32_t l = insert_two_bits(tid + 256u * i, a, b);
            C m00 = tile[l], m01 = tile[l | cj], m10 = tile[l | ci], m11 = tile[l | ci | cj];
            mixed_block_super<T>(su, m00, m01, m10, m11);
            tile[l] = m00;
            tile[l | cj] = m01;
            tile[l | ci] = m10;
            tile[l | ci | cj] = m11;
          }
        }
        break;
      }
      case kMixCNOT: {
        // the permutation of mixed_cnot_index on the local bits: columns (ac -> at), rows (bc -> bt)
        const int qt = n - 1 - op.a;
        const int ac = wide_local_rank(sg, q), at = wide_local_rank(sg, qt);
        const int bc = wide_local_rank(sg, q + n), bt = wide_local_rank(sg, qt + n);
#pragma unroll
        for (int i = 0; i < kWideElems; ++i) {
          const uint32_t l = tid + 256u * i;
          const uint32_t pl = l ^ (((l >> ac) & 1u) << at) ^ (((l >> bc) & 1u) << bt);
          if (l < pl) {
            const C tmp = tile[l];
            tile[l] = tile[pl];
            tile[pl] = tmp;
          }
        }
        break;
      }
      default: break;
    }
  }
  if (!owned) __syncthreads();
#pragma unroll
  for (int i = 0; i < kWidePairs; ++i) {
    const uint32_t l = 2u * (tid + 256u * i);
    *reinterpret_cast<V4<T>*>(rho + dst_delta + kown[i]) = *reinterpret_cast<const V4<T>*>(tile + l);
  }
}

// the diagonal of every resident sample -> probs / <Z_w> (the read-out of mixed_kernel)
template <typename T>
__global__ __launch_bounds__(256) void mixed_wide_read_out(const V2<T>* __restrict__ slabs, double* __restrict__ out,
                                                           const MixedScalars m, int64_t sample0) {
  __shared__ double s_red[256];
  mixed_read_out<T>(slabs + ((size_t)blockIdx.x << (2 * m.n)), out, s_red, m, sample0 + blockIdx.x);
}

// the sampled read-out (qsim_mixed_shots.h) in its place when the program ends in kMixShots: one workgroup per resident
// sample, keyed by the absolute row sample0 + blockIdx.x, so the chunking does not move a stream
template <typename T>
__global__ __launch_bounds__(256) void mixed_wide_sampled_read_out(const V2<T>* __restrict__ slabs,
                                                                   double* __restrict__ out, const MixedScalars m,
                                                                   int64_t sample0, const MixedShots sh) {
  __shared__ double s_cdf[1024];    // n <= 10
  __shared__ uint32_t s_cnt[1024];
  const int64_t sample = sample0 + blockIdx.x;
  mixed_sample_read_out<T>(slabs + ((size_t)blockIdx.x << (2 * m.n)), out + sample * m.out_ld, s_cdf, s_cnt, m.n, m.measure,
                           sample, sh);
}

}  // namespace qiddm
