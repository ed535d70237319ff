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
//   * GATE / RY / AmplitudeDamping / Depolarizing / the general channel on a tile wire, CNOT, the two-wire unitary and
//     the general two-wire channel with both wires in the tile (2^12 / 16 = 256 blocks of 4 x 4: one per thread);
//   * ZERO / AMP_EMBED as its first op: the tile is generated instead of read.
// The host cuts the program into segments (plan_mixed_wide in qiddm_mixed.hip) and uploads it sorted by segment.
// Wires n-1 and n-2 (q = 0, 1) belong to every tile: the two lowest column bits are local, so a lane moves two
// consecutive elements (16 bytes in float32) and four lanes cover 64 contiguous bytes.
// Per 2 x 2 block and per element the arithmetic is that of the one-workgroup engine, and so is the walk over a wire's
// blocks, on local ranks instead of global bits (MixedBlock1 and the block visitors of qsim_mixed.h).  What is the tile
// engine's own sits below in one place for all its kernels: the indices a thread owns, the copies between slab and
// tile, the walkers over owned elements and over a thread's blocks, and wide_channel_op, the channel kinds on a tile.
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

// ---- tile plumbing: every kernel of the engine (here and in qsim_mixed_wide_adjoint.h) moves and walks its tiles with these
// The global indices of the element pairs a thread owns: l = 2 (tid + 256 i), l + 1 -> k, k + 1 (lpos[0] = 0).  Ends
// in a barrier.
__device__ __forceinline__ void wide_owned_indices(const WideSegment& sg, uint32_t* s_lo, uint32_t* s_hi,
                                                   uint32_t (&kown)[kWidePairs]) {
  const int tid = threadIdx.x;
  const uint32_t base = wide_deposit<kWideMaxTileBits>(blockIdx.x, sg.gpos);  // the tile number has n_tile_bits bits
  if (tid < 64) {
    s_lo[tid] = wide_deposit<6>(tid, sg.lpos);
    s_hi[tid] = wide_deposit<kWideHiBits>(tid, sg.lpos + 6);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kWidePairs; ++i) {
    const uint32_t l = 2u * (tid + 256u * i);
    kown[i] = base | s_lo[l & 63u] | s_hi[l >> 6];
  }
}
// slab -> tile and tile -> slab, a thread its own pairs (a pair: 16 bytes in float32)
template <typename T>
__device__ __forceinline__ void wide_load_pair(V2<T>* tile, const V2<T>* slab, const uint32_t (&kown)[kWidePairs], int i) {
  *reinterpret_cast<V4<T>*>(tile + 2u * (threadIdx.x + 256u * i)) = *reinterpret_cast<const V4<T>*>(slab + kown[i]);
}
template <typename T>
__device__ __forceinline__ void wide_load_tile(V2<T>* tile, const V2<T>* slab, const uint32_t (&kown)[kWidePairs]) {
#pragma unroll
  for (int i = 0; i < kWidePairs; ++i) wide_load_pair<T>(tile, slab, kown, i);
}
template <typename T>
__device__ __forceinline__ void wide_store_tile(V2<T>* slab, const V2<T>* tile, const uint32_t (&kown)[kWidePairs],
                                                int64_t dst_delta) {
#pragma unroll
  for (int i = 0; i < kWidePairs; ++i)
    *reinterpret_cast<V4<T>*>(slab + dst_delta + kown[i]) = *reinterpret_cast<const V4<T>*>(tile + 2u * (threadIdx.x + 256u * i));
}
// every element the thread owns, for the element-wise kinds: f(l, k), l its index in the tile and k in rho
template <typename F>
__device__ __forceinline__ void wide_for_owned(const uint32_t (&kown)[kWidePairs], F&& f) {
#pragma unroll
  for (int i = 0; i < kWidePairs; ++i) {
    const uint32_t l = 2u * (threadIdx.x + 256u * i);
    f(l, kown[i]);
    f(l + 1u, kown[i] + 1u);
  }
}
// the 2 x 2 blocks of the tile wire with column bit q, by local ranks
__device__ __forceinline__ MixedBlock1 wide_block(const WideSegment& sg, int q, int n) {
  return MixedBlock1{wide_local_rank(sg, q), wide_local_rank(sg, q + n)};
}
// mixed_walk_blocks on a tile: kWideBlocks blocks a thread, a constant, so the loops unroll
template <typename T, typename F>
__device__ __forceinline__ void wide_walk_blocks(V2<T>* tile, const MixedBlock1& b, F&& f) {
#pragma unroll
  for (int i = 0; i < kWideBlocks; ++i) mixed_block_visit<T>(tile, nullptr, threadIdx.x + 256u * i, b, f);
}
// the general two-wire channel on a tile (ADJOINT: S^H): 2^12 / 16 = 256 blocks of 4 x 4, one per thread
template <typename T, bool ADJOINT>
__device__ __forceinline__ void wide_channel2(const MixedOp& op, V2<T>* tile, const double* __restrict__ gates,
                                              const MixedScalars& m, const WideSegment& sg) {
  const int n = m.n, q = n - 1 - op.wire, q2 = n - 1 - op.wire2;
  const MixedBlock2 bl = mixed_block2(wide_local_rank(sg, q), wide_local_rank(sg, q2), wide_local_rank(sg, q + n),
                                      wide_local_rank(sg, q2 + n));
  const auto su = mixed_super2<T>(op, gates);
  for (uint32_t t = threadIdx.x; t < kWideTile / 16; t += 256) mixed_block_super2<T, ADJOINT>(su, tile, nullptr, mixed_block2_base(t, bl), bl);
}

// the 4 x 4 blocks of the op's two tile wires, by local ranks (the geometry wide_channel2 above works out for itself)
__device__ __forceinline__ MixedBlock2 wide_block2(const MixedOp& op, const MixedScalars& m, const WideSegment& sg) {
  const int n = m.n, q = n - 1 - op.wire, q2 = n - 1 - op.wire2;
  return mixed_block2(wide_local_rank(sg, q), wide_local_rank(sg, q2), wide_local_rank(sg, q + n), wide_local_rank(sg, q2 + n));
}
// the two-wire unitary on a tile: U M U^dagger on its 256 blocks of 4 x 4, one per thread
template <typename T>
__device__ __forceinline__ void wide_gate2(const MixedOp& op, V2<T>* tile, const double* __restrict__ gates,
                                           const MixedScalars& m, const WideSegment& sg) {
  const MixedBlock2 bl = wide_block2(op, m, sg);
  const MixedU2<T> u = mixed_unitary2<T>(op, gates);
  for (uint32_t t = threadIdx.x; t < kWideTile / 16; t += 256) mixed_block_gate2<T, false>(u, tile, mixed_block2_base(t, bl), bl);
}

// One op of a channel kind on a tile in LDS with this sample's strength: E, or with ADJOINT E^dagger.  It is the
// channel body of mixed_wide_adjoint_channels_graded in both directions.  mixed_wide_sweep and
// mixed_wide_adjoint_channels list the same cases themselves, one walker call each: the compiler fuses the native
// arithmetic differently here (the kind is tested inside the walk) than in a walk of its own, so in float32 the two
// give different last bits, and the float64 adjoint kernel holds 8 waves with its own list and 5 through this function.
// LEVEL (MixedLevel, qsim_mixed.h): the general-channel cases the instantiation carries.  PhaseDamping works on the
// elements its thread owns (any wire; E^dagger = E).  The caller puts a barrier between ops.
template <typename T, int LEVEL, bool ADJOINT>
__device__ __forceinline__ void wide_channel_op(const MixedOp& op, V2<T>* tile, const uint32_t (&kown)[kWidePairs],
                                                const double* __restrict__ angle_rows, const double* __restrict__ gates,
                                                const MixedScalars& m, const WideSegment& sg, int64_t sample) {
  using C = V2<T>;
  const int n = m.n, q = n - 1 - op.wire;
  if constexpr (mixed_channels_of(LEVEL) >= kLevelChannel2) {
    if (op.kind == kMixChannel2) {
      wide_channel2<T, ADJOINT>(op, tile, gates, m, sg);
      return;
    }
  }
  if (op.kind == kMixPhaseDamp) {
    const T off = mixed_channel<T>(op.kind, mixed_angle(op, angle_rows, m, sample)).off;
    wide_for_owned(kown, [&](uint32_t l, uint32_t k) { tile[l] = mixed_phase_damp_elem<T>(tile[l], k, q, n, off); });
    return;
  }
  // one walk for the general and the native kinds, the kind tested inside it
  const bool general = mixed_channels_of(LEVEL) >= kLevelChannel && op.kind == kMixChannel;
  MixedSuper<T> su{};
  MixedChannel<T> ch{};
  if constexpr (mixed_channels_of(LEVEL) >= kLevelChannel) {
    if (general) su = mixed_super<T>(op, gates);
  }
  if (!general) ch = mixed_channel<T>(op.kind, mixed_angle(op, angle_rows, m, sample));
  wide_walk_blocks<T>(tile, wide_block(sg, q, n), [&](C& m00, C& m01, C& m10, C& m11) {
    if constexpr (mixed_channels_of(LEVEL) >= kLevelChannel) {
      if (general) {
        if (ADJOINT) mixed_block_super_adjoint<T>(su, m00, m01, m10, m11);
        else mixed_block_super<T>(su, m00, m01, m10, m11);
      }
    }
    if (!general) {
      if (ADJOINT) mixed_block_channel_adjoint<T>(ch, m00, m01, m10, m11);
      else mixed_block_channel<T>(ch, m00, m01, m10, m11);
    }
  });
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
  uint32_t kown[kWidePairs];
  wide_owned_indices(sg, s_lo, s_hi, kown);

  int oi = sg.op_begin;
  const int first_kind = prog[oi].kind;
  if (first_kind == kMixZero) {
    wide_for_owned(kown, [&](uint32_t l, uint32_t k) { tile[l] = C{k == 0 ? (T)1 : (T)0, (T)0}; });
    ++oi;
  } else if (first_kind == kMixAmpEmbed) {
    const double* __restrict__ row = feats + sample * m.feat_ld;
    const double inv = 1.0 / norms[resident];
    wide_for_owned(kown, [&](uint32_t l, uint32_t k) { tile[l] = mixed_embed_elem<T>(row, k, inv, m); });
    ++oi;
  } else {
    wide_load_tile<T>(tile, rho, kown);
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
        wide_for_owned(kown, [&](uint32_t l, uint32_t k) { tile[l] = mixed_phase_elem<T>(tile[l], k, q, n, up, dn); });
        break;
      }
      case kMixCZ: {
        const int qt = n - 1 - op.a;
        wide_for_owned(kown, [&](uint32_t l, uint32_t k) { tile[l] = mixed_cz_elem<T>(tile[l], k, q, qt, n); });
        break;
      }
      case kMixPhaseDamp: {
        const T off = mixed_channel<T>(op.kind, mixed_angle(op, angle_rows, m, sample)).off;
        wide_for_owned(kown, [&](uint32_t l, uint32_t k) { tile[l] = mixed_phase_damp_elem<T>(tile[l], k, q, n, off); });
        break;
      }
      case kMixRY:
      case kMixGate:
      case kMixAmpDamp:
      case kMixDepol: {  // one walk for the unitary and the native channel kinds: two cost a resident wave
        const bool unitary = op.kind == kMixRY || op.kind == kMixGate;
        MixedU<T> u{};
        MixedChannel<T> ch{};
        if (unitary) u = mixed_unitary<T>(op, angle_rows, gates, m, sample);
        else ch = mixed_channel<T>(op.kind, mixed_angle(op, angle_rows, m, sample));
        wide_walk_blocks<T>(tile, wide_block(sg, q, n), [&](C& m00, C& m01, C& m10, C& m11) {
          if (unitary) mixed_block_unitary<T>(u, m00, m01, m10, m11);
          else mixed_block_channel<T>(ch, m00, m01, m10, m11);
        });
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
      case kMixChannel: {
        if constexpr (mixed_channels_of(LEVEL) >= kLevelChannel) {
          const MixedSuper<T> su = mixed_super<T>(op, gates);
          wide_walk_blocks<T>(tile, wide_block(sg, q, n),
                              [&](C& m00, C& m01, C& m10, C& m11) { mixed_block_super<T>(su, m00, m01, m10, m11); });
        }
        break;
      }
      case kMixChannel2: {
        if constexpr (mixed_channels_of(LEVEL) >= kLevelChannel2) wide_channel2<T, false>(op, tile, gates, m, sg);
        break;
      }
      case kMixGate2: {
        if constexpr (mixed_has_gate2(LEVEL)) wide_gate2<T>(op, tile, gates, m, sg);
        break;
      }
      default: break;
    }
  }
  if (!owned) __syncthreads();
  wide_store_tile<T>(rho, tile, kown, dst_delta);
}

// the diagonal of every resident sample -> probs / <Z_w> (the read-out of mixed_kernel)
template <typename T>
__global__ __launch_bounds__(256) void mixed_wide_read_out(const V2<T>* __restrict__ slabs, double* __restrict__ out,
                                                           const MixedScalars m, int64_t sample0) {
  __shared__ double s_red[256];
  mixed_read_out<T>(slabs + ((size_t)blockIdx.x << (2 * m.n)), out, s_red, m, sample0 + blockIdx.x);
}

// the measurement table's read-out (measure 2; mixed_obs_read_out of qsim_mixed.h) in its place: the m.n_obs terms sit
// behind the m.n_ops sorted ops of the uploaded program
template <typename T>
__global__ __launch_bounds__(256) void mixed_wide_obs_read_out(const MixedOp* __restrict__ prog,
                                                               const V2<T>* __restrict__ slabs, double* __restrict__ out,
                                                               const MixedScalars m, int64_t sample0) {
  __shared__ double s_term[256];
  mixed_obs_read_out<T>(slabs + ((size_t)blockIdx.x << (2 * m.n)), out + (sample0 + blockIdx.x) * m.out_ld, s_term,
                        prog + m.n_ops, m.n_obs, m.n);
}

// the reduced density matrix's read-out (measure 8; mixed_rho_read_out of qsim_mixed.h) in its place: `mask` is the keep-mask
// of the kMixRho op the program ended in.  Grid (parts, resident samples): the workgroups of a sample share its 4^k
// output elements, each written once by one thread, so the result does not depend on `parts` or on the chunking.
template <typename T>
__global__ __launch_bounds__(256) void mixed_wide_rho_read_out(const V2<T>* __restrict__ slabs, double* __restrict__ out,
                                                               const MixedScalars m, int64_t sample0, const uint32_t mask) {
  mixed_rho_read_out<T>(slabs + ((size_t)blockIdx.y << (2 * m.n)), out + (sample0 + blockIdx.y) * m.out_ld, mask, m.n,
                        blockIdx.x, gridDim.x);
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
