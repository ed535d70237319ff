// qsim_mixed_shots.h -- the sampled read-out of the density-matrix engines (QIDDM_MIX_SHOTS, include/qiddm_hip.h):
// `shots` computational-basis outcomes per sample, drawn from the diagonal of rho in the launch that holds it, and
// handed back as the estimates a device returns -- count[k] / shots or (n+ - n-) / shots per wire.  PennyLane's
// default.mixed with shots=... does this on the host (numpy.random.choice over the probabilities).
//
// One workgroup of 256 threads per sample; both engines call the one routine below (qsim_mixed.h: where
// mixed_read_out stands in the analytic kernel; qsim_mixed_wide.h: a read-out kernel of its own over the resident slabs).
//   1. gather   p_k = max((double)Re rho_kk, 0) into LDS (a NaN counts as 0); the histogram is cleared.
//   2. scan     c_k = p_0 + ... + p_k, inclusive, float64, SEQUENTIAL in k (thread 0; loads four ahead of the dependent
//               adds): the order numpy.cumsum takes, so a CPU reference has the same boundaries bit for bit.  T = c_{D-1}.
//   3. draw     thread t takes the groups of four shots g = t, t + 256, ...: one Philox4x32-10 call per group, counter
//               (g, sample, offset lo, offset hi), key (seed lo, seed hi); shot s = 4 g + j uses word j.
//               v = ((double)word * 2^-32) * T; outcome = #{k : c_k <= v}, clamped to D - 1 (v < T, so the clamp never
//               acts): n steps of a branch-free binary search in LDS.  The first steps read one address in all lanes (a
//               broadcast); the last ones scatter -- a few-way bank conflict per ds_read_b64, against 10 Philox rounds.
//   4. count    ds_add_u32 into the histogram: integers, so the arrival order does not matter and reruns are
//               bit-identical.  <Z_w>: signed sums of the histogram per wire, int64 in registers, a wave reduction,
//               four partials per wire in LDS.  One float64 division of exact integers per output.
// `sample` is the absolute row of the batch: neither the sample loop of the one-workgroup engine nor the chunks of the
// tile-fused one move a stream.  T <= 0 or not finite: the row is NaN.
#pragma once
#include "qsim_fused.h"
#include "qsim_philox.h"

namespace qiddm {

struct MixedShots {
  uint32_t shots;             // 1 .. 2^31 - 1 (0: the read-out is analytic; the sampling kernels are not launched)
  uint32_t seed_lo, seed_hi;  // the Philox key
  uint32_t off_lo, off_hi;    // counter words 2 and 3
};

// s_cdf: max(2^n, 4 n) doubles of LDS, s_cnt: 2^n words.  Every thread of the 256 calls it; the caller's barrier follows.
template <typename T>
__device__ void mixed_sample_read_out(const V2<T>* __restrict__ rho, double* __restrict__ out_row, double* s_cdf,
                                      uint32_t* s_cnt, int n, int measure, int64_t sample, const MixedShots sh) {
  const int tid = threadIdx.x;
  const uint32_t D = 1u << n;
  for (uint32_t k = tid; k < D; k += 256) {
    s_cdf[k] = fmax((double)rho[((size_t)k << n) | k].x, 0.0);
    s_cnt[k] = 0u;
  }
  __syncthreads();
  if (tid == 0) {
    double c = 0.0;
    if (D >= 4) {
      for (uint32_t k = 0; k < D; k += 4) {
        const double p0 = s_cdf[k], p1 = s_cdf[k + 1], p2 = s_cdf[k + 2], p3 = s_cdf[k + 3];
        c += p0;
        s_cdf[k] = c;
        c += p1;
        s_cdf[k + 1] = c;
        c += p2;
        s_cdf[k + 2] = c;
        c += p3;
        s_cdf[k + 3] = c;
      }
    } else {
      c += s_cdf[0];
      s_cdf[0] = c;
      c += s_cdf[1];
      s_cdf[1] = c;
    }
  }
  __syncthreads();
  const double total = s_cdf[D - 1];
  const uint32_t width = measure == 0 ? D : (uint32_t)n;
  if (!(total > 0.0) || !isfinite(total)) {  // the same value in every thread: no barrier is skipped by some
    for (uint32_t k = tid; k < width; k += 256) out_row[k] = __builtin_nan("");
    return;
  }
  const uint32_t groups = (sh.shots + 3u) >> 2;
  for (uint32_t g = tid; g < groups; g += 256) {
    uint32_t w[4] = {g, (uint32_t)sample, sh.off_lo, sh.off_hi};
    philox4x32_10(w[0], w[1], w[2], w[3], sh.seed_lo, sh.seed_hi);
    const uint32_t left = sh.shots - 4u * g;  // >= 1; the last group may be partial
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if ((uint32_t)j < left) {
        const double v = ((double)w[j] * 2.3283064365386963e-10) * total;  // 2^-32: the first product is exact
        uint32_t pos = 0;
        for (uint32_t step = D >> 1; step > 0; step >>= 1) pos += s_cdf[pos + step - 1] <= v ? step : 0u;
        atomicAdd(&s_cnt[pos], 1u);
      }
    }
  }
  __syncthreads();
  const double shots = (double)sh.shots;
  if (measure == 0) {
    for (uint32_t k = tid; k < D; k += 256) out_row[k] = (double)s_cnt[k] / shots;
    return;
  }
  long long* s_sum = reinterpret_cast<long long*>(s_cdf);  // the prefix sums are done with: [wire][wavefront]
  for (int w = 0; w < n; ++w) {
    long long part = 0;
    for (uint32_t k = tid; k < D; k += 256) {
      const long long c = (long long)s_cnt[k];
      part += ((k >> (n - 1 - w)) & 1u) ? -c : c;
    }
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if ((tid & 63) == 0) s_sum[4 * w + (tid >> 6)] = part;
  }
  __syncthreads();
  if (tid < n) {
    const long long sum = s_sum[4 * tid] + s_sum[4 * tid + 1] + s_sum[4 * tid + 2] + s_sum[4 * tid + 3];
    out_row[tid] = (double)sum / shots;
  }
}

}  // namespace qiddm
