// qiddm_lean.hip -- C entry points of the lean sampling loop of the 8-qubit dense nets (qsim_lean.h):
// qiddm_dense_sample_lean_tables_bytes / _prepare / _check / qiddm_dense_sample_lean (include/qiddm_hip.h).
#include "capi_common.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "qsim_lean_solo.h"

namespace {

using qiddm_capi::fail;
using qiddm_capi::for_dtype;
using qiddm_capi::kMaxLds;

template <typename T>
size_t lean_lds(int n, int layers, int rounds) {
  return n == 8 ? qiddm::LeanTables<T, 8>::lds_bytes(layers, rounds) : qiddm::LeanTables<T, 6>::lds_bytes(layers, rounds);
}
template <typename T>
size_t lean_bytes(int n, int layers, int rounds) {
  return n == 8 ? qiddm::LeanTables<T, 8>::bytes(layers, rounds) : qiddm::LeanTables<T, 6>::bytes(layers, rounds);
}

// the family the lean kernel is written for: 8 or 6 wires, RZ data encoding, CZ rings, <Z> read-out
int lean_layers(const qiddm_circuit_t* c) {
  if ((c->n_qubits != 8 && c->n_qubits != 6) || c->imprimitive != QIDDM_IMP_CZ || c->encoding != QIDDM_ENC_RZ ||
      c->measure != QIDDM_MEAS_EXPZ)
    return fail(QIDDM_ERR_UNSUPPORTED, "lean sampling loop: 6 or 8 qubits, CZ rings, RZ encoding, <Z> read-out only");
  const int64_t layers = (int64_t)c->n_rounds * c->n_blocks * c->sel_layers;
  if (layers > 128)
    return fail(QIDDM_ERR_UNSUPPORTED, "lean sampling loop: %lld layers (limit 128)", (long long)layers);
  const size_t lds = for_dtype(c->dtype, [&](auto t) { return lean_lds<decltype(t)>(c->n_qubits, (int)layers, c->n_rounds); });
  if (lds > kMaxLds)
    return fail(QIDDM_ERR_UNSUPPORTED, "lean sampling loop: %lld layers need %zu B of LDS (limit %zu)",
                (long long)layers, lds, kMaxLds);
  return (int)layers;
}

// The circuits that dispatch_lean_n can route to the solo kernel (qsim_lean.h: lean_has_solo, with LPR = 14): their
// tables carry the circuit's read-out (qsim_lean_solo.h: lean_solo_readout_kernel), and the solo kernel relies on it.
constexpr int kLeanSoloLpr = 14;
bool lean_solo_family(const qiddm_circuit_t* c) {
  return c->dtype == QIDDM_F32 && c->n_qubits == 8 && c->n_blocks == 1 && c->n_blocks * c->sel_layers == kLeanSoloLpr &&
         c->n_rounds == 1;
}

qiddm::KScalars params_of(const qiddm_circuit_t* c) {
  qiddm::KScalars p;
  std::memset(&p, 0, sizeof(p));
  p.encoding = c->encoding;
  p.imprimitive = c->imprimitive;
  p.measure = c->measure;
  p.n_rounds = c->n_rounds;
  p.n_blocks = c->n_blocks;
  p.sel_layers = c->sel_layers;
  p.n_features = c->n_features;
  p.enc_scale = c->enc_scale;
  p.enc_offset = c->enc_offset;
  p.pad_with = c->pad_with;
  return p;
}

// When the instance that carries both bodies (qsim_lean.h: lean_has_solo) runs the one-wavefront-per-item body: from
// kLeanSoloMinSteps steps per launch on at every batch, below that from kLeanSoloMinItems items (batch x n_steps) on.
// A solo workgroup executes no gate (the circuit's read-out comes with the tables): its threads load linear_up's
// operands and the read-out, compute the workgroup's one row, and behind one barrier every wavefront stores that row
// once per item it was dealt: ~4.1 us whatever the launch holds up to 1 024 items, and the image stores beyond that;
// the four-wave body pays ~2.7 us per step of a sample.  Measured by tools/ab_lean_solo_threshold.py, float32, P = 784
// (profiles/lean_tabled/threshold.txt; us per launch, four-wave / solo):
//   1 step:     1 item  5.0 / 3.6     256 items 5.7 / 4.1     512 items 7.8 / 4.2    1 024 items 13.2 / 4.4
//             2 048 items 24.0 / 5.2   4 096 items 37.6 / 6.9
//   4 steps:   64 items 13.2 / 4.1    1 024 items 14.5 / 4.3
//   15 steps: 240 items 42.2 / 4.1    3 840 items 45.4 / 6.6    15 360 items 100.1 / 16.7
// Since the solo body no longer simulates there is no crossover left: it is the faster one from a single item on.
// The constants stay where they were: the four-wave body's row differs from the solo row in the last bits, so moving a
// threshold changes results, and that is a change of its own.
// (2 and 3 steps are not in the table: the step rule stays where it was measured.)
constexpr int kLeanSoloMinSteps = 4;
constexpr int64_t kLeanSoloMinItems = 1024;

int lean_cu_count() {
  static int cus[qiddm_capi::DeviceFlags::kMaxDevices] = {};
  const int dev = qiddm_capi::DeviceFlags::current();
  if (dev >= 0 && cus[dev] > 0) return cus[dev];
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev < 0 ? 0 : dev) != hipSuccess || n < 1) n = 256;
  if (dev >= 0) cus[dev] = n;
  return n;
}

// QIDDM_LEAN_SOLO_MIN_ITEMS replaces the rule by a bare item count (kernel experiments: A/B in one process; 0 = always
// the solo body, -1 = never)
bool lean_solo_wanted(int64_t items, int n_steps) {
  const char* e = std::getenv("QIDDM_LEAN_SOLO_MIN_ITEMS");
  if (e == nullptr || *e == 0) return n_steps >= kLeanSoloMinSteps || items >= kLeanSoloMinItems;
  const long long v = std::atoll(e);
  return v >= 0 && items >= (int64_t)v;
}

// Wavefronts per workgroup of the solo kernel: 8 (two per SIMD) while that gives every item a wavefront of its own on
// as many CUs as the launch can use, 16 (four per SIMD) above that.  QIDDM_LEAN_SOLO_WAVES = 8 / 16 forces the width
// (A/B runs only; read at every launch, as QIDDM_LEAN_SOLO_MIN_ITEMS is; anything else leaves the rule in place).
int lean_solo_waves(int64_t items, int64_t cus) {
  const char* e = std::getenv("QIDDM_LEAN_SOLO_WAVES");
  if (e != nullptr && *e != 0) {
    const long long v = std::atoll(e);
    if (v == 8 || v == 16) return (int)v;
  }
  return items <= 8 * cus ? 8 : 16;
}
// One workgroup per CU at most, and at either width another CU for every 8 items while the CUs last: a launch that the
// rule gives 16 wavefronts per workgroup (more than 8 items per CU) is on every CU, so the benchmark's 3 840 items are
// 15 per CU on 256 CUs -- ceil(items / 16) workgroups would be 240 of 16 items, and 16 CUs idle.
unsigned lean_solo_grid(int64_t items, int64_t cus) {
  const int64_t want = (items + 7) / 8;
  return (unsigned)(want < cus ? want : cus);
}

template <typename T, int N, int PPT, bool REUP, int LPR, bool POST>
int launch_lean(const double* x, const double* wd, const double* bd, const double* wu, const double* bu, double* y,
                const void* tables, const qiddm::QuadScalars& d, const qiddm::KScalars& p, int layers, hipStream_t st) {
  if constexpr (qiddm::lean_has_solo<T, N, PPT, REUP, LPR, POST>()) {
    const int64_t items = p.batch * d.n_steps;
    // (the body counts items and waves in 32 bits)
    if (lean_solo_wanted(items, d.n_steps) && items < ((int64_t)1 << 31) && d.out_features <= qiddm::kSoloMaxPixels) {
      static_assert(qiddm::LeanSoloLds::bytes(qiddm::kSoloMaxPixels) <= kMaxLds, "the largest image fits LDS");
      const size_t smem = qiddm::LeanSoloLds::bytes(d.out_features);   // the row: 7 KiB at 784 pixels, 8 KiB at 1 024
      const int64_t cus = lean_cu_count();                                   // one workgroup per CU at most
      const int waves = lean_solo_waves(items, cus);
      const unsigned grid = lean_solo_grid(items, cus);
      const unsigned char* tb = static_cast<const unsigned char*>(tables);
      if (waves == 16)
        return qiddm_capi::launch<qiddm::dense_lean_solo_kernel<LPR, 16>>(
            kMaxLds, dim3(grid), dim3(qiddm::solo_threads(16)), smem, st, "dense_lean_solo_kernel", wu, bu, y, tb, d, p);
      return qiddm_capi::launch<qiddm::dense_lean_solo_kernel<LPR, 8>>(
          kMaxLds, dim3(grid), dim3(qiddm::solo_threads(8)), smem, st, "dense_lean_solo_kernel", wu, bu, y, tb, d, p);
    }
  }
  const size_t smem = qiddm::LeanTables<T, N>::lds_bytes(layers, p.n_rounds,
                                                         !qiddm::lean_tables_in_registers<REUP, LPR>());
  const unsigned blocks = (unsigned)(p.batch < 2048 ? p.batch : 2048);
  return qiddm_capi::launch<qiddm::dense_lean_kernel<T, N, PPT, REUP, LPR, POST>>(
      kMaxLds, dim3(blocks), dim3(256), smem, st, "dense_lean_kernel", x, wd, bd, wu, bu, y,
      static_cast<const unsigned char*>(tables), d, p);
}

// the instantiation for this circuit: re-upload or not; layers per round compiled in for the shapes the reference's
// drivers use (src/mnist_exm.py:46-48, src/fashion_exm.py:45) -- 8 qubits: 14 (QNN_noise(784, 8, 14)) and 12 (the
// (8, 6, 2) LL / PL nets); 6 qubits: 28 (QIDDM_LL_noise(784, 6, 14, 2), the MNIST default) and 14 -- a runtime count
// otherwise
template <typename T, int N, bool POST>
int dispatch_lean_n(const double* x, const double* wd, const double* bd, const double* wu, const double* bu, double* y,
                    const void* tables, const qiddm::QuadScalars& d, const qiddm::KScalars& p, int layers, hipStream_t st) {
  const bool reup = p.n_blocks > 1;
  const int lpr = p.n_blocks * p.sel_layers;
  constexpr int kReupLpr = N == 8 ? 12 : 28;
  if (d.in_features > 1024)
    return reup ? launch_lean<T, N, 8, true, 0, POST>(x, wd, bd, wu, bu, y, tables, d, p, layers, st)
                : launch_lean<T, N, 8, false, 0, POST>(x, wd, bd, wu, bu, y, tables, d, p, layers, st);
  if (reup) {
    if (lpr == kReupLpr && p.sel_layers == 2)
      return launch_lean<T, N, 4, true, kReupLpr, POST>(x, wd, bd, wu, bu, y, tables, d, p, layers, st);
    return launch_lean<T, N, 4, true, 0, POST>(x, wd, bd, wu, bu, y, tables, d, p, layers, st);
  }
  // (the compiled-in count keeps the tables in registers for one round: qsim_lean.h)
  if (lpr == 14 && p.n_rounds == 1) return launch_lean<T, N, 4, false, 14, POST>(x, wd, bd, wu, bu, y, tables, d, p, layers, st);
  return launch_lean<T, N, 4, false, 0, POST>(x, wd, bd, wu, bu, y, tables, d, p, layers, st);
}
template <typename T>
int dispatch_lean(int n, const double* x, const double* wd, const double* bd, const double* wu, const double* bu, double* y,
                  const void* tables, const qiddm::QuadScalars& d, const qiddm::KScalars& p, int layers, hipStream_t st) {
  if (d.post_mode == 1)
    return n == 8 ? dispatch_lean_n<T, 8, true>(x, wd, bd, wu, bu, y, tables, d, p, layers, st)
                  : dispatch_lean_n<T, 6, true>(x, wd, bd, wu, bu, y, tables, d, p, layers, st);
  return n == 8 ? dispatch_lean_n<T, 8, false>(x, wd, bd, wu, bu, y, tables, d, p, layers, st)
                : dispatch_lean_n<T, 6, false>(x, wd, bd, wu, bu, y, tables, d, p, layers, st);
}

}  // namespace

extern "C" {

int64_t qiddm_dense_sample_lean_tables_bytes(const qiddm_circuit_t* c) {
  int rc = qiddm_capi::check_circuit(c);
  if (rc != QIDDM_OK) return rc;
  const int layers = lean_layers(c);
  if (layers < 0) return layers;
  return (int64_t)for_dtype(c->dtype, [&](auto t) { return lean_bytes<decltype(t)>(c->n_qubits, layers, c->n_rounds); });
}

int qiddm_dense_sample_lean_prepare(const qiddm_circuit_t* c, const double* angles, const double* w_down,
                                    const double* b_down, const double* w_up, const double* b_up, int64_t features,
                                    void* tables, void* stream) {
  const int64_t need = qiddm_dense_sample_lean_tables_bytes(c);
  if (need < 0) return (int)need;
  if (!angles || !tables || !w_down || !w_up) return fail(QIDDM_ERR_INVALID, "angles/tables/w_down/w_up is NULL");
  if (features < 1 || features > 2048) return fail(QIDDM_ERR_INVALID, "features=%lld outside 1..2048", (long long)features);
  const qiddm::KScalars p = params_of(c);
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned char* tb = static_cast<unsigned char*>(tables);
  const int f = (int)features;
  auto prepare = [&](auto N) {
    return for_dtype(c->dtype, [&](auto t) {
      hipLaunchKernelGGL((qiddm::lean_tables_kernel<decltype(t), N()>), dim3(1), dim3(256), 0, st, angles, w_down, b_down,
                         w_up, b_up, f, tb, p);
      return qiddm_capi::launched("lean_tables_kernel");
    });
  };
  const int rc = c->n_qubits == 8 ? prepare(std::integral_constant<int, 8>{}) : prepare(std::integral_constant<int, 6>{});
  if (rc != QIDDM_OK || !lean_solo_family(c)) return rc;
  // (behind the builder on the same stream: it reads the body that kernel wrote and overwrites the header's zeros)
  hipLaunchKernelGGL((qiddm::lean_solo_readout_kernel<kLeanSoloLpr>), dim3(1), dim3(qiddm::kWave), 0, st, tb);
  return qiddm_capi::launched("lean_solo_readout_kernel");
}

int qiddm_dense_sample_lean_check(const qiddm_circuit_t* c, const void* tables, void* stream) {
  const int64_t need = qiddm_dense_sample_lean_tables_bytes(c);
  if (need < 0) return (int)need;
  if (!tables) return fail(QIDDM_ERR_INVALID, "tables is NULL");
  // the header through the read-out's tag: [0] max |tan|, [kLeanReadoutDouble ..] eight floats, [kLeanReadoutTagDouble]
  double head[qiddm::kLeanReadoutTagDouble + 1] = {};
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemcpyAsync(head, tables, sizeof(head), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(QIDDM_ERR_LAUNCH, "reading the tables' header failed: %s", hipGetErrorString(e));
  const double tmax = head[0];
  if (!(tmax == tmax && tmax <= qiddm::kLeanMaxTan)) return 0;
  if (lean_solo_family(c)) {
    // the solo kernel computes nothing but linear_up: tables without this circuit's read-out are not usable
    if (head[qiddm::kLeanReadoutTagDouble] != (double)kLeanSoloLpr) return 0;
    float ez[8];
    std::memcpy(ez, &head[qiddm::kLeanReadoutDouble], sizeof(ez));
    for (float v : ez)
      if (!std::isfinite(v)) return 0;
  }
  return 1;
}

int qiddm_dense_sample_lean(const qiddm_circuit_t* c, const double* x, int64_t batch, int64_t x_ld, int64_t features,
                            const double* w_down, const double* b_down, const double* w_up, const double* b_up,
                            int32_t post_mode, double noise_factor, int32_t n_steps, double* y, int64_t y_ld,
                            int64_t y_step_stride, const void* tables, void* stream) {
  int rc = qiddm_capi::check_circuit(c);
  if (rc != QIDDM_OK) return rc;
  const int layers = lean_layers(c);
  if (layers < 0) return layers;
  if (batch < 0 || n_steps < 0) return fail(QIDDM_ERR_INVALID, "negative batch / n_steps");
  if (post_mode != 0 && post_mode != 1) return fail(QIDDM_ERR_INVALID, "post_mode must be 0 or 1");
  if (features < 1 || features > 2048) return fail(QIDDM_ERR_UNSUPPORTED, "features=%lld outside 1..2048", (long long)features);
  if (batch == 0 || n_steps == 0) return QIDDM_OK;
  if (!x || !w_down || !w_up || !y || !tables) return fail(QIDDM_ERR_INVALID, "x/w_down/w_up/y/tables is NULL");
  if (x == y) return fail(QIDDM_ERR_INVALID, "y must not alias x");
  if (x_ld < features) return fail(QIDDM_ERR_INVALID, "x_ld=%lld < features=%lld", (long long)x_ld, (long long)features);
  if (y_ld < features) return fail(QIDDM_ERR_INVALID, "y_ld=%lld < features=%lld", (long long)y_ld, (long long)features);
  if (y_step_stride < batch * y_ld - (y_ld - features))
    return fail(QIDDM_ERR_INVALID, "y_step_stride=%lld < the %lld elements of one step", (long long)y_step_stride,
                (long long)(batch * y_ld - (y_ld - features)));
  qiddm::KScalars p = params_of(c);
  p.batch = batch;
  qiddm::QuadScalars d;
  std::memset(&d, 0, sizeof(d));
  d.x_ld = x_ld;
  d.y_ld = y_ld;
  d.y_step_stride = y_step_stride;
  d.in_features = (int32_t)features;
  d.out_features = (int32_t)features;
  d.post_mode = post_mode;
  d.n_steps = n_steps;
  d.noise_factor = noise_factor;
  // (pointer and size from ONE look at the registration: the solo body stamps 8 words per workgroup when they are there)
  int64_t stamp_words = 0;
  d.stamps = qiddm_capi::stamp_buffer(8, &stamp_words);
  d.stamp_words = (int32_t)(stamp_words < INT32_MAX ? stamp_words : INT32_MAX);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return for_dtype(c->dtype, [&](auto t) {
    return dispatch_lean<decltype(t)>(c->n_qubits, x, w_down, b_down, w_up, b_up, y, tables, d, p, layers, st);
  });
}

}  // extern "C"
