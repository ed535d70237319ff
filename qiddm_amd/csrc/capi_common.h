// capi_common.h -- what the translation units behind include/qiddm_hip.h share: the thread-local
// error string, descriptor validation, launch limits, and the three helpers every launch site goes through
// (launch / for_qubits / for_dtype).
#pragma once
#include "../../include/qiddm_hip.h"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <utility>

namespace qiddm_capi {

constexpr size_t kMaxLds = 160 * 1024;  // per-workgroup LDS on gfx950

// formats the thread's error message (read back by qiddm_last_error) and returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int check_circuit(const qiddm_circuit_t* c);

// the buffer registered with qiddm_set_stamp_buffer if it holds at least `need_words` words, else nullptr; have_words:
// how many words the returned buffer holds (0 with nullptr), from the same look at the registration
unsigned long long* stamp_buffer(int64_t need_words, int64_t* have_words = nullptr);
int set_stamp_buffer(void* device_ptr, int64_t n_words);

// "done once" marker per HIP device: hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device,
// so a process that drives a second GPU has to repeat it there.  Races are benign (the call is idempotent).
struct DeviceFlags {
  static constexpr int kMaxDevices = 64;
  bool done[kMaxDevices] = {};
  static int current() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) return -1;
    return d;
  }
  bool get() const { const int d = current(); return d >= 0 && done[d]; }   // unknown device: always re-apply
  void set() { const int d = current(); if (d >= 0) done[d] = true; }
};

// a launch that needs no attribute step (no dynamic LDS, or never above 48 KiB): checks it and names it on failure
inline int launch_status(const char* what, hipError_t e) {
  if (e != hipSuccess) return fail(QIDDM_ERR_LAUNCH, "%s launch failed: %s", what, hipGetErrorString(e));
  return QIDDM_OK;
}
inline int launched(const char* what) { return launch_status(what, hipGetLastError()); }

// Launches `kern` with `smem` bytes of dynamic LDS.  Above 48 KiB the kernel first needs its
// MaxDynamicSharedMemorySize raised to `lds_limit`, once per device: `flags` remembers where that has been done
// (benign race: the attribute call is idempotent).  At or below 48 KiB this makes no HIP call beyond the launch and
// its check.  This form is for a kernel chosen at run time: one `flags` per choice.
template <typename K, typename... Args>
int launch_with(K kern, DeviceFlags& flags, size_t lds_limit, dim3 grid, dim3 block, size_t smem, hipStream_t stream,
                const char* what, const Args&... args) {
  if (smem > 48 * 1024 && !flags.get()) {
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit);
    if (ea != hipSuccess) return fail(QIDDM_ERR_LAUNCH, "hipFuncSetAttribute(LDS) failed: %s", hipGetErrorString(ea));
    flags.set();
  }
  hipLaunchKernelGGL(kern, grid, block, smem, stream, args...);
  return launched(what);
}

// the flags of one kernel instantiation
template <auto Kern>
DeviceFlags& lds_flags() {
  static DeviceFlags flags;
  return flags;
}

// the usual form: the kernel is known at compile time and brings its own flags
template <auto Kern, typename... Args>
int launch(size_t lds_limit, dim3 grid, dim3 block, size_t smem, hipStream_t stream, const char* what,
           const Args&... args) {
  return launch_with(Kern, lds_flags<Kern>(), lds_limit, grid, block, smem, stream, what, args...);
}

// Calls f(std::integral_constant<int, N>{}) for N == n, LO <= N <= HI: the one place that lists wire counts.
// The pure size helpers (LDS bytes, table bytes, block counts) come through here too and get the failure code cast
// to their return type for a width outside the range; every caller of those has already bounded n.
// (A left fold on purpose: it instantiates f in ascending N, and the order of instantiation is the order of the
// kernels in the code object.)
template <int LO, typename F, int... I>
auto for_qubits_impl(int n, const char* what, F& f, std::integer_sequence<int, I...>) {
  using R = decltype(f(std::integral_constant<int, LO>{}));
  R r{};
  const bool hit = (... || (n == LO + I ? (r = f(std::integral_constant<int, LO + I>{}), true) : false));
  if (hit) return r;
  return (R)fail(QIDDM_ERR_UNSUPPORTED, "%s: n_qubits=%d outside %d..%d", what, n, LO, LO + (int)sizeof...(I) - 1);
}
template <int LO, int HI, typename F>
auto for_qubits(int n, const char* what, F&& f) {
  return for_qubits_impl<LO>(n, what, f, std::make_integer_sequence<int, HI - LO + 1>{});
}

// calls f(float{}) or f(double{}) (check_circuit has admitted no other dtype)
template <typename F>
auto for_dtype(int dtype, F&& f) {
  return dtype == QIDDM_F32 ? f(float{}) : f(double{});
}

// wide CZ forward (qiddm_wide.hip / qsim_wide_cz.h): n = 11..16, CZ entanglers, no or RZ encoding
inline bool wide_cz_eligible(const qiddm_circuit_t* c) {
  return c->n_qubits > QIDDM_MAX_QUBITS_FUSED && c->imprimitive == QIDDM_IMP_CZ &&
         (c->encoding == QIDDM_ENC_NONE || c->encoding == QIDDM_ENC_RZ);
}
int64_t wide_cz_grid(int64_t batch, int64_t slabs);
// pass-structured reverse sweep (qsim_wide_cz_adjoint.h): one round of >= 2 layers of that family.
// QIDDM_WIDE_TILED=1 keeps the generic per-gate kernels (kernel experiments: A/B on the same box)
bool wide_cz_adjoint_eligible(const qiddm_circuit_t* c);
// register-resident reverse sweep of 10-qubit CZ circuits (qsim_cz10_adjoint.h): one round of >= 2 layers
bool cz10_adjoint_eligible(const qiddm_circuit_t* c);
// 10-qubit CZ circuits with no / RZ encoding carry BOTH tails behind the gate variants: the folded tables of the n <= 10
// forward, then the per-wire tables (2n entries per layer) of the reverse sweep
inline bool cz10_tables(const qiddm_circuit_t* c) {
  return c->n_qubits == 10 && c->imprimitive == QIDDM_IMP_CZ &&
         (c->encoding == QIDDM_ENC_NONE || c->encoding == QIDDM_ENC_RZ);
}

}  // namespace qiddm_capi

namespace qiddm { struct KScalars; }
namespace qiddm_capi {
// `tail`: the per-layer tables behind the gate variants of the gate table; `slabs`: 2^n-amplitude slabs in `ws`
int launch_wide_cz(int dtype, int n, const void* inputs, const void* tail, void* out, void* ws,
                   const qiddm::KScalars& p, int64_t slabs, void* stream);
// `partials`: `grid` slabs of `slab_stride` elements ([layer][theta | alpha][16]); `ws`: `grid` pairs of slabs
int launch_wide_cz_adjoint(int dtype, int n, const void* inputs, const void* tail, const void* gout, void* partials,
                           int64_t slab_stride, void* grad_inputs, int64_t gin_ld, void* ws, const qiddm::KScalars& p,
                           int64_t grid, void* stream);
int launch_cz10_adjoint(int dtype, const void* inputs, const void* tail, const void* gout, void* partials,
                        int64_t slab_stride, void* grad_inputs, int64_t gin_ld, const qiddm::KScalars& p, int64_t grid,
                        void* stream);
}  // namespace qiddm_capi
