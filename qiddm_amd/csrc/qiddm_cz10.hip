// qiddm_cz10.hip -- launch side of the register-resident reverse sweep of 10-qubit CZ circuits (qsim_cz10_adjoint.h).
// Reached from qiddm_backward_adjoint (qiddm_capi.hip).
#include "capi_common.h"

#include <hip/hip_runtime.h>

#include <cstdlib>

#include "qsim_cz10_adjoint.h"

namespace qiddm_capi {

bool cz10_adjoint_eligible(const qiddm_circuit_t* c) {
  static const bool off = std::getenv("QIDDM_NO_LEAN") != nullptr;   // kernel experiments: A/B on the same box
  return !off && c->n_qubits == 10 && c->imprimitive == QIDDM_IMP_CZ &&
         (c->encoding == QIDDM_ENC_NONE || c->encoding == QIDDM_ENC_RZ) && c->n_rounds == 1 &&
         (int64_t)c->n_blocks * c->sel_layers >= 2;
}

namespace {
template <typename T>
int launch_t(const void* inputs, const void* tail, const void* gout, void* partials, int64_t slab_stride,
             void* grad_inputs, int64_t gin_ld, const qiddm::KScalars& p, int64_t grid, hipStream_t st) {
  const int64_t layers = (int64_t)p.n_blocks * p.sel_layers;
  const size_t smem = qiddm::Cz10AdjSmem<T>::bytes(layers);
  if (smem > kMaxLds)
    return fail(QIDDM_ERR_UNSUPPORTED, "circuit with %lld layers needs %zu B of LDS for the reverse sweep (limit %zu)",
                (long long)layers, smem, kMaxLds);
  return launch<qiddm::cz10_adjoint_kernel<T>>(
      kMaxLds, dim3((unsigned)grid), dim3(qiddm::kCz10Waves * qiddm::kWave), smem, st, "cz10_adjoint_kernel",
      static_cast<const T*>(inputs), static_cast<const T*>(tail), static_cast<const T*>(gout),
      static_cast<T*>(partials), slab_stride, static_cast<T*>(grad_inputs), gin_ld, p);
}
}  // namespace

int launch_cz10_adjoint(int dtype, const void* inputs, const void* tail, const void* gout, void* partials,
                        int64_t slab_stride, void* grad_inputs, int64_t gin_ld, const qiddm::KScalars& p, int64_t grid,
                        void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  return for_dtype(dtype, [&](auto t) {
    return launch_t<decltype(t)>(inputs, tail, gout, partials, slab_stride, grad_inputs, gin_ld, p, grid, st);
  });
}

}  // namespace qiddm_capi
