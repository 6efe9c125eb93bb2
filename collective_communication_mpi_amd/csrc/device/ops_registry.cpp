// Collects every op family's pybind registration.
#include "ops.hpp"

namespace ccmpi {
namespace dev {

void register_layout_ops(pybind11::module_& m);
void register_gemm_ops(pybind11::module_& m);
void register_attn_ops(pybind11::module_& m);
void register_head_ops(pybind11::module_& m);
void register_wgrad_ops(pybind11::module_& m);
void register_swiglu_ops(pybind11::module_& m);
void register_grouped_gemm_ops(pybind11::module_& m);
void register_moe_gate_ops(pybind11::module_& m);
void register_moe_router_ops(pybind11::module_& m);
void register_flash_attn_ops(pybind11::module_& m);
void register_xent_ops(pybind11::module_& m);
void register_rope_ops(pybind11::module_& m);
void register_rmsnorm_ops(pybind11::module_& m);
void register_optim_ops(pybind11::module_& m);

void register_ops(pybind11::module_& m) {
  register_layout_ops(m);
  register_gemm_ops(m);
  register_attn_ops(m);
  register_head_ops(m);
  register_wgrad_ops(m);
  register_swiglu_ops(m);
  register_grouped_gemm_ops(m);
  register_moe_gate_ops(m);
  register_moe_router_ops(m);
  register_flash_attn_ops(m);
  register_xent_ops(m);
  register_rope_ops(m);
  register_rmsnorm_ops(m);
  register_optim_ops(m);
}

}  // namespace dev
}  // namespace ccmpi
