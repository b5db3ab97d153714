// ct_network.hpp -- what ct_neural.cpp and ct_bake.cpp need of ct_network.hip: the handle-free half of ct_network_create / ct_network_eval.
// ct_network_destroy, ct_debug_network_time and ct_debug_bf16_round need no handle and are defined in ct_network.hip itself.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cloudtrace.h"

namespace ct {

// Every CT_E_INVAL of ct_network_create except the NULL handle, with nothing allocated: CT_OK or CT_E_INVAL with `err` filled.
int network_validate(const CtNetworkDesc *d, CtNetwork *out, char *err, size_t err_len);
// Packs the weights on the host (padded, permuted, bf16) and uploads them to `device`, which is the current one.
int network_create(int device, const CtNetworkDesc *d, CtNetwork *out, char *err, size_t err_len);
int network_device(CtNetwork n);
uint32_t network_aux_inputs(CtNetwork n);   // A
// One launch on `stream`, HIP events of the network around it, and a wait for the stream.
int network_eval(CtNetwork n, hipStream_t stream, const uint8_t *descriptors_dev, const float *aux_dev, uint32_t count,
                 float *out_dev, char *err, size_t err_len);

} // namespace ct
