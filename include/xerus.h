// Umbrella header of the MI355X-native xerus hot path (reference include/xerus.h:31-64).
#pragma once
#include "xerus/basic.h"
#include "xerus/index.h"
#include "xerus/indexedTensor.h"
#include "xerus/indexedTensor_tensor_factorisations.h"
#include "xerus/misc/fileIO.h"
#include "xerus/misc/random.h"
#include "xerus/tensor.h"
#include "xerus/tensorNetwork.h"
#include "xerus/ttNetwork.h"
#include "xerus/algorithms/als.h"
#include "xerus/algorithms/alsEigen.h"
#include "xerus/algorithms/retractions.h"
#include "xerus/algorithms/steepestDescent.h"
#include "xerus/algorithms/cg.h"
#include "xerus/measurments.h"
#include "xerus/algorithms/adf.h"
#include "xerus/algorithms/uqAdf.h"
#include "xerus/algorithms/largestEntry.h"
#include "xerus/algorithms/randomSVD.h"
#include "xerus/algorithms/randomizedRounding.h"
#include "xerus/algorithms/decompositionAls.h"

namespace xerus {
namespace gpu {
/// device of the calling thread's context (default 0, or $XERUS_DEVICE); must be set before first use
void set_device(int _device);
int device();
/// the calling thread's xerus_amd handle (stream + caching allocator)
struct xrs_handle_s* handle();
void synchronize();
}  // namespace gpu
}  // namespace xerus
