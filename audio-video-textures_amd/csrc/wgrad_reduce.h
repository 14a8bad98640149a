// The second pass of the deterministic weight gradients (wgrad_reduce.hip), as wgrad_x3.hip and stem_train.hip call it.
#pragma once
#include "avt_common.h"

namespace avt {

// ws [nchunk][cout][E] -> dw [cout][ldw] (first E columns), chunks in ascending order.  The caller has checked the pointers
// (ws 16-byte aligned and large enough, dw 16-byte aligned) and E % 4 == 0, ldw >= E.
int wgrad_reduce(const char* who, const float* ws, float* dw, int nchunk, int cout, int E, int ldw, hipStream_t st);

}  // namespace avt
