// What other translation units may ask of a constraint system (the object is private to csrc/mnt753_r1cs.hip).
#pragma once
#include "../../include/mnt753_hip.h"

namespace mnt753 {
// the curve of a constraint system (-1 for a null one) and the device it lives on: physical HIP ordinal, *logical = logical device
int r1cs_curve(const mnt753_r1cs* r);
int r1cs_device(const mnt753_r1cs* r, int* logical);
}  // namespace mnt753
