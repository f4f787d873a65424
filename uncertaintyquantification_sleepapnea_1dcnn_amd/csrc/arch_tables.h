// Channel / kernel-size tables of the reference architecture (the default spec, cnn_baseline_train.py:59-86):
// block l maps C[l] -> C[l + 1] channels with a kernel of KS[l] taps.  Plain C++: kernels and host bindings.
#pragma once

namespace apneauq {
namespace arch {

constexpr int C[7] = {4, 128, 192, 224, 96, 256, 96};
constexpr int KS[6] = {7, 5, 3, 7, 9, 9};

}  // namespace arch
}  // namespace apneauq
