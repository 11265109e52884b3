// azr_train_common.hpp — constants of the optimiser step: the layout of the AZRW vector and of the step's slabs
// (A private header of azr_train.hip, the one translation unit that includes it: everything here has internal linkage.)
#pragma once
#include <stddef.h>
#include "azr_internal.hpp"

namespace {

using namespace azr;

constexpr int KC = 9 * NF;        // im2col row length of a tower conv
constexpr int SIN = 16;           // stem input planes padded 13 -> 16
constexpr int KS = 9 * SIN;       // im2col row length of the stem conv
constexpr float BN_EPS = 1e-3f;   // tf.layers.batch_normalization epsilon
constexpr float BN_KEEP = 0.99f;  // momentum
constexpr float L2_C = 1e-3f;     // REGULARIZATION_L2_C (build_graph.py:30)
constexpr float LR = 1e-3f, ADAM_B1 = 0.9f, ADAM_B2 = 0.999f, ADAM_EPS = 1e-8f;  // build_graph.py:31,103
constexpr int RB = 64;            // rows per block in the two-stage reductions

// AZRW offsets (same arithmetic as azr_net.hip)
constexpr size_t LAYER = (size_t)9 * NF * NF + 4 * NF;
constexpr size_t OFF_STEM_BN = 9 * 13 * NF;
constexpr size_t OFF_BLOCK0 = OFF_STEM_BN + 28;
// per-board dense-gradient partials (t_head_bwd): pd_w | pd_b | v1_w | v1_b | v2_w | v2_b
constexpr int HP_PD_W = 0, HP_PD_B = 3612, HP_V1_W = 3655, HP_V1_B = 14407, HP_V2_W = 14663, HP_V2_B = 14919, HP_FLOATS = 14920;

}  // namespace
