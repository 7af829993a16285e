// The float64 instantiation of the learner kernels (learner_impl.h), built with -ffp-contract=off: one rounding per written operation,
// as actor_f64.hip (the forward pass is the actor's chain of explicit fma either way).
#include "learner_impl.h"

LEARNER_DEFINE_LAUNCH(double)
