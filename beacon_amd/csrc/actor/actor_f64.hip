// The float64 instantiation of the actor kernel (actor_impl.h), built with -ffp-contract=off: one rounding per written operation.
#include "actor_impl.h"

ACTOR_DEFINE_LAUNCH(double)
