"""beacon_amd -- MI355X-native batched stepper for the solver hot path of jviquerat/beacon.

Batched envs (tensors on the GPU, one HIP launch per step):
    VecRayleigh, VecMixing, VecBurgers, VecShkadov, VecSloshing, VecLorenz, VecVortex
Drop-in single-env mirrors of the reference classes:  beacon_amd.envs.{rayleigh, mixing, ...}
Multi-GPU replica sharding:  beacon_amd.dist.ShardedVecEnv
Full on-device state of a batch:  VecEnv.snapshot() -> Snapshot, VecEnv.restore(snap, src, mask), VecEnv.fork(src)
Auto-reset and episode statistics on the device:  VecEnv.step_autoreset(a) -> (obs, rwd, done, trunc, EpisodeStats) -- the step, one
bookkeeping launch (episode return / length, the terminal observation in final_obs) and the masked reset of finished replicas;
VecEnv.track_episodes() for the bookkeeping alone, VecEnv.capture(..., autoreset=True) for graph rollouts across episode ends
The actor of a rollout on the device:  Actor(env, hidden=(64, 64)) -- a policy MLP and a value MLP, the draw from the project's Philox
stream, log-probability and value in ONE launch (actor.act() -> actions; libbeacon_actor.so, include/beacon_actor.h)
The PPO update of that actor on the device:  Learner(actor, lr=3e-4) -- the clipped-surrogate loss, its gradient with respect to every
parameter and Adam on actor.params in place, five launches per minibatch (learner.update(ro, adv, ret); libbeacon_learner.so,
include/beacon_learner.h)
A whole update without the host:  learner.plan(ro, epochs=10, minibatches=4, seed=7) -> Plan -- the minibatch shuffle from the project's
Philox stream, the advantage standardisation in float64, a KL early stop and a learning-rate schedule decided on the device;
plan.run(adv, ret), or plan.capture(adv, ret) for ONE graph (libbeacon_epochs.so, include/beacon_epochs.h)
Off-policy learning on the device:  TD3(env, hidden=(64, 64)) / TD3.ddpg(env) -- a deterministic policy, one or two critics, their targets
and two Adam optimisers; agent.replay(capacity) -> Replay, a ring of transitions that Rollouts are appended to; agent.act(mode=...),
mem.append(ro), agent.update(mem, n_updates, batch_size) or agent.plan(...).capture() for ONE graph (libbeacon_td3.so, include/beacon_td3.h)
Soft actor-critic over the same Replay:  SAC(env, hidden=(64, 64), alpha=1.0, auto_alpha=True) -- a tanh-squashed Gaussian policy with a
state-dependent log-std, one or two critics, their targets and a learned temperature; agent.act(mode="sample" | "deterministic" |
"uniform"), agent.update(mem, n_updates, batch_size) or agent.plan(...).capture() for ONE graph (libbeacon_sac.so, include/beacon_sac.h)
Value-based learning for the discrete envs over the same Replay:  DQN(env, hidden=(64, 64), double=True, dueling=False, huber=1.0, eps=0.1)
-- one Q network with an output per action and its target; agent.act(mode="greedy" | "epsilon" | "uniform") -> int32 [B] actions,
mem.append(ro) from int32 rollout actions, agent.update(mem, n_updates, batch_size, target_every) or agent.plan(...).capture() for ONE
graph (libbeacon_dqn.so, include/beacon_dqn.h)
Evolution strategies, one policy per member of a population:  ES(env, members=None, hidden=(64, 64), sigma=0.05, lr=0.01) -- antithetic
Gaussian perturbations of one parameter vector, replica b under member b // R of the population in ONE act launch (an MLP whose
weights differ per row group), first-episode returns as fitness, centred ranks and Adam; agent.begin(), agent.act(), agent.observe(),
agent.update(), agent.act(shared=True) to evaluate theta; no backward pass, no replay memory (libbeacon_es.so, include/beacon_es.h)
Multi-agent shkadov under one shared policy:  Actor(env, per_jet=True) -- every (replica, jet) a row of that actor and that update

Importing the package does not touch the GPU; constructing an env does, and raises if the HIP
library or a ROCm device is missing (there is no CPU fallback for the solver path)."""
from .vec import Box, Discrete, EpisodeStats, JetStats, Normalizer, Rollout, RolloutOverflow, Snapshot, VecBurgers, VecEnv, VecLorenz, VecMixing, VecRayleigh, VecShkadov, VecSloshing, VecVortex  # noqa: F401
from .actor import Actor  # noqa: F401
from .learner import Learner  # noqa: F401
from .epochs import Plan  # noqa: F401
from .td3 import TD3, Replay  # noqa: F401
from .sac import SAC  # noqa: F401
from .dqn import DQN  # noqa: F401
from .es import ES  # noqa: F401
from .lorenz import lorenz  # noqa: F401
from .vortex import vortex  # noqa: F401

__version__ = "0.1.0"

VEC_ENVS = {"rayleigh-v0": VecRayleigh, "mixing-v0": VecMixing, "burgers-v0": VecBurgers,
            "shkadov-v0": VecShkadov, "sloshing-v0": VecSloshing, "lorenz-v0": VecLorenz, "vortex-v0": VecVortex}


def make_vec(env_id, batch, **kwargs):
    """make_vec("rayleigh-v0", 512, L=2.56, H=1.28) -- env ids as listed in the reference README."""
    return VEC_ENVS[env_id](batch, **kwargs)
